"""
The wiring identity as a PermCheck (HyperPlonk's ProductCheck) a verifier can check end to end.

The reference (and `hyperplonk.py` after it) SIMULATES the wiring check: a random `eq` vector, six unrelated committed
polynomials h, num, den, v(x,0), v(x,1), v(1,x), six independent product sumchecks, and nothing that ties the grand product to 1
(hyperplonk/src/hyperplonk.rs:94-141).  Here it is the real thing.  With N = 2^mu wire slots,

    num = w + alpha sid + beta,   den = w + alpha ssigma + beta,   h = num / den,   v = product_tree(h)  (2N elements),
    v(0,x) = tree[x] = h,  v(1,x) = tree[N + x],  v(x,0) = tree[2x],  v(x,1) = tree[2x + 1]      (index bit 0 = the TOP bit)

    sum_x eq(tau, x) [ v(1,x) - v(x,0) v(x,1) + gamma ( den(x) h(x) - num(x) ) ] = 0

is proved by one degree-3 sumcheck (zk_eq_table, zk_sumcheck_wiring), closed by openings of w, sid, ssigma at the sumcheck point r
and of ONE commitment to the tree at (0,r), (1,r), (r,0), (r,1) and (1,..,1,0) -- a single commitment is what binds the four views
to each other -- and verified with the device pairing.  num and den are never committed: they are linear in w, sid, ssigma.  The
grand product is v(1,..,1,0) = tree[2N - 2]; the verifier wants it to be 1.

The SRS has mu + 1 variables (the tree's); level k of PolynomialCommitmentCub.new uses the LAST k of them, so an opening of a
mu-variate table verifies against [g2, s_1 g2, .., s_mu g2] = [pg2[0]] + pg2[2:], not against the full powers_of_g2: the verifier
holds two verifying keys (`verifying_keys`) and makes two zk_pcs_verify_batch calls, 3 openings at mu variables and 5 at mu + 1.

alpha, beta, gamma, tau and the challenges are INPUTS of the functions here (the reference pre-samples every challenge,
dhyperplonk.rs:103-109).  The non-interactive form, with every challenge derived from a Fiat-Shamir transcript that lives on the
device, is zkhip.nizk.wiring_prove_ni / wiring_verify_ni.  Single party only: the distributed and packed-share forms are not defined.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .field import R_MOD, fr_from_mont, fr_mont
from .verify import _ints, eq_eval, round_chain, round_poly_at  # noqa: F401  (round_poly_at: importable from here as before)

OPENED = ("w", "sid", "ssigma")                         # the three mu-variate openings of a proof record, at r
V_POINTS = ("(0,r)", "(1,r)", "(r,0)", "(r,1)", "(1,..,1,0)")  # the five openings of the tree's commitment


def wiring_value(eq: int, v1x: int, vx0: int, vx1: int, h: int, num: int, den: int, gamma: int) -> int:
    return eq * (v1x - vx0 * vx1 + gamma * (den * h - num)) % R_MOD


def v_points(chal) -> list:
    """the five (mu + 1)-variate points of V_POINTS as [mu + 1, 4] Montgomery Fr"""
    r = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
    zero, one = np.zeros((1, 4), dtype=np.uint64), fr_mont(1).reshape(1, 4)
    return [np.concatenate([zero, r]), np.concatenate([one, r]), np.concatenate([r, zero]), np.concatenate([r, one]),
            np.concatenate([np.repeat(one, len(r), axis=0), zero])]


def failed_checks(proof: dict, alpha, beta, gamma, tau, chal) -> list:
    """
    The verifier's field arithmetic (no GPU, no pairing) -> the numbers of the checks that fail ([] = all hold; [0]: a malformed record):
      1. p_0(0) + p_0(1) == 0 and p_i(0) + p_i(1) == p_{i-1}(r_{i-1}), by interpolation on the nodes 0 .. 3;
      2. p_{mu-1}(r_{mu-1}) == eq(tau, r) [ v(1,r) - v(r,0) v(r,1) + gamma ((w + alpha ssigma + beta) v(0,r) - (w + alpha sid + beta)) ]
         on the opened values;
      3. the opened v(1,..,1,0) == 1.
    proof: the record of wiring_prove; alpha, beta, gamma: [4]; tau, chal: [mu, 4]; all Montgomery Fr.
    """
    try:
        rounds = np.asarray(proof["rounds"], dtype=np.uint64).reshape(-1, 4, 4)
        tau_i, ch = _ints(tau), _ints(chal)
        mu = len(rounds)
        if mu == 0 or len(tau_i) != mu or len(ch) != mu or len(proof["openings"]) != len(OPENED) or len(proof["v_openings"]) != len(V_POINTS):
            return [0]
        w, sid, ssigma = (fr_from_mont(np.asarray(op[1], dtype=np.uint64).reshape(4)) for op in proof["openings"])
        v0r, v1r, vr0, vr1, prod = (fr_from_mont(np.asarray(op[0], dtype=np.uint64).reshape(4)) for op in proof["v_openings"])
    except (KeyError, ValueError, TypeError):
        return [0]
    a, b, g = (_ints(x)[0] for x in (alpha, beta, gamma))
    target = round_chain(rounds, ch)
    bad = [1] if target is None else []
    num, den = (w + a * sid + b) % R_MOD, (w + a * ssigma + b) % R_MOD
    if not bad and target != wiring_value(eq_eval(tau_i, ch), v1r, vr0, vr1, v0r, num, den, g):
        bad.append(2)
    if prod != 1:
        bad.append(3)
    return bad


def verify_rounds(proof: dict, alpha, beta, gamma, tau, chal) -> bool:
    """checks 1-3 of failed_checks"""
    return not failed_checks(proof, alpha, beta, gamma, tau, chal)


def wiring_prove(be, pcs, w, sid, ssigma, N: int, alpha, beta, gamma, tau, chal, commitments: dict | None = None, timing: dict | None = None) -> dict:
    """
    be: zkhip.Ctx; pcs: the levels of a PolynomialCommitment over mu + 1 variables (`cub.mature()`); w, sid, ssigma: device buffers of
    N = 2^mu Fr; alpha, beta, gamma: [4]; tau, chal: [mu, 4] Montgomery Fr; commitments: name -> [18] for tables committed earlier.
    -> {"rounds": [mu, 4, 4], "openings": [(commitment [18], value [4], opening proof [mu, 18])] in the order of OPENED,
        "v_commitment": [18], "v_openings": [(value [4], opening proof [mu + 1, 18])] in the order of V_POINTS}.
    A zero denominator raises ZeroDivisionError (ZK_ERR_DIV_ZERO).  timing (optional dict) receives the wall seconds of the
    derived tables (num, den, h, tree, eq) and of the sumcheck.
    """
    import time

    from . import dist_primitive as dp

    tau = np.ascontiguousarray(tau, dtype=np.uint64).reshape(-1, 4)
    chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
    mu = len(tau)
    if mu < 1 or len(chal) != mu or N != 1 << mu:
        raise ValueError("tau and chal must hold one element per variable of the N = 2^mu tables (mu >= 1)")
    t0 = time.perf_counter()
    num = be.fr_axpb(w, sid, alpha, beta, N)
    den = be.fr_axpb(w, ssigma, alpha, beta, N)
    h = be.fr_batch_div(num, den, N)
    tree = be.product_tree(h, N)
    eq = be.eq_table(tau)
    be.sync()
    t1 = time.perf_counter()
    rounds, _last = be.sumcheck_wiring(eq, tree, num, den, N, gamma, chal)
    t2 = time.perf_counter()
    if timing is not None:
        timing["tables_s"], timing["sumcheck_s"] = t1 - t0, t2 - t1
    commitments = commitments or {}
    tabs = {"w": w, "sid": sid, "ssigma": ssigma}
    comms = [np.asarray(commitments[k] if k in commitments else dp.commit(be, pcs, tabs[k], N), dtype=np.uint64).reshape(18) for k in OPENED]
    v_comm = np.asarray(dp.commit(be, pcs, tree, 2 * N), dtype=np.uint64).reshape(18)
    vp = v_points(chal)
    opens = dp.open_many(be, pcs, [tabs[k] for k in OPENED] + [tree] * len(vp), [N] * len(OPENED) + [2 * N] * len(vp), [chal] * len(OPENED) + vp)
    fmt = lambda v, pf, n: (np.asarray(v, dtype=np.uint64).reshape(4), np.asarray(pf, dtype=np.uint64).reshape(n, 18))
    return {"rounds": rounds,
            "openings": [(c,) + fmt(v, pf, mu) for c, (v, pf) in zip(comms, opens[: len(OPENED)])],
            "v_commitment": v_comm,
            "v_openings": [fmt(v, pf, mu + 1) for v, pf in opens[len(OPENED):]]}


def verifying_keys(be, powers_of_g2):
    """powers_of_g2 = [g2, s_0 g2, .., s_mu g2] of the (mu + 1)-variate SRS -> (vk_mu, vk_mu1): mu-variate tables use the last mu variables"""
    from . import dist_primitive as dp

    if isinstance(powers_of_g2, np.ndarray):  # [mu + 2, 24] Montgomery records (vk_io.vk_from_bytes)
        rec = np.ascontiguousarray(powers_of_g2, dtype=np.uint64).reshape(-1, 24)
        return dp.pcs_vk(be, np.concatenate([rec[:1], rec[2:]])), dp.pcs_vk(be, rec)
    pg2 = list(powers_of_g2)
    return dp.pcs_vk(be, [pg2[0]] + pg2[2:]), dp.pcs_vk(be, pg2)


def wiring_verify(be, vk_mu, vk_mu1, proof: dict, alpha, beta, gamma, tau, chal) -> bool:
    """verify_rounds, then check 4: w, sid, ssigma at r in one zk_pcs_verify_batch (vk_mu), the tree's five openings in another (vk_mu1)"""
    from . import dist_primitive as dp

    if not verify_rounds(proof, alpha, beta, gamma, tau, chal):
        return False
    chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
    mu = len(chal)
    u64 = lambda a, *shape: np.asarray(a, dtype=np.uint64).reshape(*shape)
    ops, vops = proof["openings"], proof["v_openings"]
    ok = dp.verify_batch(be, vk_mu, np.stack([u64(o[0], 18) for o in ops]), np.stack([u64(o[1], 4) for o in ops]),
                         np.stack([u64(o[2], mu, 18) for o in ops]), np.stack([chal] * len(ops)))
    if not np.all(ok):
        return False
    ok = dp.verify_batch(be, vk_mu1, np.stack([u64(proof["v_commitment"], 18)] * len(vops)), np.stack([u64(o[0], 4) for o in vops]),
                         np.stack([u64(o[1], mu + 1, 18) for o in vops]), np.stack(v_points(chal)))
    return bool(np.all(ok))


def wiring_prove_batched(be, pcs, w, sid, ssigma, N: int, alpha, beta, gamma, tau, chal, b_alpha, rho_mu, rho_mu1, commitments: dict | None = None,
                         timing: dict | None = None) -> dict:
    """wiring_prove with TWO opening proofs instead of eight: one batch instance of mu variables (w, sid, ssigma at r) and one of mu + 1
    (the tree at the five V_POINTS), weight base b_alpha, challenges rho_mu / rho_mu1 (zkhip.batch_open, where the record is described)"""
    from .batch_open import wiring_prove_batched as impl

    return impl(be, pcs, w, sid, ssigma, N, alpha, beta, gamma, tau, chal, b_alpha, rho_mu, rho_mu1, commitments, timing)


def wiring_verify_batched(be, vk_mu, vk_mu1, proof: dict, alpha, beta, gamma, tau, chal, b_alpha, rho_mu, rho_mu1) -> bool:
    """checks 1-3 of failed_checks on the claimed values, then the two batch instances that certify them (vk_mu, vk_mu1)"""
    from .batch_open import wiring_verify_batched as impl

    return impl(be, vk_mu, vk_mu1, proof, alpha, beta, gamma, tau, chal, b_alpha, rho_mu, rho_mu1)


def proof_digest(proof: dict) -> str:
    """SHA-256 over the record's little-endian words: rounds; per opening commitment | value | proof; the tree's commitment; per
    opening of it value | proof"""
    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    put(proof["rounds"])
    for c, v, pf in proof["openings"]:
        put(c), put(v), put(pf)
    put(proof["v_commitment"])
    for v, pf in proof["v_openings"]:
        put(v), put(pf)
    return h.hexdigest()


CIRCUIT_SEED = 0x3B1E0000  # stream k of seed S is SplitMix64(CIRCUIT_SEED + 1000 S + k)


def block_permutation(mu: int, seed: int) -> np.ndarray:
    """
    sigma on 2^mu wire slots (numpy only): inside every aligned block of B = min(8, 2^mu) slots, i -> (5 i + b) mod B with
    b = (2 seed + 1) mod 8 odd -- a full-period congruential map, so every block is ONE cycle of length B.
    """
    n = 1 << mu
    blk = min(8, n)
    i = np.arange(n, dtype=np.uint64)
    low = i & np.uint64(blk - 1)
    return (i - low) + ((np.uint64(5) * low + np.uint64((2 * seed + 1) & 7)) & np.uint64(blk - 1))


def wire_values(mu: int, seed: int) -> np.ndarray:
    """w[i] = val[i >> 3] with val from SplitMix64(CIRCUIT_SEED + 1000 seed + 1): constant on the cycles of block_permutation -> [2^mu, 4]"""
    from .field import splitmix_fr

    n = 1 << mu
    return np.repeat(splitmix_fr(max(n >> 3, 1), CIRCUIT_SEED + 1000 * seed + 1), min(8, n), axis=0)


def permuted_circuit(be, mu: int, seed: int, break_wire: int | None = None):
    """
    A satisfied copy-constraint system on the device, the same in both hosts (host/examples/wiring_check.cpp): w = wire_values,
    sid[i] = i, ssigma[i] = block_permutation(i) as field elements (slot numbers uploaded as integers and multiplied by R^2 on the
    device: their Montgomery forms); break_wire K adds 1 to w[K].  alpha, beta, gamma: one element each from streams 2, 3, 4;
    tau, chal: mu elements from streams 5, 6; the SRS trapdoor s: mu + 1 elements from stream 7.
    -> (w, sid, ssigma device buffers of 2^mu Fr, alpha [4], beta [4], gamma [4], tau [mu, 4], chal [mu, 4], s [mu + 1, 4])
    """
    from .field import splitmix_fr

    n, base = 1 << mu, CIRCUIT_SEED + 1000 * seed
    wv = wire_values(mu, seed)
    if break_wire is not None:
        wv[break_wire] = fr_mont(fr_from_mont(wv[break_wire]) + 1)
    r2 = fr_mont(1 << 256)  # the Montgomery product with it takes the integer i to the Montgomery form of i
    slots = np.zeros((n, 4), dtype=np.uint64)
    slots[:, 0] = np.arange(n, dtype=np.uint64)
    sid = be.fr_scale(be.to_device(slots), r2, n)
    slots[:, 0] = block_permutation(mu, seed)
    ssigma = be.fr_scale(be.to_device(slots), r2, n)
    one = lambda k: splitmix_fr(1, base + k)[0]
    return be.to_device(wv), sid, ssigma, one(2), one(3), one(4), splitmix_fr(mu, base + 5), splitmix_fr(mu, base + 6), splitmix_fr(mu + 1, base + 7)
