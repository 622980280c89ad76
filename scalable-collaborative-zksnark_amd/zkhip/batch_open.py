"""
Batch opening (HyperPlonk's): K evaluation claims on J polynomials of one size -> ONE degree-2 sumcheck and ONE opening proof.

J tables f_0 .. f_{J-1} of N = 2^n Fr with commitments C_j; K claims (j_k, z_k, v_k) meaning f_{j_k}(z_k) = v_k; weights
a_k = alpha^k; sumcheck challenges rho.

    E_j(x) = sum_{k : j_k = j} a_k eq(z_k, x)          (zk_eq_table_acc)
    sum_x sum_j E_j(x) f_j(x) = sum_k a_k v_k =: S     one sumcheck, rounds (t0, t1, t2) as zk_sumcheck_product (zk_sumcheck_multi)
    e_j = E_j(rho),  g = sum_j e_j f_j                 (zk_fr_lincomb), opened at rho with the existing open_: g(rho) = y,
                                                        the value the round chain ends in.  No f_j(rho) is sent.

The verifier: (1) the chain from S, (2) C_g = sum_j e_j C_j (zk_g1_lincomb) with e_j = sum_k a_k eq(z_k, rho) computed by itself,
(3) one zk_pcs_verify_batch call with the single opening (C_g, y, proof, rho).

Proof record: {"rounds": [n, 3, 4], "opening": [n, 18]}.  The claimed values v_k belong to the statement, beside the commitments.
alpha and rho are INPUTS of the functions here; zkhip.nizk derives them from a Fiat-Shamir transcript (zk_sumcheck_multi_fs draws rho
on the device).  Single party only.  Index bit 0 is the TOP bit, round 0
binds it, rho is the opening point as it stands.  One instance per table size.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .field import R_MOD, fr_from_mont, fr_mont, int_to_limbs
from .verify import _ints, eq_eval, round_chain


def _norm_claims(claims, n_tables: int, n: int) -> list:
    """-> [(j, point [n, 4] u64, value [4] u64)]; ValueError on an index out of range or a point of the wrong length"""
    out = []
    for k, (j, z, v) in enumerate(claims):
        z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
        v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1)
        if not 0 <= int(j) < n_tables:
            raise ValueError(f"claim {k}: table index {j} out of range (0 .. {n_tables - 1})")
        if len(z) != n:
            raise ValueError(f"claim {k}: point of {len(z)} coordinates, the tables have {n} variables")
        if len(v) != 4:
            raise ValueError(f"claim {k}: the value is not one Fr")
        out.append((int(j), z, v))
    if not out:
        raise ValueError("no claims")
    return out


def claim_weights(alpha, count: int) -> list:
    """a_k = alpha^k, k < count, python ints"""
    a, w, out = _ints(alpha)[0], 1, []
    for _ in range(count):
        out.append(w)
        w = w * a % R_MOD
    return out


def claimed_sum(claims, alpha) -> int:
    """S = sum_k a_k v_k"""
    return sum(a * fr_from_mont(v) for a, (_, _, v) in zip(claim_weights(alpha, len(claims)), claims)) % R_MOD


def eq_coefficients(n_tables: int, claims, alpha, rho) -> list:
    """e_j = sum_{k : j_k = j} a_k eq(z_k, rho), python ints (K n multiplications)"""
    r = _ints(rho)
    e = [0] * n_tables
    for a, (j, z, _) in zip(claim_weights(alpha, len(claims)), claims):
        e[j] = (e[j] + a * eq_eval(_ints(z), r)) % R_MOD
    return e


def combined_eq_tables(be, n_tables: int, n: int, claims, alpha) -> list:
    """E_j on the device (None for a table without claims): the first claim on a table is a_k eq(z_k, .) by zk_eq_table and, unless
    a_k = 1, one zk_fr_axpb; every later one is a zk_eq_table_acc.  No buffer is zero-filled."""
    claims = _norm_claims(claims, n_tables, n)
    N = 1 << n
    tabs = [None] * n_tables
    for a, (j, z, _) in zip(claim_weights(alpha, len(claims)), claims):
        if tabs[j] is None:
            tabs[j] = be.eq_table(z)
            if a != 1:
                tabs[j] = be.fr_scale(tabs[j], fr_mont(a), N)
        else:
            be.eq_table_acc(z, fr_mont(a), tabs[j])
    return tabs


def batch_open_prove(be, pcs, tables, N: int, claims, alpha, rho, timing: dict | None = None) -> dict:
    """
    be: zkhip.Ctx; pcs: the levels of a PolynomialCommitment (`cub.mature()`); tables: J device buffers of N = 2^n Fr; claims: list of
    (j, point [n, 4], value [4]); alpha: [4]; rho: [n, 4]; all Montgomery Fr.  -> {"rounds": [n, 3, 4], "opening": [n, 18]}.
    timing (optional dict) receives the wall seconds of the eq tables, the sumcheck and the opening.
    """
    import time

    from . import dist_primitive as dp

    rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(-1, 4)
    n = len(rho)
    if n < 1 or N != 1 << n:
        raise ValueError("rho must hold one element per variable of the N = 2^n tables (n >= 1)")
    claims = _norm_claims(claims, len(tables), n)
    t0 = time.perf_counter()
    eqs = combined_eq_tables(be, len(tables), n, claims, alpha)
    used = [j for j, e in enumerate(eqs) if e is not None]
    if timing is not None:
        be.sync()
    t1 = time.perf_counter()
    rounds, last_e, _last_f = be.sumcheck_multi([eqs[j] for j in used], [tables[j] for j in used], N, rho)
    t2 = time.perf_counter()
    g = be.fr_lincomb([tables[j] for j in used], last_e, N)
    _value, opening = dp.open_(be, pcs, g, N, rho)
    t3 = time.perf_counter()
    if timing is not None:
        timing["eq_tables_s"], timing["sumcheck_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2
    return {"rounds": rounds, "opening": np.asarray(opening, dtype=np.uint64).reshape(n, 18)}


def chain_value(proof: dict, claims, alpha, rho):
    """the round chain from S -> (ok, y): y = p_{n-1}(rho_{n-1}) as a python int (None when the chain breaks or the record is malformed)"""
    try:
        rounds = np.asarray(proof["rounds"], dtype=np.uint64).reshape(-1, 3, 4)
        ch = _ints(rho)
        if len(rounds) == 0 or len(ch) != len(rounds):
            return False, None
    except (KeyError, ValueError, TypeError):
        return False, None
    y = round_chain(rounds, ch, claimed_sum(claims, alpha))
    return y is not None, y


def failed_checks(n_tables: int, claims, proof: dict, alpha, rho, finals=None) -> list:
    """
    The verifier's field arithmetic (no GPU, no pairing) -> the numbers of the checks that fail ([] = all hold; [0]: a malformed
    record or statement):
      1. p_0(0) + p_0(1) == S = sum_k a_k v_k and p_i(0) + p_i(1) == p_{i-1}(rho_{i-1}) (dsumcheck.rs:558-588);
      2. only when `finals` = the J values f_j(rho) are given (tests that hold the tables; the real verifier gets this from the
         pairing on C_g = sum_j e_j C_j instead): p_{n-1}(rho_{n-1}) == sum_j e_j f_j(rho).
    """
    try:
        n = len(np.asarray(rho, dtype=np.uint64).reshape(-1, 4))
        claims = _norm_claims(claims, n_tables, n)
        if np.asarray(proof["opening"], dtype=np.uint64).size != n * 18:
            return [0]
    except (KeyError, ValueError, TypeError):
        return [0]
    ok, y = chain_value(proof, claims, alpha, rho)
    if not ok:
        return [0] if len(np.asarray(proof["rounds"]).reshape(-1)) != n * 12 else [1]
    if finals is not None:
        e = eq_coefficients(n_tables, claims, alpha, rho)
        if y != sum(ej * fj for ej, fj in zip(e, _ints(finals))) % R_MOD:
            return [2]
    return []


def verify_rounds(n_tables: int, claims, proof: dict, alpha, rho, finals=None) -> bool:
    return not failed_checks(n_tables, claims, proof, alpha, rho, finals)


def combined_commitment(be, commitments, claims, alpha, rho) -> np.ndarray:
    """C_g = sum_j e_j C_j (zk_g1_lincomb: canonical scalars) -> [18]"""
    comms = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 18)
    e = eq_coefficients(len(comms), claims, alpha, rho)
    return be.g1_lincomb(comms, np.stack([int_to_limbs(x, 4) for x in e]))


def batch_open_verify(be, vk, commitments, claims, proof: dict, alpha, rho) -> bool:
    """checks 1-3 of the module text; vk: dist_primitive.pcs_vk for the tables' variable count; commitments: [J, 18]"""
    from . import dist_primitive as dp

    comms = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 18)
    if failed_checks(len(comms), claims, proof, alpha, rho):
        return False
    rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(-1, 4)
    claims = _norm_claims(claims, len(comms), len(rho))
    _, y = chain_value(proof, claims, alpha, rho)
    cg = combined_commitment(be, comms, claims, alpha, rho)
    ok = dp.verify_batch(be, vk, cg.reshape(1, 18), fr_mont(y).reshape(1, 4), np.asarray(proof["opening"], dtype=np.uint64).reshape(1, len(rho), 18),
                         rho.reshape(1, len(rho), 4))
    return bool(np.all(ok))


def opening_claim(commitments, claims, proof: dict, alpha, rho):
    """what batch_open_verify hands to the pairing, without calling the device: the opening of sum_j e_j C_j at rho with the chain's
    value y -> (C [J, 18], e [J, 4] Montgomery, y [4] Montgomery, opening [n, 18], rho [n, 4]), the form of one opening of
    dist_primitive.verify_agg.  None when the chain breaks (failed_checks is not empty)"""
    comms = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 18)
    if failed_checks(len(comms), claims, proof, alpha, rho):
        return None
    rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(-1, 4)
    claims = _norm_claims(claims, len(comms), len(rho))
    _, y = chain_value(proof, claims, alpha, rho)
    e = eq_coefficients(len(comms), claims, alpha, rho)
    return comms, np.stack([fr_mont(x) for x in e]), fr_mont(y), np.asarray(proof["opening"], dtype=np.uint64).reshape(len(rho), 18), rho


def proof_digest(proof: dict) -> str:
    """SHA-256 over the record's little-endian words: rounds | opening"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(proof["rounds"], dtype="<u8").tobytes())
    h.update(np.ascontiguousarray(proof["opening"], dtype="<u8").tobytes())
    return h.hexdigest()


INSTANCE_SEED = 0x0BA70000  # stream k of seed S is SplitMix64(INSTANCE_SEED + 1000 S + k)


def random_instance(be, n: int, n_tables: int, n_claims: int, seed: int):
    """
    One instance per seed, the same in both hosts: table j = 2^n elements of stream 10 + j; claim k is on table k mod J at a point
    that is random (stream 100 + k) for k % 3 == 0, the point of claim k - 1 for k % 3 == 1, and boolean for k % 3 == 2 (coordinate i
    = bit ((k + i) & 1), the last claim's point being (1,..,1,0)); alpha: stream 1, rho: stream 2, the SRS trapdoor s: stream 3.
    The values v_k are not set here: the caller evaluates them (open_many or zk_fold).
    -> (tables, [(j, point)], alpha [4], rho [n, 4], s [n, 4])
    """
    from .field import splitmix_fr

    base = INSTANCE_SEED + 1000 * seed
    tables = [be.to_device(splitmix_fr(1 << n, base + 10 + j)) for j in range(n_tables)]
    zero, one = np.zeros(4, dtype=np.uint64), fr_mont(1)
    pts = []
    for k in range(n_claims):
        if k % 3 == 0:
            z = splitmix_fr(n, base + 100 + k)
        elif k % 3 == 1:
            z = pts[-1][1].copy()
        elif k == n_claims - 1:
            z = np.stack([one] * (n - 1) + [zero])
        else:
            z = np.stack([one if (k + i) & 1 else zero for i in range(n)])
        pts.append((k % n_tables, z))
    return tables, pts, splitmix_fr(1, base + 1)[0], splitmix_fr(n, base + 2), splitmix_fr(n, base + 3)


def evaluate_claims(be, tables, N: int, points) -> list:
    """[(j, z)] -> [(j, z, v)] with v = f_j(z) by zk_fold"""
    return [(j, z, be.fold(tables[j], N, z).download((1, 4))[0]) for j, z in points]


# ---- users: the gate ZeroCheck and the wiring PermCheck with their openings batched ----
def gate_zerocheck_prove_batched(be, pcs, tables: dict, tau, chal, alpha, rho, commitments: dict | None = None, timing: dict | None = None) -> dict:
    """
    gate_zerocheck_prove with the six openings at r = chal replaced by one batch instance (six claims at one point):
    -> {"rounds": [n, 5, 4], "commitments": [6, 18], "values": [6, 4] in the order of zerocheck.OPENED, "batch": batch record}
    """
    import time

    from . import dist_primitive as dp
    from . import zerocheck as zc

    tau = np.ascontiguousarray(tau, dtype=np.uint64).reshape(-1, 4)
    chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
    n = len(tau)
    if n < 1 or len(chal) != n:
        raise ValueError("tau and chal must hold one element per variable (n >= 1)")
    length = 1 << n
    t0 = time.perf_counter()
    eq = be.eq_table(tau)
    rounds, last = be.sumcheck_gate(eq, tables["q1"], tables["q2"], tables["a"], tables["b"], tables["c"], tables["in"], length, chal)
    t1 = time.perf_counter()
    at = {"q1": last[1], "q2": last[2], "a": last[3], "b": last[4], "c": last[5], "in": last[6]}  # the folded-out values ARE f(r)
    commitments = commitments or {}
    comms = np.stack([np.asarray(commitments[k] if k in commitments else dp.commit(be, pcs, tables[k], length), dtype=np.uint64).reshape(18) for k in zc.OPENED])
    t2 = time.perf_counter()
    values = np.stack([at[k] for k in zc.OPENED])
    claims = [(i, chal, values[i]) for i in range(len(zc.OPENED))]
    batch = batch_open_prove(be, pcs, [tables[k] for k in zc.OPENED], length, claims, alpha, rho)
    t3 = time.perf_counter()
    if timing is not None:
        timing["sumcheck_s"], timing["commit_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2
    return {"rounds": rounds, "commitments": comms, "values": values, "batch": batch}


def _as_gate_record(proof: dict) -> dict:
    return {"rounds": proof["rounds"], "openings": [(c, v, None) for c, v in zip(proof["commitments"], proof["values"])]}


def gate_zerocheck_verify_batched(be, vk, proof: dict, tau, chal, alpha, rho) -> bool:
    """the field checks of zerocheck.verify_rounds on the claimed values, then the batch instance that certifies them"""
    from . import zerocheck as zc

    try:
        values = np.asarray(proof["values"], dtype=np.uint64).reshape(len(zc.OPENED), 4)
        comms = np.asarray(proof["commitments"], dtype=np.uint64).reshape(len(zc.OPENED), 18)
        if not zc.verify_rounds(_as_gate_record(proof), tau, chal):
            return False
        claims = [(i, chal, values[i]) for i in range(len(zc.OPENED))]
        return batch_open_verify(be, vk, comms, claims, proof["batch"], alpha, rho)
    except (KeyError, ValueError, TypeError):
        return False


def wiring_prove_batched(be, pcs, w, sid, ssigma, N: int, alpha, beta, gamma, tau, chal, b_alpha, rho_mu, rho_mu1, commitments: dict | None = None,
                         timing: dict | None = None) -> dict:
    """
    wiring_prove with its eight openings replaced by two batch instances: w, sid, ssigma at r (mu variables) and the tree at the five
    V_POINTS (mu + 1 variables, J = 1, K = 5).  b_alpha: [4], rho_mu: [mu, 4], rho_mu1: [mu + 1, 4].
    -> {"rounds": [mu, 4, 4], "commitments": [3, 18], "values": [3, 4] (w, sid, ssigma), "v_commitment": [18], "v_values": [5, 4],
        "batch": record, "v_batch": record}
    """
    import time

    from . import dist_primitive as dp
    from . import wiring as wr

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
    rounds, _last = be.sumcheck_wiring(eq, tree, num, den, N, gamma, chal)
    t1 = time.perf_counter()
    commitments = commitments or {}
    tabs = {"w": w, "sid": sid, "ssigma": ssigma}
    comms = np.stack([np.asarray(commitments[k] if k in commitments else dp.commit(be, pcs, tabs[k], N), dtype=np.uint64).reshape(18) for k in wr.OPENED])
    v_comm = np.asarray(dp.commit(be, pcs, tree, 2 * N), dtype=np.uint64).reshape(18)
    t2 = time.perf_counter()
    claims = evaluate_claims(be, [tabs[k] for k in wr.OPENED], N, [(i, chal) for i in range(len(wr.OPENED))])
    v_claims = evaluate_claims(be, [tree], 2 * N, [(0, z) for z in wr.v_points(chal)])
    batch = batch_open_prove(be, pcs, [tabs[k] for k in wr.OPENED], N, claims, b_alpha, rho_mu)
    v_batch = batch_open_prove(be, pcs, [tree], 2 * N, v_claims, b_alpha, rho_mu1)
    t3 = time.perf_counter()
    if timing is not None:
        timing["sumcheck_s"], timing["commit_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2
    return {"rounds": rounds, "commitments": comms, "values": np.stack([c[2] for c in claims]), "v_commitment": v_comm,
            "v_values": np.stack([c[2] for c in v_claims]), "batch": batch, "v_batch": v_batch}


def wiring_verify_batched(be, vk_mu, vk_mu1, proof: dict, alpha, beta, gamma, tau, chal, b_alpha, rho_mu, rho_mu1) -> bool:
    """the field checks 1-3 of wiring.failed_checks on the claimed values, then the two batch instances (vk_mu, vk_mu1) that certify them"""
    from . import wiring as wr

    try:
        values = np.asarray(proof["values"], dtype=np.uint64).reshape(len(wr.OPENED), 4)
        v_values = np.asarray(proof["v_values"], dtype=np.uint64).reshape(len(wr.V_POINTS), 4)
        comms = np.asarray(proof["commitments"], dtype=np.uint64).reshape(len(wr.OPENED), 18)
        record = {"rounds": proof["rounds"], "openings": [(c, v, None) for c, v in zip(comms, values)], "v_openings": [(v, None) for v in v_values]}
        if wr.failed_checks(record, alpha, beta, gamma, tau, chal):
            return False
        chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
        claims = [(i, chal, values[i]) for i in range(len(wr.OPENED))]
        if not batch_open_verify(be, vk_mu, comms, claims, proof["batch"], b_alpha, rho_mu):
            return False
        v_claims = [(0, z, v) for z, v in zip(wr.v_points(chal), v_values)]
        return batch_open_verify(be, vk_mu1, np.asarray(proof["v_commitment"], dtype=np.uint64).reshape(1, 18), v_claims, proof["v_batch"], b_alpha, rho_mu1)
    except (KeyError, ValueError, TypeError):
        return False
