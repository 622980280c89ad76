"""
The gate identity as a ZeroCheck a verifier can check end to end.

The reference (and `hyperplonk.py` after it) SIMULATES the gate check with six independent product sumchecks on a random `eq`
vector (hyperplonk/src/hyperplonk.rs:66-93, dhyperplonk.rs:218-260).  Here it is the real thing:

    sum_x eq(tau, x) [ q1(x) (a(x) + b(x)) + q2(x) a(x) b(x) - c(x) + in(x) ] = 0

proved by one degree-4 sumcheck (zk_eq_table, zk_sumcheck_gate), closed by openings of a, b, c, in, q1, q2 at the sumcheck
point through the existing commit / open path, and verified with one batched pairing check (zk_pcs_verify_batch).

`tau` and the challenges are INPUTS of the functions here (the reference pre-samples every challenge, dhyperplonk.rs:103-109).
The non-interactive form, with every challenge derived from a Fiat-Shamir transcript that lives on the device, is
zkhip.nizk.gate_prove_ni / gate_verify_ni.  Single party only: the distributed and packed-share forms are not defined.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .field import R_MOD, fr_from_mont
from .verify import _ints, eq_eval, round_chain, round_poly_at  # noqa: F401  (the shared verifier pieces, importable from here as before)

OPENED = ("a", "b", "c", "in", "q1", "q2")  # order of the six openings in a proof record


def gate_value(eq: int, q1: int, q2: int, a: int, b: int, c: int, inp: int) -> int:
    return eq * (q1 * (a + b) + q2 * a * b - c + inp) % R_MOD


def wide_gate_value(eq: int, qL: int, qR: int, qM: int, qO: int, qC: int, qH: int, a: int, b: int, c: int, inp: int) -> int:
    """the wide Plonk gate (zk_sumcheck_gate_wide) at one point, on python ints"""
    return eq * (qL * a + qR * b + qM * a * b + qH * pow(a, 5, R_MOD) - qO * c + qC + inp) % R_MOD


def verify_rounds(proof: dict, tau, chal) -> bool:
    """
    The verifier's field arithmetic (no GPU, no pairing):
      1. p_0(0) + p_0(1) == 0;
      2. p_i(0) + p_i(1) == p_{i-1}(r_{i-1}) for every later round;
      3. p_{n-1}(r_{n-1}) == eq(tau, r) [q1(r) (a(r) + b(r)) + q2(r) a(r) b(r) - c(r) + in(r)] from the six opened values.
    proof: the record of gate_zerocheck_prove; tau, chal: [n, 4] Montgomery Fr.
    """
    rounds = np.asarray(proof["rounds"], dtype=np.uint64).reshape(-1, 5, 4)
    tau_i, ch = _ints(tau), _ints(chal)
    n = len(rounds)
    if n == 0 or len(tau_i) != n or len(ch) != n or len(proof["openings"]) != len(OPENED):
        return False
    target = round_chain(rounds, ch)
    if target is None:
        return False
    val = {name: fr_from_mont(np.asarray(op[1], dtype=np.uint64).reshape(4)) for name, op in zip(OPENED, proof["openings"])}
    return target == gate_value(eq_eval(tau_i, ch), val["q1"], val["q2"], val["a"], val["b"], val["c"], val["in"])


def gate_zerocheck_prove(be, pcs, tables: dict, tau, chal, commitments: dict | None = None, timing: dict | None = None) -> dict:
    """
    be: zkhip.Ctx; pcs: the levels of a PolynomialCommitment (`cub.mature()`); tables: device buffers of 2^n Fr under the keys
    "q1", "q2", "a", "b", "c", "in"; tau, chal: [n, 4] Montgomery Fr; commitments: name -> [18] for tables committed earlier.
    -> {"rounds": [n, 5, 4], "openings": [(commitment [18], value [4], opening proof [n, 18])] in the order of OPENED}.
    timing (optional dict) receives the wall seconds of the eq table and of the sumcheck.
    """
    import time

    from . import dist_primitive as dp

    tau = np.ascontiguousarray(tau, dtype=np.uint64).reshape(-1, 4)
    chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
    n = len(tau)
    if n < 1 or len(chal) != n:
        raise ValueError("tau and chal must hold one element per variable (n >= 1)")
    length = 1 << n
    t0 = time.perf_counter()
    eq = be.eq_table(tau)
    be.sync()
    t1 = time.perf_counter()
    rounds, _last = be.sumcheck_gate(eq, tables["q1"], tables["q2"], tables["a"], tables["b"], tables["c"], tables["in"], length, chal)
    t2 = time.perf_counter()
    if timing is not None:
        timing["eq_table_s"], timing["sumcheck_s"] = t1 - t0, t2 - t1
    commitments = commitments or {}
    comms = [np.asarray(commitments[k] if k in commitments else dp.commit(be, pcs, tables[k], length), dtype=np.uint64).reshape(18) for k in OPENED]
    opens = dp.open_many(be, pcs, [tables[k] for k in OPENED], [length] * len(OPENED), [chal] * len(OPENED))
    return {"rounds": rounds,
            "openings": [(c, np.asarray(v, dtype=np.uint64).reshape(4), np.asarray(pf, dtype=np.uint64).reshape(n, 18)) for c, (v, pf) in zip(comms, opens)]}


def gate_zerocheck_verify(be, vk, proof: dict, tau, chal) -> bool:
    """verify_rounds, then the six openings at r = chal in ONE zk_pcs_verify_batch call (vk: dist_primitive.pcs_vk)"""
    from . import dist_primitive as dp

    if not verify_rounds(proof, tau, chal):
        return False
    chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
    ops = proof["openings"]
    ok = dp.verify_batch(be, vk, np.stack([np.asarray(o[0], dtype=np.uint64).reshape(18) for o in ops]),
                         np.stack([np.asarray(o[1], dtype=np.uint64).reshape(4) for o in ops]),
                         np.stack([np.asarray(o[2], dtype=np.uint64).reshape(len(chal), 18) for o in ops]),
                         np.stack([chal] * len(ops)))
    return bool(np.all(ok))


def gate_zerocheck_prove_batched(be, pcs, tables: dict, tau, chal, alpha, rho, commitments: dict | None = None, timing: dict | None = None) -> dict:
    """gate_zerocheck_prove with ONE opening proof: the six openings at r become six claims of one batch instance with weight base alpha
    and challenges rho (zkhip.batch_open, where the record is described)"""
    from .batch_open import gate_zerocheck_prove_batched as impl

    return impl(be, pcs, tables, tau, chal, alpha, rho, commitments, timing)


def gate_zerocheck_verify_batched(be, vk, proof: dict, tau, chal, alpha, rho) -> bool:
    """verify_rounds on the claimed values, then the batch instance that certifies them: one zk_pcs_verify_batch call of one opening"""
    from .batch_open import gate_zerocheck_verify_batched as impl

    return impl(be, vk, proof, tau, chal, alpha, rho)


def proof_digest(proof: dict) -> str:
    """SHA-256 over the record's little-endian words: rounds, then per opening commitment | value | opening proof"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(proof["rounds"], dtype="<u8").tobytes())
    for c, v, pf in proof["openings"]:
        for part in (c, v, pf):
            h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    return h.hexdigest()


CIRCUIT_SEED = 0x6A7E0000  # table k of seed S comes from SplitMix64(CIRCUIT_SEED + 1000 S + k)


def satisfied_circuit(be, n: int, seed: int, break_gate: int | None = None):
    """
    A satisfied circuit on the device, the same in both hosts (host/examples/gate_check.cpp): a, b, q1, q2, in = 2^n uniform
    elements each from SplitMix64(CIRCUIT_SEED + 1000 seed + 1 .. 5) (field.splitmix_fr), c = q1 (a + b) + q2 a b + in by the
    element-wise kernels; break_gate K adds 1 to c[K].  tau, chal and the SRS trapdoor s: n elements from streams 6, 7, 8.
    -> (tables dict of device buffers, tau [n, 4], chal [n, 4], s [n, 4])
    """
    from .field import fr_mont, splitmix_fr

    m, base = 1 << n, CIRCUIT_SEED + 1000 * seed
    t = {k: be.to_device(splitmix_fr(m, base + 1 + i)) for i, k in enumerate(("a", "b", "q1", "q2", "in"))}
    lin = be.fr_mul(t["q1"], be.fr_add(t["a"], t["b"], m), m)
    t["c"] = be.fr_add(be.fr_add(lin, be.fr_mul(be.fr_mul(t["q2"], t["a"], m), t["b"], m), m), t["in"], m)
    if break_gate is not None:
        v = fr_from_mont(t["c"].download((1, 4), offset=32 * break_gate)[0])
        t["c"].upload(fr_mont(v + 1).reshape(1, 4), offset=32 * break_gate)
    return t, splitmix_fr(n, base + 6), splitmix_fr(n, base + 7), splitmix_fr(n, base + 8)
