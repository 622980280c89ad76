"""
Non-interactive gate ZeroCheck and wiring PermCheck: the batched arguments of zkhip.batch_open with EVERY challenge derived from a
Fiat-Shamir transcript (zkhip.transcript), so that no challenge is an argument of a prover or a verifier.

The prover keeps the transcript on the device: the three fused sumchecks draw round i's challenge from a hash of round i's
evaluations between their kernels (zk_sumcheck_gate_fs / _wiring_fs / _multi_fs: one enqueue, one synchronisation per sumcheck).
The verifier replays the schedule on hashlib (HostTranscript) from the record alone and then runs the EXISTING checks with the
derived challenges: zerocheck.verify_rounds / wiring.failed_checks, batch_open.failed_checks, one zk_pcs_verify_batch per instance.

Gate schedule (label "gate"):    absorb n; absorb the six commitments (zerocheck.OPENED order); tau <- n challenges;
    per round absorb its five evaluations, r_i <- challenge; absorb the six claimed values; alpha <- challenge;
    per round of the batch instance absorb (t0, t1, t2), rho_i <- challenge; the opening at rho.
Wiring schedule (label "wiring"): absorb mu; absorb the commitments of w, sid, ssigma; alpha, beta <- challenges; absorb the
    commitment of the product tree; gamma <- challenge; tau <- mu challenges; per round absorb its four evaluations, r_i <- challenge;
    absorb the three claimed values; absorb the five claimed tree values; b_alpha <- challenge; the rounds of the mu-variate batch
    instance give rho_mu, then those of the (mu + 1)-variate one give rho_mu1.

Records: those of gate_zerocheck_prove_batched / wiring_prove_batched with the variable count added ("n" / "mu").  Single party only.
"""
from __future__ import annotations

import hashlib

import numpy as np

from . import batch_open as bo
from . import wiring as wr
from . import zerocheck as zc
from .transcript import HostTranscript, Transcript
from .verify import _u64

GATE_LABEL, WIRING_LABEL = b"gate", b"wiring"


def _replay_rounds(tr, rounds: np.ndarray) -> np.ndarray:
    """absorb round i, draw challenge i -> [n, 4]"""
    return np.stack([tr.absorb(r).challenge() for r in rounds])


def _batch_prove(be, pcs, tables, N: int, claims, alpha, tr) -> tuple:
    """batch_open_prove with rho drawn from the transcript -> (record, rho)"""
    from . import dist_primitive as dp

    n = N.bit_length() - 1
    claims = bo._norm_claims(claims, len(tables), n)
    eqs = bo.combined_eq_tables(be, len(tables), n, claims, alpha)
    used = [j for j, e in enumerate(eqs) if e is not None]
    rounds, last_e, _last_f, rho = be.sumcheck_multi_fs([eqs[j] for j in used], [tables[j] for j in used], N, tr)
    g = be.fr_lincomb([tables[j] for j in used], last_e, N)
    _value, opening = dp.open_(be, pcs, g, N, rho)
    return {"rounds": rounds, "opening": _u64(opening, n, 18)}, rho


# ---- gate ----
def gate_challenges(proof: dict, label: bytes = GATE_LABEL) -> dict:
    """the verifier's replay of the gate schedule on hashlib -> {"tau", "chal", "alpha", "rho"}; ValueError / KeyError on a malformed record"""
    n = int(proof["n"])
    rounds = _u64(proof["rounds"], -1, 5, 4)
    b_rounds = _u64(proof["batch"]["rounds"], -1, 3, 4)
    if n < 1 or len(rounds) != n or len(b_rounds) != n:
        raise ValueError("the record does not hold n rounds")
    tr = HostTranscript(label)
    tr.absorb_u64(n).absorb(_u64(proof["commitments"], len(zc.OPENED), 18))
    tau = tr.challenges(n)
    chal = _replay_rounds(tr, rounds)
    alpha = tr.absorb(_u64(proof["values"], len(zc.OPENED), 4)).challenge()
    return {"tau": tau, "chal": chal, "alpha": alpha, "rho": _replay_rounds(tr, b_rounds)}


def gate_prove_ni(be, pcs, tables: dict, commitments: dict | None = None, timing: dict | None = None) -> dict:
    """
    be: zkhip.Ctx; pcs: the levels of a PolynomialCommitment; tables: device buffers of 2^n Fr under "q1", "q2", "a", "b", "c", "in";
    commitments: name -> [18] for tables committed earlier.
    -> {"n", "rounds": [n, 5, 4], "commitments": [6, 18], "values": [6, 4], "batch": {"rounds": [n, 3, 4], "opening": [n, 18]}}
    timing (optional dict) receives the wall seconds of the commitments, the gate sumcheck (with tau and the eq table) and the opening.
    """
    import time

    from . import dist_primitive as dp

    length = tables["a"].nbytes // 32
    n = length.bit_length() - 1
    if n < 1 or length != 1 << n:
        raise ValueError("the tables must hold 2^n elements, n >= 1")
    t0 = time.perf_counter()
    commitments = commitments or {}
    comms = np.stack([_u64(commitments[k] if k in commitments else dp.commit(be, pcs, tables[k], length), 18) for k in zc.OPENED])
    t1 = time.perf_counter()
    tr = Transcript(be, GATE_LABEL)
    try:
        tr.absorb_u64(n).absorb(comms)
        tau = tr.challenges(n)
        eq = be.eq_table(tau)
        rounds, last, chal = be.sumcheck_gate_fs(eq, tables["q1"], tables["q2"], tables["a"], tables["b"], tables["c"], tables["in"], length, tr)
        t2 = time.perf_counter()
        at = {"q1": last[1], "q2": last[2], "a": last[3], "b": last[4], "c": last[5], "in": last[6]}  # the folded-out values ARE f(r)
        values = np.stack([at[k] for k in zc.OPENED])
        alpha = tr.absorb(values).challenge()
        claims = [(i, chal, values[i]) for i in range(len(zc.OPENED))]
        batch, _rho = _batch_prove(be, pcs, [tables[k] for k in zc.OPENED], length, claims, alpha, tr)
    finally:
        tr.free()
    t3 = time.perf_counter()
    if timing is not None:
        timing["commit_s"], timing["sumcheck_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2
    return {"n": n, "rounds": rounds, "commitments": comms, "values": values, "batch": batch}


def gate_field_checks_ni(proof: dict, label: bytes = GATE_LABEL, finals=None) -> bool:
    """everything of gate_verify_ni but the pairing: the replay, zerocheck.verify_rounds, batch_open.failed_checks (no GPU).  finals
    (tests that hold the tables): the six f_j(rho), which stand in for the pairing's check of the value the batch chain ends in"""
    try:
        c = gate_challenges(proof, label)
        values = _u64(proof["values"], len(zc.OPENED), 4)
        if not zc.verify_rounds(bo._as_gate_record(proof), c["tau"], c["chal"]):
            return False
        claims = [(i, c["chal"], values[i]) for i in range(len(zc.OPENED))]
        return not bo.failed_checks(len(zc.OPENED), claims, proof["batch"], c["alpha"], c["rho"], finals)
    except (KeyError, ValueError, TypeError):
        return False


def gate_verify_ni(be, vk, proof: dict) -> bool:
    """the replay, then gate_zerocheck_verify_batched with the derived challenges (vk: dist_primitive.pcs_vk of n variables)"""
    try:
        c = gate_challenges(proof)
    except (KeyError, ValueError, TypeError):
        return False
    return bo.gate_zerocheck_verify_batched(be, vk, proof, c["tau"], c["chal"], c["alpha"], c["rho"])


# ---- wiring ----
def wiring_challenges(proof: dict, label: bytes = WIRING_LABEL) -> dict:
    """the verifier's replay of the wiring schedule -> {"alpha", "beta", "gamma", "tau", "chal", "b_alpha", "rho_mu", "rho_mu1"}"""
    mu = int(proof["mu"])
    rounds = _u64(proof["rounds"], -1, 4, 4)
    b_rounds, v_rounds = _u64(proof["batch"]["rounds"], -1, 3, 4), _u64(proof["v_batch"]["rounds"], -1, 3, 4)
    if mu < 1 or len(rounds) != mu or len(b_rounds) != mu or len(v_rounds) != mu + 1:
        raise ValueError("the record does not hold mu / mu + 1 rounds")
    tr = HostTranscript(label)
    tr.absorb_u64(mu).absorb(_u64(proof["commitments"], len(wr.OPENED), 18))
    alpha, beta = tr.challenges(2)
    gamma = tr.absorb(_u64(proof["v_commitment"], 18)).challenge()
    tau = tr.challenges(mu)
    chal = _replay_rounds(tr, rounds)
    tr.absorb(_u64(proof["values"], len(wr.OPENED), 4)).absorb(_u64(proof["v_values"], len(wr.V_POINTS), 4))
    b_alpha = tr.challenge()
    rho_mu = _replay_rounds(tr, b_rounds)
    return {"alpha": alpha, "beta": beta, "gamma": gamma, "tau": tau, "chal": chal, "b_alpha": b_alpha, "rho_mu": rho_mu, "rho_mu1": _replay_rounds(tr, v_rounds)}


def wiring_prove_ni(be, pcs, w, sid, ssigma, N: int, commitments: dict | None = None, timing: dict | None = None) -> dict:
    """
    pcs: the levels of a PolynomialCommitment over mu + 1 variables; w, sid, ssigma: device buffers of N = 2^mu Fr.
    -> the record of wiring_prove_batched with "mu" added.  A zero denominator raises ZeroDivisionError (ZK_ERR_DIV_ZERO).
    """
    import time

    from . import dist_primitive as dp

    mu = N.bit_length() - 1
    if mu < 1 or N != 1 << mu:
        raise ValueError("N must be 2^mu, mu >= 1")
    t0 = time.perf_counter()
    commitments = commitments or {}
    tabs = {"w": w, "sid": sid, "ssigma": ssigma}
    comms = np.stack([_u64(commitments[k] if k in commitments else dp.commit(be, pcs, tabs[k], N), 18) for k in wr.OPENED])
    tr = Transcript(be, WIRING_LABEL)
    try:
        tr.absorb_u64(mu).absorb(comms)
        alpha, beta = tr.challenges(2)
        num = be.fr_axpb(w, sid, alpha, beta, N)
        den = be.fr_axpb(w, ssigma, alpha, beta, N)
        h = be.fr_batch_div(num, den, N)
        tree = be.product_tree(h, N)
        v_comm = _u64(dp.commit(be, pcs, tree, 2 * N), 18)
        t1 = time.perf_counter()
        gamma = tr.absorb(v_comm).challenge()
        tau = tr.challenges(mu)
        eq = be.eq_table(tau)
        rounds, _last, chal = be.sumcheck_wiring_fs(eq, tree, num, den, N, gamma, tr)
        t2 = time.perf_counter()
        claims = bo.evaluate_claims(be, [tabs[k] for k in wr.OPENED], N, [(i, chal) for i in range(len(wr.OPENED))])
        v_claims = bo.evaluate_claims(be, [tree], 2 * N, [(0, z) for z in wr.v_points(chal)])
        values, v_values = np.stack([c[2] for c in claims]), np.stack([c[2] for c in v_claims])
        b_alpha = tr.absorb(values).absorb(v_values).challenge()
        batch, _ = _batch_prove(be, pcs, [tabs[k] for k in wr.OPENED], N, claims, b_alpha, tr)
        v_batch, _ = _batch_prove(be, pcs, [tree], 2 * N, v_claims, b_alpha, tr)
    finally:
        tr.free()
    t3 = time.perf_counter()
    if timing is not None:
        timing["commit_s"], timing["sumcheck_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2
    return {"mu": mu, "rounds": rounds, "commitments": comms, "values": values, "v_commitment": v_comm, "v_values": v_values, "batch": batch, "v_batch": v_batch}


def wiring_field_checks_ni(proof: dict, label: bytes = WIRING_LABEL, finals=None, v_finals=None) -> bool:
    """everything of wiring_verify_ni but the pairings (no GPU); finals / v_finals as in gate_field_checks_ni: w, sid, ssigma at rho_mu,
    the tree at rho_mu1"""
    try:
        c = wiring_challenges(proof, label)
        values, v_values = _u64(proof["values"], len(wr.OPENED), 4), _u64(proof["v_values"], len(wr.V_POINTS), 4)
        record = {"rounds": proof["rounds"], "openings": [(None, v, None) for v in values], "v_openings": [(v, None) for v in v_values]}
        if wr.failed_checks(record, c["alpha"], c["beta"], c["gamma"], c["tau"], c["chal"]):
            return False
        claims = [(i, c["chal"], values[i]) for i in range(len(wr.OPENED))]
        if bo.failed_checks(len(wr.OPENED), claims, proof["batch"], c["b_alpha"], c["rho_mu"], finals):
            return False
        v_claims = [(0, z, v) for z, v in zip(wr.v_points(c["chal"]), v_values)]
        return not bo.failed_checks(1, v_claims, proof["v_batch"], c["b_alpha"], c["rho_mu1"], v_finals)
    except (KeyError, ValueError, TypeError):
        return False


def wiring_verify_ni(be, vk_mu, vk_mu1, proof: dict) -> bool:
    """the replay, then wiring_verify_batched with the derived challenges (vk_mu, vk_mu1: wiring.verifying_keys)"""
    try:
        c = wiring_challenges(proof)
    except (KeyError, ValueError, TypeError):
        return False
    return bo.wiring_verify_batched(be, vk_mu, vk_mu1, proof, c["alpha"], c["beta"], c["gamma"], c["tau"], c["chal"], c["b_alpha"], c["rho_mu"], c["rho_mu1"])


def proof_digest(proof: dict) -> str:
    """SHA-256 over the record's little-endian words in the order of the schedule (either kind of record)"""
    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(proof["n"] if "n" in proof else proof["mu"]).to_bytes(8, "little"))
    put(proof["commitments"])
    if "v_commitment" in proof:
        put(proof["v_commitment"])
    put(proof["rounds"]), put(proof["values"])
    if "v_values" in proof:
        put(proof["v_values"])
    for b in ("batch", "v_batch"):
        if b in proof:
            put(proof[b]["rounds"]), put(proof[b]["opening"])
    return h.hexdigest()
