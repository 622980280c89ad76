"""
The lookup argument (LogUp) as a stand-alone non-interactive proof: every value of a column f lies in a table t.

N = 2^n rows; f and t hold N Fr each (pad the table by repeating an entry, pad f with any table entry).  The caller supplies the
row-to-table indices idx (u32[N], f[x] = t[idx[x]]); the multiplicities are m[y] = #{x : idx[x] = y} (zk_lookup_multiplicities, which
checks every row on the way).  A caller that only knows THAT its values lie in the table passes idx = FIND: the device finds the first
occurrence of every value itself (zk_lookup_find: idx and m in one call; `find_indices_host` is the same rule in numpy).  With a challenge beta

    df = beta + f,   dt = beta + t,   hf = 1 / df,   ht = m / dt
    sum_x 1 / (beta + f(x)) = sum_y m(y) / (beta + t(y))      <=>   f is contained in t          (N < char Fr)

and the sum together with the definitions of hf and ht is ONE degree-3 sumcheck over six tables (zk_sumcheck_lookup_fs):

    sum_x  hf(x) - ht(x)  +  E(x) [ hf(x) df(x) - 1  +  gamma ( ht(x) dt(x) - m(x) ) ]  =  0,        E = lambda eq(tau, .)

Schedule (label "lookup"):
    absorb n; absorb the commitment of t;
    absorb the commitments of f and m; beta <- challenge;
    absorb the commitments of hf and ht; gamma, lambda <- challenges; tau <- n challenges;
    per round absorb its four evaluations, r_i <- challenge;
    absorb the five claimed values f, t, m, hf, ht at r (the folded-out last values of the sumcheck: f(r) = df(r) - beta,
    t(r) = dt(r) - beta; no table is folded for a claim); b_alpha <- challenge;
    per round of the n-variate batch instance (five claims, one point) absorb (t0, t1, t2), rho_i <- challenge; the opening at rho.

Record: {"n", "commitments": [4, 18] (f, m, hf, ht), "rounds": [n, 4, 4], "values": [5, 4] (f, t, m, hf, ht), "batch": {"rounds":
[n, 3, 4], "opening": [n, 18]}}.  The verifier replays the schedule on hashlib (`challenges`), checks the field arithmetic
(`failed_checks`) and makes one zk_pcs_verify_batch call (`verify`).  Single party only.
"""
from __future__ import annotations

import hashlib

import numpy as np

from . import batch_open as bo
from .field import R_MOD, fr_from_mont, fr_mont, splitmix_fr
from .transcript import HostTranscript, Transcript
from .verify import _ints, _u64, eq_eval, round_chain

LABEL = b"lookup"
COMMITTED = ("f", "m", "hf", "ht")    # the prover's commitments of a record
OPENED = ("f", "t", "m", "hf", "ht")  # the five claimed values at r, and the tables of the batch instance
FIND = "find"                         # in the place of idx: the device finds the indices (zk_lookup_find)


def lookup_value(E: int, f: int, t: int, m: int, hf: int, ht: int, beta: int, gamma: int) -> int:
    """hf - ht + E [ hf (beta + f) - 1 + gamma ( ht (beta + t) - m ) ]"""
    return (hf - ht + E * (hf * (beta + f) - 1 + gamma * (ht * (beta + t) - m))) % R_MOD


def preprocess(be, pcs, t, powers_of_g2=None):
    """t: the table, a device buffer of N = 2^n Fr (or an [N, 4] array); pcs: the levels of a PolynomialCommitment over n variables;
    powers_of_g2 (optional): the SRS's [g2, s_0 g2, .., s_{n-1} g2], from which the pairing key of `verify` is made.
    -> (pk, vk): vk = {"n", "commitment": [18], "pcs": the pairing key or None}; pk keeps the device table."""
    from . import dist_primitive as dp

    if isinstance(t, np.ndarray):
        t = be.to_device(_u64(t, -1, 4))
    N = t.nbytes // 32
    n = N.bit_length() - 1
    if n < 1 or N != 1 << n:
        raise ValueError("the table must hold 2^n elements, n >= 1")
    comm = _u64(dp.commit(be, pcs, t, N), 18)
    vk = {"n": n, "commitment": comm, "pcs": dp.pcs_vk(be, powers_of_g2) if powers_of_g2 is not None else None}
    return {"n": n, "t": t, "commitment": comm, "pcs": pcs}, vk


def prove(be, pk: dict, f, idx, timing: dict | None = None) -> dict:
    """f: device buffer of N Fr (or an [N, 4] array); idx: N row-to-table indices (array or device buffer of u32), or FIND: the device finds
    the first occurrence of every value (the record is the one of prove with those indices) -> the record of the module text.  A row whose
    value is not the table entry it names -- with FIND: no entry at all -- raises ValueError, as does any other string; a zero denominator
    ZeroDivisionError (ZK_ERR_DIV_ZERO).  timing (optional dict) receives the wall seconds of the phases."""
    import time

    from . import dist_primitive as dp
    from .nizk import _batch_prove

    n, t, pcs = pk["n"], pk["t"], pk["pcs"]
    N = 1 << n
    if isinstance(idx, str) and idx != FIND:
        raise ValueError(f"idx must be the indices or FIND, not {idx!r}")
    if isinstance(f, np.ndarray):
        f = be.to_device(_u64(f, N, 4))
    if isinstance(idx, np.ndarray):
        idx = be.to_device(np.ascontiguousarray(idx, dtype=np.uint32).reshape(N))
    t0 = time.perf_counter()
    m = be.lookup_find(f, t, N)[1] if isinstance(idx, str) else be.lookup_multiplicities(f, t, idx, N)
    tr = Transcript(be, LABEL)
    try:
        tr.absorb_u64(n).absorb(pk["commitment"])
        c_f, c_m = (_u64(dp.commit(be, pcs, x, N), 18) for x in (f, m))
        beta = tr.absorb(np.stack([c_f, c_m])).challenge()
        zero = be.fr_sub(f, f, N)
        none = np.zeros(4, dtype=np.uint64)
        df, dt = be.fr_axpb(f, zero, none, beta, N), be.fr_axpb(t, zero, none, beta, N)
        hf = be.fr_batch_div(be.fr_axpb(zero, zero, none, fr_mont(1), N), df, N)
        ht = be.fr_batch_div(m, dt, N)
        c_hf, c_ht = (_u64(dp.commit(be, pcs, x, N), 18) for x in (hf, ht))
        t1 = time.perf_counter()
        gamma, lam = tr.absorb(np.stack([c_hf, c_ht])).challenges(2)
        tau = tr.challenges(n)
        E = be.eq_table_acc(tau, lam, zero)
        rounds, last, chal = be.sumcheck_lookup_fs([E, df, dt, m, hf, ht], N, gamma, tr)
        t2 = time.perf_counter()
        b = fr_from_mont(beta)
        values = np.stack([fr_mont((fr_from_mont(last[1]) - b) % R_MOD), fr_mont((fr_from_mont(last[2]) - b) % R_MOD), last[3], last[4], last[5]])
        b_alpha = tr.absorb(values).challenge()
        claims = [(j, chal, values[j]) for j in range(len(OPENED))]
        batch, _rho = _batch_prove(be, pcs, [f, t, m, hf, ht], N, claims, b_alpha, tr)
    finally:
        tr.free()
    t3 = time.perf_counter()
    if timing is not None:
        timing["commit_s"], timing["sumcheck_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2
    return {"n": n, "commitments": np.stack([c_f, c_m, c_hf, c_ht]), "rounds": rounds, "values": values, "batch": batch}


def challenges(vk: dict, proof: dict, label: bytes = LABEL) -> dict:
    """the verifier's replay of the schedule on hashlib -> {"beta", "gamma", "lambda", "tau", "chal", "b_alpha", "rho"}; ValueError / KeyError
    on a malformed record"""
    n = int(proof["n"])
    rounds = _u64(proof["rounds"], -1, 4, 4)
    b_rounds = _u64(proof["batch"]["rounds"], -1, 3, 4)
    if n < 1 or n != int(vk["n"]) or len(rounds) != n or len(b_rounds) != n:
        raise ValueError("the record does not hold n rounds")
    comms = _u64(proof["commitments"], len(COMMITTED), 18)
    tr = HostTranscript(label)
    tr.absorb_u64(n).absorb(_u64(vk["commitment"], 18))
    beta = tr.absorb(comms[:2]).challenge()
    gamma, lam = tr.absorb(comms[2:]).challenges(2)
    tau = tr.challenges(n)
    chal = np.stack([tr.absorb(r).challenge() for r in rounds])
    b_alpha = tr.absorb(_u64(proof["values"], len(OPENED), 4)).challenge()
    rho = np.stack([tr.absorb(r).challenge() for r in b_rounds])
    return {"beta": beta, "gamma": gamma, "lambda": lam, "tau": tau, "chal": chal, "b_alpha": b_alpha, "rho": rho}


def _claims(c: dict, proof: dict) -> list:
    values = _u64(proof["values"], len(OPENED), 4)
    return [(j, c["chal"], values[j]) for j in range(len(OPENED))]


def failed_checks(vk: dict, proof: dict, finals=None, c: dict | None = None) -> list:
    """
    The verifier's field arithmetic (no GPU, no pairing) -> [] when all checks hold, [0] for a malformed record, else [k], the FIRST check
    that fails -- the checks follow the transcript, and whatever breaks one also changes every challenge drawn after it, so the later ones
    say nothing more:
      1. p_0(0) + p_0(1) == 0 and p_i(0) + p_i(1) == p_{i-1}(r_{i-1}), by interpolation on the nodes 0 .. 3;
      2. p_{n-1}(r_{n-1}) == hf - ht + lambda eq(tau, r) [ hf (beta + f) - 1 + gamma ( ht (beta + t) - m ) ] on the claimed values;
      3. the round chain of the batch instance (batch_open.failed_checks; with `finals` = the five f_j(rho), tests that hold the
         tables, also its last value).
    """
    try:
        c = c or challenges(vk, proof)
        rounds = _u64(proof["rounds"], -1, 4, 4)
        f, t, m, hf, ht = _ints(_u64(proof["values"], len(OPENED), 4))
        if np.asarray(proof["batch"]["opening"], dtype=np.uint64).size != len(rounds) * 18:
            return [0]
    except (KeyError, ValueError, TypeError):
        return [0]
    ch = _ints(c["chal"])
    beta, gamma, lam = (_ints(c[k])[0] for k in ("beta", "gamma", "lambda"))
    target = round_chain(rounds, ch)
    if target is None:
        return [1]
    if target != lookup_value(lam * eq_eval(_ints(c["tau"]), ch) % R_MOD, f, t, m, hf, ht, beta, gamma):
        return [2]
    if bo.failed_checks(len(OPENED), _claims(c, proof), proof["batch"], c["b_alpha"], c["rho"], finals):
        return [3]
    return []


def field_checks(vk: dict, proof: dict, finals=None) -> bool:
    """everything of `verify` but the pairing (no GPU)"""
    return not failed_checks(vk, proof, finals)


def verify(be, vk: dict, proof: dict) -> bool:
    """the replay, checks 1-3, and ONE zk_pcs_verify_batch call: the opening of sum_j e_j C_j at rho (vk from `preprocess` with powers_of_g2)"""
    if vk.get("pcs") is None:
        raise ValueError("the verifying key holds no pairing key: preprocess(..., powers_of_g2=...)")
    try:
        c = challenges(vk, proof)
    except (KeyError, ValueError, TypeError):
        return False
    if failed_checks(vk, proof, c=c):
        return False
    comms = _u64(proof["commitments"], len(COMMITTED), 18)
    all5 = np.stack([comms[0], _u64(vk["commitment"], 18), comms[1], comms[2], comms[3]])  # OPENED order
    from ._lib import ZK_ERR_INVALID
    from .api import ZkError

    try:
        return bo.batch_open_verify(be, vk["pcs"], all5, _claims(c, proof), proof["batch"], c["b_alpha"], c["rho"])
    except ZkError as e:  # a point of the record that is not on the curve is refused by the pairing call: a record to reject
        if e.code != ZK_ERR_INVALID:
            raise
        return False


def proof_digest(proof: dict) -> str:
    """SHA-256 over the record's little-endian words in the order of the schedule"""
    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(proof["n"]).to_bytes(8, "little"))
    put(proof["commitments"]), put(proof["rounds"]), put(proof["values"])
    put(proof["batch"]["rounds"]), put(proof["batch"]["opening"])
    return h.hexdigest()


def find_indices_host(t, f, qk=None) -> np.ndarray:
    """numpy only -- the rule of zk_lookup_find / zk_lookup3_find on the host, for callers without a device: idx[x] = the smallest y with
    t[y] = f[x].  t, f: [N, 4] arrays of one column, or sequences of columns ([N, 4] each: (t0, t1, t2) and (a, b, c)).  qk ([N, 4], optional):
    rows with qk = 0 get 0 and are not looked up; a qk that is neither 0 nor the Montgomery form of 1 is a bad row.  A dictionary of first
    occurrences.  ValueError, in the wording of the device ("K of N rows ...", the first such row named), when rows are missing from the table
    or bad.  -> u32[N]"""
    cols = lambda a: [_u64(a, -1, 4)] if isinstance(a, np.ndarray) and a.ndim == 2 else [_u64(c, -1, 4) for c in a]
    keys = lambda cs: np.ascontiguousarray(np.concatenate(cs, axis=1), dtype="<u8")
    tk, fk = keys(cols(t)), keys(cols(f))
    N = len(tk)
    if len(fk) != N or tk.shape[1] != fk.shape[1]:
        raise ValueError("the rows and the table must have the same shape")
    first = {}
    for y in range(N):
        first.setdefault(tk[y].tobytes(), y)
    if qk is None:
        sel, bad = np.ones(N, dtype=bool), []
    else:
        q = _u64(qk, N, 4)
        zero, one = (q == 0).all(axis=1), (q == fr_mont(1)).all(axis=1)
        sel, bad = one, np.flatnonzero(~(zero | one)).tolist()
    idx = np.zeros(N, dtype=np.uint32)
    for x in np.flatnonzero(sel).tolist():
        y = first.get(fk[x].tobytes())
        if y is None:
            bad.append(x)
        else:
            idx[x] = y
    if bad:
        raise ValueError(f"find_indices_host: {len(bad)} of {N} rows are not in the table; the first is row {min(bad)}")
    return idx


# ---- the sample both hosts prove (one seed = one digest) ----
SAMPLE_SEED = 0x10C00000  # stream k of seed S is SplitMix64(SAMPLE_SEED + 1000 S + k)


def sample_lookup(n: int, seed: int, distinct: int | None = None):
    """numpy only.  A table of `distinct` different entries (stream 10; default N / 2, at least 1) padded to N = 2^n by repeating the last
    one, and a column drawn from it: idx[x] = (limb 0 of element x of stream 11) mod distinct, f[x] = t[idx[x]].  The SRS trapdoor of
    the sample is stream 3 (n Fr).  -> (t [N, 4], f [N, 4], idx u32[N])"""
    N = 1 << n
    distinct = max(N // 2, 1) if distinct is None else int(distinct)
    if not 1 <= distinct <= N:
        raise ValueError("1 <= distinct <= N is needed")
    base = SAMPLE_SEED + 1000 * seed
    t = np.empty((N, 4), dtype=np.uint64)
    t[:distinct] = splitmix_fr(distinct, base + 10)
    t[distinct:] = t[distinct - 1]
    idx = (splitmix_fr(N, base + 11)[:, 0] % np.uint64(distinct)).astype(np.uint32)
    return t, t[idx], idx


def sample_srs(n: int, seed: int) -> np.ndarray:
    """the trapdoor of the sample's SRS: n Fr of stream 3"""
    return splitmix_fr(n, SAMPLE_SEED + 1000 * seed + 3)


def sample_digest(t, f, idx) -> str:
    """SHA-256 over t | f | idx (u32) little-endian: what `lookup_check --sample-only` prints"""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(t, dtype="<u8").tobytes()), h.update(np.ascontiguousarray(f, dtype="<u8").tobytes())
    h.update(np.ascontiguousarray(idx, dtype="<u4").tobytes())
    return h.hexdigest()
