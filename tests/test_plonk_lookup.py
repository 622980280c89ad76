"""
Plonk with lookups without a GPU: the big-int model (plonk_lookup_model.py) against closed forms, the test-circuit generator row by row,
zkhip.plonk.challenges / failed_checks on the model prover's records of both gate kinds, the unmoved digests of records without a lookup,
and the presence of the new entry points in the built library, the header and the Rust binding.
"""
import ctypes
import os

import numpy as np
import pytest

import lookup_model as lm
import plonk_lookup_model as plm
import plonk_model as pm
import pyoracle as po
import widegate_model as wg
import zerocheck_model as zm

R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_lookup3_multiplicities", "zk_lookup3_terms", "zk_sumcheck_lookup_sel", "zk_sumcheck_lookup_sel_fs")
_RECORDS = {}


def _record(mu, gate, **kw):
    key = (mu, gate, tuple(sorted(kw.items())))
    if key not in _RECORDS:
        _RECORDS[key] = plm.model_record(mu, 5, gate=gate, **kw)
    return _RECORDS[key]


def _flip(a, idx):
    a = np.array(a, dtype=np.uint64, copy=True)
    a.reshape(-1)[idx] ^= np.uint64(1)
    return a


# ---- the model against closed forms ----
@pytest.mark.parametrize("n", range(1, 7))
def test_model_chain_degree_and_last_values(n):
    tabs = plm.random_tables(n, 300 + n)
    gamma, chal = po.SplitMix64(400 + n).fr_vec(1)[0], po.SplitMix64(500 + n).fr_vec(n)
    rounds, last = plm.sumcheck_lookup_sel(tabs, gamma, chal, evals=5)
    target = sum(plm.L(*[tabs[k][x] for k in plm.TABLES], gamma) for x in range(1 << n)) % R
    for p, r in zip(rounds, chal):
        assert (p[0] + p[1]) % R == target
        assert pm.interpolate(p[:4], 4) == p[4]  # degree 3
        assert pm.interpolate(p[:3], 3) != p[3]  # and no lower (random tables)
        target = pm.interpolate(p[:4], r)
    assert last == [po.fix_variable(tabs[k], chal)[0] for k in plm.TABLES]
    assert target == plm.L(*last, gamma)


@pytest.mark.parametrize("n", [1, 4])
def test_model_with_qk_one_is_the_parent_model(n):
    tabs = plm.random_tables(n, 310 + n)
    tabs["qk"] = [1] * (1 << n)
    gamma, chal = po.SplitMix64(410 + n).fr_vec(1)[0], po.SplitMix64(510 + n).fr_vec(n)
    rounds, last = plm.sumcheck_lookup_sel(tabs, gamma, chal)
    assert (rounds, last[:6]) == lm.sumcheck_lookup(tabs, gamma, chal) and last[6] == 1


def test_multiplicities3_and_the_sum_identity():
    """on a satisfied sample the seven tables sum to zero and every bracket vanishes; the refusals count their rows"""
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(4, 3)
    t = pm.circuit_ints(c)
    lk, idx = plm.lookup_ints(c)
    w, tt = [t["a"], t["b"], t["c"]], [lk["t0"], lk["t1"], lk["t2"]]
    m = plm.multiplicities3(w, tt, lk["qk"], idx)
    assert sum(m) == sum(lk["qk"]) > 0
    zeta, beta, lam, gamma = po.SplitMix64(77).fr_vec(4)
    tabs = plm.tables(w, tt, lk["qk"], m, zeta, beta, lam, po.SplitMix64(78).fr_vec(4))
    assert sum(plm.L(*[tabs[k][x] for k in plm.TABLES], gamma) for x in range(16)) % R == 0
    assert all((tabs["hf"][x] * tabs["df"][x] - tabs["qk"][x]) % R == 0 and (tabs["ht"][x] * tabs["dt"][x] - tabs["m"][x]) % R == 0 for x in range(16))
    x = lk["qk"].index(1)
    with pytest.raises(ValueError, match="1 of 16 rows"):
        plm.multiplicities3(w, tt, lk["qk"], idx[:x] + [16] + idx[x + 1:])
    with pytest.raises(ValueError, match="1 of 16 rows"):
        plm.multiplicities3(w, tt, lk["qk"][:x] + [2] + lk["qk"][x + 1:], idx)
    with pytest.raises(ValueError, match="1 of 16 rows"):
        plm.multiplicities3([t["a"], t["b"], [(v + (i == x)) % R for i, v in enumerate(t["c"])]], tt, lk["qk"], idx)
    skipped = [2**32 - 1 if q == 0 else i for q, i in zip(lk["qk"], idx)]  # the index of an unselected row is never read through
    assert plm.multiplicities3(w, tt, lk["qk"], skipped) == m


def test_lookup3_value_reduces_to_the_one_column_form():
    from zkhip import lookup as lk
    from zkhip import plonk

    E, a, b, c, t0, t1, t2, m, hf, ht, beta, gamma = po.SplitMix64(9).fr_vec(12)
    assert plonk.lookup3_value(E, a, b, c, 1, t0, t1, t2, m, hf, ht, 0, beta, gamma) == lk.lookup_value(E, a, t0, m, hf, ht, beta, gamma)
    zeta, qk = po.SplitMix64(10).fr_vec(2)
    df, dt = (beta + a + zeta * b + zeta * zeta * c) % R, (beta + t0 + zeta * t1 + zeta * zeta * t2) % R
    assert plonk.lookup3_value(E, a, b, c, qk, t0, t1, t2, m, hf, ht, zeta, beta, gamma) == plm.L(E, df, dt, m, hf, ht, qk, gamma)


# ---- the generator ----
def _broken_cycles(t, N):
    sigma = t["s0"] + t["s1"] + t["s2"]
    vals = t["a"] + t["b"] + t["c"]
    seen, bad = [False] * (3 * N), 0
    for s in range(3 * N):
        if not seen[s]:
            cyc, x = [], s
            while not seen[x]:
                seen[x] = True
                cyc.append(vals[x])
                x = sigma[x]
            bad += len(set(cyc)) > 1
    return bad


def _gate_rows(t, N, gate):
    if gate == "wide":
        return wg.row_values(t, N)
    inp = pm.in_table(t["pi"], N)
    return [zm.gate(1, t["q1"][x], t["q2"][x], t["a"][x], t["b"][x], t["c"][x], inp[x]) for x in range(N)]


@pytest.mark.parametrize("gate", [None, "wide"])
@pytest.mark.parametrize("mu", range(3, 8))
def test_generator(mu, gate):
    from zkhip import plonk

    seed = 3
    c = plonk.sample_circuit_lookup(mu, seed, gate=gate)
    N, l, D = 1 << mu, c["l"], (1 << mu) // 4
    t = (wg if gate == "wide" else pm).circuit_ints(c)
    lk, idx = plm.lookup_ints(c)
    assert c.get("gate") == gate and sorted(t["s0"] + t["s1"] + t["s2"]) == list(range(3 * N))
    assert not any(_gate_rows(t, N, gate))  # every row satisfies its gate
    assert _broken_cycles(t, N) == 0        # every cycle of sigma carries one value
    assert set(lk["qk"]) <= {0, 1} and not any(lk["qk"][:l])
    rows = [x for x in range(N) if lk["qk"][x]]
    assert rows, "no lookup rows"
    for x in rows:
        y = idx[x]
        assert y < D and (t["a"][x], t["b"][x], t["c"][x]) == (lk["t0"][y], lk["t1"][y], lk["t2"][y])
        assert t["s0"][x] == x and t["s1"][x] == N + x  # the a and b slots of a lookup row are fixed points
    assert all(lk["t2"][y] == lk["t0"][y] * lk["t1"][y] % R for y in range(N))
    assert all((lk["t0"][y], lk["t1"][y]) == (lk["t0"][D - 1], lk["t1"][D - 1]) for y in range(D, N))  # padded by repeating the last entry
    assert all(i == 0 for x, i in enumerate(idx) if not lk["qk"][x])
    m = plm.multiplicities3([t["a"], t["b"], t["c"]], [lk["t0"], lk["t1"], lk["t2"]], lk["qk"], idx)
    if mu == 5:
        assert max(m) > 1
    # the table does not depend on the witness or the gate kind, the lookup rows are those of the other kind
    other = plonk.sample_circuit_lookup(mu, seed, gate="wide" if gate is None else None)
    assert all((other["lookup"][k] == c["lookup"][k]).all() for k in ("qk", "t0", "t1", "t2")) and (other["idx"] == c["idx"]).all()
    # break_lookup: gate and wiring still hold, the triple is outside the table
    K = rows[-1]
    bc = plonk.sample_circuit_lookup(mu, seed, gate=gate, break_lookup=K)
    bt = (wg if gate == "wide" else pm).circuit_ints(bc)
    assert not any(_gate_rows(bt, N, gate)) and _broken_cycles(bt, N) == 0
    assert bt["a"][K] == (t["a"][K] + 1) % R and bt["c"][K] == bt["a"][K] * bt["b"][K] % R
    with pytest.raises(ValueError, match="1 of %d rows" % N):
        plm.multiplicities3([bt["a"], bt["b"], bt["c"]], [lk["t0"], lk["t1"], lk["t2"]], lk["qk"], idx)
    with pytest.raises(ValueError):
        plonk.sample_circuit_lookup(mu, seed, gate=gate, break_lookup=0)
    with pytest.raises(ValueError):
        plonk.sample_circuit_lookup(2, seed, gate=gate)


# ---- failed_checks on the model prover's records ----
@pytest.mark.parametrize("gate", [None, "wide"])
@pytest.mark.parametrize("mu", [3, 5])
def test_failed_checks_on_model_records(mu, gate):
    from zkhip import plonk

    vk, pi, rec, finals, v_finals, l_finals, m = _record(mu, gate)
    c = plonk.challenges(vk, pi, rec)
    for k in ("tau_p", "r_p", "tau_g", "r_g", "rho_mu", "rho_mu1", "tau_l", "r_l", "rho_l"):
        assert zm.ints(c[k]) == m[k], k
    for k in ("alpha", "beta", "gamma", "b_alpha", "zeta", "beta_l", "gamma_l", "lambda"):
        assert zm.ints([c[k]])[0] == m[k], k
    lp = rec["lookup"]
    assert lp["commitments"].shape == (3, 18) and lp["rounds"].shape == (mu, 4, 4) and lp["values"].shape == (10, 4) and lp["batch"]["rounds"].shape == (mu, 3, 4)
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals, l_finals=l_finals) == []
    assert plonk.failed_checks(vk, pi, rec) == [] and plonk.field_checks(vk, pi, rec) is True
    # wrong finals of the third instance: its last value
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals, l_finals=_flip(l_finals, 0)) == [9]
    with_lp = lambda **kw: dict(rec, lookup=dict(lp, **kw))
    # a flipped limb in lookup.rounds: the chain (every later challenge moves too: the checks after it follow)
    got = plonk.failed_checks(vk, pi, with_lp(rounds=_flip(lp["rounds"], 0)), finals, v_finals, l_finals=l_finals)
    assert 7 in got and not {1, 2, 3, 4, 5} & set(got), got
    assert 7 in plonk.failed_checks(vk, pi, with_lp(rounds=_flip(lp["rounds"], (mu - 1) * 16 + 4)))
    # a flipped limb in lookup.values: the closed form (and the batch instance that certifies the value)
    for j in (0, 3, 9):
        got = plonk.failed_checks(vk, pi, with_lp(values=_flip(lp["values"], 4 * j)), finals, v_finals, l_finals=l_finals)
        assert 8 in got and not {1, 2, 3, 4, 5, 7} & set(got), (j, got)
    # a flipped limb in round 0 of lookup.batch.rounds: the third instance's chain, and nothing else
    bad = with_lp(batch=dict(lp["batch"], rounds=_flip(lp["batch"]["rounds"], 0)))
    assert plonk.failed_checks(vk, pi, bad, finals, v_finals) == [9]
    # the digest covers the new parts
    assert plonk.proof_digest(bad) != plonk.proof_digest(rec) != plm.parent_digest(rec)


@pytest.mark.parametrize("gate", [None, "wide"])
def test_a_lying_prover_fails_the_lookup_chain(gate):
    """the break_lookup row forced through, m counted as if the row were in the table: gate and wiring hold, the LogUp sum is not zero"""
    from zkhip import plonk

    mu = 3
    c = plonk.sample_circuit_lookup(mu, 5, gate=gate)
    K = int(np.flatnonzero(c["lookup"]["qk"][:, 0])[-1])
    vk, pi, rec, finals, v_finals, l_finals, _m = _record(mu, gate, break_lookup=K, check=False)
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals, l_finals=l_finals) == [7]
    with pytest.raises(ValueError, match="1 of 8 rows"):
        plm.model_record(mu, 5, gate=gate, break_lookup=K)


def test_record_and_key_must_agree_on_the_lookup():
    from zkhip import plonk

    for gate in (None, "wide"):
        vk, pi, rec, *_ = _record(3, gate)
        if gate == "wide":
            p_vk, p_pi, p_rec, _f, _vf, _m = wg.model_record(3, 5)
        else:
            p_vk, p_pi, p_rec, _f, _vf = wg.basic_model_record(3, 5)
        assert plonk.failed_checks(p_vk, p_pi, p_rec) == []
        assert plonk.failed_checks(p_vk, p_pi, rec) == [0]  # a record with the lookup against a key without one
        assert plonk.failed_checks(vk, pi, p_rec) == [0]    # and the reverse
        assert plonk.failed_checks(vk, pi, {k: v for k, v in rec.items() if k != "lookup"}) == [0]
        with pytest.raises(ValueError):
            plonk.challenges(p_vk, p_pi, rec)
    vk, pi, rec, *_ = _record(3, None)
    wvk, wpi, wrec, *_ = _record(3, "wide")
    assert plonk.failed_checks(vk, pi, wrec) == [0] and plonk.failed_checks(wvk, wpi, rec) == [0]


# ---- records without a lookup are unmoved ----
@pytest.mark.parametrize("mu,seed", [(4, 7), (3, 5)])
def test_records_without_a_lookup_keep_their_digests(mu, seed):
    from zkhip import plonk

    vk, pi, rec, finals, v_finals = wg.basic_model_record(mu, seed)
    assert "lookup" not in rec and plonk.failed_checks(vk, pi, rec, finals, v_finals) == []
    assert plonk.proof_digest(rec) == plm.parent_digest(rec)
    assert set(plonk.challenges(vk, pi, rec)) == {"alpha", "beta", "gamma", "tau_p", "r_p", "tau_g", "r_g", "b_alpha", "rho_mu", "rho_mu1"}
    vk, pi, rec, finals, v_finals, _m = wg.model_record(mu, seed)
    assert "lookup" not in rec and plonk.failed_checks(vk, pi, rec, finals, v_finals) == []
    assert plonk.proof_digest(rec) == plm.parent_digest(rec)
    # the generators without the lookup plan give what they gave: the lookup sample differs from them on its lookup rows only
    for gate, gen in ((None, plonk.sample_circuit), ("wide", plonk.sample_circuit_wide)):
        plain, lk = gen(mu, seed), plonk.sample_circuit_lookup(mu, seed, gate=gate)
        assert (plain["public_inputs"] == lk["public_inputs"]).all() and (plain["s"] == lk["s"]).all()
        first = int(np.flatnonzero(lk["lookup"]["qk"][:, 0])[0])
        assert all((plain[k][:first] == lk[k][:first]).all() for k in ("a", "b", "c"))


def test_prove_asks_for_idx_exactly_with_a_lookup():
    from zkhip import plonk

    z = np.zeros((8, 4), dtype=np.uint64)
    pk = {"mu": 3, "l": 4, "pcs": None, "tables": {}, "commitments": None}
    with pytest.raises(ValueError, match="idx"):
        plonk.prove(None, dict(pk, lookup=True), z, z, z, z[:4])
    with pytest.raises(ValueError, match="idx"):
        plonk.prove(None, pk, z, z, z, z[:4], idx=np.zeros(8, dtype=np.uint32))


# ---- the entry points exist ----
def test_symbols_in_the_library_the_header_and_the_binding():
    import zkhip

    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    lib = ctypes.CDLL(zkhip.LIB_PATH)
    for s in SYMBOLS:
        assert f"int {s}(" in header, s
        assert f"pub fn {s}(" in rust, s
        assert getattr(lib, s) is not None, s
    assert all(hasattr(zkhip.Ctx, m) for m in ("lookup3_multiplicities", "lookup3_terms", "sumcheck_lookup_sel", "sumcheck_lookup_sel_fs"))
    val = ctypes.c_long(0)
    assert lib.zk_dbg_tune_get(b"lookupsel_local_e", ctypes.byref(val)) == 0 and val.value == 512


# ---- the compiled host's sample generator (no GPU) ----
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")


@pytest.mark.parametrize("gate", [None, "wide"])
@pytest.mark.parametrize("seed", [3, 7])
def test_sample_only_digest_is_the_same_in_both_hosts(seed, gate):
    """plonk_check --sample-only builds the circuit of sample_circuit_lookup without a device and prints the digest of its tables"""
    import subprocess

    from zkhip import plonk

    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    kind = ["--gate", "wide"] if gate else []
    for mu in (3, 6):
        c = plonk.sample_circuit_lookup(mu, seed, gate=gate)
        K = int(np.flatnonzero(c["lookup"]["qk"][:, 0])[0])
        for flags, circuit in (([], c), (["--break-lookup", str(K)], plonk.sample_circuit_lookup(mu, seed, gate=gate, break_lookup=K))):
            r = subprocess.run([os.path.join(HOST, "bin", "plonk_check"), "--mu", str(mu), "--seed", str(seed), "--lookup", *kind, "--sample-only", *flags],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stdout == f"circuit sha256 {plonk.circuit_digest(circuit)}\n", (mu, flags, r.returncode, r.stdout, r.stderr)
    plain = (plonk.sample_circuit_wide if gate else plonk.sample_circuit)(4, seed)  # without --lookup: the digest of --circuit-only, as before
    r = subprocess.run([os.path.join(HOST, "bin", "plonk_check"), "--mu", "4", "--seed", str(seed), *kind, "--sample-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == f"circuit sha256 {plonk.circuit_digest(plain)}\n"
    r = subprocess.run([os.path.join(HOST, "bin", "plonk_check"), "--mu", "2", "--lookup", "--sample-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and not r.stdout
