"""
Plonk with lookups on the device: zk_sumcheck_lookup_sel / _fs bit-exact against the big-int model (plonk_lookup_model.py) and against
zk_sumcheck_lookup where qk = 1, zk_lookup3_multiplicities against numpy.bincount and its refusals, zk_lookup3_terms against the model,
zkhip.plonk prove -> verify on sample_circuit_lookup for both gate kinds, and the compiled host (host/bin/plonk_check --lookup): one
digest for one seed, a broken lookup refused, every tampered part of the record rejected.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fs_model as fm
import lookup_model as lm
import plonk_lookup_model as plm
import plonk_model as pm
import pyoracle as po
import widegate_model as wg
import zerocheck_model as zm

pytestmark = pytest.mark.gpu

R = po.R_MOD
_MODEL = {}


def _random_case(n):
    """seven random tables (they need not satisfy the relation), gamma, challenges, and the model's run: computed once per n"""
    if n not in _MODEL:
        tabs = plm.random_tables(n, 9000 + 10 * n)
        rng = po.SplitMix64(9500 + n)
        gamma, chal = rng.fr_vec(1)[0], rng.fr_vec(n)
        _MODEL[n] = (tabs, gamma, chal, plm.sumcheck_lookup_sel(tabs, gamma, chal))
    return _MODEL[n]


def _upload(ctx, tabs, names=plm.TABLES):
    return [ctx.to_device(zm.mont(tabs[k])) for k in names]


def _check_against_model(ctx, n):
    tabs, gamma, chal, (rounds, last) = _random_case(n)
    bufs = _upload(ctx, tabs)
    got_r, got_l = ctx.sumcheck_lookup_sel(bufs, 1 << n, zm.mont([gamma])[0], zm.mont(chal))
    assert got_r.shape == (n, 4, 4) and got_l.shape == (7, 4)
    assert [zm.ints(r) for r in got_r] == rounds, n
    assert zm.ints(got_l) == last, n
    for b, k in zip(bufs, plm.TABLES):
        assert zm.ints(b.download((1 << n, 4))) == tabs[k], "an input table was written"
    return bufs, got_l


@pytest.mark.parametrize("n", range(1, 9))
def test_sumcheck_lookup_sel_small_sizes_match_the_model(ctx, n):
    """the local stage only"""
    _check_against_model(ctx, n)


@pytest.mark.parametrize("n", [10, 12])
def test_sumcheck_lookup_sel_with_hbm_passes_matches_the_model(ctx, n):
    """above the 512-element hand-over: one and three HBM passes, where hf - ht enters the wide sums"""
    bufs, last = _check_against_model(ctx, n)
    if n == 10:  # h_last is the seven tables folded by zk_fold
        _, _, chal, _ = _random_case(n)
        for k, b in enumerate(bufs):
            assert (ctx.fold(b, 1 << n, zm.mont(chal)).download((1, 4))[0] == last[k]).all(), k


class _Knob:
    def __init__(self, key, value):
        from zkhip._lib import test_hooks

        self.lib, self.key, self.value = test_hooks(), key, value

    def __enter__(self):
        v = ctypes.c_long(0)
        assert self.lib.zk_dbg_tune_get(self.key, ctypes.byref(v)) == 0
        self.found = v.value
        assert self.lib.zk_dbg_tune(self.key, self.value) == 0

    def __exit__(self, *exc):
        self.lib.zk_dbg_tune(self.key, self.found)


def _diff_fs(ctx, n):
    """the _fs form against a HostTranscript replay, the device transcript's state and the preset-challenge parent"""
    from zkhip.transcript import HostTranscript, Transcript

    tabs, gamma, _chal, _ = _random_case(n)
    bufs = _upload(ctx, tabs)
    g = zm.mont([gamma])[0]
    tr = Transcript(ctx, b"diff").absorb(b"s%d" % n)
    rounds, last, chal = ctx.sumcheck_lookup_sel_fs(bufs, 1 << n, g, tr)
    host = HostTranscript(b"diff")
    host.absorb(b"s%d" % n)
    want = np.stack([host.absorb(r).challenge() for r in rounds])
    assert (chal == want).all(), n
    assert tr.state() == host.state()  # the device transcript has absorbed every round
    p_rounds, p_last = ctx.sumcheck_lookup_sel(bufs, 1 << n, g, chal)
    assert (rounds == p_rounds).all() and (last == p_last).all(), n
    tr.free()
    return rounds, last, chal


@pytest.mark.parametrize("e", [1, 2])
def test_hbm_passes_down_to_the_last_elements(ctx, e):
    with _Knob(b"lookupsel_local_e", e):
        _check_against_model(ctx, 6)
        _diff_fs(ctx, 6)


@pytest.mark.parametrize("n", [5, 10, 12])
def test_qk_one_is_the_six_table_sumcheck(ctx, n):
    tabs, gamma, chal, _ = _random_case(n)
    one = dict(tabs, qk=[1] * (1 << n))
    bufs = _upload(ctx, one)
    g, ch = zm.mont([gamma])[0], zm.mont(chal)
    rounds, last = ctx.sumcheck_lookup_sel(bufs, 1 << n, g, ch)
    p_rounds, p_last = ctx.sumcheck_lookup(bufs[:6], 1 << n, g, ch)
    assert (rounds == p_rounds).all() and (last[:6] == p_last).all()
    assert (last[6] == zm.mont([1])[0]).all()


@pytest.mark.parametrize("n", [1, 5, 10, 12])
def test_lookup_sel_fs_equals_parent_and_model(ctx, n):
    rounds, last, chal = _diff_fs(ctx, n)
    tabs, gamma, _chal, _ = _random_case(n)
    tr_m = fm.Model(b"diff").absorb(b"s%d" % n)
    m_rounds, m_last, m_chal = fm._stepwise(tr_m, tabs, lambda cur, ch: plm.sumcheck_lookup_sel(cur, gamma, ch)[0])
    assert [zm.ints(r) for r in rounds] == m_rounds and zm.ints(chal) == m_chal
    assert zm.ints(last) == [m_last[k] for k in plm.TABLES]


# ---- multiplicities and the derived tables ----
def _columns(n, seed):
    """a table of N random triples, a random selector, indices with repeats; selected rows hold their entry, the others random values"""
    from zkhip.field import fr_mont, splitmix_fr

    N = 1 << n
    t = [splitmix_fr(N, seed + j) for j in range(3)]
    w = [splitmix_fr(N, seed + 3 + j) for j in range(3)]
    draw = splitmix_fr(N, seed + 6)
    sel = (draw[:, 0] & np.uint64(1)) == 1
    sel[0] = sel[N - 1] = True
    idx = (draw[:, 1] % np.uint64(max(N // 3, 1))).astype(np.uint32)
    for j in range(3):
        w[j][sel] = t[j][idx[sel]]
    qk = np.zeros((N, 4), dtype=np.uint64)
    qk[sel] = fr_mont(1)
    return w, t, qk, idx, sel


def _mult(ctx, w, t, qk, idx):
    N = len(qk)
    dev = lambda a: ctx.to_device(np.ascontiguousarray(a))
    return ctx.lookup3_multiplicities([dev(x) for x in w], [dev(x) for x in t], dev(qk), dev(np.ascontiguousarray(idx, dtype=np.uint32)), N).download((N, 4))


def _as_fr(counts):
    return zm.mont([int(c) for c in counts])


@pytest.mark.parametrize("n", [3, 7, 12])
def test_multiplicities(ctx, n):
    from zkhip.field import fr_mont

    N = 1 << n
    w, t, qk, idx, sel = _columns(n, 40 + n)
    good = np.bincount(idx[sel], minlength=N)
    assert (_mult(ctx, w, t, qk, idx) == _as_fr(good)).all()
    # every row names one entry: a multiplicity of N on one counter
    same = np.full(N, N - 1, dtype=np.uint32)
    ones = np.tile(fr_mont(1), (N, 1))
    want = np.zeros(N, dtype=np.int64)
    want[N - 1] = N
    assert (_mult(ctx, [x[same] for x in t], t, ones, same) == _as_fr(want)).all()
    # nothing selected: the indices are never read through
    assert (_mult(ctx, w, t, np.zeros((N, 4), dtype=np.uint64), np.full(N, 2**32 - 1, dtype=np.uint32)) == 0).all()
    # refusals, on in-range memory only: the index is checked before anything is read through it
    x = int(np.flatnonzero(sel)[-1])
    bad = idx.copy()
    bad[x] = N
    with pytest.raises(ValueError, match=f"1 of {N} rows"):
        _mult(ctx, w, t, qk, bad)
    for j in range(3):  # a difference in the top limb of a, b, c
        wj = [c.copy() for c in w]
        wj[j][x, 3] ^= np.uint64(1 << 60)
        with pytest.raises(ValueError, match=f"1 of {N} rows"):
            _mult(ctx, wj, t, qk, idx)
    two = qk.copy()
    two[x] = fr_mont(2)
    two[0] = fr_mont(2)
    with pytest.raises(ValueError, match=f"2 of {N} rows"):
        _mult(ctx, w, t, two, idx)
    assert (_mult(ctx, w, t, qk, idx) == _as_fr(good)).all()  # the ctx still works


@pytest.mark.parametrize("n", [1, 7, 12])
def test_terms_match_the_model(ctx, n):
    N = 1 << n
    rng = po.SplitMix64(60 + n)
    w, t = [rng.fr_vec(N) for _ in range(3)], [rng.fr_vec(N) for _ in range(3)]
    zeta, beta = rng.fr_vec(2)
    wb, tb = [ctx.to_device(zm.mont(x)) for x in w], [ctx.to_device(zm.mont(x)) for x in t]
    df, dt = ctx.lookup3_terms(wb, tb, N, zm.mont([zeta])[0], zm.mont([beta])[0])
    want_df, want_dt = plm.terms(w, t, zeta, beta)
    assert zm.ints(df.download((N, 4))) == want_df and zm.ints(dt.download((N, 4))) == want_dt
    for b, x in zip(wb + tb, w + t):
        assert zm.ints(b.download((N, 4))) == x, "an input was written"


def test_invalid_arguments_return_invalid_and_write_nothing(ctx):
    import zkhip
    from zkhip._lib import ZK_ERR_INVALID
    from zkhip.transcript import Transcript

    tabs, gamma, chal, _ = _random_case(4)
    bufs = _upload(ctx, tabs)
    g, ch = zm.mont([gamma])[0], zm.mont(chal)
    ptrs = (ctypes.c_void_p * 7)(*[b.ptr for b in bufs])
    tr = Transcript(ctx, b"err")
    state = tr.state()
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def raw(ptr_array, length, fs):
        out, last, co = np.full((4, 4, 4), 7, dtype=np.uint64), np.full((7, 4), 7, dtype=np.uint64), np.full((4, 4), 7, dtype=np.uint64)
        if fs:
            rc = ctx.lib.zk_sumcheck_lookup_sel_fs(ctx.h, ptr_array, length, h(g), tr.h, h(out), h(last), h(co))
        else:
            rc = ctx.lib.zk_sumcheck_lookup_sel(ctx.h, ptr_array, length, h(g), h(ch), h(out), h(last))
        assert rc == ZK_ERR_INVALID, (length, fs)
        assert (out == 7).all() and (last == 7).all() and (co == 7).all(), "an output was written"

    for fs in (False, True):
        for length in (0, 1, 3):
            raw(ptrs, length, fs)
        holed = (ctypes.c_void_p * 7)(*[b.ptr for b in bufs])
        holed[6] = None
        raw(holed, 16, fs)
        for e in (3, 1024):
            with _Knob(b"lookupsel_local_e", e):
                raw(ptrs, 16, fs)
    with pytest.raises(zkhip.ZkError) as e:
        ctx.sumcheck_lookup_sel_fs(bufs, 16, g, None)
    assert e.value.code == ZK_ERR_INVALID
    assert tr.state() == state  # nothing was absorbed by the failed calls
    tr.free()
    # zk_lookup3_multiplicities / zk_lookup3_terms: N < 2, not a power of two, a null pointer (in a column array or alone)
    idx = ctx.to_device(np.zeros(16, dtype=np.uint32))
    three = (ctypes.c_void_p * 3)(*[b.ptr for b in bufs[:3]])
    holed3 = (ctypes.c_void_p * 3)(bufs[0].ptr, None, bufs[2].ptr)
    out1, out2 = bufs[4], bufs[5]
    for N, w, qk in ((0, three, bufs[3].ptr), (1, three, bufs[3].ptr), (12, three, bufs[3].ptr), (16, holed3, bufs[3].ptr), (16, three, None)):
        assert ctx.lib.zk_lookup3_multiplicities(ctx.h, w, three, qk, idx.ptr, N, out1.ptr) == ZK_ERR_INVALID
    for N, w, z in ((0, three, h(g)), (1, three, h(g)), (12, three, h(g)), (16, holed3, h(g)), (16, three, None)):
        assert ctx.lib.zk_lookup3_terms(ctx.h, w, three, N, z, h(g), out1.ptr, out2.ptr) == ZK_ERR_INVALID
    assert zm.ints(out1.download((16, 4))) == tabs["hf"] and zm.ints(out2.download((16, 4))) == tabs["ht"]
    _check_against_model(ctx, 4)  # and the valid call still works


# ---- end to end ----
def _setup(ctx, mu, seed, gate, **kw):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(mu, seed, gate=gate, **kw)
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
    return c, pk, vk


def _flip(a, idx):
    a = np.array(a, dtype=np.uint64, copy=True)
    a.reshape(-1)[idx] ^= np.uint64(1)
    return a


@pytest.mark.parametrize("gate", [None, "wide"])
@pytest.mark.parametrize("mu", [4, 10])
def test_prove_verify_end_to_end(ctx, mu, gate):
    from zkhip import plonk

    seed = 7
    c, pk, vk = _setup(ctx, mu, seed, gate)
    pi = c["public_inputs"]
    ns = 6 if gate == "wide" else 2
    assert vk["lookup"] is True and vk.get("gate") == gate and vk["commitments"].shape == (ns + 3 + 4, 18)
    proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=c["idx"])
    lp = proof["lookup"]
    assert lp["commitments"].shape == (3, 18) and lp["rounds"].shape == (mu, 4, 4) and lp["values"].shape == (10, 4)
    assert lp["batch"]["rounds"].shape == (mu, 3, 4) and np.asarray(lp["batch"]["opening"]).shape == (mu, 18)
    assert plonk.failed_checks(vk, pi, proof) == [] and plonk.field_checks(vk, pi, proof) is True
    assert plonk.verify(ctx, vk, pi, proof) is True
    assert plonk.proof_digest(plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=c["idx"])) == plonk.proof_digest(proof)  # deterministic
    # the big-int model on the same tables, with the device's commitments: the same record field by field
    names = {"v": proof["v_commitment"], **dict(zip(plonk.LOOKUP_COMMITTED, lp["commitments"]))}
    lk, idx = plm.lookup_ints(c)
    m = plm.prove((wg if gate == "wide" else pm).circuit_ints(c), lk, idx, mu, c["l"], vk["commitments"], proof["commitments"], lambda name, _t: names[name], gate=gate)
    rec = plm.record(m, proof["commitments"])
    for key in pm.FIELD_PARTS:
        assert (np.asarray(rec[key]) == np.asarray(proof[key])).all(), key
    for key in ("batch", "v_batch"):
        assert (rec[key]["rounds"] == proof[key]["rounds"]).all(), key
    for key in ("commitments", "rounds", "values"):
        assert (rec["lookup"][key] == lp[key]).all(), key
    assert (rec["lookup"]["batch"]["rounds"] == lp["batch"]["rounds"]).all()
    finals, v_finals, l_finals = zm.mont(m["finals"]), zm.mont(m["v_finals"]), zm.mont(m["l_finals"])
    assert plonk.failed_checks(vk, pi, proof, finals, v_finals, l_finals=l_finals) == []
    assert plonk.failed_checks(vk, pi, proof, finals, v_finals, l_finals=_flip(l_finals, 4)) == [9]
    # the tampers of the CPU list
    with_lp = lambda **kw: dict(proof, lookup=dict(lp, **kw))
    for bad, check in ((with_lp(rounds=_flip(lp["rounds"], 4)), 7), (with_lp(values=_flip(lp["values"], 4 * 8)), 8),
                       (with_lp(batch=dict(lp["batch"], rounds=_flip(lp["batch"]["rounds"], 0))), 9)):
        assert check in plonk.failed_checks(vk, pi, bad) and plonk.verify(ctx, vk, pi, bad) is False, check
    assert plonk.failed_checks(vk, pi, {k: v for k, v in proof.items() if k != "lookup"}) == [0]
    assert plonk.verify(ctx, vk, pi, {k: v for k, v in proof.items() if k != "lookup"}) is False
    # a tampered opening of the third instance: the field checks hold, the pairing does not
    opening = np.array(lp["batch"]["opening"], copy=True)
    opening[0] = lp["batch"]["opening"][mu - 1]
    bad = with_lp(batch=dict(lp["batch"], opening=opening))
    assert plonk.field_checks(vk, pi, bad) is True and plonk.verify(ctx, vk, pi, bad) is False
    # a triple outside the table is refused by the prover; the next honest proof verifies
    K = int(np.flatnonzero(c["lookup"]["qk"][:, 0])[-1])
    bc = plonk.sample_circuit_lookup(mu, seed, gate=gate, break_lookup=K)
    with pytest.raises(ValueError, match=f"1 of {1 << mu} rows"):
        plonk.prove(ctx, pk, bc["a"], bc["b"], bc["c"], pi, idx=c["idx"])
    with pytest.raises(ValueError, match="idx"):
        plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi)
    assert plonk.verify(ctx, vk, pi, plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=c["idx"])) is True


def test_a_circuit_without_a_lookup_is_proved_as_before(ctx):
    """the same circuit with and without its lookup part: the plain record has no "lookup", verifies under the plain key only"""
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    c, pk, vk = _setup(ctx, 4, 7, None)
    plain = {k: v for k, v in c.items() if k not in ("lookup", "idx")}
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    p_pk, p_vk = plonk.preprocess(ctx, pcs, plain, pr.powers_of_g2(zm.ints(c["s"])))
    assert "lookup" not in p_vk and (p_vk["commitments"] == vk["commitments"][:5]).all()
    proof = plonk.prove(ctx, p_pk, c["a"], c["b"], c["c"], c["public_inputs"])
    assert "lookup" not in proof and plonk.verify(ctx, p_vk, c["public_inputs"], proof) is True
    assert plonk.proof_digest(proof) == plm.parent_digest(proof)
    assert plonk.failed_checks(vk, c["public_inputs"], proof) == [0]
    with pytest.raises(ValueError, match="idx"):
        plonk.prove(ctx, p_pk, c["a"], c["b"], c["c"], c["public_inputs"], idx=c["idx"])
    bad = dict(c, lookup=dict(c["lookup"], qk=_flip(c["lookup"]["qk"], 4 * 9)))
    with pytest.raises(ValueError, match="qk"):
        plonk.preprocess(ctx, pcs, bad)


# ---- the compiled host ----
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
PLONK_CHECK = os.path.join(HOST, "bin", "plonk_check")


def _plonk_check(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    r = subprocess.run([PLONK_CHECK, *args], capture_output=True, text=True, timeout=600)
    m = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout)
    return r, m.group(1) if m else None


@pytest.mark.parametrize("gate", [None, "wide"])
@pytest.mark.parametrize("seed", [3, 7])
def test_python_and_cpp_digests_agree(ctx, seed, gate):
    """a second implementation of the schedule and of the sample generator: one seed, one digest across the two hosts"""
    from zkhip import plonk

    mu = 10
    kind = ("--gate", "wide") if gate else ()
    r, got = _plonk_check("--mu", str(mu), "--seed", str(seed), "--lookup", *kind)
    assert r.returncode == 0 and r.stdout.endswith(" lookup: accept\n") and ("gate=wide" in r.stdout) == bool(gate), (r.returncode, r.stdout, r.stderr)
    c, pk, vk = _setup(ctx, mu, seed, gate)
    proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], idx=c["idx"])
    assert plonk.proof_digest(proof) == got
    assert plonk.verify(ctx, vk, c["public_inputs"], proof) is True


@pytest.mark.parametrize("gate", [None, "wide"])
def test_plonk_check_refuses_a_broken_lookup_and_rejects_every_tampered_part(ctx, gate):
    from zkhip import plonk

    mu, seed = 10, 7
    kind = ("--gate", "wide") if gate else ()
    c = plonk.sample_circuit_lookup(mu, seed, gate=gate)
    K = int(np.flatnonzero(c["lookup"]["qk"][:, 0])[-1])
    r, got = _plonk_check("--mu", str(mu), "--seed", str(seed), "--lookup", *kind, "--break-lookup", str(K))
    assert r.returncode == 3 and got is None and f"1 of {1 << mu} rows" in r.stderr, (r.returncode, r.stdout, r.stderr)
    r, got = _plonk_check("--mu", str(mu), "--seed", str(seed), "--lookup", *kind, "--break", "all")  # one proof, one tampered copy per part
    lines = re.findall(r"^break (\d+) (\S+): (\w+)$", r.stdout, re.M)
    assert r.returncode == 1 and got, (r.returncode, r.stdout, r.stderr)
    assert [int(k) for k, _n, _v in lines] == list(range(16)) and all(v == "reject" for _k, _n, v in lines), r.stdout
    assert [n for _k, n, _v in lines][11:] == ["lookup.commitments", "lookup.rounds", "lookup.values", "lookup.batch.rounds", "lookup.batch.opening"]
    r, got = _plonk_check("--mu", str(mu), "--seed", str(seed), "--lookup", *kind, "--break", "13")  # and one part named alone
    assert r.returncode == 1 and r.stdout.endswith(" lookup: reject\n"), (r.returncode, r.stdout, r.stderr)
