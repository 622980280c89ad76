"""
The lookup argument on the device: zk_sumcheck_lookup / _fs bit-exact against the big-int model (lookup_model.py),
zk_lookup_multiplicities against numpy.bincount and its refusals, and zkhip.lookup prove -> verify end to end.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fs_model as fm
import lookup_model as lm
import pyoracle as po

pytestmark = pytest.mark.gpu

R = po.R_MOD
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
LOOKUP_CHECK = os.path.join(HOST, "bin", "lookup_check")
_MODEL = {}


def _random_case(n, seed=0):
    """six random tables (they need not satisfy the relation), gamma, challenges, and the model's run: computed once per (n, seed)"""
    if (n, seed) not in _MODEL:
        rng = po.SplitMix64(7000 + 10 * n + seed)
        tabs = {k: rng.fr_vec(1 << n) for k in lm.TABLES}
        gamma, chal = rng.fr_vec(1)[0], rng.fr_vec(n)
        _MODEL[(n, seed)] = (tabs, gamma, chal, lm.sumcheck_lookup(tabs, gamma, chal))
    return _MODEL[(n, seed)]


def _upload(ctx, tabs):
    return [ctx.to_device(lm.mont(tabs[k])) for k in lm.TABLES]


def _check_against_model(ctx, n):
    tabs, gamma, chal, (rounds, last) = _random_case(n)
    bufs = _upload(ctx, tabs)
    got_r, got_l = ctx.sumcheck_lookup(bufs, 1 << n, lm.mont([gamma])[0], lm.mont(chal))
    assert [lm.ints(r) for r in got_r] == rounds, n
    assert lm.ints(got_l) == last, n
    for b, k in zip(bufs, lm.TABLES):
        assert lm.ints(b.download((1 << n, 4))) == tabs[k], "an input table was written"
    return bufs, got_l


@pytest.mark.parametrize("n", range(1, 9))
def test_sumcheck_lookup_small_sizes_match_the_model(ctx, n):
    _check_against_model(ctx, n)


@pytest.mark.parametrize("n", [10, 12])
def test_sumcheck_lookup_with_hbm_passes_matches_the_model(ctx, n):
    """above the 512-element hand-over: one and three HBM passes, where hf - ht enters the wide sums"""
    bufs, last = _check_against_model(ctx, n)
    _, _, chal, _ = _random_case(n)
    for k, b in enumerate(bufs):  # h_last is the six tables folded by zk_fold
        assert (ctx.fold(b, 1 << n, lm.mont(chal)).download((1, 4))[0] == last[k]).all(), k


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


@pytest.mark.parametrize("e", [1, 2])
def test_hbm_passes_down_to_the_last_elements(ctx, e):
    with _Knob(b"lookup_local_e", e):
        _check_against_model(ctx, 6)
        _diff_fs(ctx, 6)


def _diff_fs(ctx, n):
    from zkhip.transcript import HostTranscript, Transcript

    tabs, gamma, _chal, _ = _random_case(n)
    bufs = _upload(ctx, tabs)
    g = lm.mont([gamma])[0]
    tr = Transcript(ctx, b"diff").absorb(b"l%d" % n)
    rounds, last, chal = ctx.sumcheck_lookup_fs(bufs, 1 << n, g, tr)
    host = HostTranscript(b"diff")
    host.absorb(b"l%d" % n)
    want = np.stack([host.absorb(r).challenge() for r in rounds])
    assert (chal == want).all(), n
    assert tr.state() == host.state()  # the device transcript has absorbed every round
    p_rounds, p_last = ctx.sumcheck_lookup(bufs, 1 << n, g, chal)
    assert (rounds == p_rounds).all() and (last == p_last).all(), n
    tr.free()
    return rounds, last, chal


@pytest.mark.parametrize("n", [1, 5, 10, 12])
def test_lookup_fs_equals_parent_and_model(ctx, n):
    rounds, last, chal = _diff_fs(ctx, n)
    tabs, gamma, _chal, _ = _random_case(n)
    # the model driven by the model transcript: rounds, last values, challenges and the state afterwards
    from zkhip.transcript import HostTranscript

    tr_m = fm.Model(b"diff").absorb(b"l%d" % n)
    m_rounds, m_last, m_chal = fm._stepwise(tr_m, tabs, lambda cur, ch: lm.sumcheck_lookup(cur, gamma, ch)[0])
    assert [lm.ints(r) for r in rounds] == m_rounds and lm.ints(chal) == m_chal
    assert lm.ints(last) == [m_last[k] for k in lm.TABLES]
    host = HostTranscript(b"diff")
    host.absorb(b"l%d" % n)
    for r in rounds:
        host.absorb(r).challenge()
    assert host.state() == tr_m.state  # which _diff_fs found equal to the device transcript's


# ---- multiplicities ----
def _mult(ctx, t, f, idx):
    N = len(t)
    return ctx.lookup_multiplicities(ctx.to_device(f), ctx.to_device(t), ctx.to_device(np.ascontiguousarray(idx, dtype=np.uint32)), N).download((N, 4))


def _as_fr(counts):
    return lm.mont([int(c) for c in counts])


@pytest.mark.parametrize("n", [1, 7, 12])
def test_multiplicities_equal_bincount(ctx, n):
    from zkhip import lookup as lk

    N = 1 << n
    t, f, idx = lk.sample_lookup(n, 11 + n, max(N // 3, 1))
    want = np.bincount(idx, minlength=N)
    assert (_mult(ctx, t, f, idx) == _as_fr(want)).all()
    same = np.full(N, N - 1, dtype=np.uint32)  # every row names one entry: a multiplicity of N on one counter
    want = np.zeros(N, dtype=np.int64)
    want[N - 1] = N
    assert (_mult(ctx, t, t[same], same) == _as_fr(want)).all()


def test_multiplicities_refuses_rows_outside_the_table(ctx):
    """error paths on in-range memory only: the index is checked before anything is read through it"""
    from zkhip import lookup as lk

    n, N = 7, 128
    t, f, idx = lk.sample_lookup(n, 5, 40)
    good = np.bincount(idx, minlength=N)
    for bad_index in (N, 2**32 - 1):
        bad = idx.copy()
        bad[17] = bad_index
        with pytest.raises(ValueError, match="1 of 128 rows"):
            _mult(ctx, t, f, bad)
        assert (_mult(ctx, t, f, idx) == _as_fr(good)).all()  # the ctx still works
    top = f.copy()
    top[3, 3] ^= np.uint64(1 << 60)  # differs from its table entry in the top limb only
    with pytest.raises(ValueError, match="1 of 128 rows"):
        _mult(ctx, t, top, idx)
    two = f.copy()
    two[3, 0] ^= np.uint64(1)
    two[100, 1] ^= np.uint64(1)
    with pytest.raises(ValueError, match="2 of 128 rows"):
        _mult(ctx, t, two, idx)
    assert (_mult(ctx, t, f, idx) == _as_fr(good)).all()


def test_invalid_arguments_return_invalid_and_write_nothing(ctx):
    import zkhip
    from zkhip._lib import ZK_ERR_INVALID
    from zkhip.transcript import Transcript

    tabs, gamma, chal, _ = _random_case(4)
    bufs = _upload(ctx, tabs)
    g, ch = lm.mont([gamma])[0], lm.mont(chal)
    ptrs = (ctypes.c_void_p * 6)(*[b.ptr for b in bufs])
    tr = Transcript(ctx, b"err")
    state = tr.state()

    def raw(ptr_array, length, fs):
        out, last, co = np.full((4, 4, 4), 7, dtype=np.uint64), np.full((6, 4), 7, dtype=np.uint64), np.full((4, 4), 7, dtype=np.uint64)
        h = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        if fs:
            rc = ctx.lib.zk_sumcheck_lookup_fs(ctx.h, ptr_array, length, h(g), tr.h, h(out), h(last), h(co))
        else:
            rc = ctx.lib.zk_sumcheck_lookup(ctx.h, ptr_array, length, h(g), h(ch), h(out), h(last))
        assert rc == ZK_ERR_INVALID, (length, fs)
        assert (out == 7).all() and (last == 7).all() and (co == 7).all(), "an output was written"

    for fs in (False, True):
        for length in (0, 1, 3):
            raw(ptrs, length, fs)
        holed = (ctypes.c_void_p * 6)(*[b.ptr for b in bufs])
        holed[4] = None
        raw(holed, 16, fs)
        with _Knob(b"lookup_local_e", 3):
            raw(ptrs, 16, fs)
    with pytest.raises(zkhip.ZkError) as e:
        ctx.sumcheck_lookup_fs(bufs, 16, g, None)
    assert e.value.code == ZK_ERR_INVALID
    assert tr.state() == state  # nothing was absorbed by the failed calls
    tr.free()
    # zk_lookup_multiplicities: N < 2, not a power of two, a null pointer
    idx = ctx.to_device(np.zeros(16, dtype=np.uint32))
    for N, f in ((0, bufs[0].ptr), (1, bufs[0].ptr), (12, bufs[0].ptr), (16, None)):
        assert ctx.lib.zk_lookup_multiplicities(ctx.h, f, bufs[1].ptr, idx.ptr, N, bufs[2].ptr) == ZK_ERR_INVALID
    assert lm.ints(bufs[2].download((16, 4))) == tabs["dt"]
    _check_against_model(ctx, 4)  # and the valid call still works


# ---- end to end ----
@pytest.mark.parametrize("n", [4, 10])
def test_prove_verify_end_to_end(ctx, n):
    from zkhip import dist_primitive as dp
    from zkhip import lookup as lk
    from zkhip import pairing as pr

    N = 1 << n
    t, f, idx = lk.sample_lookup(n, 3, max(N // 4, 3))
    s = lk.sample_srs(n, 3)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    pk, vk = lk.preprocess(ctx, pcs, t, pr.powers_of_g2(lm.ints(s)))
    proof = lk.prove(ctx, pk, f, idx)
    assert lk.failed_checks(vk, proof) == [] and lk.field_checks(vk, proof) is True
    assert lk.verify(ctx, vk, proof) is True
    assert lk.proof_digest(lk.prove(ctx, pk, f, idx)) == lk.proof_digest(proof)  # deterministic
    # the big-int model on the same tables, with the device's commitments: the same record field by field
    names = dict(zip(lk.COMMITTED, proof["commitments"]))
    mo = lm.prove(lm.ints(f), lm.ints(t), [int(i) for i in idx], vk["commitment"], lambda name, _tab: names[name])
    rec = lm.model_record(mo)
    assert rec["n"] == proof["n"]
    for key in ("commitments", "rounds", "values"):
        assert (rec[key] == proof[key]).all(), key
    assert (rec["batch"]["rounds"] == proof["batch"]["rounds"]).all()
    assert lk.failed_checks(vk, proof, finals=lm.mont(mo["finals"])) == []
    # a flipped limb in each field of the record
    flip = lambda a, i: (lambda b: (b.__setitem__(i, b[i] ^ np.uint64(1)), b)[1])(np.array(a, copy=True))
    assert lk.failed_checks(vk, dict(proof, rounds=flip(proof["rounds"], (0, 1, 0)))) == [1]
    assert lk.failed_checks(vk, dict(proof, values=flip(proof["values"], (4, 0)))) == [2]
    assert lk.failed_checks(vk, dict(proof, commitments=flip(proof["commitments"], (2, 5)))) == [1]  # gamma, lambda, tau change
    assert lk.failed_checks(vk, dict(proof, batch=dict(proof["batch"], rounds=flip(proof["batch"]["rounds"], (n - 1, 2, 0))))) == []  # t2 of the last round: only the value the chain ends in moves
    assert lk.verify(ctx, vk, dict(proof, batch=dict(proof["batch"], rounds=flip(proof["batch"]["rounds"], (n - 1, 2, 0))))) is False
    assert lk.failed_checks(vk, dict(proof, batch=dict(proof["batch"], rounds=flip(proof["batch"]["rounds"], (0, 0, 0))))) == [3]
    assert lk.failed_checks(vk, dict(proof, n=n + 1)) == [0]
    # a tampered opening: the field checks hold, the pairing does not
    bad = dict(proof, batch=dict(proof["batch"], opening=np.array(proof["batch"]["opening"], copy=True)))
    bad["batch"]["opening"][0] = proof["batch"]["opening"][n - 1]
    assert lk.field_checks(vk, bad) is True and lk.verify(ctx, vk, bad) is False
    off_curve = dict(proof, batch=dict(proof["batch"], opening=flip(proof["batch"]["opening"], (0, 3))))  # a flipped limb: no point of the curve
    assert lk.field_checks(vk, off_curve) is True and lk.verify(ctx, vk, off_curve) is False
    # a value outside the table is refused by the prover
    out = f.copy()
    out[N - 1, 0] ^= np.uint64(1)
    with pytest.raises(ValueError):
        lk.prove(ctx, pk, out, idx)
    assert lk.verify(ctx, vk, lk.prove(ctx, pk, f, idx)) is True


# ---- the compiled host ----
def _lookup_check(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/lookup_check"])
    r = subprocess.run([LOOKUP_CHECK, *args], capture_output=True, text=True, timeout=600)
    m = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout)
    return r, m.group(1) if m else None


@pytest.mark.parametrize("seed", [3, 8])
def test_python_and_cpp_digests_agree(ctx, seed):
    from zkhip import dist_primitive as dp
    from zkhip import lookup as lk

    n = 10
    r, got = _lookup_check("--n", str(n), "--seed", str(seed))
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    t, f, idx = lk.sample_lookup(n, seed)
    pk, _vk = lk.preprocess(ctx, dp.PolynomialCommitmentCub.new(ctx, lk.sample_srs(n, seed)).mature(), t)
    assert lk.proof_digest(lk.prove(ctx, pk, f, idx)) == got


def test_lookup_check_rejects_tampered_records_and_refuses_outside_values():
    for k in range(5):
        r, got = _lookup_check("--n", "10", "--seed", "3", "--break", str(k))
        assert r.returncode == 1 and "reject" in r.stdout and got, (k, r.returncode, r.stdout, r.stderr)
    r, got = _lookup_check("--n", "10", "--seed", "3", "--outside")
    assert r.returncode == 1 and "refused" in r.stdout and "1 of 1024 rows" in r.stdout and got is None, (r.returncode, r.stdout, r.stderr)
