"""
Lookups without caller indices on the device: zk_lookup_find / zk_lookup3_find against the plain-Python model (lookup_find_model.py) --
idx element for element, m bit-identical to the multiplicities call on that idx, inputs unmodified, either output optional --, forced
collision chains (knob find_force_slot), the limb comparison, the refusals, and the provers of both hosts with FIND / --find: the digest of
the proof from the sample's own indices.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lookup_find_model as fm
import zerocheck_model as zm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")


class _Knob:
    """sets a tuning knob of the library for a with-block and puts back what it found"""

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


def _knob_value(key):
    from zkhip._lib import test_hooks

    v = ctypes.c_long(0)
    assert test_hooks().zk_dbg_tune_get(key, ctypes.byref(v)) == 0
    return v.value


def _distincts(N):
    return sorted({1, min(2, N), max(N // 2, 1), N})


def _scattered(n, seed, distinct, cols=1):
    """a table whose duplicates lie anywhere (entry y = value draw[y] mod distinct), rows drawn from it, and a selector with some zeros;
    the rows that claim nothing hold values of their own"""
    from zkhip.field import fr_mont, splitmix_fr

    N = 1 << n
    vals = [splitmix_fr(distinct, seed + j) for j in range(cols)]
    draw = splitmix_fr(N, seed + 7)
    ty, fy = (draw[:, 0] % np.uint64(distinct)).astype(np.int64), (draw[:, 1] % np.uint64(distinct)).astype(np.int64)
    fy = np.where(np.isin(fy, ty), fy, ty[0])  # only values that the table holds
    t, f = [v[ty] for v in vals], [v[fy] for v in vals]
    qk = np.zeros((N, 4), dtype=np.uint64)
    qk[(draw[:, 2] & np.uint64(3)) != 0] = fr_mont(1)
    return t, f, qk


def _dev(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a))


def _find1(ctx, t, f):
    """zk_lookup_find on host arrays -> (idx u32[N], m [N, 4]); checks that the inputs are unmodified"""
    N = len(t)
    tb, fb = _dev(ctx, t), _dev(ctx, f)
    idx, m = ctx.lookup_find(fb, tb, N)
    assert (tb.download((N, 4)) == t).all() and (fb.download((N, 4)) == f).all(), "an input was written"
    return idx.download((N,), np.uint32), m.download((N, 4))


def _find3(ctx, t, f, qk):
    N = len(qk)
    tb, fb, qb = [_dev(ctx, x) for x in t], [_dev(ctx, x) for x in f], _dev(ctx, qk)
    idx, m = ctx.lookup3_find(fb, tb, qb, N)
    for b, x in zip(tb + fb + [qb], list(t) + list(f) + [qk]):
        assert (b.download((N, 4)) == x).all(), "an input was written"
    return idx.download((N,), np.uint32), m.download((N, 4))


def _mult1(ctx, t, f, idx):
    N = len(t)
    return ctx.lookup_multiplicities(_dev(ctx, f), _dev(ctx, t), _dev(ctx, idx.astype(np.uint32)), N).download((N, 4))


def _mult3(ctx, t, f, qk, idx):
    N = len(qk)
    return ctx.lookup3_multiplicities([_dev(ctx, x) for x in f], [_dev(ctx, x) for x in t], _dev(ctx, qk), _dev(ctx, idx.astype(np.uint32)), N).download((N, 4))


def _check1(ctx, t, f):
    want, bad, _ = fm.find(t, f)
    assert bad == 0
    idx, m = _find1(ctx, t, f)
    assert idx.tolist() == want
    assert (m == _mult1(ctx, t, f, idx)).all() and (m == zm.mont(fm.multiplicities(want))).all()
    return idx, m


def _check3(ctx, t, f, qk):
    want, bad, _ = fm.find(t, f, qk)
    assert bad == 0
    idx, m = _find3(ctx, t, f, qk)
    assert idx.tolist() == want
    assert (m == _mult3(ctx, t, f, qk, idx)).all() and (m == zm.mont(fm.multiplicities(want, qk))).all()
    return idx, m


# ---- against the model ----
@pytest.mark.parametrize("n", list(range(1, 11)) + [12])
def test_lookup_find_matches_the_model(ctx, n):
    from zkhip import lookup as lk

    N = 1 << n
    for distinct in _distincts(N):
        t, f, idx = lk.sample_lookup(n, 20 + n, distinct)  # duplicates as padding: one run of equal entries at the end
        got, _ = _check1(ctx, t, f)
        assert (got == idx).all()
        t, f, _qk = _scattered(n, 1000 * n + distinct, distinct)  # duplicates anywhere
        _check1(ctx, t[0], f[0])


@pytest.mark.parametrize("n", list(range(1, 11)) + [12])
def test_lookup3_find_matches_the_model(ctx, n):
    N = 1 << n
    for distinct in _distincts(N):
        t, f, qk = _scattered(n, 2000 * n + distinct, distinct, cols=3)
        for j in range(3):
            f[j][(qk == 0).all(axis=1)] ^= np.uint64(5)  # a row that claims nothing is in no table
        idx, _ = _check3(ctx, t, f, qk)
        assert (idx[(qk == 0).all(axis=1)] == 0).all()


@pytest.mark.parametrize("gate", [None, "wide"])
def test_lookup3_find_returns_the_circuit_samples_indices(ctx, gate):
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(7, 5, gate=gate)
    L = c["lookup"]
    idx, _ = _check3(ctx, [L["t0"], L["t1"], L["t2"]], [c["a"], c["b"], c["c"]], L["qk"])
    assert (idx == c["idx"]).all()


def test_either_output_may_be_null(ctx):
    from zkhip._lib import ZK_ERR_INVALID

    n, N = 6, 64
    t, f, qk = _scattered(n, 31, 20, cols=3)
    idx, m = _check3(ctx, t, f, qk)
    tb, fb, qb = [_dev(ctx, x) for x in t], [_dev(ctx, x) for x in f], _dev(ctx, qk)
    tp, fp = (ctypes.c_void_p * 3)(*[b.ptr for b in tb]), (ctypes.c_void_p * 3)(*[b.ptr for b in fb])
    only_i, only_m = ctx.alloc(4 * N), ctx.alloc(32 * N)
    assert ctx.lib.zk_lookup3_find(ctx.h, fp, tp, qb.ptr, N, only_i.ptr, None) == 0
    assert ctx.lib.zk_lookup3_find(ctx.h, fp, tp, qb.ptr, N, None, only_m.ptr) == 0
    assert (only_i.download((N,), np.uint32) == idx).all() and (only_m.download((N, 4)) == m).all()
    assert ctx.lib.zk_lookup3_find(ctx.h, fp, tp, qb.ptr, N, None, None) == ZK_ERR_INVALID
    idx1, m1 = _check1(ctx, t[0], f[0])
    assert ctx.lib.zk_lookup_find(ctx.h, fb[0].ptr, tb[0].ptr, N, only_i.ptr, None) == 0
    assert ctx.lib.zk_lookup_find(ctx.h, fb[0].ptr, tb[0].ptr, N, None, only_m.ptr) == 0
    assert (only_i.download((N,), np.uint32) == idx1).all() and (only_m.download((N, 4)) == m1).all()
    assert ctx.lib.zk_lookup_find(ctx.h, fb[0].ptr, tb[0].ptr, N, None, None) == ZK_ERR_INVALID


# ---- collision chains ----
@pytest.mark.parametrize("distinct", [256, 128, 1])
def test_forced_collision_chains_give_the_same_result(ctx, distinct):
    """n = 8, 512 slots: every key starts at slot 0 (one chain of all keys) or three slots before the end (the chain wraps round)"""
    n, slots = 8, 512
    t, f, qk = _scattered(n, 55 + distinct, distinct, cols=3)
    off1, off3 = _check1(ctx, t[0], f[0]), _check3(ctx, t, f, qk)
    for start in (0, slots - 3):
        with _Knob(b"find_force_slot", start):
            on1, on3 = _check1(ctx, t[0], f[0]), _check3(ctx, t, f, qk)
        for a, b in zip(off1 + off3, on1 + on3):
            assert (a == b).all(), start
    assert _knob_value(b"find_force_slot") == -1  # restored


# ---- the compare decides ----
def test_entries_that_differ_in_one_limb_only(ctx):
    """a forced chain: every key meets every other, so only the limb comparison tells them apart"""
    from zkhip.field import fr_mont

    n, N = 4, 16
    perm = np.array([(5 * x + 3) % N for x in range(N)])
    ones = np.tile(fr_mont(1), (N, 1))
    with _Knob(b"find_force_slot", 0):
        for limb in (0, 3):
            t = np.full((N, 4), 5, dtype=np.uint64)
            t[:, limb] = np.arange(N, dtype=np.uint64) + np.uint64(9)
            idx, _ = _check1(ctx, t, t[perm])
            assert (idx == perm).all(), limb
            f = t[perm].copy()
            f[6, 3] ^= np.uint64(1 << 60)  # differs from every entry in the top limb
            with pytest.raises(ValueError, match=f"1 of {N} rows.*first is row 6$"):
                _find1(ctx, t, f)
        # triples that differ in c only
        t3 = [np.full((N, 4), 5, dtype=np.uint64) for _ in range(3)]
        t3[2][:, 0] = np.arange(N, dtype=np.uint64) + np.uint64(9)
        idx, _ = _check3(ctx, t3, [x[perm] for x in t3], ones)
        assert (idx == perm).all()
        f3 = [x[perm].copy() for x in t3]
        f3[2][11, 3] ^= np.uint64(1 << 60)
        with pytest.raises(ValueError, match=f"1 of {N} rows.*first is row 11$"):
            _find3(ctx, t3, f3, ones)
        for j in (0, 1):  # and a row that differs in the top limb of a or b
            g3 = [x[perm].copy() for x in t3]
            g3[j][2, 3] ^= np.uint64(1 << 60)
            with pytest.raises(ValueError, match=f"1 of {N} rows.*first is row 2$"):
                _find3(ctx, t3, g3, ones)


# ---- refusals ----
def test_refusals(ctx):
    from zkhip._lib import ZK_ERR_INVALID
    from zkhip.field import fr_mont

    n, N = 7, 128
    t, f, qk = _scattered(n, 91, 40, cols=3)
    sel = np.flatnonzero((qk != 0).any(axis=1))
    good1, good3 = _check1(ctx, t[0], f[0]), _check3(ctx, t, f, qk)
    # one and two rows that the table does not hold
    miss = [x.copy() for x in f]
    miss[1][sel[9], 2] ^= np.uint64(1)
    with pytest.raises(ValueError, match=f"zk_lookup3_find: 1 of {N} rows.*first is row {sel[9]}$"):
        _find3(ctx, t, miss, qk)
    miss[0][sel[4], 0] ^= np.uint64(1)
    with pytest.raises(ValueError, match=f"zk_lookup3_find: 2 of {N} rows.*first is row {sel[4]}$"):
        _find3(ctx, t, miss, qk)
    one = f[0].copy()
    one[100, 1] ^= np.uint64(1)
    with pytest.raises(ValueError, match=f"zk_lookup_find: 1 of {N} rows.*first is row 100$"):
        _find1(ctx, t[0], one)
    one[17, 3] ^= np.uint64(1)
    with pytest.raises(ValueError, match=f"zk_lookup_find: 2 of {N} rows.*first is row 17$"):
        _find1(ctx, t[0], one)
    # a qk of 2 is a bad row, whatever the row holds
    two = qk.copy()
    two[sel[2]] = fr_mont(2)
    with pytest.raises(ValueError, match=f"1 of {N} rows.*first is row {sel[2]}$"):
        _find3(ctx, t, f, two)
    # garbage in a row with qk = 0 is not counted
    unsel = np.flatnonzero((qk == 0).all(axis=1))
    junk = [x.copy() for x in f]
    for j in range(3):
        junk[j][unsel] = np.uint64(0x1234567)
    idx, m = _find3(ctx, t, junk, qk)
    assert (idx == good3[0]).all() and (m == good3[1]).all()
    # N = 1, N = 3, a null input: nothing is launched
    tb, fb, qb = [_dev(ctx, x) for x in t], [_dev(ctx, x) for x in f], _dev(ctx, qk)
    tp, fp = (ctypes.c_void_p * 3)(*[b.ptr for b in tb]), (ctypes.c_void_p * 3)(*[b.ptr for b in fb])
    holed = (ctypes.c_void_p * 3)(tb[0].ptr, None, tb[2].ptr)
    oi, om = ctx.alloc(4 * N), ctx.alloc(32 * N)
    for bad_n in (0, 1, 3, 96, 1 << 32):
        assert ctx.lib.zk_lookup_find(ctx.h, fb[0].ptr, tb[0].ptr, bad_n, oi.ptr, om.ptr) == ZK_ERR_INVALID, bad_n
        assert ctx.lib.zk_lookup3_find(ctx.h, fp, tp, qb.ptr, bad_n, oi.ptr, om.ptr) == ZK_ERR_INVALID, bad_n
    assert ctx.lib.zk_lookup_find(ctx.h, None, tb[0].ptr, N, oi.ptr, om.ptr) == ZK_ERR_INVALID
    assert ctx.lib.zk_lookup_find(ctx.h, fb[0].ptr, tb[0].ptr, N, None, None) == ZK_ERR_INVALID
    assert ctx.lib.zk_lookup3_find(ctx.h, fp, holed, qb.ptr, N, oi.ptr, om.ptr) == ZK_ERR_INVALID
    assert ctx.lib.zk_lookup3_find(ctx.h, fp, tp, None, N, oi.ptr, om.ptr) == ZK_ERR_INVALID
    assert ctx.lib.zk_lookup3_find(ctx.h, fp, tp, qb.ptr, N, None, None) == ZK_ERR_INVALID
    # the ctx still works
    again1, again3 = _check1(ctx, t[0], f[0]), _check3(ctx, t, f, qk)
    assert all((a == b).all() for a, b in zip(good1 + good3, again1 + again3))


# ---- the provers, Python ----
_LOOKUP_DIGEST = {}  # (n, seed) -> digest of the proof from the sample's indices
_PLONK_DIGEST = {}   # (mu, seed, gate) -> the same


def _lookup_case(ctx, n, seed):
    from zkhip import dist_primitive as dp
    from zkhip import lookup as lk
    from zkhip import pairing as pr

    t, f, idx = lk.sample_lookup(n, seed)
    s = lk.sample_srs(n, seed)
    pk, vk = lk.preprocess(ctx, dp.PolynomialCommitmentCub.new(ctx, s).mature(), t, pr.powers_of_g2(zm.ints(s)))
    return pk, vk, f, idx


@pytest.mark.parametrize("n", [4, 10])
def test_lookup_prove_with_find_gives_the_digest_of_the_given_indices(ctx, n):
    from zkhip import lookup as lk

    pk, vk, f, idx = _lookup_case(ctx, n, 3)
    given, found = lk.prove(ctx, pk, f, idx), lk.prove(ctx, pk, f, lk.FIND)
    assert lk.proof_digest(found) == lk.proof_digest(given)
    assert lk.verify(ctx, vk, found) is True and lk.verify(ctx, vk, given) is True
    _LOOKUP_DIGEST[(n, 3)] = lk.proof_digest(given)
    outside = f.copy()
    outside[(1 << n) - 1, 0] ^= np.uint64(1)
    with pytest.raises(ValueError, match=f"1 of {1 << n} rows"):
        lk.prove(ctx, pk, outside, lk.FIND)


def _plonk_case(ctx, mu, seed, gate, **kw):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(mu, seed, gate=gate, **kw)
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
    return c, pk, vk


@pytest.mark.parametrize("gate", [None, "wide"])
@pytest.mark.parametrize("mu", [4, 10])
def test_plonk_prove_with_find_gives_the_digest_of_the_given_indices(ctx, mu, gate):
    from zkhip import plonk

    c, pk, vk = _plonk_case(ctx, mu, 7, gate)
    pi, N = c["public_inputs"], 1 << mu
    given = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=c["idx"])
    found = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=plonk.FIND)
    assert plonk.proof_digest(found) == plonk.proof_digest(given)
    assert plonk.verify(ctx, vk, pi, found) is True and plonk.verify(ctx, vk, pi, given) is True
    _PLONK_DIGEST[(mu, 7, gate)] = plonk.proof_digest(given)
    # a triple outside the table is refused
    K = int(np.flatnonzero(c["lookup"]["qk"][:, 0])[-1])
    bc = plonk.sample_circuit_lookup(mu, 7, gate=gate, break_lookup=K)
    with pytest.raises(ValueError, match=f"1 of {N} rows.*first is row {K}$"):
        plonk.prove(ctx, pk, bc["a"], bc["b"], bc["c"], pi, idx=plonk.FIND)
    # indices that name a later duplicate: a valid proof of its own, not the one FIND gives
    D = N // 4
    sel = (c["lookup"]["qk"] != 0).any(axis=1)
    moved = np.where(sel & (c["idx"] == D - 1), N - 1, c["idx"]).astype(np.uint32)
    assert (moved != c["idx"]).any()
    later = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi, idx=moved)
    assert plonk.verify(ctx, vk, pi, later) is True
    assert plonk.proof_digest(later) != plonk.proof_digest(found)


# ---- the provers, C++: one child process each ----
def _run(tool, *args):
    r = subprocess.run([os.path.join(HOST, "bin", tool), *args], capture_output=True, text=True, timeout=300)
    m = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout)
    return r, m.group(1) if m else None


def test_lookup_check_with_find_prints_the_same_digest(ctx):
    from zkhip import lookup as lk

    n, seed = 10, 3
    if (n, seed) not in _LOOKUP_DIGEST:
        pk, _vk, f, idx = _lookup_case(ctx, n, seed)
        _LOOKUP_DIGEST[(n, seed)] = lk.proof_digest(lk.prove(ctx, pk, f, idx))
    r, got = _run("lookup_check", "--n", str(n), "--seed", str(seed), "--find")
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert got == _LOOKUP_DIGEST[(n, seed)]


def test_plonk_check_with_find_prints_the_same_digest(ctx):
    from zkhip import plonk

    mu, seed = 10, 7
    if (mu, seed, None) not in _PLONK_DIGEST:
        c, pk, _vk = _plonk_case(ctx, mu, seed, None)
        _PLONK_DIGEST[(mu, seed, None)] = plonk.proof_digest(plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"], idx=c["idx"]))
    r, got = _run("plonk_check", "--mu", str(mu), "--seed", str(seed), "--lookup", "--find")
    assert r.returncode == 0 and r.stdout.endswith(" lookup: accept\n"), (r.returncode, r.stdout, r.stderr)
    assert got == _PLONK_DIGEST[(mu, seed, None)]
