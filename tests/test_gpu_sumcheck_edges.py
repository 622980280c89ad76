"""
The core sumcheck family (csrc/zk_fr.hip: sumcheck, sumcheck_product, fold, open_rounds, zk_sumcheck_batch) at extreme STORED values and on
every path of its planner, bit-exact against the C oracle (which reduces after every operation) and, on constant tables, against closed
forms in big-int Python.  Which input reaches which lazily reduced bound, and which knob setting gives which plan, is proved without a
GPU in tests/test_sumcheck_edge_inputs.py; the tables, challenge sets and cases live in helpers.py so that both files speak of the same.

Highest band reached by a flat K = 4 output: [4r, 8r).  No input reaches 8r (proof and search: test_sumcheck_edge_inputs.py).
"""
import ctypes

import numpy as np
import pytest

from helpers import (BAND_CALLS, BAND_CHAL, EDGE_TABLES, M_INT, R_MOD, SC_DEFAULTS, SC_PLAN_CASES, chal_set, const_fr, edge_table, fr_limbs,
                     sc_knobs)

pytestmark = pytest.mark.gpu

RINV = pow(1 << 256, -1, R_MOD)
CHALS = ("rand", "M", "zero", "one")
CHECK_INPUT_UP_TO = 13  # log2: input tables are downloaded after each call up to this size

_TAB, _DEV, _REF = {}, {}, {}


def tab(name, n):
    if (name, n) not in _TAB:
        t = edge_table(name, n)
        t.setflags(write=False)
        _TAB[(name, n)] = t
    return _TAB[(name, n)]


def dev(ctx, name, n):
    """one upload per table: the calls must not write their inputs (checked at the small sizes), so it can be shared"""
    if (name, n) not in _DEV:
        if n >= 19 and len(_DEV) > 24:
            _DEV.clear()
        _DEV[(name, n)] = ctx.to_device(tab(name, n))
    return _DEV[(name, n)]


def chal(cname, n, head=()):
    return chal_set(cname, n, head=head)


def reference(co, mode, n, f, g, cname, head=(), npts=None):
    """the oracle's result of one call, computed once: a tuple of arrays in the order `run` returns them"""
    key = (mode, n, f, g, cname, tuple(head), npts)
    if key not in _REF:
        ch = chal(cname, n, head)
        if mode == "plain":
            e = co.sumcheck(tab(f, n), ch)
            assert not e[n, 0].any()
            _REF[key] = (e[:n], e[n, 1])
        elif mode == "product":
            _REF[key] = co.sumcheck_product_rounds(tab(f, n), tab(g, n), ch)
        elif mode == "fold":
            cur = tab(f, n)
            for i in range(n if npts is None else min(n, npts)):
                cur = co.fold(cur, ch[i])
            _REF[key] = (cur,)
        else:
            q, v = co.open_quotients(tab(f, n), ch)
            _REF[key] = (q, v)
    return _REF[key]


def run(ctx, mode, n, f, g, cname, head=(), npts=None):
    L, ch = 1 << n, chal(cname, n, head)
    if mode == "plain":
        return ctx.sumcheck(dev(ctx, f, n), L, ch)
    if mode == "product":
        return ctx.sumcheck_product(dev(ctx, f, n), dev(ctx, g, n), L, ch)
    if mode == "fold":
        rounds = n if npts is None else min(n, npts)
        return (ctx.fold(dev(ctx, f, n), L, ch[:rounds] if rounds else ch[:0]).download((L >> rounds, 4)),)
    q, v = ctx.open_rounds(dev(ctx, f, n), L, ch)
    return (q.download((L - 1, 4)) if L > 1 else np.zeros((0, 4), dtype=np.uint64), v)


def closed_form(mode, n, cf, cg, npts=None):
    """constant tables (stored integers cf, cg): what every call returns, from the module docstring of the issue's closed forms"""
    lim = lambda v: fr_limbs(v % R_MOD)
    if mode == "plain":
        return (np.array([[lim(cf << (n - i - 1))] * 2 for i in range(n)], dtype=np.uint64).reshape(n, 2, 4), lim(cf))
    if mode == "product":
        p = cf * cg * RINV % R_MOD  # the stored form of the product of the two field elements
        return (np.array([[lim(p << (n - i - 1))] * 3 for i in range(n)], dtype=np.uint64).reshape(n, 3, 4), lim(cf), lim(cg))
    if mode == "fold":
        return (const_fr(cf, 1 << (n - (n if npts is None else min(n, npts)))),)
    return (np.zeros(((1 << n) - 1, 4), dtype=np.uint64), lim(cf))


CONST = {"M": M_INT, "zero": 0}


def check(ctx, co, mode, n, f, g=None, cname="rand", head=(), npts=None, what=""):
    got = run(ctx, mode, n, f, g, cname, head, npts)
    want = reference(co, mode, n, f, g, cname, head, npts)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and (a == b).all(), f"{what} {mode} 2^{n} f={f} g={g} chal={cname} npts={npts}: output {i} differs from the oracle"
    if f in CONST and (g is None or g in CONST):
        for i, (a, b) in enumerate(zip(got, closed_form(mode, n, CONST[f], CONST.get(g, 0), npts))):
            assert (a == b).all(), f"{what} {mode} 2^{n} constant tables {f}, {g}: output {i} differs from the closed form"
    if n <= CHECK_INPUT_UP_TO:
        for name in {f, g} - {None}:
            assert (dev(ctx, name, n).download((1 << n, 4)) == tab(name, n)).all(), f"{mode} 2^{n}: input table {name} was written"
    return got


def combos(n, tables):
    """every table with every challenge set at the small sizes; every table on random challenges + the all-M table on every set above"""
    if n <= CHECK_INPUT_UP_TO:
        return [(t, c) for t in tables for c in CHALS]
    return [(t, "rand") for t in tables] + [(tables[0], c) for c in CHALS[1:]]


# 2^1 and 2^6: one workgroup; 2^9 | 2^10 (product) and 2^10 | 2^11 (one table): the first multi-workgroup stage; 2^12, 2^13; the default
# plan's first pre-round / pass
SMALL = [1, 6, 9, 10, 11, 12, 13]
TABLES1 = ("M",) + tuple(t for t in EDGE_TABLES if t != "M") + ("nearM",)
PAIRS = (("M", "M"), ("lo0_hiM", "lo0_hiM"), ("lo0_hiM", "loM_hi0"), ("bit0_M", "bitmid_M"), ("bitmid_M", "bitmid_M"), ("zero", "M"),
         ("M", "rand"), ("lo0_hiM", "rand"), ("bitmid_M", "rand"))
G16 = dict(sc_local_g=16)


@pytest.mark.parametrize("n", SMALL + [19])
def test_extreme_plain(ctx, co, n):
    for t, c in combos(n, TABLES1):
        check(ctx, co, "plain", n, t, cname=c)


@pytest.mark.parametrize("n", SMALL + [19])
def test_extreme_product(ctx, co, n):
    for (f, g), c in combos(n, PAIRS):
        check(ctx, co, "product", n, f, g, c)


@pytest.mark.parametrize("n", SMALL + [19])
def test_extreme_fold(ctx, co, n):
    for t, c in combos(n, TABLES1):
        for npts in sorted({None, 1, n // 2, n - 1} - {0}, key=str):
            if npts is None or (npts < n and (n <= CHECK_INPUT_UP_TO or c == "rand")):
                check(ctx, co, "fold", n, t, cname=c, npts=npts)


@pytest.mark.parametrize("n", SMALL + [19])
def test_extreme_open(ctx, co, n):
    for t, c in combos(n, TABLES1):
        check(ctx, co, "open", n, t, cname=c)


@pytest.mark.parametrize("n", [16, 17, 18])
@pytest.mark.parametrize("mode", ["plain", "product", "fold", "open"])
def test_extreme_through_passes(ctx, co, mode, n):
    """sc_local_g = 16: the full three-stage plan (passes with the hand-over layout, a 16-workgroup stage, the tail) at 2^16 .. 2^18"""
    with sc_knobs(**G16):
        for t, c in combos(n, PAIRS if mode == "product" else TABLES1):
            f, g = t if mode == "product" else (t, None)
            check(ctx, co, mode, n, f, g, c)
            if mode == "fold" and c == "rand":
                check(ctx, co, mode, n, f, g, c, npts=n - 12)


def test_slices_closed_form(ctx, co):
    """challenges all 0: the fold is the low slice; all ONE: the high slice -- on a random table, directly and against the oracle"""
    for knobs in ({}, G16):
        with sc_knobs(**knobs):
            for n in (1, 6, 11, 13, 17):
                for k in sorted({1, n // 2, n}):
                    lo = check(ctx, co, "fold", n, "rand", cname="zero", npts=k)[0]
                    hi = check(ctx, co, "fold", n, "rand", cname="one", npts=k)[0]
                    assert (lo == tab("rand", n)[: 1 << (n - k)]).all() and (hi == tab("rand", n)[(1 << n) - (1 << (n - k)):]).all()
                _, v0 = check(ctx, co, "open", n, "rand", cname="zero")
                _, v1 = check(ctx, co, "open", n, "rand", cname="one")
                assert (v0 == tab("rand", n)[0]).all() and (v1 == tab("rand", n)[-1]).all()


@pytest.mark.parametrize("K,lo", sorted(BAND_CHAL))
def test_flat_bands(ctx, co, K, lo):
    """a flat pass of exactly K rounds whose outputs, before the conditional subtractions, lie in [lo r, 2 lo r): fold (full, and a
    partial fold that hands back the outputs of the pass as stored) and, for K <= 3, plain"""
    head = BAND_CHAL[(K, lo)]
    for mode, k, n, npts, knobs in BAND_CALLS:
        if k == K:
            with sc_knobs(**knobs):
                for t in ("M", "nearM"):
                    check(ctx, co, mode, n, t, head=head, npts=npts, what=f"band [{lo}r, {2 * lo}r)")


def test_column_carry_under_grid_stride(ctx, co):
    """k_plain_flat with one workgroup per CU at 2^20: every lane adds four elements to each 288-bit column sum, so a lane's OWN sum
    of stored values near r passes 2^256 (from the third on) and its ninth limb is live before the wave reduction"""
    with sc_knobs(sc_local_g=16, sc_plain_wg=1, sc_k0=2):
        for t in ("M", "nearM", "lo0_hiM"):
            check(ctx, co, "plain", 20, t)


def test_batch_of_extremes(ctx, co):
    """one zk_sumcheck_batch holding all four modes on extreme tables, sizes on both sides of every stage boundary, vs the oracle"""
    for knobs in ({}, G16, dict(G16, sc_pinned_out=0)):
        with sc_knobs(**knobs):
            reqs, want = [], []
            for i, n in enumerate((1, 6, 10, 11, 13, 16, 17, 18)):
                t, c = TABLES1[i % len(TABLES1)], CHALS[i % 4]
                f, g = PAIRS[i % len(PAIRS)]
                npts = n // 2 + 1
                reqs += [("plain", dev(ctx, t, n), 1 << n, chal(c, n)), ("product", dev(ctx, f, n), dev(ctx, g, n), 1 << n, chal(c, n)),
                         ("fold", dev(ctx, t, n), 1 << n, chal(c, n)[:npts]), ("open", dev(ctx, t, n), 1 << n, chal(c, n))]
                want += [reference(co, "plain", n, t, None, c), reference(co, "product", n, f, g, c),
                         reference(co, "fold", n, t, None, c, npts=npts), reference(co, "open", n, t, None, c)]
            got = ctx.sumcheck_batch(reqs)
            for r, g_, w in zip(reqs, got, want):
                L = r[3] if r[0] == "product" else r[2]
                if r[0] == "fold":
                    g_ = (g_.download(w[0].shape),)
                elif r[0] == "open":
                    g_ = (g_[0].download((L - 1, 4)) if L > 1 else w[0], g_[1])
                assert all((a == b).all() for a, b in zip(g_, w)), (knobs, r[0], L)


# ---- part B: every path of the planner ----
def _knob_values():
    from zkhip._lib import test_hooks

    lib, out = test_hooks(), {}
    for k in SC_DEFAULTS:
        v = ctypes.c_long(0)
        assert lib.zk_dbg_tune_get(k.encode(), ctypes.byref(v)) == 0
        out[k] = v.value
    return out


_CU = []


def _cu_count():
    """read from the device (the pass knobs are workgroups per CU): hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount = 63)"""
    if not _CU:
        v = ctypes.c_int(0)
        assert ctypes.CDLL("libamdhip64.so").hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0
        _CU.append(v.value)
    return _CU[0]


def _default_bits(ctx):
    return ctx.sumcheck_product(dev(ctx, "rand", 13), dev(ctx, "nearM", 13), 1 << 13, chal("rand", 13))


def _ids():
    out = []
    for tag, _k, mode, n, npts, _t in SC_PLAN_CASES:
        out.append(f"{tag}-{mode}-{n}" + (f"-{npts}" if npts is not None else ""))
    return out


@pytest.mark.parametrize("tag,knobs,mode,n,npts,plan", SC_PLAN_CASES, ids=_ids())
def test_plan_path(ctx, co, tag, knobs, mode, n, npts, plan):
    """the knob setting of the case (plan: see helpers.sc_plan_text) on random tables and on the all-M table; afterwards every knob
    is back and a default-plan call returns the bits it returned before"""
    assert _cu_count() == 256, "the plans of helpers.SC_PLAN_CASES are worked out for the 256 CUs of an MI355X"
    found, before = _knob_values(), _default_bits(ctx)
    with sc_knobs(**knobs):
        for f, g in ((("rand", "nearM"), ("M", "M")) if mode == "product" else (("rand", None), ("M", None))):
            check(ctx, co, mode, n, f, g, npts=npts, what=f"{tag} [{plan}]")
    assert _knob_values() == found
    assert all((a == b).all() for a, b in zip(_default_bits(ctx), before))


@pytest.mark.parametrize("n", [17, 18])
def test_t1_device_and_derived_agree_on_extremes(ctx, co, n):
    """the two sides of the derive threshold (2^18) of the default plan: t1 summed on the device and t1 derived on the host are the same bits"""
    for f, g in PAIRS:
        with sc_knobs(sc_t1_device=0):
            a = check(ctx, co, "product", n, f, g)
        with sc_knobs(sc_t1_device=1):
            b = check(ctx, co, "product", n, f, g)
        assert all((x == y).all() for x, y in zip(a, b))


def test_unhonourable_knob_is_refused(ctx):
    """sc_local_threads takes 256 or 1024: any other value used to run 1024 threads silently; now the call is refused, naming the knob,
    before anything is launched, and the ctx stays usable"""
    import zkhip

    before = _default_bits(ctx)
    for mode in ("plain", "product", "fold", "open"):
        with sc_knobs(sc_local_threads=512):
            with pytest.raises(zkhip.ZkError, match="sc_local_threads") as e:
                run(ctx, mode, 12, "rand", "rand", "rand")
            assert e.value.code == -1  # ZK_ERR_INVALID
            with pytest.raises(zkhip.ZkError, match="sc_local_threads"):
                ctx.sumcheck_batch([("plain", dev(ctx, "rand", 12), 1 << 12, chal("rand", 12))])
    assert all((a == b).all() for a, b in zip(_default_bits(ctx), before))
