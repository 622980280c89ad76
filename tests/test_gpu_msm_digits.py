"""
GPU: the scalars of tests/msm_digit_cases.py -- every window at the edges of the signed recoding (last bucket, skip with a carry,
carries across limb seams, the narrow windows of an uneven layout) -- through every front end of the MSM in csrc/zk_msm.hip:
recode_windows<8> (window tables, default plan; G2), recode_all<0> and recode_fixed<C> (fused level 1, forced by knobs and
asserted from the msm_debug line), recode_windows<5> (the two GLV halves of the table-less path), behind them both level-2 sorts.

The reference is a closed form: the SRS is P_i = (k0 + i k1) G, so an MSM is ONE scalar multiplication of the generator by
sum s_i (k0 + (offset + i) k1) mod r (msm_digit_cases.expected_point) -- no MSM code on the reference side.  What the cases
reach is proved on the CPU by tests/test_msm_digit_inputs.py.
"""
import re

import numpy as np
import pytest

import msm_digit_cases as mc
import pyoracle as po
from helpers import jac_norm_to_affine, pt_ints, rand_fr

pytestmark = pytest.mark.gpu

N_SRS, N_CAT = 4096, 2048
K0, K1 = 0x1F3D5B79A2C4E6081357, 0x2B7E151628AED2A6ABF7158809CF4F3C
FORCED = dict(msm_fused_min=10, msm_np=1024)  # + msm_l2_tiled, msm_tab_spt: the knobs of test_round6_sort_kernels_on_small_ragged_batches


def to_mont(ints) -> np.ndarray:
    return np.array([po.fr_to_mont_limbs(v) for v in ints], dtype=np.uint64).reshape(-1, 4)


@pytest.fixture(scope="module")
def ctx():
    """
    this file's own zk_ctx, closed when the file is done.  Batches of a dozen items on 20..22-bit windows need ~2^21 buckets per
    item: ~10 GiB of bucket arenas, which a ctx keeps at their high-water mark.  The session's ctx must not carry that through
    the rest of the suite (the n = 24 proof of test_host_cpp.py runs in a process of its own next to it and needs the memory).
    """
    import gc

    import zkhip

    c = zkhip.Ctx(0)
    yield c
    gc.collect()
    c.close()


@pytest.fixture(scope="module")
def env(ctx):
    """one synthetic SRS with known discrete logs (once without, once with a window table), its points, one random tail"""
    fill = rand_fr(N_CAT, 4242)
    e = dict(plain=ctx.srs_generate(K0, K1, N_SRS), tab=ctx.srs_generate(K0, K1, N_SRS), fill=fill,
             fill_ints=[po.fr_from_mont_limbs(x) for x in fill])
    e["bases"] = e["plain"].download()
    yield e
    e["plain"].free(), e["tab"].free()


def build_items(fam, pad_to=0):
    """-> [(name, offset, [scalars])]: one item per family, each at its own offset into the SRS; pad_to: zero scalars appended"""
    items, off = [], 5
    for f, ms in fam.items():
        if not ms:
            continue
        sc = [k for _, k in ms]
        sc += [0] * max(0, pad_to - len(sc))
        items.append((f, off, sc))
        off += len(sc) + 3
    assert off <= N_SRS
    return items


def cat_item(fam, env):
    """all families concatenated and filled up with uniform scalars to N_CAT -> (name, offset, ints), Montgomery limbs"""
    sc = [k for ms in fam.values() for _, k in ms]
    assert len(sc) <= N_CAT
    m = to_mont(sc)
    ints = sc + env["fill_ints"][len(sc):]
    limbs = np.concatenate([m, env["fill"][len(sc):]]) if len(sc) else env["fill"].copy()
    return ("all", 1001, ints), limbs


def run_batch(ctx, srs, items, limbs=None):
    """items [(name, offset, ints)] as ONE batch on `srs` -> [affine point as ints or None]"""
    bufs = [ctx.to_device(limbs[i] if limbs and limbs[i] is not None else to_mont(sc)) for i, (_, _, sc) in enumerate(items)]
    got = ctx.msm_g1_batch([srs] * len(items), bufs, [len(sc) for _, _, sc in items], offsets=[o for _, o, _ in items])
    return [pt_ints(jac_norm_to_affine(g)) for g in got]


class Expected:
    """expected_point per (offset, scalars), computed once per width and shared by the plans that run the same items"""

    def __init__(self):
        self.memo = {}

    def __call__(self, off, sc):
        key = (off, len(sc), hash(tuple(sc)))
        if key not in self.memo:
            self.memo[key] = mc.expected_point(K0, K1, off, sc)
        return self.memo[key]


def class_lines(err: str):
    """the zk-class lines of msm_enqueue (msm_debug) -> [dict of their integer fields]"""
    return [{k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)} for ln in err.splitlines() if ln.startswith("zk-class")]


class knobs:
    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        try:
            for k, v in self.kv.items():
                self.ctx.dbg_tune(k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.dbg_tune(k, 0)  # (0 is the default of every knob used here)
        return False


def check_families(ctx, co, env, srs, c, fam, exp, what, with_oracle=True):
    """the families as one batch (one item each) plus the concatenated item; every item against the closed form"""
    items = build_items(fam)
    cat, cat_limbs = cat_item(fam, env)
    got = run_batch(ctx, srs, items + [cat], [None] * len(items) + [cat_limbs])
    for (name, off, sc), g in zip(items + [cat], got):
        assert g == exp(off, sc), f"{what}: width {c}, family {name}"
    if with_oracle:
        o = cat[1]
        assert got[-1] == pt_ints(co.msm_g1(env["bases"][o : o + N_CAT].copy(), cat_limbs)), f"{what}: width {c}, concatenated item vs the C oracle"


@pytest.mark.parametrize("c", list(mc.TABLE_WIDTHS))
def test_window_table_default_plan(ctx, co, env, c):
    """recode_windows<8> -> k_part_* -> k_part_sort: every table width the library accepts"""
    env["tab"].precompute(c)
    assert env["tab"].table_window == c
    check_families(ctx, co, env, env["tab"], c, mc.families(c, mc.FULL_BITS, mc.R_MOD), Expected(), "window table, default plan")


@pytest.mark.parametrize("c", list(range(12, 23)))
def test_window_table_fused_sort_forced(ctx, co, env, c, capfd):
    """
    k_tab_hist / k_tab_scatter on small rows: recode_all<0> for 12..15, recode_fixed<c> for 16..22, with one and two scalars per
    thread, k_part_sort (msm_l2_tiled 64 and -1: 2048-scalar rows stay below 64 entries per partition) and the tiled k_l2_*
    (msm_l2_tiled 16) behind it.  The path is asserted from the msm_debug line against the planner model.
    """
    W = mc.layout(c, mc.FULL_BITS)[0]
    fam = mc.families(c, mc.FULL_BITS, mc.R_MOD)
    env["tab"].precompute(c)
    exp = Expected()
    cat, cat_limbs = cat_item(fam, env)
    padded = build_items(fam, pad_to=-(-1024 // W))  # rows of just >= 2^10 entries: the threshold of msm_fused_min = 10
    for l2 in (64, -1, 16):
        for spt in (0, 1):
            kn = dict(FORCED, msm_l2_tiled=l2, msm_tab_spt=spt)
            with knobs(ctx, msm_debug=1, **kn):
                capfd.readouterr()
                got_cat = run_batch(ctx, env["tab"], [cat], [cat_limbs])
                line_cat = class_lines(capfd.readouterr().err)
                got = run_batch(ctx, env["tab"], padded)
                line_fam = class_lines(capfd.readouterr().err)
            what = f"fused sort forced (l2_tiled={l2}, tab_spt={spt})"
            for lines, lens in ((line_cat, [N_CAT]), (line_fam, [len(sc) for _, _, sc in padded])):
                want = mc.table_plan(c, lens, **kn)
                assert len(lines) == 1 and lines[0]["key_c"] == c and lines[0]["items"] == len(lens), (what, lines)
                assert {k: lines[0][k] for k in ("fused", "tab_c", "tiled_l2", "np")} == {k: want[k] for k in ("fused", "tab_c", "tiled_l2", "np")}, (what, c, lines[0], want)
                assert want["fused"] == 1 and want["tab_c"] == (c if c >= 16 else 0)
            assert line_cat[0]["tiled_l2"] == (1 if l2 == 16 else 0)
            assert got_cat[0] == exp(cat[1], cat[2]), f"{what}: width {c}, concatenated item"
            for (name, off, sc), g in zip(padded, got):
                assert g == exp(off, sc), f"{what}: width {c}, family {name}"


@pytest.mark.parametrize("c", [16, 20])
@pytest.mark.parametrize("rec", [96, 128])
def test_both_table_record_layouts(ctx, co, env, c, rec, capfd):
    env["tab"].precompute(c, record_bytes=rec)
    assert env["tab"].table_record == rec and env["tab"].table_window == c
    fam = mc.families(c, mc.FULL_BITS, mc.R_MOD)
    exp = Expected()
    check_families(ctx, co, env, env["tab"], c, fam, exp, f"{rec}-byte records, default plan")
    with knobs(ctx, msm_debug=1, msm_l2_tiled=16, **FORCED):
        capfd.readouterr()
        check_families(ctx, co, env, env["tab"], c, fam, exp, f"{rec}-byte records, fused sort forced", with_oracle=False)
        lines = class_lines(capfd.readouterr().err)
    assert len(lines) == 1 and (lines[0]["fused"], lines[0]["tab_c"], lines[0]["tiled_l2"]) == (1, c, 1), lines


_alone_done = set()


@pytest.mark.parametrize("c", list(mc.ENDO_WIDTHS))
def test_table_less_glv_path(ctx, co, env, c):
    """recode_windows<5> on both halves of k = k1 + k2 lambda, per-window rows (narrow rows for uneven layouts), every width"""
    fam = mc.glv_families(c)
    ctx.msm_set_window(c)
    try:
        check_families(ctx, co, env, env["plain"], c, fam, Expected(), "table-less GLV path")
    finally:
        ctx.msm_set_window(0)
    # one scalar at a time at the library's own width: the point itself, not a sum (a scalar checked for another width is not repeated)
    for f, ms in fam.items():
        for w, k in ms:
            if k in _alone_done:
                continue
            _alone_done.add(k)
            off = (k % 4093) + 1
            got = pt_ints(jac_norm_to_affine(ctx.msm_g1(env["plain"], ctx.to_device(to_mont([k])), 1, offset=off)))
            assert got == mc.expected_point(K0, K1, off, [k]), f"alone: width {c}, family {f}[{w}] = {hex(k)}"


def test_g2_per_window_rows(ctx):
    """recode_windows<8> with a bucket row per window (G2 has no split): the library's width, two forced widths, one window table"""
    from test_gpu_g2 import _aff, _seq

    n = 512
    k0, k1 = 0x5A17C3, 0x10F2E9D
    srs = ctx.srs_register_g2(_seq(n, k0, k1))
    fill = rand_fr(n, 4343)
    fill_ints = [po.fr_from_mont_limbs(x) for x in fill]

    def run(c, tag, batch):
        fam = mc.families(c, mc.FULL_BITS, mc.R_MOD)
        sc = [k for ms in fam.values() for _, k in ms][:n]
        sc = sc + fill_ints[len(sc):]
        items = [("all", 0, sc)]
        if batch:
            off = 1
            for f, ms in fam.items():
                items.append((f, off, [k for _, k in ms][: n - off]))
                off += 7
        bufs = [ctx.to_device(to_mont(s)) for _, _, s in items]
        if batch:
            got = ctx.msm_g2_batch([srs] * len(items), bufs, [len(s) for _, _, s in items], offsets=[o for _, o, _ in items])
        else:
            got = [ctx.msm_g2(srs, bufs[0], n)]
        for (name, off, s), g in zip(items, got):
            assert _aff(g) == po.g2_mul(po.G2_GEN, mc.expected_scalar(k0, k1, off, s)), f"G2 {tag}: width {c}, family {name}"

    c_def = ctx.lib.zk_msm_window(n)
    run(c_def, "table-less, the library's width", batch=False)  # (a single MSM: a batch would quantise the width)
    for c in (9, 13):  # uneven 256-bit layouts: 29 windows of 9 / 8 bits, 20 windows of 13 / 12 bits
        ctx.msm_set_window(c)
        try:
            run(c, "table-less, forced width", batch=True)
        finally:
            ctx.msm_set_window(0)
    srs.precompute(0)
    run(srs.table_window, "window table", batch=True)
    srs.free()


@pytest.fixture(scope="module")
def big(ctx):
    n = 1 << 14
    s = ctx.srs_generate(K0 + 1, K1 + 2, n)
    yield s, n
    s.free()


@pytest.mark.parametrize("c", [14, 17, 22])
def test_bucket_extremes_at_size(ctx, big, c, capfd):
    """
    2^14 scalars that put everything into the buckets at the ends: every window's last bucket (all_half), bucket 0 of one window
    (2^off(w): first, first narrow, top window), and half_w / ones_w alternating over the windows (the last bucket without a sign
    next to bucket 0 with a sign and a carry) -- default plan, and fused level 1 with the tiled level 2.  Closed form only.
    """
    srs, n = big
    srs.precompute(c)
    W, wd, off = mc.layout(c, mc.FULL_BITS)
    rem = mc.FULL_BITS % W
    fam = mc.families(c, mc.FULL_BITS, mc.R_MOD)
    half, ones = dict(fam["half"]), dict(fam["ones"])
    cases = {"all_half": [fam["all_half"][0][1]] * n}
    for w in sorted({0, rem if 0 < rem < W else W // 2, W - 1}):
        cases[f"pow[{w}]"] = [1 << off[w]] * n
    cases["half/ones alternating"] = [(half if i % 2 == 0 else ones)[(i // 2) % (W - 1)] for i in range(n)]
    k0, k1 = K0 + 1, K1 + 2
    s1 = n * k0 + k1 * (n * (n - 1) // 2)  # sum (k0 + i k1)
    for name, sc in cases.items():
        e = (sc[0] * s1 if name != "half/ones alternating" else sum(s * (k0 + i * k1) for i, s in enumerate(sc))) % mc.R_MOD
        want = po.g1_mul(po.G1_GEN, e)
        d = ctx.to_device(to_mont(sc[:1]).repeat(n, axis=0) if name != "half/ones alternating" else to_mont(sc))
        assert pt_ints(jac_norm_to_affine(ctx.msm_g1(srs, d, n))) == want, f"default plan: width {c}, {name}"
        kn = dict(FORCED, msm_l2_tiled=64)
        with knobs(ctx, msm_debug=1, **kn):
            capfd.readouterr()
            got = pt_ints(jac_norm_to_affine(ctx.msm_g1(srs, d, n)))
            lines = class_lines(capfd.readouterr().err)
        p = mc.table_plan(c, [n], **kn)
        assert p["fused"] == 1 and p["tiled_l2"] == 1
        assert len(lines) == 1 and (lines[0]["fused"], lines[0]["tab_c"], lines[0]["tiled_l2"]) == (1, p["tab_c"], 1), lines
        assert got == want, f"forced plan: width {c}, {name}"
