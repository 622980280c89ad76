"""
CPU proof that the scalars of tests/msm_digit_cases.py reach what they are named for, at every window width the library accepts:
c = 4..22 on the 256-bit layout (window tables, G2), c = 2..20 on the 129-bit layout of the two GLV halves.  The coverage table
(`msm_digit_cases.coverage`) is printed with `pytest -s`; tests/test_gpu_msm_digits.py runs the same cases on the device.
"""
import pytest

import msm_digit_cases as mc

LAYOUTS = [(c, mc.FULL_BITS, mc.R_MOD) for c in mc.TABLE_WIDTHS] + [(c, mc.ENDO_BITS, mc.LAMBDA) for c in mc.ENDO_WIDTHS]
IDS = [f"c{c}-bits{b}" for c, b, _ in LAYOUTS]


def test_layout_is_balanced_and_covers_the_bits():
    assert len(LAYOUTS) == 38
    for c, bits, _ in LAYOUTS:
        W, wd, off = mc.layout(c, bits)
        assert W == -(-bits // c) and sum(wd) == bits and max(wd) <= c and max(wd) - min(wd) <= 1
        assert off[0] == 0 and all(off[w + 1] == off[w] + wd[w] for w in range(W - 1))
        assert sorted(wd, reverse=True) == wd  # the wider windows come first: "narrow" windows are w >= rem


@pytest.mark.parametrize("c,bits,limit", LAYOUTS, ids=IDS)
def test_digits_rebuild_the_scalar_and_stay_in_range(c, bits, limit):
    W, wd, off = mc.layout(c, bits)
    fam = mc.families(c, bits, limit)
    assert set(fam) == set(mc.FAMILIES) | set(mc.SINGLES)
    assert fam["limit_minus_1"] == [(None, limit - 1)]
    for f, ms in fam.items():
        for w, k in ms:
            assert 0 <= k < limit
            tr, carry = mc.trace(k, c, bits)
            assert carry == 0, (f, w)  # no carry leaves the top window
            digits = mc.recode(k, c, bits)
            assert sum(d << o for d, o in zip(digits, off)) == k, (f, w)
            for x, (v, d, _) in enumerate(tr):
                assert -((1 << (wd[x] - 1)) - 1) <= d <= 1 << (wd[x] - 1), (f, w, x)
                assert 0 <= v <= 1 << wd[x]


@pytest.mark.parametrize("c,bits,limit", LAYOUTS, ids=IDS)
def test_no_family_loses_more_than_its_top_window_member(c, bits, limit):
    W, _, _ = mc.layout(c, bits)
    fam = mc.families(c, bits, limit)
    for f in mc.FAMILIES:
        lost = sorted(set(range(W)) - {w for w, _ in fam[f]})
        if (c, bits) == (2, 129) and f in ("half_plus_1", "ones", "low_ones"):
            # the one layout where the limit lambda (not 2^128) costs a second member: window 63 is bits 126..127, lambda's are
            # 0b10, so no half of a split scalar has the field 3 there -- these three members do not exist below lambda
            assert limit >> 126 == 2 and lost == [W - 2, W - 1], (f, lost)
        else:
            assert lost in ([], [W - 1]), (f, lost)
    for f in mc.SINGLES:
        # (the same field 3 in bits 126..127 puts all_half_plus_1 of that layout above lambda)
        assert len(fam[f]) == (0 if (c, bits, f) == (2, 129, "all_half_plus_1") else 1), f


@pytest.mark.parametrize("c,bits,limit", LAYOUTS, ids=IDS)
def test_coverage_table_has_no_empty_cell_below_the_top_window(c, bits, limit):
    W, wd, off = mc.layout(c, bits)
    cells = mc.coverage(c, bits, limit)
    may_be_empty = mc.top_window_cells(c, bits)
    # ... and a skip with a carry out needs the all-ones field: where that alone is >= the limit no scalar has it (the top window
    # always; window 63 of the 2-bit GLV layout too, see test_no_family_loses_more_than_its_top_window_member)
    unreachable = {f"skip_carry[{w}]" for w in range(1, W) if ((1 << wd[w]) - 1) << off[w] >= limit}
    assert unreachable - may_be_empty == ({"skip_carry[63]"} if (c, bits) == (2, 129) else set())
    may_be_empty |= unreachable
    print(f"\ncoverage c={c} bits={bits} W={W} widths={wd[0]}x{bits % W or W}+{wd[-1]}x{W - (bits % W or W)}")
    for cell, names in cells.items():
        print(f"  {cell:22s} {', '.join(names[:4])}{' ...' if len(names) > 4 else ''}{'' if names else '-'}")
        assert names or cell in may_be_empty, cell
    # the cells that must exist: every window's last bucket, every window's skip-with-carry but the first, every seam of the layout
    assert all(f"last_bucket[{w}]" in cells for w in range(W)) and all(f"skip_carry[{w}]" in cells for w in range(1, W))
    assert cells["carry_into_top"]
    for s in range(32, bits, 32):
        straddled = [w for w in range(W) if off[w] < s < off[w] + wd[w]]
        assert len(straddled) <= 1 and all(f"seam[{s}]@{w}" in cells for w in straddled)
    if 0 < bits % W < W - 1:
        assert cells["narrow_recentred"]
    # the top window's own edges come from the largest scalars: its digit for limit - 1 is the largest any scalar gives
    top = lambda k: mc.recode(k, c, bits)[W - 1]
    assert top(limit - 1) == max(top(k) for ms in mc.families(c, bits, limit).values() for _, k in ms) > 0


@pytest.mark.parametrize("c", list(mc.ENDO_WIDTHS))
def test_glv_pairs_are_split_back_into_their_halves(c):
    """every (k1, k2) pair is kept, k < r, and floor / remainder by lambda give the two members back"""
    fam = mc.families(c, mc.ENDO_BITS, mc.LAMBDA)
    glv = mc.glv_families(c)
    members = {k for ms in fam.values() for _, k in ms}
    seen1, seen2 = set(), set()
    for f, ms in glv.items():
        assert len(ms) == len(fam[f]), f  # no pair is lost: k1 < lambda, k2 < lambda => k < lambda^2 + lambda + 1 = r
        for (w, k), (w1, k1) in zip(ms, fam[f]):
            assert k < mc.R_MOD and mc.glv_split(k) == (k1, k // mc.LAMBDA) and k // mc.LAMBDA in members
            seen1.add(k1), seen2.add(k // mc.LAMBDA)
    assert seen1 == members
    for i, f in enumerate(mc.FAMILIES):  # as k2: every member whose window the family before it still has
        before = {w for w, _ in fam[mc.FAMILIES[i - 1]]}
        assert seen2 >= {k for w, k in fam[f] if w in before}, f


def test_expected_point_is_the_sum_of_the_srs_points():
    import pyoracle as po

    k0, k1 = 0x1234, 0x77
    sc = [3, 0, mc.R_MOD - 1, 1 << 200]
    acc = None
    for i, s in enumerate(sc):
        acc = po.g1_add(acc, po.g1_mul(po.g1_mul(po.G1_GEN, k0 + (5 + i) * k1), s))
    assert mc.expected_point(k0, k1, 5, sc) == acc


KNOBS = dict(msm_fused_min=10, msm_np=1024)


def test_planner_model_forced_knobs_take_the_fused_sort_on_every_width_12_to_22():
    """the knobs of the forced-plan GPU tests: what they make msm_enqueue choose, per width and item length"""
    for l2 in (64, -1):
        for spt in (0, 1):
            for c in range(12, 23):
                W = mc.layout(c, mc.FULL_BITS)[0]
                p = mc.table_plan(c, [2048, 64, 1], msm_l2_tiled=l2, msm_tab_spt=spt, **KNOBS)
                assert p["fused"] == 1 and p["np"] == 1024, (c, p)
                assert p["tab_c"] == (c if c >= 16 else 0), (c, p)
                assert p["spt"] == (1 if spt == 1 or W > 16 else 2)
                assert p["tiled_l2"] == 0  # 2048 scalars: W * 2048 / 1024 < 64 entries per partition at every width
                p = mc.table_plan(c, [1 << 14], msm_l2_tiled=l2, msm_tab_spt=spt, **KNOBS)
                assert p["fused"] == 1 and p["tiled_l2"] == (1 if l2 > 0 else 0), (c, p)  # 2^14 scalars: >= 192 per partition
                # the threshold itself: a family item padded so that its row reaches 2^10 entries
                short = -(-1024 // W)
                assert mc.table_plan(c, [short], msm_l2_tiled=l2, **KNOBS)["fused"] == 1
                assert mc.table_plan(c, [(1023 // W) & ~3], msm_l2_tiled=l2, **KNOBS)["fused"] == 0
            # 11 bits and below: 24+ windows (> kTabW) or fewer than 1024 buckets
            for c in range(4, 12):
                assert mc.table_plan(c, [2048], msm_l2_tiled=l2, msm_tab_spt=spt, **KNOBS)["fused"] == 0
    # a tiled level 2 on 2048-scalar items needs a lower threshold: 16 entries per partition
    for c in range(12, 23):
        assert mc.table_plan(c, [2048], msm_l2_tiled=16, **KNOBS)["tiled_l2"] == 1
    # the default plan keeps both off below 2^23 entries per row
    for c in mc.TABLE_WIDTHS:
        p = mc.table_plan(c, [1 << 14])
        assert p["fused"] == 0 and p["tiled_l2"] == 0
    # 16 / 17 and 20 / 21 share a layout (so recode_fixed<17> and <21> are the code of <16> and <20> under another name)
    assert mc.layout(16, 256) == mc.layout(17, 256) and mc.layout(20, 256) == mc.layout(21, 256)
    assert len({tuple(mc.layout(c, 256)[1]) for c in range(16, 23)}) == 5
    assert mc.layout(23, 256)[0] == 12 and mc.layout(24, 256)[0] == 11  # (instantiated, unreachable: precompute stops at 22)
