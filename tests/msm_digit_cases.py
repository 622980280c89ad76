"""
The MSM's scalar-to-bucket front end restated in big-int Python, and the scalars that sit on its edges.

csrc/zk_msm.hip recodes a scalar into signed window digits three times (recode_windows<NL> of k_digits; recode_all<0> and
recode_fixed<C, w> of the fused level-1 sort), all by one rule over the balanced layout of msm_layout:

    v = field(w) + carry;  v > 2^(cw-1): digit = v - 2^cw, carry out;  digit 0 is skipped (no bucket)

so a digit lies in [-(2^(cw-1) - 1), 2^(cw-1)] and bucket |digit| - 1 of a window of cw bits runs up to 2^(cw-1) - 1 = nb - 1.
Uniform scalars reach the ends of that range with probability 2^-cw per digit; the families below reach them in every window.

No GPU, no numpy: tests/test_msm_digit_inputs.py proves what the cases reach (the coverage table of `coverage`),
tests/test_gpu_msm_digits.py runs them through every path of the library against `expected_point`.
"""
import pyoracle as po

R_MOD = po.R_MOD
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF  # k = k1 + k2 * LAMBDA: the split of the table-less G1 path (glv_split)
FULL_BITS, ENDO_BITS = 256, 129  # kFullBits (window tables, G2), kEndoBits (the two halves of the split)
TABLE_WIDTHS = range(4, 23)      # zk_srs_precompute: msm_pick_window_full's floor .. kMaxTableBits
ENDO_WIDTHS = range(2, 21)       # zk_msm_set_window
assert (LAMBDA * LAMBDA + LAMBDA + 1) % R_MOD == 0


def layout(c: int, bits: int):
    """msm_layout: -> (W, [width of window w], [bit offset of window w]); the first `rem` windows are one bit wider"""
    W = (bits + c - 1) // c
    base, rem = bits // W, bits % W
    return W, [base + (1 if w < rem else 0) for w in range(W)], [w * base + min(w, rem) for w in range(W)]


def trace(k: int, c: int, bits: int):
    """-> ([(v, digit, carry_out) per window], carry out of the top window); digit 0 = skipped"""
    W, wd, off = layout(c, bits)
    carry, out = 0, []
    for w in range(W):
        cw = wd[w]
        v = ((k >> off[w]) & ((1 << cw) - 1)) + carry
        d, carry = (v - (1 << cw), 1) if v > (1 << (cw - 1)) else (v, 0)
        out.append((v, d, carry))
    return out, carry


def recode(k: int, c: int, bits: int):
    """the signed digits of k, lowest window first (0: the window is skipped)"""
    return [d for _, d, _ in trace(k, c, bits)[0]]


FAMILIES = ("half", "half_plus_1", "ones", "pow_minus_1", "low_ones", "pow")  # one member per window
SINGLES = ("all_half", "all_half_plus_1", "limit_minus_1", "limit_minus_2", "all_ones")


def families(c: int, bits: int, limit: int):
    """
    -> {family: [(w or None, scalar)]}, every scalar < limit (a member >= limit is left out, nothing else is).
      half          2^(cw-1) << off(w)        digit +2^(cw-1): the last bucket of window w, not recentred
      half_plus_1   (2^(cw-1) + 1) << off(w)  the smallest recentred value: digit -(2^(cw-1) - 1), carry into w + 1
      ones          (2^cw - 1) << off(w)      digit -1, carry
      pow_minus_1   2^off(w) - 1              -1 in window 0, v = 2^cw (skip, carry on) in windows 1 .. w-1, +1 in window w
      low_ones      2^(off(w) + cw) - 1       the same one window further, from the other side of the window's top bit
      pow           2^off(w)                  digit +1 alone: bucket 0
      all_half / all_half_plus_1              every window below the top at 2^(cw-1) / 2^(cw-1) + 1
      limit_minus_1, limit_minus_2, all_ones  the largest scalars: the top window's own edges
    """
    W, wd, off = layout(c, bits)
    fam = {f: [] for f in FAMILIES}
    for w in range(W):
        h, m = 1 << (wd[w] - 1), (1 << wd[w]) - 1
        fam["half"].append((w, h << off[w]))
        fam["half_plus_1"].append((w, (h + 1) << off[w]))
        fam["ones"].append((w, m << off[w]))
        fam["pow_minus_1"].append((w, (1 << off[w]) - 1))
        fam["low_ones"].append((w, (1 << (off[w] + wd[w])) - 1))
        fam["pow"].append((w, 1 << off[w]))
    fam["all_half"] = [(None, sum((1 << (wd[w] - 1)) << off[w] for w in range(W - 1)))]
    fam["all_half_plus_1"] = [(None, sum(((1 << (wd[w] - 1)) + 1) << off[w] for w in range(W - 1)))]
    fam["limit_minus_1"] = [(None, limit - 1)]
    fam["limit_minus_2"] = [(None, limit - 2)]
    ones = (1 << limit.bit_length()) - 1
    fam["all_ones"] = [(None, ones if ones < limit else ones >> 1)]
    return {f: [(w, k) for w, k in ms if k < limit] for f, ms in fam.items()}


def glv_families(c: int):
    """
    the table-less G1 path: -> {family: [(w or None, k)]} with k = k1 + k2 * LAMBDA, both halves members of families(c, 129, LAMBDA).
    k1 runs through the family; k2 is the member of the same window in the next family (so both halves of a scalar sit on different
    edges, and every member is a k1 once and a k2 once).  k1 < LAMBDA makes the split unique: the device sees exactly (k1, k2).
    """
    fam = families(c, ENDO_BITS, LAMBDA)
    out = {}
    for group in (FAMILIES, SINGLES):  # (the partner of a per-window family is a per-window family)
        for i, f in enumerate(group):
            other = dict(fam[group[(i + 1) % len(group)]])
            out[f] = []
            for w, k1 in fam[f]:
                k2 = other.get(w, fam["limit_minus_1"][0][1])  # (the partner lost this window's member: the largest half)
                k = k1 + k2 * LAMBDA
                if k1 < LAMBDA and k < R_MOD:
                    out[f].append((w, k))
    return out


def glv_split(k: int):
    return k % LAMBDA, k // LAMBDA


def seams(c: int, bits: int):
    """[(32-bit seam, window)] for every window whose field has bits on both sides of a limb boundary"""
    W, wd, off = layout(c, bits)
    return [(s, w) for s in range(32, bits, 32) for w in range(W) if off[w] < s < off[w] + wd[w]]


def coverage(c: int, bits: int, limit: int):
    """
    the coverage table of one width: {cell: [names of the cases that reach it]}.  Cells:
      last_bucket[w]   digit +2^(cw-1) in window w (bucket nb - 1 of a row as wide as the window)
      skip_carry[w]    v == 2^cw in window w >= 1: the digit is skipped and the carry goes on
      carry_into_top   a carry enters the top window
      seam[s]@w        a recentred digit in window w, whose field straddles bit s = 32 j
      narrow_recentred a recentred digit in the first window that is one bit narrower (w = rem), if the layout is uneven
    A cell of the top window can only be filled by limit_minus_1, limit_minus_2, all_ones or all_half (no family member with
    a set top bit is below the limit): those cells may stay empty.
    """
    W, wd, off = layout(c, bits)
    base, rem = bits // W, bits % W
    cells = {f"last_bucket[{w}]": [] for w in range(W)}
    cells.update({f"skip_carry[{w}]": [] for w in range(1, W)})
    cells["carry_into_top"] = []
    cells.update({f"seam[{s}]@{w}": [] for s, w in seams(c, bits)})
    if 0 < rem < W:
        cells["narrow_recentred"] = []
    for f, ms in families(c, bits, limit).items():
        for mw, k in ms:
            name = f if mw is None else f"{f}[{mw}]"
            tr, _ = trace(k, c, bits)
            for w, (v, d, carry) in enumerate(tr):
                if d == 1 << (wd[w] - 1):
                    cells[f"last_bucket[{w}]"].append(name)
                if w >= 1 and v == 1 << wd[w]:
                    cells[f"skip_carry[{w}]"].append(name)
                if d < 0:
                    for s, sw in seams(c, bits):
                        if sw == w:
                            cells[f"seam[{s}]@{w}"].append(name)
                    if w == rem and 0 < rem < W:
                        cells["narrow_recentred"].append(name)
            if W >= 2 and tr[W - 2][2]:
                cells["carry_into_top"].append(name)
    return cells


def top_window_cells(c: int, bits: int):
    """the cells of `coverage` that belong to the top window (the named exception to 'no empty cell')"""
    W, _, _ = layout(c, bits)
    rem = bits % W
    top = {f"last_bucket[{W - 1}]", f"skip_carry[{W - 1}]"} | {f"seam[{s}]@{w}" for s, w in seams(c, bits) if w == W - 1}
    if rem == W - 1:
        top.add("narrow_recentred")
    return top


def expected_scalar(k0: int, k1: int, offset: int, scalars) -> int:
    return sum(s * (k0 + (offset + i) * k1) for i, s in enumerate(scalars)) % R_MOD


def expected_point(k0: int, k1: int, offset: int, scalars):
    """the MSM of `scalars` over the synthetic SRS P_i = (k0 + i k1) G from `offset` on: one scalar multiplication, no MSM code"""
    return po.g1_mul(po.G1_GEN, expected_scalar(k0, k1, offset, scalars))


# ---- the planner's conditions for the sort of a window-table class, restated from msm_enqueue ----
K_TAB_W, K_MAX_PARTS, K_MAX_LOW, K_SORT_THREADS, K_L2_TILE = 22, 1024, 2048, 1024, 16 * 1024
TAB_WIDTHS_KNOWN = tuple(range(16, 25))  # ZK_TAB_WIDTHS (23, 24: instantiated, but zk_srs_precompute stops at 22)


def table_plan(c: int, lens, msm_fused_min=0, msm_l2_tiled=0, msm_np=0, msm_tab_spt=0):
    """
    one class of window-table items of `lens` scalars on a c-bit table -> dict(fused, tab_c, tiled_l2, np, row_len, spt): what
    the msm_debug line of msm_enqueue prints for it (fused: k_tab_hist / k_tab_scatter; tab_c: the compile-time layout of
    recode_fixed, 0 = recode_all<0>; tiled_l2: k_l2_* instead of k_part_sort)
    """
    W, wd, _ = layout(c, FULL_BITS)
    cmax = max(wd)
    nb = 1 << (cmax - 1)
    ns = max((n + 3) & ~3 for n in lens)
    row_len, rows = W * ns, len(lens)
    want = 256
    while want < K_MAX_PARTS and row_len // want > 16384:
        want <<= 1
    if msm_np:
        want = msm_np
    while want < K_MAX_PARTS and nb // want > K_MAX_LOW:
        want <<= 1
    np_ = min(nb, want)
    low_bits = 0
    while (np_ << low_bits) < nb:
        low_bits += 1
    fused = W <= K_TAB_W and np_ == K_MAX_PARTS and msm_fused_min >= 0 and row_len >= 1 << (msm_fused_min if msm_fused_min > 0 else 23)
    tab_c, spt = 0, 2
    if fused:
        spt = 1 if (W > 16 or msm_tab_spt == 1) else 2
        tab_c = c if c in TAB_WIDTHS_KNOWN else 0  # (recode_fixed<c> derives its layout from c as msm_layout does)
        nch = -(-ns // (spt * K_SORT_THREADS))
        if rows * np_ * nch > 64 << 20:
            fused = False
    tiled = msm_l2_tiled >= 0 and row_len // np_ >= (msm_l2_tiled if msm_l2_tiled > 0 else 8192) and (msm_l2_tiled > 0 or row_len >= 1 << 23)
    if tiled and rows * (row_len // K_L2_TILE + np_) * (1 << low_bits) > 64 << 20:
        tiled = False
    return dict(fused=int(fused), tab_c=tab_c if fused else 0, tiled_l2=int(tiled), np=np_, row_len=row_len, spt=spt)
