"""
Degenerate points and scalars for the G1 point maps and SRS builders of csrc/zk_srs.hip, with closed-form expectations.

Every input point is a*G with `a` known here, so every expected output is ONE scalar multiplication of the generator by an
integer computed in Python mod r.  Nothing below adds points: a case is a table of exponents (0 = the point at infinity, the
all-zero record) and a function that gives the exponent of every output.

    MapCase     zk_g1_apply_matrix      out[j*osv + r*osr] = sum_c M[r][c] * in[j*isv + c*isc]
    PackedCase  zk_srs_to_packed        on a level made by zk_srs_generate: level[i] = (k0 + i k1) G
    PowersCase  zk_srs_powers           level k, index j: E_k[j] * g, E_0 = [1], E_k = E_{k-1} (1 - s) ++ E_{k-1} s, s = s_{n-k}
    SeqCase     zk_srs_generate         P_i = (k0 + i k1) G

No GPU, no numpy, no zkhip: tests/test_g1_map_cases.py proves that every case has the property it is named for and that the
closed forms agree with the Python oracle's own additions; tests/test_gpu_g1_map_edges.py runs them on the device.
"""
import pyoracle as po

R = po.R_MOD
Q = po.Q_MOD
MONT_ONE = (1 << 256) % R          # the stored (Montgomery) form of 1: `one_m` of srs_powers
MONT_INV = pow(1 << 256, -1, R)
INV2 = pow(2, -1, R)
DECOY = 999331                     # the exponent of the points parked in the gaps of a strided input: read by mistake, they change the result
COLS = (1, 2, 8, 9, 13)            # below / at / above the `cols >= 8` switch of g1_apply_matrix_internal; 9 and 13: odd levels of the pair tree
EDGE_ENTRIES = (R - 1, 1 << 254, (1 << 32) - 1, 1 << 32, 1, 0, (1 << 64) - 1, 1 << 64, (1 << 224) + (1 << 31))


def _scalars(seed: int, n: int):
    return po.SplitMix64(seed).fr_vec(n)


def _small(j: int, c: int) -> int:
    """small distinct exponents: no two terms of one vector share a point"""
    return 1000 * (j + 1) + 17 * c + 3


class MapCase:
    def __init__(self, name, matrix, exps, prop, aim, isv=None, isc=1, osv=None, osr=1):
        self.name, self.matrix, self.exps, self.prop, self.aim = name, matrix, exps, prop, aim
        self.rows, self.cols, self.k = len(matrix), len(matrix[0]) if matrix else 0, len(exps)
        self.isv = self.cols if isv is None else isv
        self.isc = isc
        self.osv = self.rows if osv is None else osv
        self.osr = osr
        self.in_len = (self.k - 1) * self.isv + max(self.cols - 1, 0) * self.isc + 1
        self.out_len = (self.k - 1) * self.osv + (self.rows - 1) * self.osr + 1 + 2  # two records behind the last output stay guarded

    def knob_applies(self) -> bool:
        """whether g1_map_by_column chooses the form (g1_apply_matrix_internal: cols >= 8 && total < 16384 && total * cols <= 2^18)"""
        t = self.rows * self.k
        return self.cols >= 8 and t < 16384 and t * self.cols <= 1 << 18

    def in_slot(self, j, c):
        return j * self.isv + c * self.isc

    def out_slot(self, j, r):
        return j * self.osv + r * self.osr

    def in_exps(self):
        """exponent per input record; the records no (j, c) names hold DECOY * G"""
        buf = [DECOY] * self.in_len
        for j in range(self.k):
            for c in range(self.cols):
                buf[self.in_slot(j, c)] = self.exps[j][c] % R
        return buf

    def out_exp(self, j, r) -> int:
        return sum(m * a for m, a in zip(self.matrix[r], self.exps[j])) % R

    def expected(self):
        """{output record: exponent}; every other record of the output buffer must keep its guard bytes"""
        return {self.out_slot(j, r): self.out_exp(j, r) for j in range(self.k) for r in range(self.rows)}


def batch_lanes(total: int) -> int:
    """T of xyzz_to_affine_batch: lane t of k_batch_affine owns the outputs {t + i T}"""
    return max(1, (total + 63) // 64)


def map_cases():
    out = []
    small = lambda k, cols: [[_small(j, c) for c in range(cols)] for j in range(k)]
    for cols in COLS:
        full = lambda seed, cols=cols: _scalars(seed * 100 + cols, cols)
        out.append(MapCase(f"a1_zero_matrix_c{cols}", [[0] * cols for _ in range(2)], small(3, cols), ("zero_matrix",),
                           "g1_apply_matrix_internal top = -1: the ladders of k_g1_apply_matrix / k_g1_scale_cols run no step"))
        out.append(MapCase(f"a2_zero_row_c{cols}", [full(21), [0] * cols, full(22)], small(3, cols), ("zero_row", 1),
                           "k_g1_apply_matrix: a row whose bit test never fires, doublings of infinity only (xyzz30_dbl on infinity)"))
        out.append(MapCase(f"a3_bits01_c{cols}", [[(c + 1) % 2 for c in range(cols)], [1] * cols, [0] * (cols - 1) + [1]], small(3, cols), ("top_bit", 0),
                           "top = 0: one ladder step, xyzz30_madd onto infinity (the set branch) then generic additions"))
        rows7 = {1: 9, 2: 5}.get(cols, 3)
        m7 = [[EDGE_ENTRIES[(r * cols + c + (r if cols % 9 == 0 else 0)) % 9] for c in range(cols)] for r in range(rows7)]
        out.append(MapCase(f"a7_limb_edges_c{cols}", m7, small(2, cols), ("edge_entries",),
                           "the bit extraction Mr[c*8 + (b>>5)] >> (b&31) at bits 0, 31, 32, 63, 64, 224, 254 and all bits of r - 1"))
        inf = [[0] * cols,
               [0 if c == 0 else _small(1, c) for c in range(cols)],
               [0 if c == cols - 1 else _small(2, c) for c in range(cols)],
               [0 if c % 2 == 0 else _small(3, c) for c in range(cols)]]
        out.append(MapCase(f"a8_infinities_c{cols}", [full(81), full(82)], inf, ("infinity_slots",),
                           "xyzz30_madd's `aff30_is_inf(p)` return; in the column form infinite terms through xyzz30_add's first two lines"))
    for cols in (1, 9):
        out.append(MapCase(f"a8_all_infinity_c{cols}", [_scalars(8300 + cols, cols), _scalars(8400 + cols, cols)], [[0] * cols for _ in range(3)], ("all_outputs_zero",),
                           "k_batch_affine: the only lane owns only infinities, the prefix product stays 1 and f30_inv(1) is taken"))
    for cols in (2, 8, 9, 13):
        out.append(MapCase(f"a4_equal_points_c{cols}", [[1] * cols], [[4242 + 1000 * j] * cols for j in range(2)], ("equal_terms",),
                           "joint: set, then P + P in xyzz30_madd (same-x branch, xyzz30_dbl_affine), then generic; column form: P + P, 2P + 2P, "
                           "4P + 4P in xyzz30_add (same-x branch, xyzz30_dbl) with the copied odd term of k_xyzz_pair_sums added later"))
        pairs = [[(a if c % 2 == 0 else R - a) for c in range(cols) for a in [77 + 1000 * j + 13 * (c // 2)]] for j in range(2)]
        out.append(MapCase(f"a5_cancelling_pairs_c{cols}", [[1] * cols], pairs, ("cancelling_pairs",),
                           "xyzz30_madd / xyzz30_add same-x branch with R != 0: set_inf, then additions onto an infinite accumulator"))
    for name, row in (("a6_1_rm1", [1, R - 1]), ("a6_rm1_rm1_2", [R - 1, R - 1, 2])):
        for cols, front in ((len(row), 0), (8, 0), (9, 9 - len(row))):
            m = [0] * front + row + [0] * (cols - front - len(row))
            out.append(MapCase(f"{name}_c{cols}", [m], [[5151 + 1000 * j] * cols for j in range(2)], ("late_cancel",),
                               "a full 255-bit ladder on equal points whose sum is r P: the cancellation (xyzz30_madd same-x, R != 0) comes in the last "
                               "two steps of k_g1_apply_matrix; column form: (-P) + (-P) doubling and (-2P) + 2P cancellation in xyzz30_add"))
    # strides: 3 rows, 4 vectors
    for cols in (2, 9):
        m = [_scalars(9100 + 10 * cols + r, cols) for r in range(3)]
        e = small(4, cols)
        aim = "the index arithmetic j*isv + c*isc of k_g1_apply_matrix / k_g1_scale_cols and j*osv + r*osr of k_copy96_strided"
        for name, kw in (("in_vec_gaps", dict(isv=cols + 3)), ("in_comp_gaps", dict(isc=2, isv=2 * cols + 1)), ("comp_major", dict(isc=4, isv=1)),
                         ("out_row_major", dict(osv=1, osr=4)), ("out_vec_gaps", dict(osv=5)), ("out_row_gaps", dict(osv=1, osr=7)),
                         ("comp_major_out_gaps", dict(isc=4, isv=1, osv=6, osr=2))):
            out.append(MapCase(f"a9_{name}_c{cols}", m, e, ("strides",), aim, **kw))
    # counts: the lane guards t >= rows*k and T = ceil(total / 64) of k_batch_affine going 1 -> 2 -> 4 -> 5
    for rows, k in ((1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 256), (1, 257), (5, 13), (3, 85), (2, 128)):
        T = batch_lanes(rows * k)
        dead = (lambda j, T=T: j % T == 1) if T > 1 else (lambda j: j % 3 == 1)
        e = [[0 if dead(j) else 1 + (5 * j + 3 * c) % 97 for c in range(8)] for j in range(k)]
        m = [[(3 + 5 * r + 7 * c) % 16 + (1 << 200 if c == r else 0) for c in range(8)] for r in range(rows)]
        out.append(MapCase(f"a10_count_{rows}x{k}", m, e, ("inf_lane", T),
                           "`t >= rows*k` guards of all five kernels; k_batch_affine lanes that own only infinities next to lanes that own none"))
    out.append(MapCase("a11_no_columns", [[], []], [[], [], []], ("all_outputs_zero",), "cols = 0: g1_apply_matrix_ref's span and an empty ladder"))
    return out


class PackedCase:
    """zk_srs_to_packed(level, row, l) on level = zk_srs_generate(k0, k1, n): out[c] = sum_{j < min(l, n)} row[j] * level[c l + j]"""

    def __init__(self, name, k0, k1, n, l, row, prop, aim):
        self.name, self.k0, self.k1, self.n, self.l, self.row, self.prop, self.aim = name, k0, k1, n, l, row, prop, aim
        self.cols = min(l, n)
        self.count = 1 if n < l else n // l

    def level_exp(self, i):
        return (self.k0 + i * self.k1) % R

    def expected(self):
        return [sum(self.row[j] * self.level_exp(c * self.l + j) for j in range(self.cols)) % R for c in range(self.count)]


def packed_cases():
    out = []
    k0, k1 = _scalars(1201, 2)
    for n, l in ((1, 2), (3, 8), (5, 13), (9, 13)):
        out.append(PackedCase(f"a12_short_level_n{n}_l{l}", k0, k1, n, l, _scalars(1210 + l, l), ("short",),
                              "srs_to_packed: cols = min(l, n), one chunk; the level is zero-extended, the row's tail is not read"))
    for n, l, zeros in ((32, 2, (0,)), (32, 8, (1, 3, 4, 6)), (32, 13, (0, 12))):
        row = [0 if j in zeros else v for j, v in enumerate(_scalars(1220 + l, l))]
        out.append(PackedCase(f"a12_row_zeros_l{l}", k0, k1, n, l, row, ("row_zeros",), "columns whose ladder adds nothing; n % l != 0 drops the level's tail"))
    for l in (2, 8, 9, 13):
        out.append(PackedCase(f"a12_ones_equal_points_l{l}", k0, 0, 32, l, [1] * l, ("equal_terms",),
                              "all points of the level equal (step = infinity in fill_sequence_affine); same-x doublings as in a4"))
    return out


class PowersCase:
    def __init__(self, name, s, g_exp, prop, aim):
        self.name, self.s, self.g_exp, self.prop, self.aim = name, s, g_exp, prop, aim

    def exponents(self):
        """E_k for k = 0..n, in Fr (base 1)"""
        n, E, out = len(self.s), [1], [[1]]
        for k in range(1, n + 1):
            sv = self.s[n - k]
            E = [e * (1 - sv) % R for e in E] + [e * sv % R for e in E]
            out.append(E)
        return out

    def expected(self):
        """levels of exponents of G"""
        return [[e * self.g_exp % R for e in E] for E in self.exponents()]

    def choice(self, k, j):
        """the variables whose value (True) or complement (False) multiply into E_k[j]: bit (m - 1) of j chooses for s_{n-m}, m = 1..k"""
        n = len(self.s)
        return [(n - m, bool((j >> (m - 1)) & 1)) for m in range(1, k + 1)]


def powers_cases():
    out = []
    a, b = _scalars(1301, 2)
    fb = "k_fixed_base_mul: "
    out.append(PowersCase("b_edge_values", [0, 1, R - 1, INV2, (1 << 248) - 1], 1, ("edge_values",),
                          fb + "digits 0..30 = 0xff and digit 31 = 0 (level 1), exponents 0 and r - 1, whole sub-trees at infinity"))
    out.append(PowersCase("b_window31_byte", [7, 0x55 << 248], 1, ("single_byte", 31), fb + "31 skipped windows, then the table's last row: set from infinity at j = 31"))
    out.append(PowersCase("b_window0_byte", [7, 0xAB], 1, ("single_byte", 0), fb + "window 0 alone, 31 skipped windows after it"))
    for name, s, var, val in (("first_0", [0, a, b], 0, 0), ("last_0", [a, b, 0], 2, 0), ("first_1", [1, a, b], 0, 1), ("last_1", [a, b, 1], 2, 1)):
        out.append(PowersCase(f"b_s_{name}", s, 1, ("half_infinite", var, val),
                              "k_eq_expand with s or 1 - s = 0; srs_powers' host 1 - s: s = 0 no borrow and d = R, s = 1 gives d = 0; "
                              "k_fixed_base_mul on exponent 0 (no addition at all), k_batch_affine lanes of infinities"))
    out.append(PowersCase("b_no_variables", [], 1, ("nvars0",), "srs_powers with nvars = 0: one level of one point, no k_eq_expand"))
    out.append(PowersCase("b_custom_base", [a, R - 1, 0, b], 0xDEADBEEF, ("custom_base",), "build_fixed_base_table on a base other than the generator"))
    out.append(PowersCase("b_infinite_base", [a, b], 0, ("infinite_base",), "build_fixed_base_table with aff_inf(g): a table of infinities, every madd returns at once"))
    for name, sm in (("below_one", MONT_ONE - 1), ("above_one", MONT_ONE + 1), ("stored_max", R - 1), ("stored_1", 1)):
        out.append(PowersCase(f"b_mont_{name}", [a, sm * MONT_INV % R], 1, ("mont_form", sm),
                              "srs_powers' host subtraction one_m - s in Montgomery form: " + ("no borrow" if sm <= MONT_ONE else "borrow, + r")))
    return out


def seq_sizes(n: int):
    """the level sizes of fill_sequence_affine: n points <- their T starting points <- ... <- the first <= 1024 points from the host"""
    sizes = [n]
    while sizes[-1] > 1024:
        sizes.append(min(sizes[-1], max(1024, (sizes[-1] + 63) // 64)))
    return sizes


class SeqCase:
    def __init__(self, name, k0, k1, n, prop, aim, sample=None):
        self.name, self.k0, self.k1, self.n, self.prop, self.aim = name, k0 % R, k1 % R, n, prop, aim
        self.sample = sample  # indices checked (None: all)

    def exp(self, i):
        return (self.k0 + i * self.k1) % R

    def indices(self):
        return list(range(self.n)) if self.sample is None else self.sample


def _sample(n, special, seed):
    rng = po.SplitMix64(seed)
    idx = {0, n - 1}
    for i in special:
        idx.update(x for x in (i - 1, i, i + 1) if 0 <= x < n)
    want = len(idx) + 64
    while len(idx) < want:
        idx.add(rng.next() % n)
    return sorted(idx)


def seq_cases():
    out = []
    k0, k1 = _scalars(1401, 2)
    n = 3100  # [3100, 1024]: the host's 1024 points, lane t of k_seq_walk stores t, t + 1024, t + 2048 and, below 28, t + 3072
    host = "fill_sequence_affine's host chain (jac_add_mixed), k_aff_to_xyzz, "
    out.append(SeqCase("c_k0_zero", 0, k1, n, ("inf_at", [0]), host + "k_seq_walk lane 0 starts from infinity: set at 1024 (xyzz30_madd set branch), then stepT + stepT, the same-x doubling, at 2048"))
    out.append(SeqCase("c_k1_zero", k0, 0, n, ("constant",), "a step of infinity: stepT = (0, 0), every xyzz30_madd of k_seq_walk returns at once"))
    out.append(SeqCase("c_both_zero", 0, 0, n, ("all_zero",), "infinity + infinity everywhere; k_batch_affine lanes of infinities only"))
    out.append(SeqCase("c_k0_eq_k1", k1, k1, n, ("dbl_at", 1, 2047),
                       host + "doubling at 0 -> 1 (jac_add_mixed U2 == x); k_seq_walk lane 1023 holds 1024 k1 G = stepT: xyzz30_madd same-x, R = 0, at index 2047"))
    out.append(SeqCase("c_inf_at_5", -5 * k1, k1, n, ("inf_at", [5]), host + "cancellation and restart inside the host chain; lane 5 walks from infinity: set at 1029, same-x doubling at 2053"))
    out.append(SeqCase("c_inf_at_1029", -1029 * k1, k1, n, ("inf_at", [1029]),
                       "k_seq_walk lane 5 starts at -stepT: xyzz30_madd same-x, R != 0, stores infinity at 1029, the next step adds onto infinity at 2053, the one after doubles stepT at 3077"))
    for m in (1, 63, 64, 65, 1024, 1025):
        out.append(SeqCase(f"c_n{m}", 0, k1, m, ("inf_at", [0]), "sizes at the edges of k_batch_affine's T = ceil(n / 64) and of the host part (1025: one device step)"))
    n3 = 70000  # [70000, 1094, 1024]
    out.append(SeqCase("c_three_levels_k0_eq_k1", k1, k1, n3, ("dbl_at", 1, 2187), "two k_seq_walk levels; lane 1093 of the last holds 1094 k1 G = stepT: doubling at 2187",
                       sample=_sample(n3, (5, 1023, 1024, 1093, 1094, 2187, 1099, 2193, 3287), 1402)))
    out.append(SeqCase("c_three_levels_inf_at_1099", -1099 * k1, k1, n3, ("inf_at", [1099]), "lane 5 of the last level starts at -stepT: infinity at 1099, set at 2193, same-x doubling at 3287",
                       sample=_sample(n3, (5, 1023, 1024, 1093, 1094, 2187, 1099, 2193, 3287), 1403)))
    return out
