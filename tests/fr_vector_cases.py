"""
Edge values, launch-boundary sizes and references for the Fr vector kernels at the bottom of csrc/zk_fr.hip:

    zk_fr_add / sub / mul   out[i] = a[i] op b[i]
    zk_fr_axpb              out[i] = a[i] + alpha b[i] + beta      (a = NULL: alpha b + beta, what fr_scale calls)
    zk_fr_batch_div         out[i] = num[i] / den[i]               (Montgomery's trick over the strided chains of k_batch_div)
    zk_product_tree         level l >= 1 at tree[2N - 2N/2^l ...), N/2^l entries; level 0 = the leaves; tree[2N-1] = 0
    zk_fr_deinterleave      even[i] = t[2i], odd[i] = t[2i+1]
    zk_fr_apply_matrix      out[r] = sum_c M[r][c] in[c]
    zk_fr_ntt_map           c = IDFT_A(in zero-padded); c[i] *= scale[i]; e = DFT_B(c zero-padded); out[r] = e[r step]

Everything here is a Python integer mod r: no numpy, no zkhip, neither oracle.  A reference takes and returns FIELD VALUES; what a
kernel reads is the stored (Montgomery) form v 2^256 mod r, which `to_mont` / `fr_bytes` produce.  The Montgomery map is a
bijection of [0, r), so a list of stored integers s is fed to a kernel as the values `from_mont(s)`: every edge below is used both
as a value and as a stored integer (`stored_twin`), because it is the STORED integers that meet the carries and the conditional
subtractions of the kernels.

tests/test_fr_vector_cases.py checks these references against both oracles and that the cases are the edges they are named for;
tests/test_gpu_fr_vector_edges.py runs them on the device.
"""
import random

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MONT = (1 << 256) % R              # R mod r: the stored form of 1
MONT_INV = pow(1 << 256, -1, R)
TWO_ADICITY = 32
ROOT = pow(7, (R - 1) >> TWO_ADICITY, R)   # a 2^32-th root of unity (7 generates Fr*)
K_BLOCK = 256                      # lanes per workgroup of every kernel here
GRID_BLOCKS_PER_CU = 8             # grid_for(): at most 8 * cu_count workgroups, the lanes stride over the rest
DIV_CHUNK = 16                     # kDivChunk: elements per lane of k_batch_div
TREE_LEVELS = 9                    # levels one k_tree launch builds
P_BLOCK = 4099                     # prime: a tiled block never lines up with a wave, a workgroup or the grid


def to_mont(v: int) -> int:
    return v * MONT % R


def from_mont(s: int) -> int:
    return s * MONT_INV % R


def fr_bytes(stored) -> bytes:
    """stored integers -> the 32-byte little-endian records a kernel reads (np.frombuffer(.., '<u8').reshape(-1, 4))"""
    return b"".join(int(s).to_bytes(32, "little") for s in stored)


def mont_bytes(values) -> bytes:
    return fr_bytes(to_mont(v) for v in values)


# ---- references (field values in, field values out) ----
def ref_add(a, b):
    return [(x + y) % R for x, y in zip(a, b)]


def ref_sub(a, b):
    return [(x - y) % R for x, y in zip(a, b)]


def ref_mul(a, b):
    return [x * y % R for x, y in zip(a, b)]


def ref_axpb(a, b, alpha, beta):
    """a + alpha b + beta; a = None is the kernel's null-a branch"""
    if a is None:
        return [(alpha * y + beta) % R for y in b]
    return [(x + alpha * y + beta) % R for x, y in zip(a, b)]


def ref_div(num, den):
    """per element num * den^(r-2): no shared inversion, so no chain of the kernel's is restated"""
    if any(d % R == 0 for d in den):
        raise ZeroDivisionError("zero denominator")
    return [n * pow(d, R - 2, R) % R for n, d in zip(num, den)]


def ref_product_tree(x):
    """2N entries: the leaves, then level l = 1 .. log2 N at offset 2N - 2N/2^l, each the products of the pairs of the level below; last entry 0"""
    N = len(x)
    assert N >= 1 and N & (N - 1) == 0
    tree, level = list(x), list(x)
    while len(level) > 1:
        level = [level[2 * i] * level[2 * i + 1] % R for i in range(len(level) // 2)]
        tree += level
    assert len(tree) == 2 * N - 1
    return tree + [0]


def tree_level_offset(N: int, l: int) -> int:
    return 0 if l == 0 else 2 * N - ((2 * N) >> l)


def tree_launches(N: int):
    """[(in_level, in_len, levels)] of product_tree(): what each k_tree launch starts from and how far it goes"""
    out, lvl, ln, total = [], 0, N, N.bit_length() - 1
    while lvl < total:
        k = min(TREE_LEVELS, total - lvl)
        out.append((lvl, ln, k))
        lvl, ln = lvl + k, ln >> k
    return out


def ref_deinterleave(t):
    return list(t[0::2]), list(t[1::2])


def ref_apply_matrix(M, vec):
    return [sum(m * v for m, v in zip(row, vec)) % R for row in M]


def omega(n: int) -> int:
    """the primitive n-th root of unity every radix-2 domain of size n uses"""
    assert n >= 1 and n & (n - 1) == 0 and n <= 1 << TWO_ADICITY
    return pow(ROOT, (1 << TWO_ADICITY) // n, R)


class NttTables:
    """
    the arguments of zk_fr_ntt_map from the definition in include/zkhip.h: winv = A/2 powers of omega_A^-1, w = B/2 powers of omega_B
    (one entry where the domain has fewer than two points: the caller's arrays are never empty), scale[i] = A^-1 off^i, i < min(A, B)
    """

    def __init__(self, A, B, off=1, n_in=None, take=None, step=1):
        self.A, self.B, self.off = A, B, off % R
        self.n_in = A if n_in is None else n_in
        self.take = B if take is None else take
        self.step = step
        self.wA, self.wB = omega(A), omega(B)
        wi = pow(self.wA, -1, R)
        self.pa = [pow(wi, i, R) for i in range(A)]          # every power of omega_A^-1 and of omega_B: the sums below index them
        self.pb = [pow(self.wB, i, R) for i in range(B)]
        self.winv, self.w = self.pa[: max(A // 2, 1)], self.pb[: max(B // 2, 1)]
        ainv = pow(A, -1, R)
        self.scale = [ainv * pow(self.off, i, R) % R for i in range(min(A, B))]

    def variant(self, n_in=None, take=None, step=None):
        t = NttTables.__new__(NttTables)
        t.__dict__.update(self.__dict__)
        t.n_in = self.n_in if n_in is None else n_in
        t.take = self.take if take is None else take
        t.step = self.step if step is None else step
        return t

    def valid(self) -> bool:
        """what fr_ntt_map accepts"""
        p2 = lambda x: x >= 1 and x & (x - 1) == 0
        return p2(self.A) and p2(self.B) and self.A <= 512 and self.B <= 512 and self.n_in <= self.A and (self.take - 1) * self.step < self.B

    def vpb(self) -> int:
        """vectors per workgroup of k_fr_ntt_map"""
        return K_BLOCK // max(max(self.A, self.B) // 2, 1)


def ntt_coeffs(t: NttTables, vec):
    """the min(A, B) scaled coefficients: two dense sums straight from the definition, O(A n_in)"""
    A, keep = t.A, min(t.A, t.B)
    x = [v % R for v in vec[: t.n_in]]
    pa = t.pa
    nz = [(j, v) for j, v in enumerate(x) if v]
    return [sum(v * pa[(i * j) % A] for j, v in nz) % R * t.scale[i] % R for i in range(keep)]


def ntt_eval(t: NttTables, c):
    """out[r] = sum_i c[i] omega_B^(i r step), r < take: O(take min(A, B))"""
    B, pb = t.B, t.pb
    nz = [(i, v) for i, v in enumerate(c) if v]
    return [sum(v * pb[(i * r * t.step) % B] for i, v in nz) % R for r in range(t.take)]


def ref_ntt_map(t: NttTables, vec):
    return ntt_eval(t, ntt_coeffs(t, vec))


def ntt_dense_matrix(t: NttTables):
    """the take x n_in matrix of the same map: column c is the image of the c-th unit vector"""
    cols = [ref_ntt_map(t, [1 if k == c else 0 for k in range(t.n_in)]) for c in range(t.n_in)]
    return [[cols[c][r] for c in range(t.n_in)] for r in range(t.take)]


# ---- case lists ----
EDGE = [
    0, 1, 2, R - 1, R - 2,
    (R - 1) // 2, (R + 1) // 2,
    (1 << 32) - 1, 1 << 32,
    (1 << 64) - 1, 1 << 64,
    1 << 128, 1 << 254,
    MONT, MONT * MONT % R,            # the Montgomery constants R mod r and R^2 mod r as plain values
    (R - 1) * MONT_INV % R,           # the value whose stored form is r - 1
    ((1 << 256) - 1) % R,             # 0xFFFFFFFF in every 32-bit limb, reduced
]
EDGE_NONZERO = [e for e in EDGE if e]


def _plain_pairs():
    pairs = [(a, b) for a in EDGE for b in EDGE]
    for a in EDGE:  # what the cross product misses: a + b = r, r + 1, r - 1 and a - b = 0 for EVERY a
        pairs += [(a, (R - a) % R), (a, (R - a + 1) % R), (a, (R - a - 1) % R), (a, a)]
    return pairs


def stored_twin(pairs):
    """the pairs whose STORED forms are the given integers"""
    return [(from_mont(a), from_mont(b)) for a, b in pairs]


def binary_pairs():
    """(a, b) as field values: EDGE x EDGE and the complements, once as values and once as stored integers"""
    p = _plain_pairs()
    return p + stored_twin(p)


def axpb_scalars(seed: int = 11):
    """(alpha, beta), all 16 combinations of {0, 1, r - 1, one random value}"""
    x = random.Random(seed).randrange(3, R - 1)
    s = (0, 1, R - 1, x)
    return [(al, be) for al in s for be in s]


def rand_vec(n: int, seed: int):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


def long_block(seed: int = 1):
    """(a, b): P_BLOCK rows, the binary pairs first, uniform rows behind them.  A test computes its reference ONCE on the block;
    row i of a long vector is row i mod P_BLOCK of the block (`tile_index`)"""
    pairs = binary_pairs()
    assert len(pairs) < P_BLOCK
    fill = P_BLOCK - len(pairs)
    a = [p[0] for p in pairs] + rand_vec(fill, 2 * seed)
    b = [p[1] for p in pairs] + rand_vec(fill, 2 * seed + 1)
    return a, b


def tile(block, n: int):
    return [block[i % len(block)] for i in range(n)]


def grid_sizes(cu: int):
    """element-wise lengths around the launch boundaries: one workgroup -1/0/+1 and a full grid + one workgroup + one lane"""
    return [K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, n_grid(cu)]


def n_grid(cu: int) -> int:
    return GRID_BLOCKS_PER_CU * K_BLOCK * cu + K_BLOCK + 1


# ---- zk_fr_batch_div ----
DIV_SIZES = [1, 2, 15, 16, 17, 31, 33, 16 * 256 - 1, 16 * 256, 16 * 256 + 1, 16 * 257 + 5]
DIV_DEN_KINDS = ("edge", "ones", "minus_ones")


def div_threads(n: int) -> int:
    return (n + DIV_CHUNK - 1) // DIV_CHUNK


def div_chain(n: int, t: int):
    """the indices lane t of k_batch_div owns, in the order it walks them"""
    T = div_threads(n)
    return [t + k * T for k in range(DIV_CHUNK) if t + k * T < n]


def div_case(n: int, den_kind: str, seed: int = 5):
    """(num, den): the numerator of row i is 0, 1, r - 1, its own denominator or uniform by i mod 5 (5 and the 16 edge denominators
    are coprime: every pairing turns up within 80 rows)"""
    rnd = rand_vec(n, seed + n)
    if den_kind == "edge":
        den = [EDGE_NONZERO[i % len(EDGE_NONZERO)] for i in range(n)]
    elif den_kind == "ones":
        den = [1] * n
    elif den_kind == "minus_ones":
        den = [R - 1] * n
    else:
        raise ValueError(den_kind)
    num = [(0, 1, R - 1, den[i], rnd[i])[i % 5] for i in range(n)]
    return num, den


def div_zero_positions(n: int):
    """{name: indices of the zero denominators}: the ends of the first chain, the second pass of lane 0, the short last chain, a lane
    of the second workgroup, everything.  Positions a size does not have are left out."""
    T = div_threads(n)
    last = div_chain(n, T - 1)
    pos = {"first": [0], "last": [n - 1], "end_of_first_pass": [T - 1], "all": list(range(n))}
    if T < n:
        pos["second_pass_of_lane0"] = [T]
    if len(last) < DIV_CHUNK:
        pos["end_of_short_last_chain"] = [last[-1]]
    if T > K_BLOCK:
        pos["second_workgroup"] = [K_BLOCK + 1 + T]  # lane 257, its second element
    return pos


DIV_ZERO_SIZES = [33, 16 * 257 + 5]


# ---- zk_product_tree ----
TREE_SIZES = [2, 4, 512, 1024, 1 << 18, 1 << 19]
TREE_REFUSED = [0, 3, 1000]
TREE_ZERO_AT = [0, 511, 512, -1]   # -1: the last leaf


def tree_const(N: int, leaf: int):
    """all leaves equal: level l holds leaf^(2^l) everywhere -> [(offset, count, value)] per level, then the closing 0"""
    out = [(tree_level_offset(N, l), N >> l, pow(leaf, 1 << l, R)) for l in range(N.bit_length())]
    return out + [(2 * N - 1, 1, 0)]


def tree_one_zero(N: int, j: int):
    """leaves 1 except a zero at j: -> the set of tree positions holding 0 (the ancestors j >> l, and the last entry); all others hold 1"""
    return {tree_level_offset(N, l) + (j >> l) for l in range(N.bit_length())} | {2 * N - 1}


def factorial_mod(n: int) -> int:
    f = 1
    for i in range(2, n + 1):
        f = f * i % R
    return f


# ---- zk_fr_ntt_map ----
NTT_PAIRS = [(1, 1), (1, 8), (8, 1), (2, 512), (512, 2), (512, 512), (256, 512), (64, 16)]
NTT_REFUSED = [  # (A, B, n_in, take, step, why)
    (1024, 8, 8, 8, 1, "A above 512"),
    (24, 8, 8, 8, 1, "A no power of two"),
    (8, 8, 9, 8, 1, "n_in = A + 1"),
    (8, 8, 8, 5, 2, "(take - 1) step = B"),
]
INPUT_KINDS = ("zero", "delta_first", "delta_last", "minus_ones", "random0", "random1")


def ntt_offset(A: int, B: int) -> int:
    """the coset factor of a pair: g^-1 upwards (pack), g downwards (unpack), 1 between equal domains and another value at (1, 1)"""
    if A == B:
        return 1 if A > 1 else 5
    return pow(7, -1, R) if A < B else 7


def ntt_ks(t: NttTables):
    v = t.vpb()
    return sorted({k for k in (1, v - 1, v, v + 1) if k > 0})


def ntt_variants(A: int, B: int):
    """[(n_in, take, step)]: the full map, then each parameter moved alone, then all three at their smallest"""
    n_ins = sorted({A, max(A // 2, 1), 1}, reverse=True)
    sels = [(B, 1)] + ([(B // 2, 2)] if B >= 2 else []) + ([(1, 1)] if B > 1 else [])
    out = [(A, B, 1)]
    out += [(n, B, 1) for n in n_ins[1:]]
    out += [(A, tk, st) for tk, st in sels[1:]]
    if len(n_ins) > 1 and len(sels) > 1:
        out += [(n_ins[-1], sels[-1][0], sels[-1][1]), (n_ins[1], sels[1][0], sels[1][1])]
    seen, uniq = set(), []
    for v in out:
        if v not in seen:
            seen.add(v)
            uniq.append(v)
    return uniq


def ntt_input(kind: str, n_in: int, seed: int):
    if kind == "zero":
        return [0] * n_in
    if kind == "delta_first":
        return [1] + [0] * (n_in - 1)
    if kind == "delta_last":
        return [0] * (n_in - 1) + [1]
    if kind == "minus_ones":
        return [R - 1] * n_in
    if kind in ("random0", "random1"):
        return rand_vec(512, seed + int(kind[-1]))[:n_in]  # a prefix of ONE vector per pair: a test can share its reference
    raise ValueError(kind)
