"""
CPU: the references and the cases of tests/fr_vector_cases.py are worth trusting.

  * the Python-integer references agree with both oracles wherever those have the operation: fr_add / sub / mul / div and
    product_tree of the plain-C oracle, product_tree and PackedSharingParams.pack_from_public / unpack / unpack2 of the Python one
    (the transform map through the tables zkhip.pss hands to the library)
  * the transform map written from its definition agrees with the dense-matrix map for l = 1, 2, 4, and the tables built here from
    the header's definition are the tables the PSS callers build
  * the inputs are the edges they are named for: sums r - 1, r, r + 1, differences 0 and -1, the product of two r - 1, both as
    values and as stored integers; zero denominators at the ends of the chains the kernel walks; sizes on both sides of every
    launch boundary
"""
import numpy as np
import pytest

import fr_vector_cases as fc
import pyoracle as po

R = fc.R


def limbs(stored) -> np.ndarray:
    return np.frombuffer(fc.fr_bytes(stored), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4)]


def test_constants_and_conversions():
    assert R == po.R_MOD and fc.ROOT == po.FR_ROOT_OF_UNITY and fc.MONT == po.FR_R % R
    for v in fc.EDGE:
        assert po.fr_to_mont_limbs(v) == [int(x) for x in limbs([fc.to_mont(v)])[0]]
        assert fc.from_mont(fc.to_mont(v)) == v
    assert fc.fr_bytes([1, 1 << 64]) == (1).to_bytes(32, "little") + (1 << 64).to_bytes(32, "little")
    assert pow(fc.omega(512), 512, R) == 1 and pow(fc.omega(512), 256, R) == R - 1 and fc.omega(1) == 1 and fc.omega(2) == R - 1


def test_edge_values_are_edges():
    assert len(set(fc.EDGE)) == len(fc.EDGE) == 17 and all(0 <= e < R for e in fc.EDGE) and 0 not in fc.EDGE_NONZERO
    stored = {fc.to_mont(e) for e in fc.EDGE}
    assert R - 1 in stored and fc.MONT in stored                       # stored r - 1; the stored form of 1
    assert ((1 << 256) - 1) % R in fc.EDGE and (R - 1) // 2 + (R + 1) // 2 == R


def test_binary_pairs_hit_the_edges_of_the_reductions():
    pairs = fc.binary_pairs()
    assert len(pairs) == 2 * (17 * 17 + 4 * 17) and all(0 <= a < R and 0 <= b < R for a, b in pairs)
    for view in (lambda v: v, fc.to_mont):  # as values and as the stored integers the kernels add and subtract
        sums = {view(a) + view(b) for a, b in pairs}
        diffs = {view(a) - view(b) for a, b in pairs}
        assert {R - 1, R, R + 1, 0, 2 * R - 2} <= sums                  # the conditional subtraction on both sides of r, and the largest sum
        assert {0, -1, 1, R - 1, -(R - 1)} <= diffs                    # the borrow on both sides of 0, and the widest differences
        assert (R - 1, R - 1) in {(view(a), view(b)) for a, b in pairs}  # the largest product
        for e in fc.EDGE:  # every edge meets its complement, its complement +-1 and itself
            assert {(e, (R - e) % R), (e, (R - e + 1) % R), (e, (R - e - 1) % R), (e, e)} <= {(view(a), view(b)) for a, b in pairs}


def test_axpb_scalars():
    sc = fc.axpb_scalars()
    assert len(set(sc)) == 16 and {0, 1, R - 1} <= {a for a, _ in sc} and {a for a, _ in sc} == {b for _, b in sc}
    assert all(0 <= a < R and 0 <= b < R for a, b in sc)


def test_long_block():
    a, b = fc.long_block()
    pairs = fc.binary_pairs()
    assert len(a) == len(b) == fc.P_BLOCK == 4099 and all(fc.P_BLOCK % p for p in range(2, 65))
    assert list(zip(a, b))[: len(pairs)] == pairs and all(0 <= x < R for x in a + b)
    assert len(set(a[len(pairs):])) > 3000                             # the fill is not one value
    assert fc.tile([5, 6, 7], 7) == [5, 6, 7, 5, 6, 7, 5]


@pytest.mark.parametrize("cu", [256, 304, 64])
def test_grid_sizes_take_the_second_trip(cu):
    n = fc.n_grid(cu)
    full = fc.GRID_BLOCKS_PER_CU * fc.K_BLOCK * cu
    assert full < n < 2 * full and n % fc.K_BLOCK and fc.grid_sizes(cu) == [255, 256, 257, n]
    # the lanes that take a second trip: a whole workgroup and one lane of the next
    assert n - full == fc.K_BLOCK + 1


def test_elementwise_references_match_the_c_oracle():
    import coracle as co

    a, b = fc.long_block()
    a, b = a[:1200], b[:1200]
    A, B = limbs(map(fc.to_mont, a)), limbs(map(fc.to_mont, b))
    assert ints(co.fr_add(A, B)) == [fc.to_mont(v) for v in fc.ref_add(a, b)]
    assert ints(co.fr_sub(A, B)) == [fc.to_mont(v) for v in fc.ref_sub(a, b)]
    assert ints(co.fr_mul(A, B)) == [fc.to_mont(v) for v in fc.ref_mul(a, b)]
    for al, be in fc.axpb_scalars()[::5]:
        n = len(a)
        exp = co.fr_add(co.fr_add(A, co.fr_mul(np.tile(limbs([fc.to_mont(al)]), (n, 1)), B)), np.tile(limbs([fc.to_mont(be)]), (n, 1)))
        assert ints(exp) == [fc.to_mont(v) for v in fc.ref_axpb(a, b, al, be)]
        assert fc.ref_axpb(None, b, al, be) == fc.ref_axpb([0] * n, b, al, be)
    nz = [(x, y) for x, y in zip(a, b) if y]
    num, den = [x for x, _ in nz], [y for _, y in nz]
    assert ints(co.fr_div(limbs(map(fc.to_mont, num)), limbs(map(fc.to_mont, den)))) == [fc.to_mont(v) for v in fc.ref_div(num, den)]
    with pytest.raises(ZeroDivisionError):
        fc.ref_div([1, 2], [3, 0])


@pytest.mark.parametrize("N", [1, 2, 4, 8, 512, 1024])
def test_product_tree_reference_matches_both_oracles(N):
    import coracle as co

    x = fc.rand_vec(N, 40 + N)
    tree = fc.ref_product_tree(x)
    assert tree == po.product_tree(x)
    assert ints(co.product_tree(limbs(map(fc.to_mont, x)))) == [fc.to_mont(v) for v in tree]
    # the layout in words: level l at 2N - 2N/2^l, its entry i the product of entries 2i, 2i+1 of the level below; the header's
    # form tree[N + j] = tree[2j] tree[2j+1] is the same statement
    assert tree[:N] == x and tree[2 * N - 1] == 0
    for l in range(1, N.bit_length()):
        lo, up = fc.tree_level_offset(N, l - 1), fc.tree_level_offset(N, l)
        assert all(tree[up + i] == tree[lo + 2 * i] * tree[lo + 2 * i + 1] % R for i in range(N >> l))
    assert all(tree[N + j] == tree[2 * j] * tree[2 * j + 1] % R for j in range(N - 1))


def test_product_tree_closed_forms_and_launches():
    for N in (2, 4, 1024):
        for leaf in (2, R - 1):
            tree = fc.ref_product_tree([leaf] * N)
            exp = [None] * (2 * N)
            for off, cnt, v in fc.tree_const(N, leaf):
                exp[off:off + cnt] = [v] * cnt
            assert exp == tree
        assert all(v == 1 for _, _, v in fc.tree_const(N, R - 1)[1:-1])  # (r - 1)^2 = 1: level 1 on is all 1
        for j in fc.TREE_ZERO_AT:
            j = j % N
            tree = fc.ref_product_tree([0 if i == j else 1 for i in range(N)])
            assert {i for i, v in enumerate(tree) if v == 0} == fc.tree_one_zero(N, j) and set(tree) <= {0, 1}
    assert fc.ref_product_tree(list(range(1, 1025)))[2046] == fc.factorial_mod(1024)
    # what the sizes reach: one launch with one live lane; two full launches; a third launch that starts on a level of 2 entries
    assert fc.tree_launches(2) == [(0, 2, 1)] and fc.tree_launches(1024) == [(0, 1024, 9), (9, 2, 1)]
    assert fc.tree_launches(1 << 16) == [(0, 1 << 16, 9), (9, 128, 7)]
    assert fc.tree_launches(1 << 18) == [(0, 1 << 18, 9), (9, 512, 9)]
    assert fc.tree_launches(1 << 19) == [(0, 1 << 19, 9), (9, 1024, 9), (18, 2, 1)]
    assert all(N == 0 or N & (N - 1) for N in fc.TREE_REFUSED)


def test_deinterleave_and_matrix_references():
    t = fc.rand_vec(14, 3)
    ev, od = fc.ref_deinterleave(t)
    assert ev == [t[2 * i] for i in range(7)] and od == [t[2 * i + 1] for i in range(7)]
    M = [fc.rand_vec(3, 8 + r) for r in range(2)]
    v = fc.rand_vec(3, 20)
    assert fc.ref_apply_matrix(M, v) == [(M[r][0] * v[0] + M[r][1] * v[1] + M[r][2] * v[2]) % R for r in range(2)]


@pytest.mark.parametrize("n", fc.DIV_SIZES)
def test_div_cases(n):
    T = fc.div_threads(n)
    chains = [fc.div_chain(n, t) for t in range(T)]
    assert sorted(i for c in chains for i in c) == list(range(n)) and all(1 <= len(c) <= fc.DIV_CHUNK for c in chains)
    for kind in fc.DIV_DEN_KINDS:
        num, den = fc.div_case(n, kind)
        assert len(num) == len(den) == n and all(0 < d < R for d in den) and all(0 <= x < R for x in num)
        q = fc.ref_div(num, den)
        assert all(x * d % R == y for x, d, y in zip(q, den, num))
        if n >= 80 and kind == "edge":
            assert {(i % 5, d) for i, d in enumerate(den)} == {(k, d) for k in range(5) for d in fc.EDGE_NONZERO}
            assert all(q[i] == 1 for i in range(3, n, 5)) and all(q[i] == 0 for i in range(0, n, 5))
    assert {1, R - 1} <= set(fc.EDGE_NONZERO)


def test_div_sizes_and_zero_positions():
    assert {16 * 256 - 1, 16 * 256, 16 * 256 + 1} <= set(fc.DIV_SIZES)  # 255 lanes + a short one, one full workgroup, a second workgroup of one lane
    assert [fc.div_threads(n) for n in (4095, 4096, 4097)] == [256, 256, 257]
    assert any(len(fc.div_chain(n, fc.div_threads(n) - 1)) < fc.DIV_CHUNK for n in fc.DIV_SIZES)
    for n in fc.DIV_ZERO_SIZES:
        T, pos = fc.div_threads(n), fc.div_zero_positions(n)
        assert pos["first"] == [0] and pos["last"] == [n - 1] and pos["all"] == list(range(n))
        assert fc.div_chain(n, 0)[0] == 0 and fc.div_chain(n, 0)[1] == pos["second_pass_of_lane0"][0] == T
        assert pos["end_of_first_pass"] == [T - 1] == [fc.div_chain(n, T - 1)[0]]
        last = fc.div_chain(n, T - 1)
        assert len(last) < fc.DIV_CHUNK and pos["end_of_short_last_chain"] == [last[-1]] and last[-1] + T >= n
        assert all(0 <= i < n for p in pos.values() for i in p)
    big = fc.div_zero_positions(16 * 257 + 5)
    i = big["second_workgroup"][0]
    lane = i % fc.div_threads(16 * 257 + 5)
    assert lane // fc.K_BLOCK == 1 and i in fc.div_chain(16 * 257 + 5, lane)[1:] and "second_workgroup" not in fc.div_zero_positions(33)


# ---- the transform map ----
def _pss_tables(pp, kind):
    """(the tables zkhip.pss hands to zk_fr_ntt_map as integers, the same tables from the definition)"""
    t = pp.ntt_tables(kind)
    off = {"pack": pow(7, -1, R), "unpack": 7, "unpack2": 7}[kind]
    mine = fc.NttTables(t["A"], t["B"], off, t["n_in"], t["take"], t["step"])
    return t, mine


@pytest.mark.parametrize("l", [1, 2, 4])
def test_transform_map_matches_the_oracle_and_the_dense_map(l):
    from zkhip.pss import PackedSharingParams

    pp, opp = PackedSharingParams(l), po.PackedSharingParams(l)
    for kind, fn, mat, n_in in (("pack", opp.pack_from_public, [row[:l] for row in pp.pack_matrix], l),
                                ("unpack", opp.unpack, pp.unpack_matrix, pp.n), ("unpack2", opp.unpack2, pp.unpack2_matrix, pp.n)):
        t, mine = _pss_tables(pp, kind)
        for name in ("winv", "w", "scale"):  # the callers' tables ARE the header's definition
            assert [fc.from_mont(s) for s in ints(t[name])] == getattr(mine, name), (kind, name)
        assert mine.valid() and (mine.A, mine.B, mine.n_in) == (t["A"], t["B"], n_in)
        assert fc.ntt_dense_matrix(mine) == [[m % R for m in row] for row in mat], kind
        for seed in range(3):
            v = fc.rand_vec(n_in, 900 + 10 * l + seed)
            out = fc.ref_ntt_map(mine, v)
            assert out == fn(v) == fc.ref_apply_matrix(mat, v), (kind, seed)


def test_transform_map_is_two_dfts():
    """the reference against the textbook sums written out once more, on a pair with every parameter off its default"""
    t = fc.NttTables(8, 4, off=7, n_in=5, take=2, step=2)
    v = fc.rand_vec(5, 77)
    x = v + [0, 0, 0]
    wi = pow(fc.omega(8), -1, R)
    c = [sum(x[j] * pow(wi, i * j, R) for j in range(8)) * pow(8, -1, R) * pow(7, i, R) % R for i in range(8)][:4]
    e = [sum(c[i] * pow(fc.omega(4), i * r, R) for i in range(4)) % R for r in range(4)]
    assert fc.ref_ntt_map(t, v) == [e[0], e[2]]
    one = fc.NttTables(1, 1, off=5)  # the domain of one point: out = in * scale[0], and scale[0] = 1
    assert fc.ref_ntt_map(one, [12345]) == [12345] and one.winv == [1] and one.w == [1] and one.vpb() == 256


def test_transform_cases():
    assert set(fc.NTT_PAIRS) >= {(1, 1), (512, 512), (2, 512), (512, 2)}
    for A, B in fc.NTT_PAIRS:
        t = fc.NttTables(A, B, fc.ntt_offset(A, B))
        v = t.vpb()
        assert t.valid() and v == 256 // max(max(A, B) // 2, 1) and 0 not in fc.ntt_ks(t)
        assert set(fc.ntt_ks(t)) == {k for k in (1, v - 1, v, v + 1) if k}  # both sides of one workgroup's worth of vectors
        var = fc.ntt_variants(A, B)
        assert var[0] == (A, B, 1) and all(t.variant(*x).valid() for x in var) and len(set(var)) == len(var)
        assert {x[0] for x in var} == {A, max(A // 2, 1), 1}
        assert {(x[1], x[2]) for x in var} == {(B, 1), (1, 1)} | ({(B // 2, 2)} if B >= 2 else set())
        for kind in fc.INPUT_KINDS:
            for n_in in {x[0] for x in var}:
                vec = fc.ntt_input(kind, n_in, 5)
                assert len(vec) == n_in and all(0 <= x < R for x in vec)
        assert fc.ntt_input("random0", 1, 5) == fc.ntt_input("random0", A, 5)[:1] and fc.ntt_input("delta_last", A, 0)[-1] == 1
    assert 2 * 512 * 32 == 32768  # (512, .): one vector per workgroup, two buffers of 512 Fr
    for A, B, n_in, take, step, why in fc.NTT_REFUSED:
        t = fc.NttTables.__new__(fc.NttTables)
        t.A, t.B, t.n_in, t.take, t.step = A, B, n_in, take, step
        assert not t.valid(), why
