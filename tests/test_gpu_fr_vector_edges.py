"""
GPU: the Fr vector kernels at the bottom of csrc/zk_fr.hip on the cases of tests/fr_vector_cases.py -- edge values as field values
and as stored integers, lengths on both sides of every launch boundary, and every refusal.  The references are the Python-integer
ones of that module (tests/test_fr_vector_cases.py checks them against both oracles); every comparison is bit-exact on Montgomery
limbs.  What is reached here and nowhere else in the per-kernel tests:

    k_fr_binary / k_fr_axpb / k_fr_deinterleave    the second trip of the grid-stride loop (n_grid = 8 * 256 * CU + 257 rows)
    k_fr_axpb                                      the null-a branch (fr_scale) on scalars 0, 1, r - 1; output = input
    k_batch_div                                    n = 16 * 256 -1/0/+1, short last chains, zeros at the chain ends, the flag after a zero
    k_tree                                         a full second launch (2^18), a third launch on a level of 2 (2^19), one live lane (2, 4)
    k_fr_ntt_map                                   domains 1 and 512, k on both sides of one workgroup's vectors, n_in < A, the refusals
    k_fr_apply_matrix                              zero, delta and r - 1 inputs, strided both ways
"""
import numpy as np
import pytest

import fr_vector_cases as fc

pytestmark = pytest.mark.gpu

R = fc.R
GUARD = np.array([0xA5A5A5A5DEADBEEF, 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x5A5A5A5AFEEDFACE], dtype=np.uint64)  # >= 2^255: no Fr


def S(stored) -> np.ndarray:
    """stored integers -> limbs [n, 4]"""
    return np.frombuffer(fc.fr_bytes(stored), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def L(values) -> np.ndarray:
    """field values -> Montgomery limbs [n, 4]"""
    return S(fc.to_mont(v) for v in values)


def guards(n: int) -> np.ndarray:
    return np.tile(GUARD, (n, 1))


@pytest.fixture(scope="module")
def cu():
    """the device's CU count as torch reports it, asked in a child process once per run of this file: torch brings its own copy of
    the HIP runtime, and importing it here would put a second runtime under every later test of the session"""
    import subprocess
    import sys

    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    n = int(out.stdout.split()[-1])
    assert 1 <= n <= 4096
    return n


@pytest.fixture(scope="module")
def blk():
    """the block of the long-vector generator and every element-wise reference on it, computed once"""
    a, b = fc.long_block()
    d = dict(a=a, b=b, A=L(a), B=L(b), pairs=len(fc.binary_pairs()))
    d["add"], d["sub"], d["mul"] = L(fc.ref_add(a, b)), L(fc.ref_sub(a, b)), L(fc.ref_mul(a, b))
    return d


@pytest.fixture(scope="module")
def long_vec(ctx, cu, blk):
    """the block tiled to n_grid rows, on the device once; a shorter test vector is a prefix of it"""
    n = fc.n_grid(cu)
    full = fc.GRID_BLOCKS_PER_CU * fc.K_BLOCK * cu
    assert n > full and n % fc.K_BLOCK != 0  # the lanes of the first 257 rows take a second trip; the length is no multiple of a workgroup
    idx = np.arange(n) % fc.P_BLOCK
    hA, hB = blk["A"][idx], blk["B"][idx]
    return dict(n=n, idx=idx, hA=hA, hB=hB, dA=ctx.to_device(hA), dB=ctx.to_device(hB), sizes=[blk["pairs"]] + fc.grid_sizes(cu))


def run_guarded(ctx, n, call):
    """run call(out) on a buffer of n rows and two guard rows behind them -> the n rows; the guard rows must survive"""
    out = ctx.to_device(guards(n + 2))
    call(out)
    got = out.download((n + 2, 4))
    assert (got[n:] == GUARD).all(), "wrote past the end of the output"
    return got[:n]


# ---- add / sub / mul / axpb / scale ----
@pytest.mark.parametrize("op", ["add", "sub", "mul"])
def test_binary_edges_and_grid_stride(ctx, blk, long_vec, op):
    """the edge pairs at their own length, one workgroup -1/0/+1, and a length that sends 257 lanes round the grid-stride loop again"""
    fn = getattr(ctx, "fr_" + op)
    lv = long_vec
    for n in lv["sizes"]:
        got = run_guarded(ctx, n, lambda out: fn(lv["dA"], lv["dB"], n, out=out))
        exp = blk[op][lv["idx"][:n]]
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, (op, n, bad[:8])
    assert (lv["dA"].download((lv["n"], 4)) == lv["hA"]).all() and (lv["dB"].download((lv["n"], 4)) == lv["hB"]).all()  # inputs untouched


def test_axpb_and_scale_every_scalar_pair(ctx, blk, long_vec):
    """a + alpha b + beta with alpha, beta in {0, 1, r - 1, random}^2, with a given and through fr_scale's null a (beta = 0 there: the
    four alphas), at every length of the element-wise tests"""
    lv = long_vec
    a, b = blk["a"], blk["b"]
    for al, be in fc.axpb_scalars():
        exp_blk = L(fc.ref_axpb(a, b, al, be))
        m_al, m_be = S([fc.to_mont(al)])[0], S([fc.to_mont(be)])[0]
        for n in lv["sizes"]:
            got = run_guarded(ctx, n, lambda out: ctx.fr_axpb(lv["dA"], lv["dB"], m_al, m_be, n, out=out))
            assert (got == exp_blk[lv["idx"][:n]]).all(), (hex(al), hex(be), n)
        # a = NULL with this beta, through the C entry point (fr_scale fixes beta = 0)
        exp_null = L(fc.ref_axpb(None, b, al, be))
        for n in lv["sizes"]:
            got = run_guarded(ctx, n, lambda out: ctx._check(ctx.lib.zk_fr_axpb(ctx.h, 0, lv["dB"].ptr, m_al.ctypes.data, m_be.ctypes.data, out.ptr, n)))
            assert (got == exp_null[lv["idx"][:n]]).all(), ("null a", hex(al), hex(be), n)
        if be == 0:
            for n in lv["sizes"]:
                got = run_guarded(ctx, n, lambda out: ctx.fr_scale(lv["dB"], m_al, n, out=out))
                assert (got == exp_null[lv["idx"][:n]]).all(), ("scale", hex(al), n)
    assert (lv["dA"].download((lv["n"], 4)) == lv["hA"]).all() and (lv["dB"].download((lv["n"], 4)) == lv["hB"]).all()


def test_elementwise_output_may_be_an_input(ctx, blk, long_vec):
    """
    Aliasing IS in use: zkhip/serialize.py converts a freshly uploaded table in place with fr_scale(buf, R^2, n, out=buf) (out = b of
    zk_fr_axpb).  include/zkhip.h therefore states that d_out may be d_a or d_b of the five element-wise calls, and this test holds
    them to it: out = a and out = b for add / sub / mul / axpb, out = b for scale, on 257 rows and on the length that takes the
    second grid-stride trip (a lane must have read row i of both inputs before it stores row i, on every trip).
    """
    lv = long_vec
    al, be = fc.axpb_scalars()[-1]  # both random
    m_al, m_be = S([fc.to_mont(al)])[0], S([fc.to_mont(be)])[0]
    exp = dict(add=blk["add"], sub=blk["sub"], mul=blk["mul"], axpb=L(fc.ref_axpb(blk["a"], blk["b"], al, be)),
               scale=L(fc.ref_axpb(None, blk["b"], al, 0)))
    calls = dict(add=lambda a, b, n, out: ctx.fr_add(a, b, n, out=out), sub=lambda a, b, n, out: ctx.fr_sub(a, b, n, out=out),
                 mul=lambda a, b, n, out: ctx.fr_mul(a, b, n, out=out), axpb=lambda a, b, n, out: ctx.fr_axpb(a, b, m_al, m_be, n, out=out),
                 scale=lambda a, b, n, out: ctx.fr_scale(b, m_al, n, out=out))
    for n in (fc.K_BLOCK + 1, lv["n"]):
        want = {k: v[lv["idx"][:n]] for k, v in exp.items()}
        for op, call in calls.items():
            for alias in ("a", "b"):
                if op == "scale" and alias == "a":
                    continue
                # two guard rows behind the aliased operand: they are part of neither the input nor the output
                x = ctx.to_device(np.concatenate([lv["hA" if alias == "a" else "hB"][:n], guards(2)]))
                call(x if alias == "a" else lv["dA"], x if alias == "b" else lv["dB"], n, x)
                got = x.download((n + 2, 4))
                assert (got[:n] == want[op]).all() and (got[n:] == GUARD).all(), (op, alias, n)
    assert (lv["dA"].download((lv["n"], 4)) == lv["hA"]).all() and (lv["dB"].download((lv["n"], 4)) == lv["hB"]).all()


# ---- deinterleave ----
def test_deinterleave_lengths_and_guards(ctx, cu, long_vec):
    """even / odd rows of the tiled block at n = 1, 255, 256, 257 and n_grid; nothing behind either output is touched"""
    lv = long_vec
    for n in [1] + fc.grid_sizes(cu):
        m = 2 * n
        t = np.concatenate([lv["hA"], lv["hB"]])[:m] if m > lv["n"] else lv["hA"][:m]
        d_t = ctx.to_device(t)
        even, odd = ctx.to_device(guards(n + 2)), ctx.to_device(guards(n + 2))
        ctx._check(ctx.lib.zk_fr_deinterleave(ctx.h, d_t.ptr, even.ptr, odd.ptr, n))
        ge, go = even.download((n + 2, 4)), odd.download((n + 2, 4))
        assert (ge[:n] == t[0::2]).all() and (go[:n] == t[1::2]).all(), n
        assert (ge[n:] == GUARD).all() and (go[n:] == GUARD).all(), n
        assert (d_t.download((m, 4)) == t).all()


# ---- batch division ----
@pytest.mark.parametrize("n", fc.DIV_SIZES)
def test_batch_div_sizes_and_edge_operands(ctx, n):
    """every size around a chunk and around a workgroup of lanes; denominators from the edge list, all 1, all r - 1; numerators 0, 1,
    r - 1, the denominator itself, random.  The reference inverts every denominator on its own (d^(r-2))."""
    for kind in fc.DIV_DEN_KINDS:
        num, den = fc.div_case(n, kind)
        hn, hd = L(num), L(den)
        dn, dd = ctx.to_device(hn), ctx.to_device(hd)
        got = run_guarded(ctx, n, lambda out: ctx.fr_batch_div(dn, dd, n, out=out))
        exp = L(fc.ref_div(num, den))
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, (n, kind, bad[:8])
        assert (dn.download((n, 4)) == hn).all() and (dd.download((n, 4)) == hd).all()


@pytest.mark.parametrize("n", fc.DIV_ZERO_SIZES)
def test_batch_div_zero_denominators(ctx, n):
    """a zero at each end of a chain, in the short last chain, in the second workgroup, everywhere: ZeroDivisionError, inputs intact,
    and the very next call on the same ctx divides exactly (the flag is cleared per call)"""
    num, den = fc.div_case(n, "edge")
    hn, exp = L(num), L(fc.ref_div(num, den))
    dn, d_good = ctx.to_device(hn), ctx.to_device(L(den))
    pos = fc.div_zero_positions(n)
    assert set(pos) >= {"first", "last", "end_of_first_pass", "second_pass_of_lane0", "end_of_short_last_chain", "all"}
    assert ("second_workgroup" in pos) == (n > fc.DIV_CHUNK * fc.K_BLOCK)
    for name, where in pos.items():
        bad_den = list(den)
        for i in where:
            bad_den[i] = 0
        hd = L(bad_den)
        dd = ctx.to_device(hd)
        out = ctx.to_device(guards(n + 2))
        with pytest.raises(ZeroDivisionError):
            ctx.fr_batch_div(dn, dd, n, out=out)
        assert (dn.download((n, 4)) == hn).all() and (dd.download((n, 4)) == hd).all(), name
        assert (out.download((n + 2, 4))[n:] == GUARD).all(), name
        got = run_guarded(ctx, n, lambda o: ctx.fr_batch_div(dn, d_good, n, out=o))
        assert (got == exp).all(), ("after", name)


def test_batch_div_refuses_aliasing_and_accepts_nothing(ctx):
    from zkhip._lib import ZK_ERR_INVALID

    n = 100
    num, den = fc.div_case(n, "edge")
    hn, hd = L(num), L(den)
    dn, dd = ctx.to_device(hn), ctx.to_device(hd)
    lib = ctx.lib
    assert lib.zk_fr_batch_div(ctx.h, dn.ptr, dd.ptr, dn.ptr, n) == ZK_ERR_INVALID   # out is num
    assert lib.zk_fr_batch_div(ctx.h, dn.ptr, dd.ptr, dd.ptr, n) == ZK_ERR_INVALID   # out is den
    assert (dn.download((n, 4)) == hn).all() and (dd.download((n, 4)) == hd).all()     # nothing was written
    from zkhip import ZkError

    with pytest.raises(ZkError) as e:
        ctx.fr_batch_div(dn, dd, n, out=dd)
    assert e.value.code == ZK_ERR_INVALID
    out = ctx.to_device(guards(4))
    assert lib.zk_fr_batch_div(ctx.h, dn.ptr, dd.ptr, out.ptr, 0) == 0 and lib.zk_fr_batch_div(ctx.h, 0, 0, 0, 0) == 0  # n = 0: OK
    assert (out.download((4, 4)) == GUARD).all()
    assert (run_guarded(ctx, n, lambda o: ctx.fr_batch_div(dn, dd, n, out=o)) == L(fc.ref_div(num, den))).all()


# ---- product tree ----
def _tree(ctx, x_limbs, N):
    out = ctx.to_device(guards(2 * N + 2))
    d_x = ctx.to_device(x_limbs)
    ctx.product_tree(d_x, N, out=out)
    got = out.download((2 * N + 2, 4))
    assert (got[2 * N:] == GUARD).all(), "wrote past the 2N entries"
    assert (d_x.download((N, 4)) == x_limbs).all()
    assert (got[:N] == x_limbs).all() and not got[2 * N - 1].any()  # the lower half is the input, the last entry is 0
    return got[: 2 * N]


@pytest.mark.parametrize("N", fc.TREE_SIZES)
def test_product_tree_sizes_and_closed_forms(ctx, co, N):
    """random leaves against the Python-integer tree (N <= 1024) or the C oracle (2^18: two full launches, 2^19: a third launch on a
    level of two entries), then inputs whose tree is known in closed form and depends on neither"""
    x = fc.rand_vec(N, 70 + N.bit_length())
    x[N // 3] = 0  # a zero leaf among random ones
    hx = L(x)
    got = _tree(ctx, hx, N)
    exp = L(fc.ref_product_tree(x)) if N <= 1024 else co.product_tree(hx)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (N, bad[:8])
    one, zero = L([1])[0], np.zeros(4, dtype=np.uint64)
    # all leaves 2: level l is 2^(2^l) everywhere; all leaves r - 1: 1 from level 1 on
    for leaf in (2, R - 1):
        got = _tree(ctx, np.tile(L([leaf])[0], (N, 1)), N)
        for off, cnt, v in fc.tree_const(N, leaf):
            assert (got[off:off + cnt] == L([v])[0]).all(), (N, hex(leaf), off)
    # leaves 1 except one zero: at every level exactly the ancestor of that leaf is 0
    for j in sorted({j % N for j in fc.TREE_ZERO_AT}):
        hx = np.tile(one, (N, 1))
        hx[j] = zero
        got = _tree(ctx, hx, N)
        zeros = set(np.nonzero(~got.any(axis=1))[0].tolist())
        assert zeros == fc.tree_one_zero(N, j), (N, j)
        ones = (got == one).all(axis=1)
        assert ones.sum() == 2 * N - len(zeros), (N, j)
    if N == 1024:  # leaves 1 .. 1024: the root is 1024!
        got = _tree(ctx, L(range(1, N + 1)), N)
        assert (got[2 * N - 2] == L([fc.factorial_mod(N)])[0]).all()


def test_product_tree_refusals(ctx):
    from zkhip._lib import ZK_ERR_INVALID

    x = ctx.to_device(L(fc.rand_vec(1024, 9)))
    out = ctx.to_device(guards(2048))
    for N in fc.TREE_REFUSED:
        assert ctx.lib.zk_product_tree(ctx.h, x.ptr, N, out.ptr) == ZK_ERR_INVALID, N
    assert (out.download((2048, 4)) == GUARD).all()


# ---- the transform map and the dense map ----
class _Layout:
    """where vector j keeps component c (input) / row r (output): 'vec' = one vector after the other with a gap row between vectors,
    'party' = component-major, what an all-gather delivers (in[c * (k + 1) + j]); the gaps hold decoys (input) or guards (output)"""

    def __init__(self, kind, k, width):
        self.sv, self.sc = (width + 1, 1) if kind == "vec" else (1, k + 1)
        self.rows = (k - 1) * self.sv + (width - 1) * self.sc + 1 + 2

    def at(self, j, c):
        return j * self.sv + c * self.sc


def _tables_arg(t: fc.NttTables) -> dict:
    return dict(A=t.A, B=t.B, n_in=t.n_in, take=t.take, step=t.step, winv=L(t.winv), w=L(t.w), scale=L(t.scale))


def _run_maps(ctx, t, targ, k, rot, in_kind, out_kind, cache, dense):
    """k vectors, vector j of input kind (j + rot) mod 6, through zk_fr_ntt_map (and zk_fr_apply_matrix where `dense` is given):
    every output row against the reference, every other row of the output buffer against its guard"""
    li, lo = _Layout(in_kind, k, t.n_in), _Layout(out_kind, k, t.take)
    h_in = S(fc.rand_vec(li.rows, 31 + k))  # decoys everywhere a vector does not live: read by mistake, they change the result
    exp = guards(lo.rows)
    for j in range(k):
        kind = fc.INPUT_KINDS[(j + rot) % len(fc.INPUT_KINDS)]
        vec = fc.ntt_input(kind, t.n_in, 1000 * t.A + t.B)
        key = (kind, t.n_in)
        if key not in cache:
            cache[key] = fc.ntt_coeffs(t, vec)
        sel = (key, t.take, t.step)
        if sel not in cache:
            cache[sel] = L(fc.ntt_eval(t, cache[key]))
        rows = [li.at(j, c) for c in range(t.n_in)]
        h_in[rows] = L(vec)
        exp[[lo.at(j, r) for r in range(t.take)]] = cache[sel]
    d_in = ctx.to_device(h_in)
    out = ctx.to_device(guards(lo.rows))
    ctx.fr_ntt_map(targ, d_in, li.sv, li.sc, k, lo.sv, lo.sc, out=out)
    got = out.download((lo.rows, 4))
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, ("ntt_map", t.A, t.B, t.n_in, t.take, t.step, k, in_kind, out_kind, bad[:8])
    if dense is not None:
        out = ctx.to_device(guards(lo.rows))
        ctx.fr_apply_matrix(dense, d_in, li.sv, li.sc, k, lo.sv, lo.sc, out=out)
        got = out.download((lo.rows, 4))
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, ("apply_matrix", t.A, t.B, t.n_in, t.take, t.step, k, in_kind, out_kind, bad[:8])
    assert (d_in.download((li.rows, 4)) == h_in).all()


def _sweep(ctx, base, targ_of):
    """every k around one workgroup's vectors x every (n_in, take, step) variant x both layouts; the input kinds rotate so that each
    kind opens and closes a launch somewhere in the sweep"""
    rot, cache = 0, {}  # the references of one pair, shared by its variants: keyed by input and selection
    for n_in, take, step in fc.ntt_variants(base.A, base.B):
        t = base.variant(n_in, take, step)
        targ = targ_of(t)
        dense = None
        if t.A * t.B <= 4096:
            dense = L([m for row in fc.ntt_dense_matrix(t) for m in row]).reshape(t.take, t.n_in, 4)
        for k in fc.ntt_ks(t):
            for in_kind, out_kind in (("vec", "party"), ("party", "vec")):
                _run_maps(ctx, t, targ, k, rot, in_kind, out_kind, cache, dense)
                rot += 1


@pytest.mark.parametrize("A,B", fc.NTT_PAIRS, ids=["%dx%d" % p for p in fc.NTT_PAIRS])
def test_ntt_map_domains_from_the_definition(ctx, A, B):
    """
    Tables built from the header's definition (omega_A, omega_B from the 2-adic root, scale[i] = A^-1 off^i).  For each pair:
    k = 1, vpb - 1, vpb, vpb + 1 vectors; n_in = A, A/2, 1; (take, step) = (B, 1), (B/2, 2), (1, 1); inputs party-major -> outputs
    vector-major and the reverse, both with non-unit strides and a gap row between neighbours.  Vector j of a launch is all zero,
    a single 1 in front, a single 1 at n_in - 1, all r - 1 or one of two random vectors, by (j + launch number) mod 6.  EVERY output
    vector is compared with the two-dense-DFT reference (no cut at 512 x 512: its launches hold at most two vectors); where
    A * B <= 4096 the same inputs also go through zk_fr_apply_matrix with the dense matrix of the same reference.
    """
    base = fc.NttTables(A, B, fc.ntt_offset(A, B))
    _sweep(ctx, base, _tables_arg)


@pytest.mark.parametrize("l", [1, 32])
def test_ntt_map_with_the_pss_tables(ctx, l):
    """the tables the PSS callers pass (PackedSharingParams.ntt_tables) at the smallest and at a large packing factor: pack 2l -> 8l,
    unpack 8l -> 2l, unpack2 8l -> 4l every second slot; the same sweep, the reference from the definition"""
    from zkhip.pss import PackedSharingParams

    pp = PackedSharingParams(l)
    for kind, off in (("pack", pow(7, -1, R)), ("unpack", 7), ("unpack2", 7)):
        pt = pp.ntt_tables(kind)
        base = fc.NttTables(pt["A"], pt["B"], off, pt["n_in"], pt["take"], pt["step"])
        for name in ("winv", "w", "scale"):
            assert (np.asarray(pt[name]).reshape(-1, 4) == L(getattr(base, name))).all(), (kind, name)
        cache = {}
        dense = L([m for row in fc.ntt_dense_matrix(base) for m in row]).reshape(base.take, base.n_in, 4) if base.A * base.B <= 4096 else None
        for rot, k in enumerate(fc.ntt_ks(base)):
            _run_maps(ctx, base, pt, k, rot, "vec", "party", cache, dense)      # pack's layout: out[p * k' + j]
            _run_maps(ctx, base, pt, k, rot + 3, "party", "vec", cache, dense)  # unpack's layout: in[i * k' + j]


def test_ntt_map_refusals(ctx):
    """A above 512, A no power of two, n_in above A, a selection that leaves the output domain: ZK_ERR_INVALID and no launch (the
    output keeps its guard); k = 0 or take = 0: OK and no launch"""
    from zkhip._lib import ZK_ERR_INVALID

    d_in = ctx.to_device(L(fc.rand_vec(2048, 3)))
    out = ctx.to_device(guards(4096))
    tab = L(fc.rand_vec(1024, 4))

    def call(A, B, n_in, take, step, k):
        return ctx.lib.zk_fr_ntt_map(ctx.h, A, tab.ctypes.data, B, tab.ctypes.data, tab.ctypes.data, n_in, take, step, d_in.ptr, n_in, 1, out.ptr, take, 1, k)

    for A, B, n_in, take, step, why in fc.NTT_REFUSED:
        assert call(A, B, n_in, take, step, 2) == ZK_ERR_INVALID, why
    assert call(8, 8, 8, 8, 1, 0) == 0 and call(8, 8, 8, 0, 1, 2) == 0
    assert (out.download((4096, 4)) == GUARD).all()
    t = fc.NttTables(8, 8)
    good = ctx.fr_ntt_map(_tables_arg(t), d_in, 8, 1, 2, 8, 1).download((16, 4))  # and the ctx is usable afterwards
    vec = [fc.from_mont(int.from_bytes(r.tobytes(), "little")) for r in d_in.download((16, 4))]
    assert (good == L(fc.ref_ntt_map(t, vec[:8]) + fc.ref_ntt_map(t, vec[8:]))).all()
