"""
GPU: the G1 point maps and SRS builders of csrc/zk_srs.hip (outside the MSM) on degenerate points and scalars -- equal points,
cancelling pairs, infinities, zero and extreme scalars, every count at which a lane guard or the lane count of the batched
normalisation changes.  The cases are tests/g1_map_cases.py; tests/test_g1_map_cases.py proves on the CPU that each one has
the property it is named for.

The reference shares no code with the kernels: every input is a*G with `a` known, so every expected record is ONE scalar
multiplication of the generator (C oracle, coracle.g1_mul_affine) by an exponent computed in Python mod r.  Comparisons are
bit-exact on the downloaded 96-byte affine records, infinity is the all-zero record, and no non-infinite record may hold a
coordinate >= q (a missing canonicalisation on a rare path).  zk_g1_apply_matrix and zk_srs_to_packed run in both kernel
forms (g1_map_by_column 0 | 1) wherever the knob decides, and the two must agree byte for byte.

What each group is aimed at (csrc/zk_srs.hip, csrc/curve30.cuh):

  a1  zero matrix          g1_apply_matrix_internal :251-257 top = -1; the ladders :201 / :222 run no step; output pre-filled with a guard
  a2  zero row             k_g1_apply_matrix :202-204, bit test never true; xyzz30_dbl on infinity curve30.cuh:112
  a3  0/1 matrix           top = 0, one step; xyzz30_madd set branch curve30.cuh:134-139
  a4  equal points         joint :204: set, P + P = xyzz30_madd same-x, R = 0 (curve30.cuh:154-156, xyzz30_dbl_affine), then generic;
                           column form: k_xyzz_pair_sums :234 -> xyzz30_add same-x (curve30.cuh:184-185, xyzz30_dbl) at P + P, 2P + 2P, 4P + 4P,
                           the copied odd term (:234, `: a`) added last (cols = 9) or mid-tree (cols = 13)
  a5  (P, -P, Q, -Q, ..)   same-x with R != 0: xyzz30_set_inf (curve30.cuh:157, :186), then xyzz30_madd / xyzz30_add onto infinity (:134, :171-172)
  a6  [1, r-1], [r-1, r-1, 2] on equal points, also padded to 8 and 9 columns: a 255-bit ladder whose only cancellation comes at bit 1 or 0
  a7  r-1, 2^254, 2^32-1, 2^32, 2^64-1, 2^64, 2^224+2^31, 1, 0 mixed: the bit extraction of :204 / :224 across the 32-bit words
  a8  infinite inputs      xyzz30_madd curve30.cuh:133; all-infinite outputs: k_batch_affine :69 never multiplies, f30_inv(1) at :71
  a9  strides              j*isv + c*isc (:204, :219), g1_apply_matrix_ref's span :323, k_copy96_strided :242; guard words in the gaps stay
  a10 counts               total in {1, 63, 64, 65, 255, 256, 257}: `t >= rows*k` guards (:196, :216, :231, :239) and T = ceil(total/64) of
                           xyzz_to_affine_batch :120; k_batch_affine lanes that own only infinities (:69, :76) beside lanes that own none
  a11 cols = 0             accepted: every output is infinity
  a12 zk_srs_to_packed     srs_to_packed :504 cols = min(l, n) (short level), zero coefficients, a row of ones on equal points
  b   zk_srs_powers        k_eq_expand :352-358 with s, 1 - s in {0, 1, r - 1}; k_fixed_base_mul :367-370: exponent 0 (every digit skipped),
                           digits 0..30 = 0xff, one byte in window 31 / window 0; build_fixed_base_table :377-394 on a custom and on the
                           infinite base; the host's one_m - s :451-469 with and without borrow
  c   zk_srs_generate      fill_sequence_affine :130-181: the host chain :139-144 through doubling and infinity, k_aff_to_xyzz :30-38 on
                           infinity, k_seq_walk :51-54 from infinity (set at 1024, then stepT + stepT: same-x doubling at 2048), onto -stepT
                           (infinity stored at 1029, set at 2053, doubling at 3077), onto stepT (same-x doubling at 2047), a step of
                           infinity; three levels at n = 70000 on a sampled index set
"""
import numpy as np
import pytest

import g1_map_cases as gc
import pyoracle as po
from helpers import pt_mont

pytestmark = pytest.mark.gpu

R, Q = gc.R, gc.Q
MAP, PACKED, POWERS, SEQ = gc.map_cases(), gc.packed_cases(), gc.powers_cases(), gc.seq_cases()
G_MONT = pt_mont(po.G1_GEN)
GUARD = np.uint64(0xA5A55A5AC3C33C3C)
_records = {}  # exponent -> the 96-byte record of exponent * G: computed once, shared by every test of the file, never changed


def limbs(v: int):
    return [(v >> (64 * i)) & po.MASK64 for i in range(4)]


def canon(ints) -> np.ndarray:
    return np.array([limbs(v) for v in ints], dtype=np.uint64).reshape(-1, 4)


def mont(ints) -> np.ndarray:
    return np.array([po.fr_to_mont_limbs(v) for v in ints], dtype=np.uint64).reshape(-1, 4)


def records(co, exps) -> np.ndarray:
    """[n, 12]: exponent * G per entry by one scalar multiplication of the generator each; 0 -> the all-zero record"""
    out = np.zeros((len(exps), 12), dtype=np.uint64)
    for i, e in enumerate(exps):
        e %= R
        if e == 0:
            continue
        r = _records.get(e)
        if r is None:
            r = _records[e] = co.g1_mul_affine(G_MONT, np.array(limbs(e), dtype=np.uint64))
            r.setflags(write=False)
        out[i] = r
    return out


def assert_canonical(got: np.ndarray):
    """no coordinate of a downloaded record is >= q"""
    for i, rec in enumerate(np.asarray(got).reshape(-1, 12)):
        for half in (rec[:6], rec[6:]):
            assert sum(int(w) << (64 * j) for j, w in enumerate(half)) < Q, f"record {i}: coordinate >= q"


def assert_records(got: np.ndarray, want: np.ndarray, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} records differ, first at {bad[:8].tolist()}"


def forms_of(applies: bool):
    """the values of g1_map_by_column to run: both where the knob decides the form, the default alone elsewhere"""
    return (0, 1) if applies else (1,)


# ---- A: zk_g1_apply_matrix ----
@pytest.mark.parametrize("case", MAP, ids=[c.name for c in MAP])
def test_g1_apply_matrix(ctx, co, case):
    d_in = ctx.to_device(records(co, case.in_exps()))
    m = np.zeros((case.rows, case.cols, 4), dtype=np.uint64)
    if case.cols:
        m[:] = canon([v for row in case.matrix for v in row]).reshape(case.rows, case.cols, 4)
    want = np.full((case.out_len, 12), GUARD, dtype=np.uint64)  # "untouched" cannot pass for "infinity"
    exp = case.expected()
    want[list(exp)] = records(co, list(exp.values()))
    outs = {}
    try:
        for form in forms_of(case.knob_applies()):
            ctx.dbg_tune("g1_map_by_column", form)
            d_out = ctx.to_device(np.full((case.out_len, 12), GUARD, dtype=np.uint64))
            ctx.g1_apply_matrix(m, d_in, case.isv, case.isc, case.k, case.osv, case.osr, out=d_out)
            outs[form] = d_out.download((case.out_len, 12))
    finally:
        ctx.dbg_tune("g1_map_by_column", 1)
    for form, got in outs.items():
        assert_canonical(got[list(exp)])
        assert_records(got, want, (case.name, "per-term" if form else "per-output"))
    if len(outs) == 2:
        assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("case", PACKED, ids=[c.name for c in PACKED])
def test_srs_to_packed(ctx, co, case):
    level = ctx.srs_generate(case.k0, case.k1, case.n)
    try:
        assert_records(level.download(), records(co, [case.level_exp(i) for i in range(case.n)]), (case.name, "level"))
        want = records(co, case.expected())
        outs = {}
        try:
            for form in forms_of(case.cols >= 8):
                ctx.dbg_tune("g1_map_by_column", form)
                packed = ctx.srs_to_packed(level, canon(case.row), case.l)
                outs[form] = packed.download()
                packed.free()
        finally:
            ctx.dbg_tune("g1_map_by_column", 1)
        for form, got in outs.items():
            assert len(got) == case.count
            assert_canonical(got)
            assert_records(got, want, (case.name, "per-term" if form else "per-output"))
        if len(outs) == 2:
            assert outs[0].tobytes() == outs[1].tobytes()
    finally:
        level.free()


# ---- B: zk_srs_powers ----
@pytest.mark.parametrize("case", POWERS, ids=[c.name for c in POWERS])
def test_srs_powers(ctx, co, case):
    """the header gives h_g96 as a point in the reference affine layout, where x = y = 0 is infinity: the infinite base is accepted
    and every point of every level is infinity"""
    n = len(case.s)
    g = None if case.g_exp == 1 else records(co, [case.g_exp])[0]
    levels = ctx.srs_powers(mont(case.s), g=g)
    try:
        assert len(levels) == n + 1
        exp = case.expected()
        for k in range(n + 1):
            got = levels[k].download()
            assert_canonical(got)
            assert_records(got, records(co, exp[k]), (case.name, "level", k))
            if case.prop[0] == "half_infinite":  # the exact positions: the index bit that chooses the variable set to 0 (or 1)
                var, val = case.prop[1:]
                bit = n - 1 - var
                zero = [j for j in range(1 << k) if not got[j].any()]
                assert zero == ([j for j in range(1 << k) if ((j >> bit) & 1) == 1 - val] if k > bit else []), (case.name, k)
            if case.prop[0] == "infinite_base":
                assert not got.any()
    finally:
        for lv in levels:
            lv.free()


# ---- C: zk_srs_generate ----
@pytest.mark.parametrize("case", SEQ, ids=[c.name for c in SEQ])
def test_srs_generate(ctx, co, case):
    srs = ctx.srs_generate(case.k0, case.k1, case.n)
    try:
        assert len(srs) == case.n
        idx = case.indices()
        got = srs.download()[idx]
    finally:
        srs.free()
    assert_canonical(got)
    want = records(co, [case.exp(i) for i in idx])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{case.name}: {bad.size} points differ, first at indices {[idx[b] for b in bad[:8]]}"
    if case.prop[0] == "inf_at":
        assert [i for i, rec in zip(idx, got) if not rec.any()] == case.prop[1]
