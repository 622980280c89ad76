"""
CPU companion of tests/test_gpu_fused_edges.py.  fused_edge_cases.engine restates in big-int Python the INTEGERS the fused engines hold
(csrc/zk_fused.cuh, csrc/zk_fs.hip with the shared arithmetic of csrc/zk_gate.cuh): for a case and a grid geometry -- CU count,
workgroups per CU, blocks of 256, waves of 64, the grid-stride assignment of k_sc_pass / k_fs_pass -- each lane's 17-limb sum per
evaluation, each wave's sum, the pass total W = W0 + W1 2^256 + W2 2^512, the lane's g0 and gd, and the reduced result
W0 R^-1 + W1 + W2 R.  This file ties that restatement to the independent identity models and then proves, case by case, which
condition each input of the GPU test reaches (COVERAGE):

  C1  a pass total with W2 >= 1 (w2), with W2 >= 2^6 (w2_64, mu = 10), and a wave whose sum gets limb 16 from the shuffle's
      gate_wide_add while every lane's limb 16 is still zero (shuffle16)
  C2  W0 and W1 in each of [0, r), [r, 2r), [2r, 2^256): in the last band the second fp_reduce_once does work (w0_0 .. w1_2).
      On W1 its work SHOWS only where W0 R^-1 + (W1 - 2r) + W2 R >= 2r, each term reduced (w1_late: the lateW1 pattern, found by
      search): otherwise the two fr_add that follow subtract the r it left.  On W0 it never shows: fr_mul(w0, 1) is exact for any
      w0 < 2^256, (w0 + m r) / 2^256 <= r for m < 2^256, and its own conditional subtraction makes that canonical -- the second
      fp_reduce_once of w0 is redundant and no input tells a build without it apart (test_second_reduction_of_w0_is_redundant)
  C3  a single lane's sum >= 2^512 inside the pass loop (lane512: the large cases)
  C4  a carry out of limb 15 in gate_wide_add_hi (hi_carry: lookup and lookup_sel, the large cases)
  C5  an unreduced fr_add sum of exactly r in the t-stepping v + d (step_r) and in the fold lo + r (hi - lo) (fold_r); d = M (d_M)
  C6  both operands of fp_mac_wide equal to M at every pair and t of a pass (mac_M)

Both engines hold the same integers in pass p when they fold by the same challenges: the transcript-driven form evaluates the tables
it has just folded, with the same grid, so a lane owns the same pairs.  The code that produces them differs (k_sc_pass / k_fs_pass,
k_sc_reduce / k_fs_reduce_hash, the folds), hence one COVERAGE row per engine; a transcript-driven row is proved on the challenges
hashlib derives.

NOT reachable: fold_r in the transcript-driven form.  lo + x = r with x = c d R^-1 mod r < r needs lo != 0 and, for d != 0, the one
challenge c = (r - lo) R / d mod r; d = 0 gives x = 0 and lo = r is no stored value.  A challenge there is 254 bits of a SHA-256
digest of the round's evaluations, so placing it means finding a preimage; test_fold_of_exactly_r_needs_a_chosen_challenge asserts
that none of the transcript-driven cases meets it.  The preset-challenge form reaches it with (lo, hi) = (M, 0) and c = ONE: M + 1 = r.
"""
import pytest

import fused_edge_cases as fe
from helpers import M_INT, ONE_INT, R_MOD

r = R_MOD
CU = 256  # MI355X
KINDS = sorted(fe.KINDS)
_RUN = {}


def run(kind, mu, local_e, pattern, gname, cname):
    """the engine on one case (cname None: the transcript-driven form), once"""
    key = (kind, mu, local_e, pattern, gname, cname)
    if key not in _RUN:
        chal = None if cname is None else fe.challenges(cname, mu)
        _RUN[key] = fe.engine(kind, fe.inputs(kind, pattern, mu)[0], fe.gamma_of(kind, pattern, gname, mu), chal, local_e=local_e, cu=CU)
    return _RUN[key]


def reached(res):
    """the conditions one run of the engine meets"""
    got = set(res["flags"])
    for per_t in res["passes"]:
        for s in per_t:
            got.add("w0_%d" % s["w0_band"]), got.add("w1_%d" % s["w1_band"])
            got |= {name for name, hit in (("w2", s["w2"] >= 1), ("w2_64", s["w2"] >= 64), ("shuffle16", s["wave_from_shuffle"]),
                                           ("lane512", s["lane_max"] >> 512), ("hi_carry", s["hi_carry"]), ("w1_late", s["w1_late"])) if hit}
        if all(s["mac_M"] for s in per_t):
            got.add("mac_M")
    return got


def cases(kind, engine):
    for mu, local_e in fe.SHAPES:
        if engine == "preset":
            for p, g, c in fe.combos(kind, mu):
                yield (mu, local_e, p, g, c)
        else:
            for p, g in fe.fs_combos(kind, mu):
                yield (mu, local_e, p, g, None)


# ---- the restatement against the identity models ----
@pytest.mark.parametrize("kind", KINDS)
def test_engine_equals_the_identity_models(kind):
    """every case of the GPU test up to mu = 6, both forms, and the mu = 10 cases of the preset-challenge form"""
    models = {}
    for mu, local_e, p, g, c in cases(kind, "preset"):
        if (mu, p, g, c) not in models:
            models[(mu, p, g, c)] = fe.model_preset(kind, fe.inputs(kind, p, mu)[0], fe.gamma_of(kind, p, g, mu), fe.challenges(c, mu), check_mont=c == "rand")
        res = run(kind, mu, local_e, p, g, c)
        assert (res["rounds"], res["last"]) == models[(mu, p, g, c)], (kind, mu, local_e, p, g, c)
    for mu, local_e, p, g, _ in cases(kind, "fs"):
        if mu > 6:
            continue
        if (mu, p, g) not in models:
            models[(mu, p, g)] = fe.model_fs(kind, fe.inputs(kind, p, mu)[0], fe.gamma_of(kind, p, g, mu))
        res = run(kind, mu, local_e, p, g, None)
        assert (res["rounds"], res["last"], res["chal"]) == models[(mu, p, g)], (kind, mu, local_e, p, g)


@pytest.mark.parametrize("kind", KINDS)
def test_macM_puts_M_into_both_operands(kind):
    """C6, from the constants alone: eq = M and the bracket on the constants = M (the comment at fused_edge_cases.MAC_M solves each Kind)"""
    K = fe.KINDS[kind]
    const, fixed = fe.MAC_M[kind]
    v = fe.const_values(kind, const)
    for gamma in ([fixed] if fixed is not None else [fe.scalar(g) for g in fe.NAMES]):
        assert v[0] == M_INT and K.inner(gamma, v) == M_INT
    assert (M_INT * M_INT) * 5 >> 512 == 1 and (M_INT * M_INT) * 4 >> 512 == 0  # five near-maximal products reach limb 16, four do not


@pytest.mark.parametrize("kind", KINDS)
def test_closed_form_equals_the_identity_model(kind):
    """constant tables at mu = 4 and 6: the macM constants and those of the large case (the lookups' hf = M / it)"""
    K = fe.KINDS[kind]
    large = fe.large_case(kind, CU)
    for const, gamma in ((fe.MAC_M[kind][0], fe.gamma_of(kind, "macM", "rand", 4)), (large[2], large[3])):
        for mu in (4, 6):
            ins = {k: [const.get(k, 0)] * (2 << mu if k == "tree" else 1 << mu) for k in K.uploaded}
            for cname in ("rand", "M"):
                assert fe.closed_form(kind, const, gamma, mu) == fe.model_preset(kind, ins, gamma, fe.challenges(cname, mu)), (kind, mu, cname)
            res = fe.engine(kind, ins, gamma, None, local_e=2)
            assert (res["rounds"], res["last"]) == fe.closed_form(kind, const, gamma, mu)


# ---- which case reaches which condition ----
# condition -> engine -> kind -> (mu, local_e, pattern, gamma, challenge set or None); found by scanning fe.combos / fe.fs_combos in
# order for the first case that meets it, checked here by running that case
COVERAGE = {
    "w2": {
        "preset": {"gate": (4, 2, 'allM', 'none', 'rand'), "gate_wide": (4, 2, 'allM', 'none', 'rand'), "lookup": (4, 2, 'allNearM', 'rand', 'rand'), "lookup_sel": (4, 2, 'allNearM', 'rand', 'rand'), "perm3": (4, 2, 'allM', 'zero', 'rand'), "wiring": (4, 2, 'allM', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'allM', 'none', None), "gate_wide": (4, 2, 'allM', 'none', None), "lookup": (4, 2, 'allNearM', 'rand', None), "lookup_sel": (4, 2, 'allNearM', 'rand', None), "perm3": (4, 2, 'allM', 'zero', None), "wiring": (4, 2, 'allM', 'rand', None)},
    },
    "w2_64": {
        "preset": {"gate": (10, None, 'allM', 'none', 'rand'), "gate_wide": (10, None, 'allM', 'none', 'rand'), "lookup": (10, None, 'macM', 'fixed', 'rand'), "lookup_sel": (10, None, 'macM', 'one', 'rand'), "perm3": (10, None, 'macM', 'fixed', 'rand'), "wiring": (10, None, 'allM', 'rand', 'rand')},
        "fs": {"gate": (10, None, 'allM', 'none', None), "gate_wide": (10, None, 'allM', 'none', None), "lookup": (10, None, 'macM', 'fixed', None), "lookup_sel": (10, None, 'macM', 'one', None), "perm3": (10, None, 'macM', 'fixed', None), "wiring": (10, None, 'allM', 'rand', None)},
    },
    "shuffle16": {
        "preset": {"gate": (4, 2, 'allM', 'none', 'rand'), "gate_wide": (4, 2, 'allM', 'none', 'rand'), "lookup": (4, 2, 'allNearM', 'rand', 'rand'), "lookup_sel": (4, 2, 'allNearM', 'rand', 'rand'), "perm3": (4, 2, 'allM', 'zero', 'rand'), "wiring": (4, 2, 'allM', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'allM', 'none', None), "gate_wide": (4, 2, 'allM', 'none', None), "lookup": (4, 2, 'allNearM', 'rand', None), "lookup_sel": (4, 2, 'allNearM', 'rand', None), "perm3": (4, 2, 'allM', 'zero', None), "wiring": (4, 2, 'allM', 'rand', None)},
    },
    "w0_0": {
        "preset": {"gate": (4, 2, 'allM', 'none', 'rand'), "gate_wide": (4, 2, 'allM', 'none', 'rand'), "lookup": (4, 2, 'allM', 'M', 'rand'), "lookup_sel": (4, 2, 'allM', 'zero', 'rand'), "perm3": (4, 2, 'allM', 'rand', 'rand'), "wiring": (4, 2, 'allM', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'allM', 'none', None), "gate_wide": (4, 2, 'allM', 'none', None), "lookup": (4, 2, 'allM', 'M', None), "lookup_sel": (4, 2, 'allM', 'zero', None), "perm3": (4, 2, 'allM', 'rand', None), "wiring": (4, 2, 'allM', 'rand', None)},
    },
    "w0_1": {
        "preset": {"gate": (4, 2, 'allM', 'none', 'rand'), "gate_wide": (4, 2, 'allM', 'none', 'rand'), "lookup": (4, 2, 'allM', 'rand', 'rand'), "lookup_sel": (4, 2, 'allM', 'rand', 'rand'), "perm3": (4, 2, 'allM', 'rand', 'rand'), "wiring": (4, 2, 'allM', 'M', 'rand')},
        "fs": {"gate": (4, 2, 'allM', 'none', None), "gate_wide": (4, 2, 'allM', 'none', None), "lookup": (4, 2, 'allM', 'rand', None), "lookup_sel": (4, 2, 'allM', 'rand', None), "perm3": (4, 2, 'allM', 'rand', None), "wiring": (4, 2, 'allM', 'M', None)},
    },
    "w0_2": {
        "preset": {"gate": (4, 2, 'allM', 'none', 'rand'), "gate_wide": (4, 2, 'allNearM', 'none', 'rand'), "lookup": (4, 2, 'allM', 'zero', 'rand'), "lookup_sel": (4, 2, 'allM', 'rand', 'rand'), "perm3": (4, 2, 'allNearM', 'rand', 'rand'), "wiring": (4, 2, 'allNearM', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'allM', 'none', None), "gate_wide": (4, 2, 'allNearM', 'none', None), "lookup": (4, 2, 'allM', 'zero', None), "lookup_sel": (4, 2, 'allM', 'rand', None), "perm3": (4, 2, 'allNearM', 'rand', None), "wiring": (4, 2, 'allNearM', 'zero', None)},
    },
    "w1_0": {
        "preset": {"gate": (4, 2, 'allM', 'none', 'rand'), "gate_wide": (4, 2, 'allM', 'none', 'rand'), "lookup": (4, 2, 'allM', 'rand', 'rand'), "lookup_sel": (4, 2, 'allM', 'rand', 'rand'), "perm3": (4, 2, 'allM', 'rand', 'rand'), "wiring": (4, 2, 'allM', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'allM', 'none', None), "gate_wide": (4, 2, 'allM', 'none', None), "lookup": (4, 2, 'allM', 'rand', None), "lookup_sel": (4, 2, 'allM', 'rand', None), "perm3": (4, 2, 'allM', 'rand', None), "wiring": (4, 2, 'allM', 'rand', None)},
    },
    "w1_1": {
        "preset": {"gate": (4, 2, 'allM', 'none', 'rand'), "gate_wide": (4, 2, 'allM', 'none', 'rand'), "lookup": (4, 2, 'allNearM', 'rand', 'rand'), "lookup_sel": (4, 2, 'allM', 'M', 'rand'), "perm3": (4, 2, 'allM', 'zero', 'rand'), "wiring": (4, 2, 'allM', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'allM', 'none', None), "gate_wide": (4, 2, 'allM', 'none', None), "lookup": (4, 2, 'allNearM', 'rand', None), "lookup_sel": (4, 2, 'allM', 'M', None), "perm3": (4, 2, 'allM', 'zero', None), "wiring": (4, 2, 'allM', 'rand', None)},
    },
    "w1_2": {
        "preset": {"gate": (4, 2, 'rot0', 'none', 'rand'), "gate_wide": (4, 2, 'rot0', 'none', 'rand'), "lookup": (4, 2, 'allNearM', 'zero', 'rand'), "lookup_sel": (4, 2, 'allNearM', 'M', 'rand'), "perm3": (4, 2, 'allM', 'one', 'rand'), "wiring": (4, 2, 'allNearM', 'one', 'rand')},
        "fs": {"gate": (4, 2, 'rot0', 'none', None), "gate_wide": (4, 2, 'rot0', 'none', None), "lookup": (4, 2, 'allNearM', 'zero', None), "lookup_sel": (4, 2, 'allNearM', 'M', None), "perm3": (4, 2, 'allM', 'one', None), "wiring": (4, 2, 'allNearM', 'one', None)},
    },
    "w1_late": {
        "preset": {"gate": (10, None, 'lateW1', 'none', 'rand'), "gate_wide": (10, None, 'lateW1', 'none', 'rand'), "lookup": (10, None, 'lateW1', 'fixed', 'rand'), "lookup_sel": (10, None, 'lateW1', 'one', 'rand'), "perm3": (10, None, 'lateW1', 'fixed', 'rand'), "wiring": (10, None, 'lateW1', 'fixed', 'rand')},
        "fs": {"gate": (10, None, 'lateW1', 'none', None), "gate_wide": (10, None, 'lateW1', 'none', None), "lookup": (10, None, 'lateW1', 'fixed', None), "lookup_sel": (10, None, 'lateW1', 'one', None), "perm3": (10, None, 'lateW1', 'fixed', None), "wiring": (10, None, 'lateW1', 'fixed', None)},
    },
    "step_r": {
        "preset": {"gate": (4, 2, 'loM_hi0', 'none', 'rand'), "gate_wide": (4, 2, 'loM_hi0', 'none', 'rand'), "lookup": (4, 2, 'loM_hi0', 'rand', 'rand'), "lookup_sel": (4, 2, 'loM_hi0', 'rand', 'rand'), "perm3": (4, 2, 'loM_hi0', 'rand', 'rand'), "wiring": (4, 2, 'loM_hi0', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'loM_hi0', 'none', None), "gate_wide": (4, 2, 'loM_hi0', 'none', None), "lookup": (4, 2, 'loM_hi0', 'rand', None), "lookup_sel": (4, 2, 'loM_hi0', 'rand', None), "perm3": (4, 2, 'loM_hi0', 'rand', None), "wiring": (4, 2, 'loM_hi0', 'rand', None)},
    },
    "fold_r": {
        "preset": {"gate": (4, 2, 'loM_hi0', 'none', 'one'), "gate_wide": (4, 2, 'loM_hi0', 'none', 'one'), "lookup": (4, 2, 'loM_hi0', 'rand', 'one'), "lookup_sel": (4, 2, 'loM_hi0', 'rand', 'one'), "perm3": (4, 2, 'loM_hi0', 'rand', 'one'), "wiring": (4, 2, 'loM_hi0', 'rand', 'one')},
    },
    "d_M": {
        "preset": {"gate": (4, 2, 'lo0_hiM', 'none', 'rand'), "gate_wide": (4, 2, 'lo0_hiM', 'none', 'rand'), "lookup": (4, 2, 'lo0_hiM', 'rand', 'rand'), "lookup_sel": (4, 2, 'lo0_hiM', 'rand', 'rand'), "perm3": (4, 2, 'lo0_hiM', 'rand', 'rand'), "wiring": (4, 2, 'lo0_hiM', 'rand', 'rand')},
        "fs": {"gate": (4, 2, 'lo0_hiM', 'none', None), "gate_wide": (4, 2, 'lo0_hiM', 'none', None), "lookup": (4, 2, 'lo0_hiM', 'rand', None), "lookup_sel": (4, 2, 'lo0_hiM', 'rand', None), "perm3": (4, 2, 'lo0_hiM', 'rand', None), "wiring": (4, 2, 'lo0_hiM', 'rand', None)},
    },
    "mac_M": {
        "preset": {"gate": (4, 2, 'macM', 'none', 'rand'), "gate_wide": (4, 2, 'macM', 'none', 'rand'), "lookup": (4, 2, 'macM', 'fixed', 'rand'), "lookup_sel": (4, 2, 'macM', 'rand', 'rand'), "perm3": (4, 2, 'macM', 'fixed', 'rand'), "wiring": (4, 2, 'macM', 'fixed', 'rand')},
        "fs": {"gate": (4, 2, 'macM', 'none', None), "gate_wide": (4, 2, 'macM', 'none', None), "lookup": (4, 2, 'macM', 'fixed', None), "lookup_sel": (4, 2, 'macM', 'rand', None), "perm3": (4, 2, 'macM', 'fixed', None), "wiring": (4, 2, 'macM', 'fixed', None)},
    },
}
CONDITIONS = ("w2", "w2_64", "shuffle16", "w0_0", "w0_1", "w0_2", "w1_0", "w1_1", "w1_2", "w1_late", "step_r", "fold_r", "d_M", "mac_M")
UNREACHABLE = {("fold_r", "fs")}


def test_coverage_table_is_complete_and_true():
    for cond in CONDITIONS:
        for engine in ("preset", "fs"):
            if (cond, engine) in UNREACHABLE:
                assert engine not in COVERAGE.get(cond, {})
                continue
            for kind in KINDS:
                case = COVERAGE[cond][engine][kind]
                assert case in set(cases(kind, engine)), (cond, engine, kind, "is not a case of the GPU test")
                assert cond in reached(run(kind, *case)), (cond, engine, kind, case)
    for engine in ("preset", "fs"):
        for kind in KINDS:  # C1 in full: at mu = 10 many partials with limb 16 set are added by the reduce kernel
            case = COVERAGE["w2_64"][engine][kind]
            res = run(kind, *case)
            assert case[0] == 10 and len(res["passes"][0]) == fe.KINDS[kind].evals and res["passes"][0][0]["w2"] >= 64


def test_fold_of_exactly_r_needs_a_chosen_challenge():
    """see the module docstring: no transcript-driven case meets it, the preset-challenge form does with (M, 0) and c = ONE"""
    for kind in KINDS:
        for case in cases(kind, "fs"):
            if case[0] <= 6:
                assert "fold_r" not in run(kind, *case)["flags"], (kind, case)
    assert (M_INT + fe.mul(ONE_INT, (0 - M_INT) % r)) == r


# ---- the large cases: C3 and C4 ----
@pytest.mark.parametrize("cu", [256, 304, 128, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_large_case_reaches_2_to_512_in_one_lane(kind, cu):
    """the size the GPU test picks for a device of `cu` CUs: the busiest lane of the first pass (the same pairs in k_sc_pass and
    k_fs_pass<false>) passes 2^512 after its fifth product and, for the lookups, its g0 = M carries out of limb 15"""
    K = fe.KINDS[kind]
    mu, tune, const, gamma, it = fe.large_case(kind, cu)
    per_cu = 1 if K.pass_wg else K.per_cu
    assert tune == ({K.pass_wg: 1} if K.pass_wg else {})
    it2, p, g0 = fe.lane_model(kind, const, gamma, mu, cu, per_cu)
    v = fe.const_values(kind, const)
    assert it2 == it >= 5 and v[0] == M_INT and K.inner(gamma, v) == M_INT and p == it * M_INT * M_INT and p >> 512 >= 1
    if K.free:
        assert g0 == M_INT and (((p >> 256) & fe.MASK) + g0) >> 256 == 1
    if cu == 256:
        assert mu == (21 if kind == "lookup" else 20) and it == 8
    assert mu <= 22


def test_lane_model_is_the_engine_on_a_small_grid():
    """the closed lane model against the engine's lanes: 2 CUs, one workgroup each, 2^12 constants -> 4 products per lane, then 8 on 1 CU"""
    for kind in KINDS:
        K = fe.KINDS[kind]
        _, _, const, gamma, _ = fe.large_case(kind, CU)
        ins = {k: [const.get(k, 0)] * (2 << 12 if k == "tree" else 1 << 12) for k in K.uploaded}
        for cu, want_it in ((2, 4), (1, 8)):
            it, p, g0 = fe.lane_model(kind, const, gamma, 12, cu, 1)
            s = fe.engine(kind, ins, gamma, None, cu=cu, per_cu=1)["passes"][0][0]
            assert it == want_it == s["iters"] and s["lane_max"] == p + (g0 << 256) and bool(p >> 512) == (it >= 5)


def test_second_reduction_of_w0_is_redundant():
    """the Montgomery product of ANY w0 < 2^256 with the plain integer 1 is (w0 + m r) / 2^256 with m < 2^256: at most r, so the one
    conditional subtraction of fr_mul leaves the canonical w0 R^-1 whether w0 was reduced once, twice or not at all"""
    R = fe.R
    assert (R - 1 + (R - 1) * r) // R <= r
    ninv = (-pow(r, -1, R)) % R
    for w0 in (0, r - 1, r, 2 * r - 1, 2 * r, R - 1, fe.LATE_E + r):
        m = w0 * ninv % R
        t = (w0 + m * r) // R
        assert (w0 + m * r) % R == 0 and t <= r and t % r == w0 * fe.RINV % r


# ---- the capacity statement of zk_gate.cuh ----
def test_capacity_of_the_544_bit_sums():
    """every product at (r-1)^2, 2^34 pairs of a pass of 2^35 elements, and one free term < r 2^256 per lane of at most 2^17 lanes"""
    assert (1 << 34) * M_INT * M_INT + (1 << 17) * (M_INT << 256) < 1 << 544
    assert (1 << 35) * M_INT * M_INT >= 1 << 544  # and no factor of two to spare: kGateMaxLog = 35 is the bound
    assert (1 << 34) * (M_INT * M_INT + (M_INT << 256)) > 1 << 544  # one free term per index PAIR would not fit
    assert r * r < 83 * (1 << 510) // 100 and (r << 256) < 1 << 511
