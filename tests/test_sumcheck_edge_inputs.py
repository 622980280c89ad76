"""
CPU companion of tests/test_gpu_sumcheck_edges.py: a big-int restatement of what the lazily reducing kernels of csrc/zk_fr.hip hold as
INTEGERS (written from the comments there: the flat weights, the flat sum before its conditional subtractions, the 288-bit column sums,
the 544-bit totals of a product pass), used to prove that the inputs of the GPU test reach the branches they are there for, and a
restatement of sc_plan (helpers.sc_plan_model) that proves the same of its knob settings.

The flat output before the peel is v = (T + m r) / 2^256 with T = sum_s e_s w_s and m = -T / r mod 2^256.  The 2^K weights are the
eq-polynomial of the K challenges built level by level, w[2S] + w[2S+1] = w[S] or w[S] + r, so sum_s w_s <= ONE + (2^K - 1) r and, with
every e_s <= r - 1,  v < r/2^256 (0.2083 + 2^K - 1) r + r:  2.453 r (K = 2), 4.264 r (K = 3), 7.886 r (K = 4).  The code's own bound
(0.4528 2^K + 1) r allows 8.24 r at K = 4, but NO input reaches 8 r: the highest band of K = 4 is [4r, 8r) and w9_csub<3> never
subtracts.  The search (helpers.BAND_CHAL): challenge sets drawn from SplitMix64(9000 + K), the first whose window
[T/2^256, T/2^256 + r) on the all-M table has at least a fifth inside the band; 100 000 draws per K found every band below 8 r.
A table of M alone gives v = k r - 1 (its fold is M), so the top bands of K = 2 and 3 need the `nearM` table, whose quotient m varies.
"""
import pytest

import pyoracle as po
from helpers import BAND_CALLS, BAND_CHAL, M_INT, ONE_INT, R_MOD, SC_PLAN_CASES, chal_set, edge_table, fr_ints, sc_plan_model, sc_plan_text

r = R_MOD
R = 1 << 256
RINV = pow(R, -1, r)
NEG_RINV = (-pow(r, -1, R)) % R  # -1/r mod 2^256
CU = 256  # MI355X

def montmul(a, b):
    return a * b * RINV % r


def flat_weights(chal):
    """w[S], S < 2^K: MSB of S <-> the first challenge; every weight canonical"""
    w = [ONE_INT]
    for c in chal:
        nx = []
        for x in w:
            hi = montmul(x, c)
            nx += [(x - hi) % r, hi]
        w = nx
    return w


def flat_raw(elems, w):
    """-> (v, T): the 9-limb value the reduction leaves and the 544-bit sum it started from"""
    T = sum(e * x for e, x in zip(elems, w))
    m = T * NEG_RINV % R
    assert (T + m * r) % R == 0
    return (T + m * r) >> 256, T


def peel(v, K):
    for S in range(K - 1, -1, -1):
        if v >= r << S:
            v -= r << S
    return v


def band(v):
    return 0 if v < r else 1 if v < 2 * r else 2 if v < 4 * r else 4 if v < 8 * r else 8


def flat_pass(tab, chal, K, sample=None):
    """one flat pass over the stored integers `tab` -> (outputs, set of bands, largest T)"""
    q = len(tab) >> K
    w = flat_weights(chal[:K])
    outs, bands, tmax = [], set(), 0
    for j in range(q if sample is None else min(q, sample)):
        v, T = flat_raw([tab[j + s * q] for s in range(1 << K)], w)
        assert v < (r * (1 << K) * r >> 256) + r and T < 1 << 544
        bands.add(band(v))
        tmax = max(tmax, T)
        outs.append(peel(v, K))
    return outs, bands, tmax


def test_emulation_is_the_fold():
    """the restated flat pass = K rounds of fix_variable, on random and on extreme tables: the peel always lands on the canonical value"""
    for K in (1, 2, 3, 4):
        for name in ("rand", "M", "nearM", "lo0_hiM", "bit0_M"):
            tab = fr_ints(edge_table(name, 7))
            for cname in ("rand", "M", "zero", "one"):
                ch = fr_ints(chal_set(cname, K))
                outs, _, _ = flat_pass(tab, ch, K)
                want = [x * RINV % r for x in tab]
                for c in ch:
                    want = po.fold(want, c * RINV % r)
                assert outs == [x * R % r for x in want], (K, name, cname)


def test_weight_sum_bound_and_the_unreachable_band():
    """sum w <= ONE + (2^K - 1) r for every challenge set tried, so no K = 4 output reaches 8 r (module docstring)"""
    rng = po.SplitMix64(31)
    for K in (2, 3, 4):
        top = ONE_INT + ((1 << K) - 1) * r
        sets = [[rng.fr() for _ in range(K)] for _ in range(300)] + [list(BAND_CHAL[k]) for k in BAND_CHAL if k[0] == K] + [[M_INT] * K, [0] * K, [ONE_INT] * K]
        for ch in sets:
            s = sum(flat_weights(ch))
            assert s % r == ONE_INT and s <= top
        assert ((top * M_INT) >> 256) + r < 8 * r
    assert (((ONE_INT + 15 * r) * M_INT) >> 256) + r > 7 * r  # ... while [4r, 8r) is wide open


@pytest.mark.parametrize("K,lo", sorted(BAND_CHAL))
def test_band_fixtures_reach_their_band(K, lo):
    """each hard-coded challenge set puts outputs of the GPU test's own tables (M and nearM at the lengths it uses) into its band"""
    assert lo * r < ((r << K) * r >> 256) + r, "a band the code's own bound does not allow"
    calls = [c for c in BAND_CALLS if c[1] == K]
    assert {c[0] for c in calls} == ({"fold", "plain"} if K <= 3 else {"fold"}) and any(c[3] == K for c in calls)
    for mode, _, n, npts, knobs in calls:
        stages, tail, _ = sc_plan_model(mode, 1 << n, npts, cu=CU, **knobs)
        assert stages[0]["kind"] == "pass" and stages[0]["k"] == K and stages[0]["form"] == "flat"
        assert npts is None or (len(stages) == 1 and tail is None), "the partial fold hands back the outputs of the pass itself"
        _, bands, tmax = flat_pass(fr_ints(edge_table("nearM", n)), list(BAND_CHAL[(K, lo)]), K, sample=256)
        assert lo in bands and tmax < 1 << 544, (mode, n, bands)
        _, bands, _ = flat_pass(fr_ints(edge_table("M", n)), list(BAND_CHAL[(K, lo)]), K, sample=2)
        assert len(bands) == 1  # (the all-M table: one value, k r - 1)


def test_the_search_finds_the_fixtures():
    """the search of the module docstring, re-run for the bands it finds within a hundred draws"""
    for K, lo, index in ((2, 1, 0), (2, 2, 60), (3, 2, 0), (3, 1, 3), (4, 2, 0), (4, 4, 2)):
        rng = po.SplitMix64(9000 + K)
        for i in range(index + 1):
            ch = [rng.fr() for _ in range(K)]
            low = sum(flat_weights(ch)) * r >> 256
            if low + 4 * r // 5 >= lo * r and low + r // 5 < 2 * lo * r:
                break
        assert i == index and tuple(ch) == BAND_CHAL[(K, lo)], (K, lo)


def test_column_sums_overflow_256_bits_and_fit_288():
    """k_plain_flat: a lane's own column sum carries into its ninth limb from the third M on, and the call's sums stay far inside 288 bits"""
    assert 2 * M_INT < 1 << 256 <= 3 * M_INT
    knobs = dict(sc_local_g=16, sc_plain_wg=1, sc_k0=2)
    stages, _, _ = sc_plan_model("plain", 1 << 20, cu=CU, **knobs)
    assert stages[0]["form"] == "flat" and stages[0]["iters"] >= 3, "the grid-stride case of the GPU test: every lane adds >= 3 elements per column"
    assert stages[0]["iters"] * M_INT >= 1 << 256
    for name in ("M", "lo0_hiM", "bit0_M"):
        tab = fr_ints(edge_table(name, 12))
        q = len(tab) >> 2
        cols = [sum(tab[S * q:(S + 1) * q]) for S in range(4)]
        assert max(cols) >= 1 << 256 and max(cols) < 1 << 288
    assert (1 << 25) * M_INT < 1 << 288  # a column of the largest table the family takes (2^26, one round)


def product_pass_totals(f, g, chal, K):
    """the integer totals (t0, t1, t2) of each round of a K-round product pass over stored integers, factors NOT reduced"""
    tot = []
    for rd in range(K):
        h = len(f) // 2
        t0 = t1 = t2 = 0
        nf, ng = [], []
        for j in range(h):
            df, dg = (f[j + h] - f[j]) % r, (g[j + h] - g[j]) % r
            a, b = f[j + h] + df, g[j + h] + dg  # fr_add_nored: up to 2r - 2
            assert a < 1 << 256 and b < 1 << 256
            t0 += f[j] * g[j]
            t1 += f[j + h] * g[j + h]
            t2 += a * b
            nf.append((f[j] + montmul(chal[rd], df)) % r)
            ng.append((g[j] + montmul(chal[rd], dg)) % r)
        tot.append((t0, t1, t2))
        f, g = nf, ng
    return tot


def test_product_totals_use_limb_16_and_fit_544():
    n = 10
    f = fr_ints(edge_table("lo0_hiM", n))
    ch = fr_ints(chal_set("rand", 3))
    tot = product_pass_totals(f, f, ch, 3)
    assert tot[0][2] == (1 << (n - 1)) * (2 * r - 2) ** 2, "every first-round factor is 2r - 2"
    assert tot[0][2] >= 1 << 512, "limb 16 is in use"
    # the same tables at the largest length the GPU test gives a pass (2^20), and the bound the kernel states (2^25 products)
    assert (1 << 19) * (2 * r - 2) ** 2 < 1 << 544 and (1 << 25) * (2 * r - 2) ** 2 < 1 << 544
    for name_f, name_g in (("M", "M"), ("loM_hi0", "lo0_hiM"), ("bitmid_M", "bit0_M")):
        tot = product_pass_totals(fr_ints(edge_table(name_f, n)), fr_ints(edge_table(name_g, n)), ch, 3)
        assert max(max(t) for t in tot) < 1 << 544
    # bitmid_M meets its extreme pair in round n - 1 - n//2: the factor 2r - 2 appears there, not in the first round
    f = fr_ints(edge_table("bitmid_M", 4))
    tot = product_pass_totals(f, f, [0, 0, 0], 2)
    assert tot[0][2] == 4 * M_INT ** 2 and tot[1][2] == 4 * (2 * r - 2) ** 2


def test_plan_cases_reach_what_they_are_named_for():
    """part B: the plan recorded beside every case is the model's, and each group's plans show the path the group is there for"""
    by = {}
    for tag, knobs, mode, n, npts, text in SC_PLAN_CASES:
        assert sc_plan_text(mode, 1 << n, npts, cu=CU, **knobs) == text, (tag, mode, n)
        assert n <= 20
        by.setdefault(tag, []).append((mode, n, npts, knobs, sc_plan_model(mode, 1 << n, npts, cu=CU, **knobs)))
    loc = lambda st: [s for s in st if s["kind"] == "local"]
    pas = lambda st: [s for s in st if s["kind"] == "pass"]
    for g in (16, 32, 128, 512):
        for mode in ("plain", "product", "fold", "open"):
            pres = {loc(p[0])[0]["pre"] for m, n, _, _, p in by["local_g%d" % g] if m == mode and loc(p[0])[0]["G"] == g}
            assert pres == {0, 1}, (g, mode)
    assert all(loc(p[0])[0]["ho"] == bool(pas(p[0])) and not loc(p[0])[0]["xcd"] for *_, p in by["local_g16"])
    assert all(loc(p[0])[0]["xcd"] for *_, p in by["xcd1"]) and not any(loc(p[0])[0]["xcd"] for *_, p in by["xcd0"])
    assert any(pas(p[0]) for *_, p in by["xcd1"]) and any(not pas(p[0]) for *_, p in by["xcd1"])
    assert all(pas(p[0])[-1]["ho"] for *_, p in by["handover1"]) and not any(s["ho"] for *_, p in by["handover0"] for s in p[0])
    assert not any(loc(p[0])[0]["pre"] for *_, p in by["pre0"])
    declined = [(m, n) for m, n, _, _, p in by["pre1"] if not loc(p[0])[0]["pre"]]
    assert declined and all(loc(p[0])[0]["pre"] for m, n, _, _, p in by["pre2"] if (m, n) in declined), "sc_pre = 2 forces what the rule declines"
    for kf in (1, 2, 3, 4):
        assert [(s["k"], s["form"]) for *_, p in by["kf%d" % kf] for s in pas(p[0])] == [(kf, "flat")]
    assert [s["k"] for *_, p in by["kf4_twice"] for s in pas(p[0])] == [4, 4]
    for k0 in (1, 2, 3):
        assert all(s["form"] == "rounds" for tag in ("kf0", "kf0_k0_%d" % k0, "plain_flat0_k0_%d" % k0) for *_, p in by[tag] for s in pas(p[0]))
        for tag in ("kf0_k0_%d" % k0, "plain_flat0_k0_%d" % k0, "plain_flat1_k0_%d" % k0):
            assert any(s["k"] == k0 for *_, p in by[tag] for s in pas(p[0])), tag
        assert all(s["form"] == "flat" for m, *_, p in by["plain_flat1_k0_%d" % k0] if m == "plain" for s in pas(p[0]))
    for kp in (1, 2, 3):
        assert any(s["k"] == kp for *_, p in by["kp%d" % kp] for s in pas(p[0]))
    assert all(pas(p[0])[0]["k"] == 3 and not p[2] for *_, p in by["kp3_t1dev"]), "three-round passes, t1 never derived: the FULLT1 kernel"
    for tag in ("pass_wg1", "flat_wg1", "plain_wg1"):
        for m, n, _, knobs, p in by[tag]:
            s = pas(p[0])[0]
            assert (s["m"] >> s["k"]) > 256 * CU and s["blocks"] == CU and s["iters"] >= 2, (tag, m)
            assert s["form"] == ("rounds" if tag == "pass_wg1" else "flat")
    ends = {(n, npts): text for _, _, _, n, npts, text in SC_PLAN_CASES if npts is not None}
    assert ends[(18, 2)] == "P2" and ends[(18, 3)] == "P3" and ends[(18, 7)].endswith("L16+pre:4") and ends[(18, 14)].endswith("L16+pre:11")
    assert ends[(18, 16)].endswith("T16:2") and ends[(19, 5)].endswith("L16+pre:1")


def test_default_plan_sizes_of_part_a():
    """part A: where the default plan has its first multi-workgroup stage and its first passes (the sizes the GPU test straddles)"""
    assert sc_plan_text("plain", 1 << 10) == "T1024:10" and sc_plan_text("plain", 1 << 11) == "L2:10 T2:1"
    assert sc_plan_text("product", 1 << 9) == "T512:9" and sc_plan_text("product", 1 << 10) == "L2:9 T2:1"
    assert sc_plan_text("product", 1 << 19).startswith("P1h") and sc_plan_text("plain", 1 << 20).startswith("P2h")
    assert sc_plan_text("product", 1 << 18) == "L256+pre:10 T256:8" and sc_plan_text("plain", 1 << 19) == "L256+pre:11 T256:8"
    # the two sides of the derive threshold
    assert not sc_plan_model("product", 1 << 17)[2] and sc_plan_model("product", 1 << 18)[2]
