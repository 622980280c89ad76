"""shared test utilities: seeded inputs in the reference's memory layouts"""
import numpy as np

import coracle as co
import pyoracle as po


def pt_mont(P):
    if P is None:
        return np.zeros(12, dtype=np.uint64)
    return np.array(po.fq_to_mont_limbs(P[0]) + po.fq_to_mont_limbs(P[1]), dtype=np.uint64)


def pt_ints(a12):
    a = np.asarray(a12, dtype=np.uint64).reshape(12)
    if not a.any():
        return None
    return (po.fq_from_mont_limbs(a[:6]), po.fq_from_mont_limbs(a[6:]))


def jac_norm_to_affine(j18):
    """normalised Jacobian [18] (library output) -> affine Montgomery [12] (zeros = infinity)"""
    j = np.asarray(j18, dtype=np.uint64).reshape(18)
    if not j[12:].any():
        return np.zeros(12, dtype=np.uint64)
    one = np.array(po.fq_to_mont_limbs(1), dtype=np.uint64)
    assert (j[12:] == one).all(), "library results must be normalised (z = R mod q)"
    return j[:12].copy()


_G = None


def synthetic_bases(n: int, seed: int) -> np.ndarray:
    """P_i = (k0 + i*k1)*G as affine Montgomery [n,12] -- same points as pyoracle.g1_bases(n, seed)"""
    rng = po.SplitMix64(seed)
    k0, k1 = rng.fr(), rng.fr()
    start = pt_mont(po.g1_mul(po.G1_GEN, k0))
    step = pt_mont(po.g1_mul(po.G1_GEN, k1))
    return co.g1_arith_seq(start, step, n), (k0, k1)


def rand_fr(n: int, seed: int) -> np.ndarray:
    """uniform Fr limbs [n,4] (interpreted as Montgomery form)"""
    return co.rand_fr(seed, n)


def oracle_msm_chunked(bases: np.ndarray, scalars: np.ndarray, threads: int = 0) -> np.ndarray:
    """
    the C oracle's MSM on many host threads: contiguous chunks (ctypes releases the GIL), partial results added with
    the python oracle's group law -> affine Montgomery [12].  A 2^24-point MSM that takes ~200 s on one core of the
    port finishes in seconds on the GPU box's cores.
    """
    import os
    from concurrent.futures import ThreadPoolExecutor

    m = len(scalars)
    threads = threads or max(1, min(64, (os.cpu_count() or 1) // 2))
    chunks = max(threads, (m + (1 << 18) - 1) >> 18)  # <= 2^18 points per chunk keeps every worker busy to the end
    bounds = [m * i // chunks for i in range(chunks + 1)]
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda i: co.msm_g1(bases[bounds[i] : bounds[i + 1]], scalars[bounds[i] : bounds[i + 1]]), range(chunks)))
    acc = None
    for pt in parts:
        acc = po.g1_add(acc, pt_ints(pt))
    return pt_mont(acc)


# ---- the core sumcheck family (csrc/zk_fr.hip): extreme stored values, knobs, and a model of its planner ----
R_MOD = po.R_MOD
M_INT = R_MOD - 1                 # the largest stored value: every lazily reduced bound is a bound on stored integers
ONE_INT = (1 << 256) % R_MOD      # R mod r: the stored form of the field's 1


def fr_limbs(v: int) -> np.ndarray:
    """a stored 256-bit integer as raw limbs [4] (NOT converted: the value is what the kernels read)"""
    return np.array([(v >> (64 * i)) & po.MASK64 for i in range(4)], dtype=np.uint64)


def fr_ints(a) -> list:
    """raw limbs [..., 4] -> stored integers"""
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192 for x in a]


def const_fr(v: int, n: int) -> np.ndarray:
    return np.tile(fr_limbs(v), (n, 1))


EDGE_TABLES = ("M", "zero", "lo0_hiM", "loM_hi0", "bit0_M", "bitmid_M")


def edge_table(name: str, n: int, seed: int = 0) -> np.ndarray:
    """
    the tables of extreme stored values, 2^n elements.  lo0_hiM: every pair of the first round is (0, M), so the product sumcheck's
    factor f_hi + (f_hi - f_lo) is 2r - 2 and every difference is M; bit<k>_M: M where bit k of the index is set, so the same pair
    meets round n-1-k -- bit 0 in the last round (the single-workgroup stage), the middle bit inside a pass or a local stage.
    """
    L = 1 << n
    if name == "rand":
        return rand_fr(L, 4100 + 16 * n + seed)
    if name == "nearM":  # M - (64-bit hash of the index): as large as M to one part in 2^190, but the Montgomery quotient of a flat sum varies
        h = (np.arange(L, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        t = const_fr(M_INT, L)
        t[:, 1] -= (h > t[:, 0]).astype(np.uint64)  # (limb 1 of M is not 0: the borrow stops there)
        t[:, 0] -= h
        return t
    if name.startswith("const"):
        return const_fr(po.SplitMix64(77 + seed).fr(), L)
    t = np.zeros((L, 4), dtype=np.uint64)
    m = fr_limbs(M_INT)
    if name == "M":
        t[:] = m
    elif name == "lo0_hiM":
        t[L // 2:] = m
    elif name == "loM_hi0":
        t[: max(L // 2, 1)] = m
    elif name in ("bit0_M", "bitmid_M"):
        k = 0 if name == "bit0_M" else n // 2
        t[((np.arange(L) >> k) & 1) == 1] = m
    elif name != "zero":
        raise ValueError(name)
    return t


# challenge sets found by the search of tests/test_sumcheck_edge_inputs.py (stored Montgomery forms, first round first): with
# every loaded element at M they put the output of a K-round flat pass, before its conditional subtractions, into the band
# [lo r, hi r).  BAND_CHAL[(K, lo)]
BAND_CHAL = {  # index in the stream SplitMix64(9000 + K): (2,1) 0, (2,2) 60, (3,1) 3, (3,2) 0, (3,4) 6878, (4,1) 59286, (4,2) 0, (4,4) 2
    (2, 1): (0x6d16d9e65ea114ef50c95eab8cbbb4ff10a9b6b1ff8e5f8db56cd76f96b91a16, 0x064b08cf5385334fdfed6337d0bd8da195363526e80403a5e7b53317047b8cbe),
    (2, 2): (0x44a1e42dcb5dd8435f125796e687a72ec429d3115d6503119fce34b2fa44b343, 0x3eb7c0674ff4576e0d6d30a2ce3645543b37c32674b23359fc7eaef3b4b8323d),
    (3, 1): (0x5c5ed863258e08b326c3677c46c4ea377310ecf6ab9b610e5c9acbd6d438baf2, 0x08b115fa3f52520cc0c62eadf41d500c238e91f6680c69873e79be15c58707b1, 0x2fc56406cc87ac8858373688aae5c88b60b76c0ce758a53ecf3e6599bf58dd40),
    (3, 2): (0x1e57f2ffda7a891881bf9ac18d68fbae00f491d1152bc66f76aeef7b71c918a5, 0x6c292c7285770dd1d96663deff2119f5742637a0e18ad031b08d1b838f1c0c39, 0x37a98de1f01f3a71518d430c90b9c36a8b29c6d78a6f56d06524f16a90bb905e),
    (3, 4): (0x3e8c0e6f8d06073146c0f91b35800d55a07376d8e911ee1a8eba200bef7190b2, 0x2cae68f07047e8abb16841d2706a20ec95195adbf878561694beb940e7fdf339, 0x5f8e9b08f0c245ae8c55dedc1a3afcfcff22cdaccc34fa8189095cd742a2fba3),
    (4, 1): (0x140ae24edb19bfa9d8e161cf45838b817340cc056c2c781288467c4fd394e57b, 0x4c1379bab6f8268cf14714ac15669658a046d5f3ed8453407b4c6e3623340437, 0x6520685cb4d2f2f1aea3c0bf1936abca02160d892c6ecfbf3a1b50c4cdb3c7aa, 0x0008be3173d159019099f7eb2656a897f9089f40d4a401b756ccec2a5b9ed7d1),
    (4, 2): (0x5b1eb71f5d24413a2679e344506917a8f0c315345fac0bdbb3d4069e1ed24d5a, 0x49711897febcb37820e51c687919dc04961b8ca4b125fde72f226d148928845a, 0x19b302ec92f682728e45859a7c6239ef2c692c37d223914eb5cbef4faddc26b4, 0x48c81772241e100567adc5502509f2306bfffdc18cc9d0be51ce1a7bd9fc99a6),
    (4, 4): (0x02033a17ff8d5cfa45da957fe0750a1dcddd93b91336f7e21d4649171e00ea7b, 0x736727a07d3d03fbcf4a3fa6965b8285bf0096351b6506122cb4094726ddbb77, 0x243e251e9cbdef5dfb90a69528b4f0d674023bbc55fbfcb58d61ae2452780dbd, 0x120773c88c2e215a6ec88a662cdca628c036c4c1102d3394f1b63733bac1fc80),
}


# the calls that carry them: (mode, K, log2 length, fold points or None, knobs) -- the FIRST pass of each is a flat pass of exactly K rounds;
# the partial folds end with that pass, so its outputs are compared as stored (the stages behind a pass multiply and reduce again)
BAND_CALLS = [("fold", K, 14 + K, None, dict(sc_local_g=16, sc_kf=K)) for K in (2, 3, 4)] + \
             [("fold", K, 15 + K, K, dict(sc_local_g=16, sc_kf=K)) for K in (2, 3, 4)] + \
             [("plain", 2, 16, None, dict(sc_local_g=16, sc_k0=2)), ("plain", 3, 18, None, dict(sc_local_g=16, sc_k0=3))]


def chal_set(name: str, n: int, seed: int = 0, head=()) -> np.ndarray:
    """n challenges [n,4]: rand | M | zero | one; `head` replaces the first len(head) of them (stored integers)"""
    n = max(n, 1)
    if name == "rand":
        c = rand_fr(n, 5200 + 16 * n + seed)
    else:
        c = const_fr({"M": M_INT, "zero": 0, "one": ONE_INT}[name], n)
    c = c.copy()
    for i, v in enumerate(head[:n]):
        c[i] = fr_limbs(v)
    return c


SC_DEFAULTS = dict(sc_pass_wg=0, sc_local_g=256, sc_local_threads=1024, sc_xcd=1, sc_kf=4, sc_plain_flat=1, sc_kp=2, sc_k0=3, sc_flat_wg=64,
                   sc_plain_wg=3, sc_pre=1, sc_pinned_out=1, sc_handover=1, sc_t1_device=0)
SC_MODES = {"plain": 0, "product": 1, "fold": 2, "open": 3}


class sc_knobs:
    """set sumcheck-family knobs for a block; every one goes back to the value zk_dbg_tune_get returned, whatever happens inside"""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        import ctypes

        from zkhip._lib import test_hooks

        self.lib, self.found = test_hooks(), {}
        for k in self.knobs:
            v = ctypes.c_long(0)
            assert self.lib.zk_dbg_tune_get(k.encode(), ctypes.byref(v)) == 0, k
            self.found[k] = v.value
        try:
            for k, v in self.knobs.items():
                assert self.lib.zk_dbg_tune(k.encode(), v) == 0, k
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in self.found.items():
            self.lib.zk_dbg_tune(k.encode(), v)
        return False


def _ilog2(x: int) -> int:
    return max(x.bit_length() - 1, 0)


def sc_plan_model(mode: str, length: int, rounds=None, cu: int = 256, **knobs):
    """
    what sc_plan of csrc/zk_fr.hip decides for one call, restated from its text: -> (stages, tail, derive).  A stage is a dict
    kind 'pass' (k rounds, m elements in, blocks, iters = grid-stride iterations of a lane, ho = stores the hand-over layout,
    form 'flat' | 'rounds') or 'local' (G workgroups of E elements, pre, k rounds, ho = reads the hand-over layout, xcd = slice
    map on); tail = (elements, rounds) of the closing single-workgroup launch or None; derive: the host derives t1 (product).
    """
    t = dict(SC_DEFAULTS)
    t.update(knobs)
    md = SC_MODES[mode]
    n = _ilog2(length)
    rounds = n if rounds is None else min(rounds, n)
    emax = 512 if md == 1 else 1024
    g0 = t["sc_local_g"]
    kf = min(max(t["sc_kf"], 0), 4)
    flat_fold = md == 2 and kf > 0
    plain_flat = md == 0 and t["sc_plain_flat"] != 0
    kmax = kf if flat_fold else min(max(t["sc_kp"] if md == 1 else t["sc_k0"], 1), 3)
    use_pre = t["sc_pre"] != 0
    if use_pre and md != 1 and t["sc_pre"] == 1 and rounds == n:
        base = _ilog2(emax * g0)
        need_pre, need_no = max(0, n - (base + 1)), max(0, n - base)
        cnt_pre, cnt_no = -(-need_pre // kmax), -(-need_no // kmax)
        last_no = need_no - (cnt_no - 1) * kmax
        if need_pre > 0 and cnt_no == cnt_pre and (md == 2 or last_no <= 2):
            use_pre = False
    local_max = emax * g0 * (2 if use_pre else 1)
    stages, mm, dd = [], length, 0
    while dd < rounds and mm > emax:
        if mm > local_max:
            k = min(kmax, rounds - dd, _ilog2(mm) - _ilog2(local_max))
            q = mm >> k
            if flat_fold or plain_flat:
                per_cu = max(1, t["sc_plain_wg"] if plain_flat else t["sc_flat_wg"])
            else:
                per_cu = t["sc_pass_wg"] or (2 if md == 1 else 4)
            blocks = min(-(-q // 256), max(cu * per_cu, -(-q // (256 * 32))))
            stages.append(dict(kind="pass", k=k, m=mm, blocks=blocks, iters=-(-q // (blocks * 256)), ho=False,
                               form="flat" if (flat_fold or plain_flat) else "rounds"))
            mm = q
        else:
            pre = int(mm > emax * g0)
            G = (mm // emax) >> pre
            k = min(_ilog2(emax) + pre, rounds - dd)
            stages.append(dict(kind="local", k=k, m=mm, G=G, E=emax, pre=pre, ho=False, xcd=bool(t["sc_xcd"]) and G % 32 == 0))
            mm = G * (emax >> (k - pre))
        dd += k
    if t["sc_handover"]:
        for a, b in zip(stages, stages[1:]):
            if a["kind"] == "pass" and b["kind"] == "local" and b["G"] >= 16 and b["G"] % 16 == 0 and b["G"] * (b["E"] << b["pre"]) == b["m"]:
                a["ho"] = b["ho"] = True
    tail = (mm, rounds - dd) if (dd < rounds or md != 2) else None
    derive = md == 1 and not t["sc_t1_device"] and (length >= 1 << 18 or (bool(stages) and stages[0]["kind"] == "pass"))
    return stages, tail, derive


def sc_plan_text(mode: str, length: int, rounds=None, cu: int = 256, **knobs) -> str:
    """the plan in one line: P<k>[h][x<iters>] per pass (h: hand-over store), L<G>[+pre]:<k> per local stage, T<m>:<k> the tail"""
    stages, tail, _ = sc_plan_model(mode, length, rounds, cu, **knobs)
    out = []
    for s in stages:
        if s["kind"] == "pass":
            out.append("P%d%s%s" % (s["k"], "h" if s["ho"] else "", "x%d" % s["iters"] if s["iters"] > 1 else ""))
        else:
            out.append("L%d%s:%d" % (s["G"], "+pre" if s["pre"] else "", s["k"]))
    if tail:
        out.append("T%d:%d" % tail)
    return " ".join(out) or "-"


# part B of tests/test_gpu_sumcheck_edges.py: (knob under test, knobs set, mode, log2 length, fold points or None, the plan sc_plan_text gives);
# tests/test_sumcheck_edge_inputs.py checks the last column against the model and that each group reaches what it is named for
SC_PLAN_CASES = [
    ('local_g16', {'sc_local_g': 16}, 'plain', 16, None, 'P2h L16:10 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'product', 13, None, 'L16:9 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'product', 15, None, 'P1h L16+pre:10 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'product', 16, None, 'P2h L16+pre:10 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'fold', 16, None, 'P2h L16:10 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'fold', 17, None, 'P3h L16:10 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'fold', 19, None, 'P4h L16+pre:11 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'open', 16, None, 'P2h L16:10 T16:4'),
    ('local_g16', {'sc_local_g': 16}, 'open', 17, None, 'P2h L16+pre:11 T16:4'),
    ('local_g32', {'sc_local_g': 32}, 'plain', 16, None, 'L32+pre:11 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'plain', 17, None, 'P2h L32:10 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'plain', 18, None, 'P2h L32+pre:11 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'product', 14, None, 'L32:9 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'product', 15, None, 'L32+pre:10 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'product', 16, None, 'P1h L32+pre:10 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'fold', 16, None, 'L32+pre:11 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'fold', 17, None, 'P2h L32:10 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'fold', 18, None, 'P3h L32:10 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'open', 16, None, 'L32+pre:11 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'open', 17, None, 'P2h L32:10 T32:5'),
    ('local_g32', {'sc_local_g': 32}, 'open', 18, None, 'P2h L32+pre:11 T32:5'),
    ('local_g128', {'sc_local_g': 128}, 'plain', 17, None, 'L128:10 T128:7'),
    ('local_g128', {'sc_local_g': 128}, 'plain', 18, None, 'L128+pre:11 T128:7'),
    ('local_g128', {'sc_local_g': 128}, 'product', 16, None, 'L128:9 T128:7'),
    ('local_g128', {'sc_local_g': 128}, 'product', 17, None, 'L128+pre:10 T128:7'),
    ('local_g128', {'sc_local_g': 128}, 'fold', 17, None, 'L128:10 T128:7'),
    ('local_g128', {'sc_local_g': 128}, 'fold', 18, None, 'L128+pre:11 T128:7'),
    ('local_g128', {'sc_local_g': 128}, 'open', 17, None, 'L128:10 T128:7'),
    ('local_g128', {'sc_local_g': 128}, 'open', 18, None, 'L128+pre:11 T128:7'),
    ('local_g512', {'sc_local_g': 512}, 'plain', 19, None, 'L512:10 T512:9'),
    ('local_g512', {'sc_local_g': 512}, 'plain', 20, None, 'L512+pre:11 T512:9'),
    ('local_g512', {'sc_local_g': 512}, 'product', 18, None, 'L512:9 T512:9'),
    ('local_g512', {'sc_local_g': 512}, 'product', 19, None, 'L512+pre:10 T512:9'),
    ('local_g512', {'sc_local_g': 512}, 'fold', 19, None, 'L512:10 T512:9'),
    ('local_g512', {'sc_local_g': 512}, 'fold', 20, None, 'L512+pre:11 T512:9'),
    ('local_g512', {'sc_local_g': 512}, 'open', 19, None, 'L512:10 T512:9'),
    ('local_g512', {'sc_local_g': 512}, 'open', 20, None, 'L512+pre:11 T512:9'),
    ('pre0', {'sc_local_g': 16, 'sc_pre': 0}, 'plain', 16, None, 'P2h L16:10 T16:4'),
    ('pre0', {'sc_local_g': 16, 'sc_pre': 0}, 'plain', 17, None, 'P3h L16:10 T16:4'),
    ('pre0', {'sc_local_g': 16, 'sc_pre': 0}, 'product', 15, None, 'P2h L16:9 T16:4'),
    ('pre0', {'sc_local_g': 16, 'sc_pre': 0}, 'fold', 18, None, 'P4h L16:10 T16:4'),
    ('pre0', {'sc_local_g': 16, 'sc_pre': 0}, 'open', 16, None, 'P2h L16:10 T16:4'),
    ('pre1', {'sc_local_g': 16, 'sc_pre': 1}, 'plain', 16, None, 'P2h L16:10 T16:4'),
    ('pre1', {'sc_local_g': 16, 'sc_pre': 1}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('pre1', {'sc_local_g': 16, 'sc_pre': 1}, 'product', 15, None, 'P1h L16+pre:10 T16:4'),
    ('pre1', {'sc_local_g': 16, 'sc_pre': 1}, 'fold', 18, None, 'P4h L16:10 T16:4'),
    ('pre1', {'sc_local_g': 16, 'sc_pre': 1}, 'open', 16, None, 'P2h L16:10 T16:4'),
    ('pre2', {'sc_local_g': 16, 'sc_pre': 2}, 'plain', 16, None, 'P1h L16+pre:11 T16:4'),
    ('pre2', {'sc_local_g': 16, 'sc_pre': 2}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('pre2', {'sc_local_g': 16, 'sc_pre': 2}, 'product', 15, None, 'P1h L16+pre:10 T16:4'),
    ('pre2', {'sc_local_g': 16, 'sc_pre': 2}, 'fold', 18, None, 'P3h L16+pre:11 T16:4'),
    ('pre2', {'sc_local_g': 16, 'sc_pre': 2}, 'open', 16, None, 'P1h L16+pre:11 T16:4'),
    ('handover0', {'sc_local_g': 16, 'sc_handover': 0}, 'plain', 17, None, 'P2 L16+pre:11 T16:4'),
    ('handover0', {'sc_local_g': 16, 'sc_handover': 0}, 'product', 16, None, 'P2 L16+pre:10 T16:4'),
    ('handover0', {'sc_local_g': 16, 'sc_handover': 0}, 'fold', 18, None, 'P4 L16:10 T16:4'),
    ('handover0', {'sc_local_g': 16, 'sc_handover': 0}, 'fold', 19, None, 'P4 L16+pre:11 T16:4'),
    ('handover0', {'sc_local_g': 16, 'sc_handover': 0}, 'open', 16, None, 'P2 L16:10 T16:4'),
    ('handover1', {'sc_local_g': 16, 'sc_handover': 1}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('handover1', {'sc_local_g': 16, 'sc_handover': 1}, 'product', 16, None, 'P2h L16+pre:10 T16:4'),
    ('handover1', {'sc_local_g': 16, 'sc_handover': 1}, 'fold', 18, None, 'P4h L16:10 T16:4'),
    ('handover1', {'sc_local_g': 16, 'sc_handover': 1}, 'fold', 19, None, 'P4h L16+pre:11 T16:4'),
    ('handover1', {'sc_local_g': 16, 'sc_handover': 1}, 'open', 16, None, 'P2h L16:10 T16:4'),
    ('xcd0', {'sc_local_g': 32, 'sc_xcd': 0}, 'plain', 17, None, 'P2h L32:10 T32:5'),
    ('xcd0', {'sc_local_g': 32, 'sc_xcd': 0}, 'product', 16, None, 'P1h L32+pre:10 T32:5'),
    ('xcd0', {'sc_local_g': 32, 'sc_xcd': 0}, 'fold', 16, None, 'L32+pre:11 T32:5'),
    ('xcd0', {'sc_local_g': 32, 'sc_xcd': 0}, 'open', 18, None, 'P2h L32+pre:11 T32:5'),
    ('xcd1', {'sc_local_g': 32, 'sc_xcd': 1}, 'plain', 17, None, 'P2h L32:10 T32:5'),
    ('xcd1', {'sc_local_g': 32, 'sc_xcd': 1}, 'product', 16, None, 'P1h L32+pre:10 T32:5'),
    ('xcd1', {'sc_local_g': 32, 'sc_xcd': 1}, 'fold', 16, None, 'L32+pre:11 T32:5'),
    ('xcd1', {'sc_local_g': 32, 'sc_xcd': 1}, 'open', 18, None, 'P2h L32+pre:11 T32:5'),
    ('kf0', {'sc_local_g': 16, 'sc_kf': 0}, 'fold', 17, None, 'P3h L16:10 T16:4'),
    ('kf1', {'sc_local_g': 16, 'sc_kf': 1}, 'fold', 16, None, 'P1h L16+pre:11 T16:4'),
    ('kf2', {'sc_local_g': 16, 'sc_kf': 2}, 'fold', 16, None, 'P2h L16:10 T16:4'),
    ('kf3', {'sc_local_g': 16, 'sc_kf': 3}, 'fold', 17, None, 'P3h L16:10 T16:4'),
    ('kf4', {'sc_local_g': 16, 'sc_kf': 4}, 'fold', 18, None, 'P4h L16:10 T16:4'),
    ('kf4_twice', {'sc_local_g': 4, 'sc_kf': 4}, 'fold', 20, None, 'P4 P4 L4:10 T4:2'),
    ('kf0_k0_1', {'sc_local_g': 16, 'sc_kf': 0, 'sc_k0': 1}, 'fold', 16, None, 'P1h L16+pre:11 T16:4'),
    ('plain_flat0_k0_1', {'sc_local_g': 16, 'sc_plain_flat': 0, 'sc_k0': 1}, 'plain', 16, None, 'P1h L16+pre:11 T16:4'),
    ('plain_flat0_k0_1', {'sc_local_g': 16, 'sc_plain_flat': 0, 'sc_k0': 1}, 'plain', 18, None, 'P1 P1 P1h L16+pre:11 T16:4'),
    ('plain_flat1_k0_1', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 1}, 'plain', 16, None, 'P1h L16+pre:11 T16:4'),
    ('plain_flat1_k0_1', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 1}, 'plain', 18, None, 'P1 P1 P1h L16+pre:11 T16:4'),
    ('plain_flat1_k0_1', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 1}, 'open', 16, None, 'P1h L16+pre:11 T16:4'),
    ('plain_flat1_k0_1', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 1}, 'open', 18, None, 'P1 P1 P1h L16+pre:11 T16:4'),
    ('kf0_k0_2', {'sc_local_g': 16, 'sc_kf': 0, 'sc_k0': 2}, 'fold', 16, None, 'P2h L16:10 T16:4'),
    ('plain_flat0_k0_2', {'sc_local_g': 16, 'sc_plain_flat': 0, 'sc_k0': 2}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('plain_flat0_k0_2', {'sc_local_g': 16, 'sc_plain_flat': 0, 'sc_k0': 2}, 'plain', 18, None, 'P2 P2h L16:10 T16:4'),
    ('plain_flat1_k0_2', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 2}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('plain_flat1_k0_2', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 2}, 'plain', 18, None, 'P2 P2h L16:10 T16:4'),
    ('plain_flat1_k0_2', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 2}, 'open', 17, None, 'P2h L16+pre:11 T16:4'),
    ('plain_flat1_k0_2', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 2}, 'open', 18, None, 'P2 P2h L16:10 T16:4'),
    ('kf0_k0_3', {'sc_local_g': 16, 'sc_kf': 0, 'sc_k0': 3}, 'fold', 17, None, 'P3h L16:10 T16:4'),
    ('plain_flat0_k0_3', {'sc_local_g': 16, 'sc_plain_flat': 0, 'sc_k0': 3}, 'plain', 18, None, 'P3h L16+pre:11 T16:4'),
    ('plain_flat1_k0_3', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 3}, 'plain', 18, None, 'P3h L16+pre:11 T16:4'),
    ('plain_flat1_k0_3', {'sc_local_g': 16, 'sc_plain_flat': 1, 'sc_k0': 3}, 'open', 18, None, 'P3h L16+pre:11 T16:4'),
    ('kp1', {'sc_local_g': 16, 'sc_kp': 1}, 'product', 15, None, 'P1h L16+pre:10 T16:4'),
    ('kp1', {'sc_local_g': 16, 'sc_kp': 1}, 'product', 17, None, 'P1 P1 P1h L16+pre:10 T16:4'),
    ('kp2', {'sc_local_g': 16, 'sc_kp': 2}, 'product', 16, None, 'P2h L16+pre:10 T16:4'),
    ('kp2', {'sc_local_g': 16, 'sc_kp': 2}, 'product', 17, None, 'P2 P1h L16+pre:10 T16:4'),
    ('kp3', {'sc_local_g': 16, 'sc_kp': 3}, 'product', 17, None, 'P3h L16+pre:10 T16:4'),
    ('kp3_t1dev', {'sc_local_g': 16, 'sc_kp': 3, 'sc_t1_device': 1}, 'product', 17, None, 'P3h L16+pre:10 T16:4'),
    ('kp3_t1dev', {'sc_local_g': 16, 'sc_kp': 3, 'sc_t1_device': 1}, 'product', 18, None, 'P3 P1h L16+pre:10 T16:4'),
    ('pass_wg1', {'sc_local_g': 16, 'sc_pass_wg': 1, 'sc_kf': 0, 'sc_plain_flat': 0, 'sc_k0': 2, 'sc_kp': 2}, 'plain', 20, None, 'P2x4 P2 P2h L16:10 T16:4'),
    ('pass_wg1', {'sc_local_g': 16, 'sc_pass_wg': 1, 'sc_kf': 0, 'sc_plain_flat': 0, 'sc_k0': 2, 'sc_kp': 2}, 'product', 20, None, 'P2x4 P2 P2h L16+pre:10 T16:4'),
    ('pass_wg1', {'sc_local_g': 16, 'sc_pass_wg': 1, 'sc_kf': 0, 'sc_plain_flat': 0, 'sc_k0': 2, 'sc_kp': 2}, 'fold', 20, None, 'P2x4 P2 P2h L16:10 T16:4'),
    ('pass_wg1', {'sc_local_g': 16, 'sc_pass_wg': 1, 'sc_kf': 0, 'sc_plain_flat': 0, 'sc_k0': 2, 'sc_kp': 2}, 'open', 20, None, 'P2x4 P2 P2h L16:10 T16:4'),
    ('flat_wg1', {'sc_local_g': 16, 'sc_flat_wg': 1, 'sc_kf': 2}, 'fold', 20, None, 'P2x4 P2 P2h L16:10 T16:4'),
    ('plain_wg1', {'sc_local_g': 16, 'sc_plain_wg': 1, 'sc_k0': 2}, 'plain', 20, None, 'P2x4 P2 P2h L16:10 T16:4'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'plain', 12, None, 'L4:10 T4:2'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'product', 12, None, 'L8:9 T8:3'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'product', 15, None, 'P1h L16+pre:10 T16:4'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'fold', 12, None, 'L4:10 T4:2'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'fold', 19, None, 'P4h L16+pre:11 T16:4'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'open', 12, None, 'L4:10 T4:2'),
    ('local_threads256', {'sc_local_g': 16, 'sc_local_threads': 256}, 'open', 17, None, 'P2h L16+pre:11 T16:4'),
    ('local_threads256_default_g', {'sc_local_threads': 256}, 'plain', 19, None, 'L256+pre:11 T256:8'),
    ('local_threads256_default_g', {'sc_local_threads': 256}, 'product', 18, None, 'L256+pre:10 T256:8'),
    ('local_threads256_default_g', {'sc_local_threads': 256}, 'fold', 19, None, 'L256+pre:11 T256:8'),
    ('local_threads256_default_g', {'sc_local_threads': 256}, 'open', 19, None, 'L256+pre:11 T256:8'),
    ('pinned_out0', {'sc_local_g': 16, 'sc_pinned_out': 0}, 'plain', 9, None, 'T512:9'),
    ('pinned_out0', {'sc_local_g': 16, 'sc_pinned_out': 0}, 'plain', 17, None, 'P2h L16+pre:11 T16:4'),
    ('pinned_out0', {'sc_local_g': 16, 'sc_pinned_out': 0}, 'product', 9, None, 'T512:9'),
    ('pinned_out0', {'sc_local_g': 16, 'sc_pinned_out': 0}, 'product', 16, None, 'P2h L16+pre:10 T16:4'),
    ('pinned_out0', {'sc_local_g': 16, 'sc_pinned_out': 0}, 'fold', 17, None, 'P3h L16:10 T16:4'),
    ('pinned_out0', {'sc_local_g': 16, 'sc_pinned_out': 0}, 'open', 9, None, 'T512:9'),
    ('pinned_out0', {'sc_local_g': 16, 'sc_pinned_out': 0}, 'open', 17, None, 'P2h L16+pre:11 T16:4'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 18, 2, 'P2'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 18, 3, 'P3'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 18, 7, 'P3h L16+pre:4'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 18, 14, 'P3h L16+pre:11'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 18, 16, 'P3h L16+pre:11 T16:2'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 19, 1, 'P1'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 19, 4, 'P4'),
    ('partial_fold', {'sc_local_g': 16}, 'fold', 19, 5, 'P4h L16+pre:1'),
]
