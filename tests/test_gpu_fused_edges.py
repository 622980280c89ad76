"""
The six fused identity sumchecks in both forms -- preset challenges (csrc/zk_fused.cuh) and transcript-driven (csrc/zk_fs.hip) -- at
extreme STORED values, bit-exact against the identities' big-int models and, on constant tables, against closed forms.  What they
share and the core family does not use is the lazily reduced arithmetic of csrc/zk_gate.cuh: per-lane 17-limb sums of raw 512-bit
products (fp_mac_wide), their addition across lanes (gate_wide_add), the lookups' free term at weight 2^256 (gate_wide_add_hi) and the
one reduction W0 R^-1 + W1 + W2 R (gate_reduce_value).  The cases live in tests/fused_edge_cases.py; which case sets limb 16 through
the wave shuffle, which passes 2^512 inside one lane, which carries out of limb 15 and which puts W0 / W1 into which band of
[0, r), [r, 2r), [2r, 2^256) is proved without a GPU in tests/test_fused_edge_inputs.py.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import fused_edge_cases as fe
from helpers import fr_ints, fr_limbs

pytestmark = pytest.mark.gpu

KINDS = sorted(fe.KINDS)
_MODEL, _FS_MODEL = {}, {}


def limbs(xs):
    return np.array([fr_limbs(x) for x in xs], dtype=np.uint64).reshape(-1, 4)


class knobs:
    """set tuning knobs for a block; every one goes back to the value zk_dbg_tune_get returned, whatever happens inside"""

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        from zkhip._lib import test_hooks

        self.lib, self.found = test_hooks(), {}
        for k in self.kv:
            v = ctypes.c_long(0)
            assert self.lib.zk_dbg_tune_get(k.encode(), ctypes.byref(v)) == 0, k
            self.found[k] = v.value
        try:
            for k, v in self.kv.items():
                assert self.lib.zk_dbg_tune(k.encode(), v) == 0, k
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in self.found.items():
            self.lib.zk_dbg_tune(k.encode(), v)
        return False


def call(ctx, kind, d, N, gamma, chal=None, tr=None):
    """the preset-challenge form (chal) or the transcript-driven one (tr) on device buffers d: name -> buffer"""
    K = fe.KINDS[kind]
    g = fr_limbs(gamma)
    tail = (limbs(chal),) if tr is None else (tr,)
    sfx = "" if tr is None else "_fs"
    if kind == "gate":
        return getattr(ctx, "sumcheck_gate" + sfx)(*[d[k] for k in K.uploaded], N, *tail)
    if kind == "wiring":
        return getattr(ctx, "sumcheck_wiring" + sfx)(d["eq"], d["tree"], d["num"], d["den"], N, g, *tail)
    if kind == "perm3":
        return getattr(ctx, "sumcheck_perm3" + sfx)(d["eq"], d["tree"], [d["n0"], d["n1"], d["n2"]], [d["d0"], d["d1"], d["d2"]], N, g, *tail)
    if kind == "gate_wide":
        return getattr(ctx, "sumcheck_gate_wide" + sfx)([d[k] for k in K.uploaded], N, *tail)
    name = "sumcheck_lookup" if kind == "lookup" else "sumcheck_lookup_sel"
    return getattr(ctx, name + sfx)([d[k] for k in K.uploaded], N, g, *tail)


def fresh(ctx):
    from zkhip.transcript import Transcript

    return Transcript(ctx, b"diff").absorb(fe.SEED)


def replay(rounds):
    """the challenges of a transcript-driven call from its evaluations, by hashlib (fs_model.py's definition) -> (stored challenges, state)"""
    import fs_model as fm

    tr = fm.Model(b"diff").absorb(fe.SEED)
    chal = [tr.absorb(np.ascontiguousarray(p, dtype="<u8").tobytes()).challenge() for p in rounds]
    return fe.to_stored(chal), tr.state


def model(kind, pattern, gname, cname, mu):
    key = (kind, pattern, gname, cname, mu)
    if key not in _MODEL:
        _MODEL[key] = fe.model_preset(kind, fe.inputs(kind, pattern, mu)[0], fe.gamma_of(kind, pattern, gname, mu), fe.challenges(cname, mu))
    return _MODEL[key]


def upload(ctx, ins):
    return {k: ctx.to_device(limbs(v)) for k, v in ins.items()}


def unchanged(d, ins, what):
    for k, v in ins.items():
        assert fr_ints(d[k].download((len(v), 4))) == v, f"{what}: input table {k} was written"


def same(got_rounds, got_last, want, K, mu, what):
    assert got_rounds.shape == (mu, K.evals, 4) and got_last.shape == (len(K.tables), 4), what
    got = [fr_ints(p) for p in got_rounds]
    for i in range(mu):
        assert got[i] == want[0][i], f"{what}: round {i} differs"
    assert fr_ints(got_last) == want[1], f"{what}: last values differ"


@pytest.mark.parametrize("mu,local_e", fe.SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_preset_form_on_extreme_stored_values(ctx, kind, mu, local_e):
    K = fe.KINDS[kind]
    by_pattern = {}
    for p, g, c in fe.combos(kind, mu):
        by_pattern.setdefault(p, []).append((g, c))
    with knobs(**{K.knob: local_e}):
        for p, gcs in by_pattern.items():
            ins = fe.inputs(kind, p, mu)[0]
            d = upload(ctx, ins)
            for g, c in gcs:
                what = f"{kind} mu={mu} local_e={local_e} {p} gamma={g} chal={c}"
                rounds, last = call(ctx, kind, d, 1 << mu, fe.gamma_of(kind, p, g, mu), chal=fe.challenges(c, mu))
                same(rounds, last, model(kind, p, g, c, mu), K, mu, what)
            unchanged(d, ins, f"{kind} mu={mu} {p}")


@pytest.mark.parametrize("mu,local_e", fe.SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_transcript_form_on_extreme_stored_values(ctx, kind, mu, local_e):
    """a fresh transcript per call: the challenges are hashlib's, the parent returns the same bits on them, and both match the model"""
    K = fe.KINDS[kind]
    with knobs(**{K.knob: local_e}):
        for p, g in fe.fs_combos(kind, mu):
            what = f"{kind} mu={mu} local_e={local_e} {p} gamma={g} (transcript)"
            ins, gamma = fe.inputs(kind, p, mu)[0], fe.gamma_of(kind, p, g, mu)
            d = upload(ctx, ins)
            tr = fresh(ctx)
            rounds, last, chal = call(ctx, kind, d, 1 << mu, gamma, tr=tr)
            want_chal, state = replay(rounds)
            assert chal.shape == (mu, 4) and fr_ints(chal) == want_chal and tr.state() == state, f"{what}: challenges differ from the hashlib replay"
            tr.free()
            p_rounds, p_last = call(ctx, kind, d, 1 << mu, gamma, chal=want_chal)
            assert (rounds == p_rounds).all() and (last == p_last).all(), f"{what}: differs from the parent on its own challenges"
            key = (kind, p, g, mu)
            if key not in _FS_MODEL:
                _FS_MODEL[key] = fe.model_fs(kind, ins, gamma)
            same(rounds, last, _FS_MODEL[key][:2], K, mu, what)
            assert want_chal == _FS_MODEL[key][2], what
            unchanged(d, ins, what)


# ---- one lane past 2^512 (C3) and the free term's carry out of limb 15 (C4): constant tables at the smallest size that gets there ----
def cu_count():
    """read from the device (the passes launch workgroups per CU): hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount = 63)"""
    v = ctypes.c_int(0)
    assert ctypes.CDLL("libamdhip64.so").hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0
    return v.value


@pytest.mark.parametrize("kind", KINDS)
def test_one_lane_passes_2_to_512(ctx, kind):
    """
    macM constants (both operands of every fp_mac_wide are M); the size comes from the companion's lane model fed this device's CU count:
    the busiest lane of the first pass sums `it` >= 5 products of (r-1)^2 ~ 0.205 * 2^512, so the carry of its last column into limb 16
    is set inside the loop, and for the lookups hf = M / it makes its g0 = M, which carries out of limb 15 when it is added at 2^256.
    Expected: the closed form h (E B R^-1 + F) of every round and the constants as last values, in both forms.
    """
    K = fe.KINDS[kind]
    cu = cu_count()
    case = fe.large_case(kind, cu)
    assert case is not None, f"{kind}: with {cu} CUs no table of up to 2^22 elements takes one lane past 2^512"
    mu, tune, const, gamma, it = case
    per_cu = 1 if K.pass_wg else K.per_cu
    it2, p, g0 = fe.lane_model(kind, const, gamma, mu, cu, per_cu)
    assert it2 == it >= 5 and p >> 512, "C3 is not reached"
    assert not K.free or (((p >> 256) & fe.MASK) + g0) >> 256, "C4 is not reached"
    N = 1 << mu
    bufs = {}  # one device buffer per distinct constant (the tree: 2N elements): inputs are never written (the small cases prove it)
    d = {}
    for k in K.uploaded:
        key = (const.get(k, 0), 2 * N if k == "tree" else N)
        if key not in bufs:
            bufs[key] = ctx.to_device(np.tile(fr_limbs(key[0]), (key[1], 1)))
        d[k] = bufs[key]
    want = fe.closed_form(kind, const, gamma, mu)
    with knobs(**tune):
        rounds, last = call(ctx, kind, d, N, gamma, chal=fe.challenges("rand", mu))
        same(rounds, last, want, K, mu, f"{kind} 2^{mu} constants, {it} products per lane")
        tr = fresh(ctx)
        rounds, last, chal = call(ctx, kind, d, N, gamma, tr=tr)
        same(rounds, last, want, K, mu, f"{kind} 2^{mu} constants, {it} products per lane (transcript)")
        want_chal, state = replay(rounds)
        assert fr_ints(chal) == want_chal and tr.state() == state
        tr.free()
