"""
The six preset-challenge fused sumchecks share one engine (csrc/zk_fused.cuh): every identity through one table of the shapes at which
the shared driver can go wrong -- 0, 1, 2 and 3 HBM passes (no arena, arena 0, arenas 0 and 1, arena 0 reused), a local stage of zero
rounds, and the shortest legal table -- bit-exact against the big-int models of the identities' own tests.  The grid-stride path of
the passes needs tables of 2^18 elements and stays with the large-size tests of each identity.
"""
import ctypes

import pytest

import lookup_model as lm
import plonk_lookup_model as plm
import plonk_model as pm
import pyoracle as po
import widegate_model as wg
import wiring_model as wm
import zerocheck_model as zm

pytestmark = pytest.mark.gpu


def _tree_call(name, nums, dens):
    """the identities on the product tree: eq, the tree (2N elements, its four views are only the model's) and the num / den columns"""

    def call(ctx, d, N, gamma, chal):
        n, dn = [d[k] for k in nums], [d[k] for k in dens]
        if len(nums) == 1:
            n, dn = n[0], dn[0]
        return getattr(ctx, name)(d["eq"], d["tree"], n, dn, N, gamma, chal)

    return call


# kind -> (its hand-over knob, the model's tables, what is uploaded, model(tabs, gamma, chal), call(ctx, buffers, N, gamma, chal))
KINDS = {
    "gate": (b"gate_local_e", zm.TABLES, zm.TABLES, lambda t, g, ch: zm.sumcheck_gate(t, ch),
             lambda ctx, d, N, g, ch: ctx.sumcheck_gate(*[d[k] for k in zm.TABLES], N, ch)),
    "wiring": (b"wiring_local_e", wm.TABLES, ("eq", "tree", "num", "den"), wm.sumcheck_wiring, _tree_call("sumcheck_wiring", ("num",), ("den",))),
    "perm3": (b"perm3_local_e", pm.TABLES, ("eq", "tree", "n0", "n1", "n2", "d0", "d1", "d2"), pm.sumcheck_perm3,
              _tree_call("sumcheck_perm3", ("n0", "n1", "n2"), ("d0", "d1", "d2"))),
    "gate_wide": (b"gatew_local_e", wg.TABLES, wg.TABLES, lambda t, g, ch: wg.sumcheck_gate_wide(t, ch),
                  lambda ctx, d, N, g, ch: ctx.sumcheck_gate_wide([d[k] for k in wg.TABLES], N, ch)),
    "lookup": (b"lookup_local_e", lm.TABLES, lm.TABLES, lm.sumcheck_lookup,
               lambda ctx, d, N, g, ch: ctx.sumcheck_lookup([d[k] for k in lm.TABLES], N, g, ch)),
    "lookup_sel": (b"lookupsel_local_e", plm.TABLES, plm.TABLES, plm.sumcheck_lookup_sel,
                   lambda ctx, d, N, g, ch: ctx.sumcheck_lookup_sel([d[k] for k in plm.TABLES], N, g, ch)),
}

# (value of the kind's *_local_e knob or None for its default, mu): with the knob at 2, mu = 1 .. 4 are 0 .. 3 HBM passes; with it at 1
# the local stage has zero rounds and only hands back the last values; the default at mu = 1 is the shortest legal table
SHAPES = [(2, 1), (2, 2), (2, 3), (2, 4), (1, 3), (None, 1)]

# the order of the tables is the order of the calls' arguments and of their last values: what this file relies on in the models
assert zm.TABLES == ("eq", "q1", "q2", "a", "b", "c", "in") and wm.TABLES == ("eq", "v1x", "vx0", "vx1", "h", "num", "den")
assert pm.TABLES == ("eq", "v1x", "vx0", "vx1", "h", "n0", "n1", "n2", "d0", "d1", "d2")
assert wg.TABLES == ("eq", "qL", "qR", "qM", "qO", "qC", "qH", "a", "b", "c", "in")
assert lm.TABLES == ("E", "df", "dt", "m", "hf", "ht") and plm.TABLES == lm.TABLES + ("qk",)

_CASES = {}


def _case(kind, mu):
    """random tables (the rounds are defined for ANY tables), gamma, challenges and the model's run: computed once per (kind, mu)"""
    if (kind, mu) not in _CASES:
        _knob, tables, uploaded, model, _call = KINDS[kind]
        rng = po.SplitMix64(7700 + 100 * sorted(KINDS).index(kind) + mu)
        N = 1 << mu
        ins = {k: rng.fr_vec(2 * N if k == "tree" else N) for k in uploaded}
        tabs = dict(ins)
        if "tree" in ins:
            tabs.update(wm.views(ins["tree"]))
        gamma, chal = rng.fr(), rng.fr_vec(mu)
        _CASES[(kind, mu)] = (ins, gamma, chal, model({k: tabs[k] for k in tables}, gamma, chal))
    return _CASES[(kind, mu)]


@pytest.mark.parametrize("local_e,mu", SHAPES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_kind_through_the_shared_driver(ctx, kind, local_e, mu):
    from zkhip._lib import test_hooks

    knob, tables, uploaded, _model, call = KINDS[kind]
    ins, gamma, chal, (want_rounds, want_last) = _case(kind, mu)
    lib = test_hooks()
    found = ctypes.c_long(0)
    assert lib.zk_dbg_tune_get(knob, ctypes.byref(found)) == 0
    try:
        if local_e is not None:
            assert lib.zk_dbg_tune(knob, local_e) == 0
        d = {k: ctx.to_device(zm.mont(v)) for k, v in ins.items()}
        rounds, last = call(ctx, d, 1 << mu, zm.mont([gamma])[0], zm.mont(chal))
    finally:
        lib.zk_dbg_tune(knob, found.value)
    assert rounds.shape == (mu, len(want_rounds[0]), 4) and last.shape == (len(tables), 4)
    assert [zm.ints(r) for r in rounds] == want_rounds
    assert zm.ints(last) == want_last
    for k, v in ins.items():
        assert zm.ints(d[k].download((len(v), 4))) == v, f"input table {k} was written"
