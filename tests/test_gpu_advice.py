"""
Advice rows on the device: zk_plonk_witness / zk_plonk_witness_lookup on plans of zk_witness_plan_create_advice, limb for limb against the
model of the rules (advice_model.py), and zk_witness_plan_info against the model's plan -- one flat level of more than 256 advice rows
(the grid kernel) over the shifts, widths and inputs at the edges of the 32- and 64-bit limbs, runs of levels in one workgroup, levels of
exactly 256 and 257 rows, an advice plan with a lookup (also under find_force_slot), all-zero advice through the new creator, every refusal
with its exact numbers, and the check's four / six numbers on an advice plan.  All at N <= 2^11.
"""
import numpy as np
import pytest

import advice_model as am
import witness_lookup_model as wlm
import witness_model as wm
from test_gpu_witness_lookup import _Knob

pytestmark = pytest.mark.gpu

R = wm.R
LK = ("qk", "t0", "t1", "t2")
SHIFTS = (0, 60, 63, 64, 127, 128, 191, 192, 254)
WIDTHS = (1, 8, 32, 63, 64)
VALUES = (0, 1, R - 1, (1 << 64) - 1, 1 << 64, 1 << 254)


def _rand(k: int) -> int:
    """a fixed stream of integers below r with bits everywhere"""
    return pow(0x9E3779B97F4A7C15 + 2 * k + 1, 5 + k % 7, R)


def device_witness(ctx, c: dict, free_limbs, lookup: bool = False):
    """-> (pk, plan, the three wire columns as arrays, the error message or None)"""
    from zkhip import plonk

    pk, plan = plonk.witness_key(ctx, c), plonk.witness_plan(ctx, c, lookup=lookup)
    N = 1 << c["mu"]
    out = tuple(ctx.alloc(32 * N) for _ in range(3))
    sels, pi, lk = plonk._witness_args(pk, plan, c["public_inputs"])
    message = None
    try:
        ctx.plonk_witness(plan, sels, pi, None if free_limbs is None else ctx.to_device(free_limbs), out, **lk)
    except ValueError as e:
        message = str(e)
    return pk, plan, [x.download((N, 4)) for x in out], message


def assert_equals_model(ctx, c: dict, lookup: bool = False, free=None):
    """free: the integers below 2^256 the caller stores (default: the circuit's); a value at or above r is stored as it stands"""
    free = c["free"] if free is None else free
    p = am.plan(c, lookup)
    pk, plan, got, message = device_witness(ctx, c, am.free_limbs(free), lookup)
    assert message is None, message
    assert plan.info() == am.info(p)
    want = am.generate(c, p, c["public_inputs"], am.free_values(free))
    for name, g, w in zip("abc", got, want):
        bad = np.nonzero((g != wm.limbs(w)).any(axis=1))[0]
        assert not len(bad), (name, int(bad[0]), p["advice"][int(bad[0])])
    return pk, plan, got, p


def flat_items() -> list:
    """every (shift, width) of the lists that is a code, the pairs with shift + width = 255, INV0; each on the edge values and random ones"""
    codes = [am.bits(s, w) for s in SHIFTS for w in WIDTHS if s + w <= 255] + [am.bits(255 - w, w) for w in WIDTHS] + [am.bits(24, 16), am.bits(56, 16), am.bits(40, 64)]
    items, k = [], 0
    for code in codes:
        for v in VALUES + (_rand(k), _rand(k + 1)):
            items.append((code, v))
        k += 2
    for v in VALUES + tuple(_rand(1000 + i) for i in range(40)):
        items.append((am.INV0, v))
    return items


def test_one_flat_level_on_the_grid(ctx):
    items = flat_items()
    mu, l = 9, 4
    assert 256 < len(items) <= (1 << mu) - l and any(am.known(c) and (c >> 8 & 0xFF) + (c >> 16 & 0xFF) == 255 for c, _ in items)
    c = am.flat(mu, l, items)
    _, plan, got, p = assert_equals_model(ctx, c)
    assert plan.info() == {"levels": 1, "max_level_rows": l + len(items), "launches": 1}
    # the bit fields against their definition, not only against the model's function
    cs = wm.ints(got[2])
    for i, (code, v) in enumerate(items):
        if code != am.INV0:
            assert cs[l + i] == (v >> (code >> 8 & 0xFF)) & ((1 << (code >> 16 & 0xFF)) - 1)
        else:
            assert cs[l + i] * v % R == (1 if v else 0)


def test_free_values_at_or_above_r_are_reduced_first(ctx):
    """stored limbs in [r, 2^256), below 3 r: the Montgomery form is reduced below r by at most two subtractions, then the advice acts"""
    stored = [R, R + 1, 2 * R - 1, 2 * R, 2 * R + 12345, (1 << 256) - (1 << 32), (1 << 256) - 1, (1 << 255) + 7]
    items = [(code, v) for v in stored for code in (am.INV0, am.bits(0, 64), am.bits(60, 8), am.bits(191, 64), am.bits(254, 1))]
    items += [(am.bits(7 * (i % 30), 13), _rand(i)) for i in range(300 - len(items))]  # a grid level
    c = am.flat(9, 4, items)
    assert_equals_model(ctx, c)
    small = am.flat(6, 4, items[:40])  # and in the single-workgroup kernel
    assert_equals_model(ctx, small)


def test_two_hundred_alternating_levels_in_one_workgroup(ctx):
    mu, l, levels = 8, 4, 200
    c = am.inverse_chain(mu, l, levels)
    _, plan, got, _ = assert_equals_model(ctx, c)
    assert plan.info() == {"levels": levels + 1, "max_level_rows": l + 1, "launches": 1}
    cs = wm.ints(got[2])
    assert cs[l] == 12346 and cs[l + 2] == cs[l + 1] == pow(12346, -1, R) and cs[l + 3] == 12346 and cs[l + 4] == 12346  # the inverse of the inverse


def test_levels_that_mix_gate_and_advice_rows(ctx):
    c = am.mixed(10, 4, 100, 9)  # nine levels of 100 rows: gate rows, INV0 rows and bit fields side by side, each reading the level below
    _, plan, _, p = assert_equals_model(ctx, c)
    assert plan.info()["launches"] == 1 and all({am.GATE, am.ADVICE} <= {p["kind"][x] for x in rows} for rows in p["levels"])


@pytest.mark.parametrize("width", [252, 253])
def test_the_launch_split_boundary(ctx, width):
    """with the four input rows level 0 has exactly 256 / 257 rows: the last level of a run, or a grid launch of its own; two levels follow"""
    c = am.mixed(10, 4, width, 3)
    _, plan, _, p = assert_equals_model(ctx, c)
    assert len(p["levels"][0]) == width + 4
    assert plan.info() == {"levels": 3, "max_level_rows": width + 4, "launches": 1 if width == 252 else 2}


def lookup_circuit(mu: int = 9, l: int = 4, width: int = 60, k: int = 4) -> dict:
    """level 0: `width` lookup rows on free pairs (XOR of two k-bit values; every third pair is in no entry: c = 0); level 1: an advice row on
    each -- INV0 or a bit field; level 2: a gate row c = 5 a + 2 on each advice output; then 300 advice rows on free values so that level 0
    is a grid launch"""
    N = 1 << mu
    low = (1 << k) - 1
    rows = []
    for j in range(width):
        rows.append(am.lookup_row(("free", (3 * j + 1) & low), ("free", ((j * j + 11) & low) + (1 << k if j % 3 == 2 else 0))))
    for j in range(width):
        rows.append(am.advice_row(am.INV0 if j % 2 else am.bits(j % 3, 2), ("c", l + j)))
    for j in range(width):
        rows.append(am.gate_row(("c", l + width + j), qL=5, qC=2))
    for j in range(300):
        rows.append(am.advice_row(am.bits(j % 200, 1 + j % 64) if j % 4 else am.INV0, ("free", _rand(j))))
    return am.circuit_of(mu, l, rows, wlm.xor_table(N, k))


def test_an_advice_plan_with_a_lookup(ctx):
    from zkhip import plonk

    c = lookup_circuit()
    p = am.plan(c, True)
    assert {am.GATE, am.LOOKUP, am.ADVICE} <= set(p["kind"]) and len(p["levels"]) == 3 and len(p["levels"][0]) > 256
    pk, plan, got, message = device_witness(ctx, c, am.free_limbs(c["free"]), True)
    assert plan.info() == am.info(p) == {"levels": 3, "max_level_rows": 364, "launches": 2}
    want = am.generate(c, p, c["public_inputs"], c["free"])
    for name, g, w in zip("abc", got, want):
        assert (g == wm.limbs(w)).all(), name
    rep = am.check(c, p, *want, c["public_inputs"])
    assert rep["bad_lookups"] == 20 and rep["bad_rows"] == rep["bad_copies"] == 0  # the pairs outside the table: reported, and 0 went on
    assert message.endswith(f"20 of 512 rows with qk = 1 hold a triple that is no table entry; the first is row {rep['first_bad_lookup']}")
    assert plonk.check_witness(ctx, pk, plan, *[ctx.to_device(g) for g in got], c["public_inputs"]) == rep
    with _Knob(b"find_force_slot", 0):  # one collision chain from slot 0: the same wires
        _, _, forced, message2 = device_witness(ctx, c, am.free_limbs(c["free"]), True)
    assert message2 == message and all((f == g).all() for f, g in zip(forced, got))


def test_all_zero_advice_is_the_old_plan(ctx):
    from zkhip import plonk

    c = wm.wide_edge()
    free = wm.limbs(c["free"])
    zero = dict(c, advice=np.zeros(8, dtype=np.uint32))
    old, new = plonk.witness_plan(ctx, c), plonk.witness_plan(ctx, zero)
    assert plonk.witness_plan(ctx, zero, advice=False).info() == old.info() == new.info()
    pk = plonk.witness_key(ctx, c)
    a = [x.download((8, 4)) for x in plonk.witness(ctx, pk, old, c["public_inputs"], free)]
    b = [x.download((8, 4)) for x in plonk.witness(ctx, pk, new, c["public_inputs"], free)]
    assert all((x == y).all() for x, y in zip(a, b))
    basic = wm.flat(5)  # the basic gate: all-zero advice is accepted, and is the plain plan
    zb = dict(basic, advice=np.zeros(32, dtype=np.uint32))
    assert plonk.witness_plan(ctx, zb).info() == plonk.witness_plan(ctx, basic).info()
    with pytest.raises(ValueError, match="advice=True needs"):
        plonk.witness_plan(ctx, c, advice=True)


def _refused(ctx, c: dict, lookup: bool = False) -> str:
    from zkhip import plonk

    with pytest.raises(ValueError) as model:
        am.plan(c, lookup)
    with pytest.raises(ValueError) as dev:
        plonk.witness_plan(ctx, c, lookup=lookup)
    assert str(dev.value) == "zk_witness_plan_create_advice: " + str(model.value)
    return str(model.value)


def test_refusals(ctx):
    mu, l = 5, 4
    N = 1 << mu
    ok_rows = [am.advice_row(am.INV0, ("free", 3)) for _ in range(10)]
    # qO != 0 on advice rows
    rows = list(ok_rows)
    rows[3] = am.advice_row(am.INV0, ("free", 3), qO=1)
    rows[7] = am.advice_row(am.bits(0, 8), ("free", 3), qO=5, qL=1)
    assert _refused(ctx, am.circuit_of(mu, l, rows)) == f"2 of {N} advice rows also compute by the gate or the table; the first is row {l + 3}"
    # qk = 1 on an advice row (with qO = 0 it would be lookup-computing), and one that is both
    rows = list(ok_rows)
    rows[2] = dict(am.advice_row(am.INV0, ("free", 3)), qk=1)
    rows[5] = dict(am.advice_row(am.INV0, ("free", 3), qO=1), qk=1)
    c = am.circuit_of(mu, l, rows, wlm.xor_table(N, 2))
    assert _refused(ctx, c, True) == f"2 of {N} advice rows also compute by the gate or the table; the first is row {l + 2}"
    # without the lookup row l + 2 is a plain advice row: one conflict is left
    assert _refused(ctx, c, False) == f"1 of {N} advice rows also compute by the gate or the table; the first is row {l + 5}"
    # the basic gate: every advice row
    basic = wm.flat(mu)
    adv = np.zeros(N, dtype=np.uint32)
    adv[[9, 17, 30]] = (am.INV0, am.bits(3, 3), am.INV0)
    assert _refused(ctx, dict(basic, advice=adv)) == f"3 of {N} advice rows also compute by the gate or the table; the first is row 9"
    # unknown codes: kind 3, width 0, width 65, shift + width = 256, a high byte set -- and the known neighbours of each pass
    for code in (3, am.bits(5, 0), am.bits(5, 65), am.bits(192, 64), am.bits(255, 1), am.INV0 | 1 << 24, am.bits(0, 8) | 1 << 31):
        rows = list(ok_rows)
        rows[6] = am.advice_row(code, ("free", 3))
        assert _refused(ctx, am.circuit_of(mu, l, rows)) == f"1 of {N} advice codes are unknown; the first is row {l + 6}"
    rows = [am.advice_row(code, ("free", 3)) for code in (3, am.INV0, am.bits(0, 65), am.bits(191, 64), am.bits(254, 1), 0xFF)]
    assert _refused(ctx, am.circuit_of(mu, l, rows)) == f"3 of {N} advice codes are unknown; the first is row {l}"
    # an advice row whose a is a copy of its own c, and a gate row that reads it
    rows = list(ok_rows)
    rows[4] = am.advice_row(am.INV0, ("c", l + 4))
    rows[8] = am.gate_row(("c", l + 4), qL=1)
    assert _refused(ctx, am.circuit_of(mu, l, rows)) == f"2 of {N} rows depend on their own output; the first is row {l + 4}"


def test_check_witness_on_an_advice_plan(ctx):
    """the check's four numbers: any wires against the gates and the classes, the advice values not among them"""
    from zkhip import plonk

    c = am.mixed(8, 4, 30, 4)
    pk, plan, got, p = assert_equals_model(ctx, c)
    ints = [wm.ints(g) for g in got]
    last = [x for x in p["levels"][-1] if p["kind"][x] == am.ADVICE][0]  # nobody reads it: any value passes
    ints[2][last] = (ints[2][last] + 99) % R
    first = [x for x in p["levels"][0] if p["kind"][x] == am.ADVICE][0]  # the level above reads it: its copies differ now
    ints[2][first] = (ints[2][first] + 1) % R
    mid = [x for x in p["levels"][1] if p["kind"][x] == am.ADVICE][3]
    ints[0][mid] = (ints[0][mid] + 1) % R                                # an a wire of an advice row: a bad copy, never a bad gate row
    rep = am.check(c, p, *ints, c["public_inputs"])
    assert rep["bad_rows"] == 0 and rep["bad_copies"] == 2
    assert plonk.check_witness(ctx, pk, plan, *[wm.limbs(w) for w in ints], c["public_inputs"]) == rep
