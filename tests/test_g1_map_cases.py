"""
CPU: the cases of tests/g1_map_cases.py are what they claim to be.

  * the closed-form exponent of an output agrees with the Python oracle's own additions, on at most 8 points per case
  * each case has the property it is named for (two equal terms, a cancelling pair, a zero row, an exponent = 0 at the stated index)
  * every scalar a case hands to the library is below r
"""
import pytest

import g1_map_cases as gc
import pyoracle as po

R = gc.R
MAP, PACKED, POWERS, SEQ = gc.map_cases(), gc.packed_cases(), gc.powers_cases(), gc.seq_cases()
_pts = {}


def pt(e):
    e %= R
    if e not in _pts:
        _pts[e] = po.g1_mul(po.G1_GEN, e)
    return _pts[e]


def chain(scalars, exps):
    """sum_c scalars[c] * (exps[c] G), term by term with the oracle's group law"""
    acc = None
    for m, a in zip(scalars, exps):
        acc = po.g1_add(acc, po.g1_mul(pt(a), m))
    return acc


def ids(cases):
    return [c.name for c in cases]


def test_names_are_unique_and_every_aim_is_stated():
    names = ids(MAP) + ids(PACKED) + ids(POWERS) + ids(SEQ)
    assert len(set(names)) == len(names)
    assert all(c.aim for c in MAP + PACKED + POWERS + SEQ)


# ---- A: zk_g1_apply_matrix ----
@pytest.mark.parametrize("case", MAP, ids=ids(MAP))
def test_map_case(case):
    assert all(0 <= m < R for row in case.matrix for m in row) and all(0 <= a < R for v in case.exps for a in v)
    assert all(len(row) == case.cols for row in case.matrix) and all(len(v) == case.cols for v in case.exps)
    # the layouts: no two terms share an input record, no two outputs share an output record, all inside the buffers
    ins = [case.in_slot(j, c) for j in range(case.k) for c in range(case.cols)]
    outs = list(case.expected())
    assert len(set(ins)) == len(ins) and len(outs) == case.rows * case.k and max(ins, default=0) < case.in_len and max(outs) < case.out_len - 2
    # closed form == the oracle's additions, on the first and the last output (one output where a sum has 8 or more terms)
    for j, r in {(0, 0), (case.k - 1, case.rows - 1)} if case.cols < 8 else {(case.k - 1, case.rows - 1)}:
        assert chain(case.matrix[r], case.exps[j]) == pt(case.out_exp(j, r)), (j, r)
    kind = case.prop[0]
    top = max((m.bit_length() - 1 for row in case.matrix for m in row), default=-1)
    if kind == "zero_matrix":
        assert top == -1 and set(case.expected().values()) == {0} and all(a for v in case.exps for a in v)
    elif kind == "zero_row":
        z = case.prop[1]
        assert not any(case.matrix[z]) and all(any(row) for i, row in enumerate(case.matrix) if i != z)
        assert all((case.out_exp(j, r) == 0) == (r == z) for j in range(case.k) for r in range(case.rows))
    elif kind == "top_bit":
        assert top == case.prop[1] and all(any(row) for row in case.matrix)
    elif kind == "edge_entries":
        assert {m for row in case.matrix for m in row} == set(gc.EDGE_ENTRIES) and top == 254
    elif kind == "infinity_slots":
        assert not any(case.exps[0]) and case.exps[1][0] == 0 and case.exps[2][-1] == 0 and all(case.exps[3][c] == 0 for c in range(0, case.cols, 2))
        assert all(case.out_exp(0, r) == 0 for r in range(case.rows))
        if case.cols > 2:
            assert all(case.out_exp(j, r) for j in (1, 2, 3) for r in range(case.rows))
    elif kind == "all_outputs_zero":
        assert set(case.expected().values()) == {0} and (case.cols == 0 or any(m for row in case.matrix for m in row))
    elif kind == "equal_terms":
        for j, v in enumerate(case.exps):
            assert len(set(v)) == 1 and v[0] and case.out_exp(j, 0) == case.cols * v[0] % R
        assert case.matrix == [[1] * case.cols]
    elif kind == "cancelling_pairs":
        for j, v in enumerate(case.exps):
            assert all((v[c] + v[c + 1]) % R == 0 and v[c] for c in range(0, case.cols - 1, 2))
            assert all(po.g1_add(pt(v[c]), pt(v[c + 1])) is None and pt(v[c])[0] == pt(v[c + 1])[0] for c in range(0, case.cols - 1, 2))
            assert case.out_exp(j, 0) == (v[-1] if case.cols % 2 else 0)
    elif kind == "late_cancel":
        (row,) = case.matrix
        nz = [m for m in row if m]
        assert sum(nz) in (R, 2 * R) and max(nz) == R - 1 and top == 254
        # the running sum of the joint ladder, sum_c (M[c] >> b), reaches a multiple of r only at bit 1 or 0: no earlier cancellation
        hits = [b for b in range(255) if sum(m >> b for m in nz) % R == 0]
        assert hits and max(hits) <= 1
        assert all(len(set(v)) == 1 and v[0] for v in case.exps) and set(case.expected().values()) == {0}
    elif kind == "strides":
        gaps_in = case.in_len > case.k * case.cols or case.isc != 1
        gaps_out = case.out_len - 2 > case.k * case.rows or case.osr != 1
        assert gaps_in or gaps_out
        assert case.in_exps().count(gc.DECOY) == case.in_len - case.k * case.cols
    elif kind == "inf_lane":
        T, total = case.prop[1], case.rows * case.k
        assert T == gc.batch_lanes(total) and case.cols == 8 and case.knob_applies()
        zero = {r * case.k + j for j in range(case.k) for r in range(case.rows) if case.out_exp(j, r) == 0}  # t of the kernels: r * k + j
        assert len(zero) < total and (zero or total == 1)
        if T > 1 and (case.rows == 1 or case.k % T == 0):  # lane 1 owns only infinities, lanes 0 and 2 (or 0 alone at T = 2) own none
            assert zero == {t for t in range(total) if t % T == 1}
    else:
        raise AssertionError(kind)


def test_map_cases_cover_both_forms_and_every_width():
    for tag in ("a1_", "a2_", "a3_", "a7_", "a8_infinities"):
        assert {c.cols for c in MAP if c.name.startswith(tag)} == set(gc.COLS)
    for tag in ("a4_", "a5_"):
        assert {c.cols for c in MAP if c.name.startswith(tag)} == {2, 8, 9, 13}
    assert {c.rows * c.k for c in MAP if c.name.startswith("a10")} == {1, 63, 64, 65, 255, 256, 257}
    assert {gc.batch_lanes(c.rows * c.k) for c in MAP if c.name.startswith("a10")} == {1, 2, 4, 5}
    assert any(c.knob_applies() for c in MAP) and any(not c.knob_applies() for c in MAP)


@pytest.mark.parametrize("case", PACKED, ids=ids(PACKED))
def test_packed_case(case):
    assert len(case.row) == case.l and all(0 <= v < R for v in case.row) and case.k0 < R and case.k1 < R
    exp = case.expected()
    assert len(exp) == case.count == max(1, case.n // case.l)
    c = case.count - 1
    assert chain(case.row[: case.cols], [case.level_exp(c * case.l + j) for j in range(case.cols)]) == pt(exp[c])
    kind = case.prop[0]
    if kind == "short":
        assert case.n < case.l and case.count == 1 and all(case.row)
    elif kind == "row_zeros":
        assert 0 in case.row and any(case.row) and case.n >= case.l
    elif kind == "equal_terms":
        assert case.k1 == 0 and case.k0 and case.row == [1] * case.l and set(exp) == {case.l * case.k0 % R}
    else:
        raise AssertionError(kind)


# ---- B: zk_srs_powers ----
def digits(e):
    return [(e >> (8 * j)) & 0xFF for j in range(32)]


@pytest.mark.parametrize("case", POWERS, ids=ids(POWERS))
def test_powers_case(case):
    n = len(case.s)
    assert n <= 5 and all(0 <= v < R for v in case.s) and 0 <= case.g_exp < R
    E = case.exponents()
    assert [len(lv) for lv in E] == [1 << k for k in range(n + 1)]
    # the exponent is the product the index bits choose
    for k in range(n + 1):
        for j in (0, (1 << k) - 1, (1 << k) // 3):
            want = 1
            for var, taken in case.choice(k, j):
                want = want * (case.s[var] if taken else 1 - case.s[var]) % R
            assert E[k][j] == want
    # the oracle's literal construction (two scalar multiplications per point and level) on the last three variables: a level depends
    # on the variables behind it only, so these are levels 0..3 of the case itself -- 8 points at the most
    m = min(n, 3)
    g = pt(case.g_exp)
    lv = po.srs_powers(g, case.s[n - m:])
    assert lv[m] == [pt(e) for e in case.expected()[m]]
    kind = case.prop[0]
    if kind == "edge_values":
        assert {0, 1, R - 1, gc.INV2, (1 << 248) - 1} == set(case.s) and 2 * gc.INV2 % R == 1
        assert digits(E[1][1]) == [0xFF] * 31 + [0]
        assert 0 in E[n] and any(E[n])
    elif kind == "single_byte":
        d = digits(E[1][1])
        assert [j for j in range(32) if d[j]] == [case.prop[1]]
    elif kind == "half_infinite":
        var, val = case.prop[1:]
        assert case.s[var] == val and all(v not in (0, 1) for i, v in enumerate(case.s) if i != var)
        bit = n - 1 - var  # the index bit that chooses s_var; it exists from level n - var on
        for k in range(n + 1):
            zero = {j for j, e in enumerate(E[k]) if e == 0}
            if k <= bit:
                assert not zero
            else:  # s = 0 kills the indices with the bit set, s = 1 the others: exactly half the level
                assert zero == {j for j in range(1 << k) if ((j >> bit) & 1) == (1 - val)} and len(zero) == (1 << k) // 2
    elif kind == "nvars0":
        assert E == [[1]]
    elif kind == "custom_base":
        assert case.g_exp not in (0, 1) and case.expected()[0] == [case.g_exp]
    elif kind == "infinite_base":
        assert case.g_exp == 0 and all(e == 0 for lv_ in case.expected() for e in lv_) and g is None
    elif kind == "mont_form":
        sm = case.prop[1]
        assert case.s[-1] * (1 << 256) % R == sm and 0 < sm < R
        assert (sm > gc.MONT_ONE) == ("borrow, + r" in case.aim)
    else:
        raise AssertionError(kind)


def test_powers_cases_take_both_branches_of_the_host_subtraction():
    stored = {v * (1 << 256) % R for c in POWERS for v in c.s}
    assert {gc.MONT_ONE - 1, gc.MONT_ONE, gc.MONT_ONE + 1, 0, R - 1} <= stored
    assert gc.MONT_ONE == 0x1824B159ACC5056F998C4FEFECBC4FF55884B7FA0003480200000001FFFFFFFE  # `one_m` of srs_powers


# ---- C: zk_srs_generate ----
def test_seq_sizes():
    assert gc.seq_sizes(3100) == [3100, 1024] and gc.seq_sizes(70000) == [70000, 1094, 1024]
    assert [gc.seq_sizes(n) for n in (1, 1024, 1025)] == [[1], [1024], [1025, 1024]]


@pytest.mark.parametrize("case", SEQ, ids=ids(SEQ))
def test_seq_case(case):
    assert 0 <= case.k0 < R and 0 <= case.k1 < R
    idx = case.indices()
    assert idx == sorted(set(idx)) and idx[0] == 0 and idx[-1] == case.n - 1
    assert (case.sample is None) == (case.n <= 3100) and len(idx) <= max(3100, 100)
    sizes = gc.seq_sizes(case.n)
    kind = case.prop[0]
    special = []
    if kind == "inf_at":
        special = case.prop[1]
        assert [i for i in idx if case.exp(i) == 0] == special
        (z,) = special
        if z >= 1024:  # a lane of the last walk starts at -stepT: T = sizes[1] points per step
            T = sizes[1]
            assert z - T < T and (case.exp(z - T) + T * case.k1) % R == 0 and case.exp(z + T) == T * case.k1 % R and z + T < case.n
            assert {z - T, z, z + T, z + 2 * T} <= set(idx) and case.exp(z + 2 * T) == 2 * T * case.k1 % R  # -stepT, infinity, stepT (set), 2 stepT (doubling)
    elif kind == "constant":
        assert case.k1 == 0 and case.k0 and {case.exp(i) for i in idx} == {case.k0}
    elif kind == "all_zero":
        assert {case.exp(i) for i in idx} == {0}
    elif kind == "dbl_at":
        host, dev = case.prop[1:]
        T = sizes[1]
        assert case.exp(host - 1) == case.k1  # the host chain adds the step to itself
        assert dev - T == T - 1 and case.exp(dev - T) == T * case.k1 % R  # the last lane's start is the walk's step
        assert dev in idx and dev - 1 in idx and dev + 1 in idx
        special = [dev]
    else:
        raise AssertionError(kind)
    # closed form == the oracle's repeated addition of the step, on 8 consecutive points that pass through the special index
    lo = max(0, min((special or [0])[0] - 4, case.n - 8))
    P, step = pt(case.exp(lo)), pt(case.k1)
    for i in range(lo, min(lo + 8, case.n)):
        assert P == pt(case.exp(i)), i
        P = po.g1_add(P, step)
