"""
Poseidon zkhip-poseidon-v1 without a GPU: the constants against their SHA-256 rule and the properties the instance rests on, the host rules
of zkhip/poseidon.py against the independent model (poseidon_model.py), the circuit builder row by row in the model's evaluator, and the
permutation / Merkle gadgets on honest and broken paths.
"""
import random

import numpy as np
import pytest

import poseidon_model as pm

R = pm.R
# SHA-256 over rc[0..194] then M row-major, 32 little-endian bytes per canonical integer: computed once by poseidon_model.constants_sha256()
CONSTANTS_SHA256 = "595936b37cc528e9dab0fe4a22ec4aabf1f8afa10f8bbdb5e560f80d3ffce2ec"


def mont_ints(limbs):
    return pm._ints(limbs)


def rand_states(count, seed):
    rng = random.Random(seed)
    return [tuple(rng.randrange(R) for _ in range(3)) for _ in range(count)]


# ---- constants ----
def test_constants_follow_the_sha256_rule():
    from zkhip import poseidon as ps

    rc, M = pm.constants()
    p = ps.params()
    assert (p["rf"], p["rp"]) == (8, 57) and len(rc) == 195
    assert p["rc"] == rc and p["mds"] == M
    assert mont_ints(p["rc_mont"]) == rc and mont_ints(p["mds_mont"]) == [v for row in M for v in row]
    assert pm.constants_sha256() == CONSTANTS_SHA256
    for i in range(3):
        for j in range(3):
            assert M[i][j] * (i + j + 3) % R == 1


def test_matrix_is_mds_and_the_sbox_is_a_bijection():
    import math
    from itertools import combinations

    _, M = pm.constants()
    assert all(v % R for row in M for v in row)
    for r2 in combinations(range(3), 2):
        for c2 in combinations(range(3), 2):
            assert (M[r2[0]][c2[0]] * M[r2[1]][c2[1]] - M[r2[0]][c2[1]] * M[r2[1]][c2[0]]) % R != 0
    det = sum(M[0][j] * (M[1][(j + 1) % 3] * M[2][(j + 2) % 3] - M[1][(j + 2) % 3] * M[2][(j + 1) % 3]) for j in range(3)) % R
    assert det != 0
    assert math.gcd(5, R - 1) == 1


# ---- host rules ----
def test_host_rules_equal_the_model():
    from zkhip import poseidon as ps

    states = [(0, 0, 0), (R - 1, R - 1, R - 1)] + rand_states(16, 1)
    for s in states:
        assert ps.permute_host(s) == pm.permute(s)
        assert ps.hash2_host(s[1], s[2]) == pm.hash2(s[1], s[2]) == pm.permute((0, s[1], s[2]))[0]
    rng = random.Random(2)
    for n in (1, 2, 8):
        leaves = [rng.randrange(R) for _ in range(n)]
        tree = ps.merkle_host(leaves)
        assert len(tree) == 2 * n - 1 and tree == pm.merkle(leaves)
    for i in range(8):  # (tree: the n = 8 one)
        sibs, bits = ps.merkle_path(tree, 8, i)
        assert (sibs, bits) == pm.path_of(tree, 8, i) and bits[0] == i & 1
        assert pm.root_of_path(leaves[i], sibs, bits) == tree[-1] == ps.path_root_host(leaves[i], sibs, bits)
    with pytest.raises(ValueError):
        ps.merkle_host([1, 2, 3])


def test_other_constants_are_other_data():
    from zkhip import poseidon as ps

    rc, M = pm.derived_constants(2, 1, b"test-instance")
    p = ps.make_params(2, 1, rc, M)
    for s in rand_states(4, 3):
        assert ps.permute_host(s, p) == pm.permute(s, rf=2, rp=1, consts=(rc, M)) != pm.permute(s)


# ---- the builder ----
def test_every_primitive_row_holds_in_the_evaluator():
    from zkhip.circuit import Builder

    b = Builder()
    p0, p1, p2 = b.public(), b.public(), b.public()
    x, y, bit = b.private(), b.private(), b.private()
    u = b.lin(3, x, R - 2, y, 7)
    v = b.mul(u, p0, k=5, kc=11)
    w = b.pow5(v, kc=13)
    z = b.lin(0, None, 0, None, 0)
    b.assert_zero_of(1, w, -1, w, 0, 0)
    b.assert_bool(bit)
    t = b.lin(1, p1, 0, None, 0)
    b.assert_equal(t, p1)
    with pytest.raises(ValueError, match="precede"):
        b.public()
    circuit, layout = b.build()
    assert (circuit["gate"], circuit["l"], circuit["mu"]) == ("wide", 4, 4)  # 3 publics pad to l = 4; 4 + 7 rows = 11 <= 16
    assert (layout.N, layout.l, layout.rows) == (16, 4, 11)
    xv, yv, pub = 1234567, R - 5, [21, 22, 23, 0]
    free = {layout.slot(x): xv, layout.slot(y): yv, layout.slot(bit): 1}
    ev = pm.evaluate(circuit, pub, free)
    assert ev["bad_rows"] == [] and ev["bad_copies"] == []
    c = ev["c"]
    uv = (3 * xv - 2 * yv + 7) % R
    vv = (5 * uv * 21 + 11) % R
    assert c[layout.row(u)] == uv and c[layout.row(v)] == vv and c[layout.row(w)] == (pow(vv, 5, R) + 13) % R
    assert c[layout.row(z)] == 0 and c[layout.row(t)] == 22 and c[:4] == pub
    assert [layout.row(q) for q in (p0, p1, p2, u, v, w, z, t)] == [0, 1, 2, 4, 5, 6, 7, 10]
    # the free array is the same thing on limbs
    arr = layout.free({x: xv, y: yv, bit: 1})
    assert arr.shape == (48, 4) and mont_ints(arr[[layout.slot(x), layout.slot(y), layout.slot(bit)]]) == [xv, yv, 1]
    # unused rows: all-zero selectors
    for k in ("qL", "qR", "qM", "qO", "qC", "qH"):
        assert not np.asarray(circuit[k])[11:].any()
    # a bit that is no bit breaks exactly its assert row
    free[layout.slot(bit)] = 2
    assert pm.evaluate(circuit, pub, free)["bad_rows"] == [9]


def test_sigma_is_one_ascending_cycle_per_class():
    from zkhip.circuit import Builder

    b = Builder()
    p0 = b.public()
    x = b.private()
    u = b.lin(1, x, 1, x, 0)      # row 1: a = x, b = x
    v = b.mul(u, x)               # row 2: a = u, b = x
    b.assert_equal(v, p0)
    circuit, layout = b.build()
    N = 4
    assert (circuit["mu"], circuit["l"]) == (2, 1)
    sigma = [int(s) for s in circuit["sigma"]]
    assert sorted(sigma) == list(range(3 * N))
    cycles = {(1, N + 1, N + 2): "x", (2, 2 * N + 1): "u", (2 * N, 2 * N + 2): "v = p0"}
    seen = set()
    for cyc in cycles:
        for s, t in zip(cyc, cyc[1:] + cyc[:1]):
            assert sigma[s] == t
        seen |= set(cyc)
    assert all(sigma[s] == s for s in range(3 * N) if s not in seen)
    assert layout.slot(x) == 1 and layout.slot(v) == layout.slot(p0) == 2 * N
    # mu covers 2 l as well: 5 publics pad to l = 8 and force N = 16 without any other row
    b = Builder()
    for _ in range(5):
        b.public()
    circuit, _ = b.build()
    assert (circuit["l"], circuit["mu"]) == (8, 4)
    b = Builder()
    b.lin(0, None, 0, None, 1)
    circuit, _ = b.build()
    assert (circuit["l"], circuit["mu"]) == (1, 1)


# ---- the gadgets ----
def test_permutation_gadget_rows_and_value():
    from zkhip import poseidon as ps
    from zkhip.circuit import Builder

    b = Builder()
    s = [b.private() for _ in range(3)]
    out = ps.permutation_gadget(b, s)
    circuit, layout = b.build()
    assert layout.rows - layout.l == 474 and circuit["mu"] == 9
    state = rand_states(1, 5)[0]
    ev = pm.evaluate(circuit, [0], {layout.slot(v): x for v, x in zip(s, state)})
    assert ev["bad_rows"] == [] and ev["bad_copies"] == []
    assert tuple(ev["c"][layout.row(o)] for o in out) == pm.permute(state)


@pytest.fixture(scope="module")
def merkle_cases():
    """depth -> (circuit, layout, vars, leaves, tree): built once, left unchanged"""
    from zkhip import poseidon as ps

    rng = random.Random(11)
    out = {}
    for depth in (1, 2):
        leaves = [rng.randrange(R) for _ in range(1 << depth)]
        out[depth] = ps.merkle_circuit(depth) + (leaves, pm.merkle(leaves))
    return out


def free_dict(free):
    return {int(s): v for s, v in zip(np.flatnonzero(np.asarray(free).any(axis=1)), mont_ints(free[np.asarray(free).any(axis=1)]))}


@pytest.mark.parametrize("depth,mu", [(1, 9), (2, 10)])
def test_merkle_circuit_on_honest_and_broken_paths(merkle_cases, depth, mu):
    from zkhip import poseidon as ps

    circuit, layout, v, leaves, tree = merkle_cases[depth]
    n = 1 << depth
    assert circuit["mu"] == mu and circuit["l"] == 1 and layout.rows == 1 + 480 * depth
    root = tree[-1]
    index = n - 1 if depth == 1 else 2  # bits (1) and (0, 1): both orders of the children occur
    sibs, bits = pm.path_of(tree, n, index)
    free = free_dict(ps.merkle_witness_inputs(layout, v, leaves[index], sibs, bits))
    ev = pm.evaluate(circuit, [root], free)
    assert ev["bad_rows"] == [] and ev["bad_copies"] == []
    out_slot = 2 * layout.N + layout.row(v["out"])
    assert ev["c"][layout.row(v["out"])] == root and any(out_slot in cy and 2 * layout.N in cy for cy in ev["classes"])
    # a flipped bit: every gate holds, the output is another value than the public root -- a class mismatch
    flipped = free_dict(ps.merkle_witness_inputs(layout, v, leaves[index], sibs, [bits[0] ^ 1] + bits[1:]))
    ev = pm.evaluate(circuit, [root], flipped)
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [out_slot]
    # a wrong root
    ev = pm.evaluate(circuit, [(root + 1) % R], free)
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [out_slot]
    # a bit of value 2: its assert_bool row (the first row of its level) is a bad gate row
    two = free_dict(ps.merkle_witness_inputs(layout, v, leaves[index], sibs, [2] + bits[1:]))
    assert pm.evaluate(circuit, [root], two)["bad_rows"][0] == 1


def test_circuit_digest_is_stable():
    from zkhip import poseidon as ps
    from zkhip.circuit import circuit_digest

    d = [circuit_digest(ps.merkle_circuit(2)[0]) for _ in range(2)]
    assert d[0] == d[1] and len(d[0]) == 64
    assert circuit_digest(ps.merkle_circuit(1)[0]) != d[0]
