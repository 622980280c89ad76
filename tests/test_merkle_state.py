"""
The host rules of the Merkle state tree (zkhip.poseidon.update_host / paths_host) and the update circuit (merkle_update_circuit) against the
independent model (merkle_state_model.py on poseidon_model.py).  No GPU: the rules on python integers at n = 1, 2, 4, 64, every refusal with
its message, the circuit's documented row counts, every row holding in pm.evaluate on honest chains, and the row or copy that each kind of
dishonest input violates.
"""
import random

import pytest

import merkle_state_model as msm
import poseidon_model as pm

R = pm.R


@pytest.fixture(scope="module")
def trees():
    """n -> (leaves, the model's tree), built once and left unchanged"""
    rng = random.Random(31)
    out = {}
    for n in (1, 2, 4, 64):
        leaves = [rng.randrange(R) for _ in range(n)]
        out[n] = (leaves, pm.merkle(leaves))
    return out


def write_sets(n):
    """(name, writes): leaf 0, leaf n - 1, an adjacent pair, all leaves, and repeats whose last write must win"""
    rng = random.Random(32 + n)
    v = lambda: rng.randrange(R)
    sets = [("first", [(0, v())]), ("last", [(n - 1, v())]), ("all", [(i, v()) for i in range(n)]), ("repeat", [(n - 1, v()), (0, v()), (n - 1, v()), (0, v())])]
    if n >= 2:
        sets.append(("pair", [(2 * (n // 4) + 1, v()), (2 * (n // 4), v())]))  # the two children of one parent, the right one first
        sets.append(("all shuffled twice", rng.sample([(i, v()) for i in range(n)] + [(i, v()) for i in range(n)], 2 * n)))
    return sets


@pytest.mark.parametrize("n", [1, 2, 4, 64])
def test_update_host_equals_the_rebuild(trees, n):
    from zkhip import poseidon as ps

    _, tree = trees[n]
    for name, writes in write_sets(n):
        got = ps.update_host(tree, n, writes)
        assert got == msm.update(tree, n, writes), name
        assert got is not tree and tree == trees[n][1]
    assert ps.update_host(tree, n, []) == tree
    # two updates in sequence are the model's two
    a, b = write_sets(n)[0][1], write_sets(n)[1][1]
    assert ps.update_host(ps.update_host(tree, n, a), n, b) == msm.update(msm.update(tree, n, a), n, b)


def test_update_host_touches_only_the_nodes_above_a_write(trees):
    """a tree whose untouched nodes are NOT hashes of their children keeps them: the rule hashes nothing but the written leaves' ancestors"""
    from zkhip import poseidon as ps

    n = 64
    fake = list(range(1000, 1000 + 2 * n - 1))
    got = ps.update_host(fake, n, [(5, 77), (40, 78)])
    above = set()
    for i in (5, 40):
        lo, cnt = 0, n
        while cnt > 1:
            lo, cnt, i = lo + cnt, cnt // 2, i // 2
            above.add(lo + i)
    changed = {k for k in range(2 * n - 1) if got[k] != fake[k]}
    assert changed == above | {5, 40} and len(above) == 11  # 6 + 6 ancestors, the root shared
    assert got[n + 2] == pm.hash2(fake[4], 77) and got[2 * n - 2] == pm.hash2(got[2 * n - 4], got[2 * n - 3])


@pytest.mark.parametrize("n", [1, 2, 4, 64])
def test_paths_host_equals_the_model(trees, n):
    from zkhip import poseidon as ps

    leaves, tree = trees[n]
    indices = [0, n - 1, n // 2, 0, n - 1] + list(range(n - 1, -1, -1))
    got = ps.paths_host(tree, n, indices)
    assert got == msm.paths(tree, n, indices)
    assert all(len(p) == n.bit_length() - 1 for p in got)
    assert all(msm.root(leaves[i], p, i) == tree[-1] for i, p in zip(indices, got))


def test_refusals(trees):
    from zkhip import poseidon as ps

    _, tree = trees[4]
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_paths: 2 of 4 indices are not below n = 4; the first is position 1$"):
        ps.paths_host(tree, 4, [3, 4, 0, 9])
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_paths: 1 of 1 indices are not below n = 4; the first is position 0$"):
        ps.paths_host(tree, 4, [-1])
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_update: 1 of 3 indices are not below n = 4; the first is position 2$"):
        ps.update_host(tree, 4, [(0, 1), (3, 1), (4, 1)])
    for bad_n in (0, 3, 8):
        with pytest.raises(ValueError, match="2n - 1 elements"):
            ps.update_host(tree, bad_n, [])
        with pytest.raises(ValueError, match="2n - 1 elements"):
            ps.paths_host(tree, bad_n, [])
    for depth, count in ((0, 1), (1, 0)):
        with pytest.raises(ValueError, match="depth >= 1 and count >= 1"):
            ps.merkle_update_circuit(depth, count)
    circuit, layout, v = ps.merkle_update_circuit(1, 1)
    with pytest.raises(ValueError, match="number of writes"):
        ps.merkle_update_inputs(layout, v, [])
    with pytest.raises(ValueError, match="depth"):
        ps.merkle_update_inputs(layout, v, [(1, 2, [3, 4], [0])])


# ---- the circuit ----
CASES = [(1, 1), (2, 1), (2, 2)]


@pytest.fixture(scope="module")
def circuits():
    """(depth, count) -> (circuit, layout, vars, tree, writes, steps, trees): an honest chain per case, built once and left unchanged"""
    from zkhip import poseidon as ps

    rng = random.Random(33)
    out = {}
    for depth, count in CASES:
        n = 1 << depth
        tree = pm.merkle([rng.randrange(R) for _ in range(n)])
        # indices whose bits differ at every level between the writes: (1), (1, 0) = 1 and then (0, 1) = 2
        writes = [((1, 2)[i] % n, rng.randrange(R)) for i in range(count)]
        steps, after = msm.chain(tree, n, writes)
        out[depth, count] = ps.merkle_update_circuit(depth, count) + (tree, writes, steps, after)
    return out


def slot_of(layout, var):
    return 2 * layout.N + layout.row(var)


@pytest.mark.parametrize("depth,count,mu", [(1, 1, 10), (2, 1, 11), (2, 2, 12)])
def test_update_circuit_rows_and_honest_chain(circuits, depth, count, mu):
    from zkhip import poseidon as ps

    circuit, layout, v, tree, writes, steps, after = circuits[depth, count]
    assert circuit["l"] == 2 and layout.rows == 2 + 959 * depth * count and circuit["mu"] == mu
    # per level: the bit's assertion, then 479 rows for the old node and 479 for the new one
    # (a hash's output is the first of the permutation's three outputs: two lin rows each, so it sits 4 rows before the end of its 479)
    w = v["writes"]
    assert layout.row(w[0]["old_out"]) == 2 + 959 * (depth - 1) + 479 - 4 and layout.row(w[0]["new_out"]) == 2 + 959 * depth - 1 - 4
    assert layout.row(w[-1]["new_out"]) == layout.rows - 1 - 4
    pi = [tree[-1], after[-1][-1]]
    assert pi[1] == msm.update(tree, 1 << depth, writes)[-1]
    ev = pm.evaluate(circuit, pi, msm.free_slots(ps.merkle_update_inputs(layout, v, steps)))
    assert ev["bad_rows"] == [] and ev["bad_copies"] == []
    for i, wi in enumerate(w):
        assert ev["c"][layout.row(wi["old_out"])] == after[i][-1] and ev["c"][layout.row(wi["new_out"])] == after[i + 1][-1]
    # the copy classes: old root with the first old chain, each new chain with the next old chain, the last new chain with the new root
    together = lambda s, t: any(s in cy and t in cy for cy in ev["classes"])
    N = layout.N
    assert together(2 * N, slot_of(layout, w[0]["old_out"])) and together(2 * N + 1, slot_of(layout, w[-1]["new_out"]))
    for a, b in zip(w, w[1:]):
        assert together(slot_of(layout, a["new_out"]), slot_of(layout, b["old_out"]))
    # one sibling and one bit variable feed both chains: their classes hold slots of both
    first_bit_rows = [x for cy in ev["classes"] if 2 in cy for x in cy]
    assert 2 in first_bit_rows and N + 2 in first_bit_rows and len(first_bit_rows) == 4  # assert_bool's a and b, the two mul rows


def test_update_circuit_violations(circuits):
    from zkhip import poseidon as ps

    circuit, layout, v, tree, writes, steps, after = circuits[1, 1]
    w = v["writes"][0]
    old_slot, new_slot = slot_of(layout, w["old_out"]), slot_of(layout, w["new_out"])
    pi = [tree[-1], after[-1][-1]]
    old_leaf, new_leaf, sibs, bits = steps[0]
    run = lambda pub, step: pm.evaluate(circuit, pub, msm.free_slots(ps.merkle_update_inputs(layout, v, [step])))
    ev = run(pi, ((old_leaf + 1) % R, new_leaf, sibs, bits))  # a wrong old leaf: only the old chain misses its class
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [old_slot]
    ev = run(pi, (old_leaf, new_leaf, [(sibs[0] + 1) % R], bits))  # a wrong sibling: both chains use it
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [old_slot, new_slot]
    ev = run(pi, (old_leaf, new_leaf, sibs, [bits[0] ^ 1]))  # a flipped bit: every gate holds, both outputs are other values
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [old_slot, new_slot]
    ev = run(pi, (old_leaf, new_leaf, sibs, [2]))  # a bit of value 2: its ONE assert_bool row, the first after the public rows
    assert ev["bad_rows"] == [2]
    ev = run([pi[0], (pi[1] + 1) % R], steps[0])  # a wrong new root
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [new_slot]
    ev = run([(pi[0] + 1) % R, pi[1]], steps[0])  # a wrong old root
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [old_slot]


def test_a_chain_must_continue_from_the_root_it_produced(circuits):
    from zkhip import poseidon as ps

    circuit, layout, v, tree, writes, steps, after = circuits[2, 2]
    n = 4
    # the second write is honest on ANOTHER tree than the one the first write produced; the public new root is that chain's own result
    other = msm.update(after[1], n, [(0, 12345)])
    (i2, v2), = writes[1:]
    step2 = (other[i2], v2, pm.path_of(other, n, i2)[0], msm.bits_of(i2, 2))
    pi = [tree[-1], msm.update(other, n, [(i2, v2)])[-1]]
    ev = pm.evaluate(circuit, pi, msm.free_slots(ps.merkle_update_inputs(layout, v, [steps[0], step2])))
    assert ev["bad_rows"] == [] and ev["bad_copies"] == [slot_of(layout, v["writes"][1]["old_out"])]


def test_update_circuit_digest_is_stable():
    from zkhip import poseidon as ps
    from zkhip.circuit import circuit_digest

    d = {case: circuit_digest(ps.merkle_update_circuit(*case)[0]) for case in CASES}
    assert len(set(d.values())) == 3 and d[1, 1] == circuit_digest(ps.merkle_update_circuit(1)[0])
    assert d[1, 1] == DIGEST_1_1
    assert circuit_digest(ps.merkle_circuit(1)[0]) not in d.values()


DIGEST_1_1 = "290ed8986488c464fcc9ea771174ce7e944e0637b9d2615d13a27874f4d0bd66"
