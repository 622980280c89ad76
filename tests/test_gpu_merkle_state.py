"""
The Merkle state tree on the device (zk_poseidon_merkle_paths / _roots / _update) bit for bit against the independent model
(merkle_state_model.py: an update is a rebuild of the whole tree): the gather at sizes around a wave and a workgroup with repeated, unsorted
indices; the roots of honest and altered paths; updates of one leaf, an adjacent pair and two halves, of 63 .. 257 leaves and of all leaves,
through the per-level launches and the single workgroup; untouched elements keeping their bits; the refusals; and one proved chain of two
writes through witness -> prove -> verify_bytes.
"""
import random

import numpy as np
import pytest

import merkle_state_model as msm
import poseidon_model as pm
from merkle_state_model import ints, limbs

pytestmark = pytest.mark.gpu
R = pm.R


@pytest.fixture(scope="module")
def pos(ctx):
    from zkhip import poseidon as ps

    p = ps.Poseidon(ctx)
    yield p
    p.free()


@pytest.fixture(scope="module")
def trees():
    """n -> the model's tree of n seeded leaves: built once, shared, left unchanged"""
    rng = random.Random(41)
    return {n: pm.merkle([rng.randrange(R) for _ in range(n)]) for n in (1, 2, 4, 64, 512, 1024)}


def some_indices(n, count, seed):
    """`count` indices below n: unsorted, with repeats, 0 and n - 1 among them (count = 1: n - 1 alone)"""
    rng = random.Random(seed)
    idx = [n - 1, 0, n - 1, n // 2, 0][:count] + [rng.randrange(n) for _ in range(max(count - 5, 0))]
    rng.shuffle(idx)
    return idx


# ---- paths ----
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n", [1, 2, 4, 64, 1024])
def test_paths(ctx, pos, trees, n, count):
    tree, d = trees[n], n.bit_length() - 1
    idx = some_indices(n, count, 100 * n + count)
    d_tree = ctx.to_device(limbs(tree))
    out = ctx.alloc(32 * (count * d + 1))
    guard = limbs([R - 1] * (count * d + 1))
    out.upload(guard)
    pos.paths(d_tree, n, idx, out=out)
    got = out.download((count * d + 1, 4))
    want = [s for p in msm.paths(tree, n, idx) for s in p]
    assert len(want) == count * d and (got[:count * d] == limbs(want).reshape(-1, 4)).all() and (got[count * d] == guard[0]).all()
    assert (d_tree.download((2 * n - 1, 4)) == limbs(tree)).all()


# ---- roots ----
def test_roots_of_honest_and_altered_paths(ctx, pos, trees):
    n, d, count = 64, 6, 65
    tree = trees[n]
    idx = some_indices(n, count, 7)
    d_tree = ctx.to_device(limbs(tree))
    sibs = pos.paths(d_tree, n, idx)
    leaves = [tree[i] for i in idx]
    d_leaves = ctx.to_device(limbs(leaves))
    assert ints(pos.roots(d_leaves, idx, sibs, d).download((count, 4))) == [tree[-1]] * count
    assert pos.verify_paths(tree[-1], d_leaves, idx, sibs, d).all()
    # a changed leaf (path 3), a changed sibling (path 5, level 2), a changed index bit (path 7, bit 1; path 9, the top bit)
    h_sibs = [ints(row) for row in sibs.download((count, d, 4))]
    leaves[3] = (leaves[3] + 1) % R
    h_sibs[5][2] = (h_sibs[5][2] + 1) % R
    idx[7] ^= 2
    idx[9] ^= 32
    want = [msm.root(leaf, s, i) for leaf, s, i in zip(leaves, h_sibs, idx)]
    altered = (3, 5, 7, 9)
    assert all((want[k] != tree[-1]) == (k in altered) for k in range(count))
    d_leaves, d_sibs = ctx.to_device(limbs(leaves)), ctx.to_device(limbs([s for p in h_sibs for s in p]))
    assert ints(pos.roots(d_leaves, idx, d_sibs, d).download((count, 4))) == want
    ok = pos.verify_paths(tree[-1], d_leaves, idx, d_sibs, d)
    assert ok.dtype == bool and [k for k in range(count) if not ok[k]] == list(altered)
    # in place, and depth 0: the leaves themselves
    pos.roots(d_leaves, idx, d_sibs, d, out=d_leaves)
    assert ints(d_leaves.download((count, 4))) == want
    assert ints(pos.roots(d_leaves, [0] * count, None, 0).download((count, 4))) == want


def test_roots_of_257_paths_of_depth_10(ctx, pos, trees):
    n, count = 1024, 257
    tree = trees[n]
    idx = some_indices(n, count, 8)
    sibs = pos.paths(ctx.to_device(limbs(tree)), n, idx)
    assert pos.verify_paths(tree[-1], ctx.to_device(limbs([tree[i] for i in idx])), idx, sibs, 10).all()


# ---- update ----
def run_update(ctx, pos, start, n, writes):
    """the device tree after pos.update of `writes` = [(index, value)] on the list `start`"""
    d_tree = ctx.to_device(limbs(start))
    pos.update(d_tree, n, [i for i, _ in writes], limbs([v for _, v in writes]))
    return ints(d_tree.download((2 * n - 1, 4)))


@pytest.mark.parametrize("n", [2, 64, 512, 1024])
def test_update_of_one_leaf_a_pair_and_two_halves(ctx, pos, trees, n):
    rng = random.Random(50 + n)
    v = lambda: rng.randrange(R)
    q = 2 * (n // 4)
    for writes in ([(n - 1, v())], [(q + 1, v()), (q, v())], [(n - 2, v()), (1 % n, v())]):
        assert run_update(ctx, pos, trees[n], n, writes) == msm.update(trees[n], n, writes), writes


@pytest.fixture(scope="module")
def writes257(trees):
    """257 writes to a tree of 1024 leaves in any order, at least 15 of them to a leaf written before (the last wins), leaves 0 and 1023 among
    them, and the model's tree after them"""
    rng = random.Random(61)
    where = rng.sample(range(1024), 240) + [0, 1023]
    where += rng.sample(where, 15)
    rng.shuffle(where)
    writes = [(i, rng.randrange(R)) for i in where]
    assert len(writes) == 257
    return writes, msm.update(trees[1024], 1024, writes)


@pytest.mark.parametrize("count", [63, 64, 65, 257])
def test_update_counts(ctx, pos, trees, writes257, count):
    writes, after = writes257
    want = after if count == 257 else msm.update(trees[1024], 1024, writes[:count])
    assert run_update(ctx, pos, trees[1024], 1024, writes[:count]) == want


@pytest.mark.parametrize("tail", [0, 1, 8, 64, 256])
def test_update_launch_paths(ctx, pos, trees, writes257, tail):
    """257 writes, about 230 distinct parents on the first level.  tail 256: one workgroup walks all ten levels; 64, 8, 1: level launches while
    a level has more parents than that, the workgroup for the rest (1: only the root); 0: level launches alone.  And a five-write update of
    64 leaves through the same knob"""
    writes, after = writes257
    small = [(9, 1), (8, 2), (63, 3), (0, 4), (40, 5)]
    ctx.dbg_tune("poseidon_tail_nodes", tail)
    try:
        got = run_update(ctx, pos, trees[1024], 1024, writes)
        got_small = run_update(ctx, pos, trees[64], 64, small)
    finally:
        ctx.dbg_tune("poseidon_tail_nodes", 256)
    assert got == after and got_small == msm.update(trees[64], 64, small)


@pytest.mark.parametrize("tail", [256, 4, 0])
def test_update_leaves_every_other_element_alone(ctx, pos, tail):
    """the buffer holds a pattern, not a tree: after an update the written leaves and the nodes above them are what the model says, and every
    other element still holds the pattern"""
    n = 64
    pattern = [(R - 1 - 1000 * k) % R for k in range(2 * n - 1)]
    writes = [(5, 77), (4, 78), (40, 79), (63, 80)]
    ctx.dbg_tune("poseidon_tail_nodes", tail)
    try:
        got = run_update(ctx, pos, pattern, n, writes)
    finally:
        ctx.dbg_tune("poseidon_tail_nodes", 256)
    want = msm.update_touched(pattern, n, writes)
    # 4 leaves; parents 2, 20, 31; then 1, 10, 15; 0, 5, 7; 0, 2, 3; 0, 1; the root
    assert got == want and sum(a != b for a, b in zip(want, pattern)) == 4 + 3 + 3 + 3 + 3 + 2 + 1


def test_update_of_all_leaves_is_a_rebuild_and_of_none_is_nothing(ctx, pos, trees):
    n = 64
    rng = random.Random(62)
    leaves = [rng.randrange(R) for _ in range(n)]
    pattern = [(R - 1 - 1000 * k) % R for k in range(2 * n - 1)]
    order = rng.sample(range(n), n)
    assert run_update(ctx, pos, pattern, n, [(i, leaves[i]) for i in order]) == pm.merkle(leaves)
    assert run_update(ctx, pos, pattern, n, []) == pattern
    assert run_update(ctx, pos, trees[1], 1, [(0, 5), (0, 6)]) == [6]


def test_two_updates_in_sequence(ctx, pos, trees):
    n = 512
    first, second = [(3, 10), (400, 11), (2, 12)], [(400, 13), (511, 14)]
    d_tree = ctx.to_device(limbs(trees[n]))
    pos.update(d_tree, n, [i for i, _ in first], limbs([v for _, v in first]))
    pos.update(d_tree, n, [i for i, _ in second], limbs([v for _, v in second]))
    assert ints(d_tree.download((2 * n - 1, 4))) == msm.update(msm.update(trees[n], n, first), n, second)


def test_other_constants(ctx):
    """rf = 2, rp = 1 with model-derived constants: the update and the roots hash with the params they are given"""
    from zkhip import poseidon as ps

    rc, M = pm.derived_constants(2, 1, b"test-instance")
    kw = {"rf": 2, "rp": 1, "consts": (rc, M)}
    n, rng = 64, random.Random(63)
    tree = pm.merkle([rng.randrange(R) for _ in range(n)], **kw)
    writes = [(i, rng.randrange(R)) for i in rng.sample(range(n), 20)]
    other = ps.Poseidon(ctx, ps.make_params(2, 1, rc, M))
    try:
        got = run_update(ctx, other, tree, n, writes)
        want = msm.update(tree, n, writes, **kw)
        assert got == want
        idx = [i for i, _ in writes]
        d_tree = ctx.to_device(limbs(want))
        assert other.verify_paths(want[-1], ctx.to_device(limbs([want[i] for i in idx])), idx, other.paths(d_tree, n, idx), 6).all()
    finally:
        other.free()


# ---- refusals ----
def test_refusals(ctx, pos, trees):
    import zkhip
    from zkhip import poseidon as ps
    from zkhip._lib import ZK_ERR_INVALID

    n = 64
    tree = limbs(trees[n])
    d_tree, d_vals = ctx.to_device(tree), ctx.to_device(limbs([1, 2, 3, 4]))
    out = ctx.alloc(32 * 6 * 4)
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_paths: 2 of 4 indices are not below n = 64; the first is position 1$"):
        pos.paths(d_tree, n, [63, 64, 0, 1 << 40], out=out)
    with pytest.raises(ValueError, match="power of two"):
        pos.paths(d_tree, 48, [0], out=out)
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_roots: 1 of 4 indices have bits at or above depth 6; the first is position 3$"):
        pos.roots(d_vals, [0, 63, 5, 64], out, 6)
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_roots: 3 of 4 indices have bits at or above depth 0; the first is position 1$"):
        pos.roots(d_vals, [0, 1, 1, 1], None, 0)
    with pytest.raises(ValueError, match="at most 40"):
        pos.roots(d_vals, [0], out, 41)
    # the C call takes strictly ascending indices only (device values go to it as they are)
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_update: 1 of 4 indices are not below n = 64; the first is position 3$"):
        pos.update(d_tree, n, [0, 1, 2, 64], d_vals)
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_update: 1 of 4 indices are not above the one before them \(strictly ascending indices are needed\); the first is position 2$"):
        pos.update(d_tree, n, [0, 5, 5, 6], d_vals)
    with pytest.raises(ValueError, match=r"^zk_poseidon_merkle_update: 2 of 4 indices are not above the one before them .*; the first is position 1$"):
        pos.update(d_tree, n, [9, 3, 4, 1], d_vals)
    with pytest.raises(ValueError, match="power of two"):
        pos.update(d_tree, 0, [0], d_vals)
    idx = np.array([0, 2, 1], dtype=np.uint64)
    assert ctx.lib.zk_poseidon_merkle_update(ctx.h, pos.h, d_tree.ptr, n, idx.ctypes.data, d_vals.ptr, 3) == ZK_ERR_INVALID
    assert ctx.lib.zk_poseidon_merkle_update(ctx.h, pos.h, d_tree.ptr, n, None, d_vals.ptr, 3) == ZK_ERR_INVALID  # a null argument
    assert ctx.lib.zk_poseidon_merkle_update(ctx.h, pos.h, d_tree.ptr, n, None, None, 0) == 0  # count = 0 reads nothing
    with pytest.raises(ValueError, match="one value per index"):
        pos.update(d_tree, n, [1, 2], limbs([1]))
    # nothing above was enqueued
    assert (d_tree.download((2 * n - 1, 4)) == tree).all()
    # params of another ctx
    second = zkhip.Ctx(0)
    foreign = ps.Poseidon(second)
    try:
        one = np.zeros(1, dtype=np.uint64)
        assert ctx.lib.zk_poseidon_merkle_update(ctx.h, foreign.h, d_tree.ptr, n, one.ctypes.data, d_vals.ptr, 1) == ZK_ERR_INVALID
        assert b"another ctx" in ctx.lib.zk_last_error(ctx.h)
        assert ctx.lib.zk_poseidon_merkle_roots(ctx.h, foreign.h, d_vals.ptr, one.ctypes.data, out.ptr, 6, 1, out.ptr) == ZK_ERR_INVALID
        assert b"another ctx" in ctx.lib.zk_last_error(ctx.h)
    finally:
        foreign.free()
        second.close()
    assert (d_tree.download((2 * n - 1, 4)) == tree).all()


# ---- a proved chain of two writes ----
def test_two_chained_writes_are_proved_and_verified(ctx, pos):
    """merkle_update_circuit(2, 2): the tree, both updates and both paths on the device; witness, prove, verify_bytes; the broken chains refused"""
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip import poseidon as ps
    from zkhip.field import splitmix_fr

    depth, n, seed = 2, 4, 7
    d_tree = pos.merkle(ctx.to_device(splitmix_fr(n, seed)), n)
    old_root = ints(d_tree.download((2 * n - 1, 4)))[-1]
    writes = [(1, 1001), (2, 1002)]
    steps = []
    for i, v in writes:
        before = ints(d_tree.download((2 * n - 1, 4)))
        sibs = ints(pos.paths(d_tree, n, [i]).download((depth, 4)))
        steps.append((before[i], v, sibs, msm.bits_of(i, depth)))
        pos.update(d_tree, n, [i], limbs([v]))
    after = ints(d_tree.download((2 * n - 1, 4)))
    model_steps, model_trees = msm.chain(pm.merkle(ints(splitmix_fr(n, seed))), n, writes)
    assert steps == model_steps and after == model_trees[-1] and old_root == model_trees[0][-1]

    circuit, layout, v = ps.merkle_update_circuit(depth, 2)
    s = splitmix_fr(circuit["mu"] + 1, seed + 1)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    pk, vk = plonk.preprocess(ctx, pcs, circuit, pr.powers_of_g2(ints(s)))
    plan = plonk.witness_plan(ctx, circuit)
    pi = limbs([old_root, after[-1]])
    a, b, c = plonk.witness(ctx, pk, plan, pi, ps.merkle_update_inputs(layout, v, steps))
    proof = plonk.prove(ctx, pk, a, b, c, pi)
    data = plonk.proof_to_bytes(proof)
    assert plonk.verify_bytes(ctx, vk, pi, data) is True
    assert plonk.verify_bytes(ctx, vk, limbs([old_root, old_root]), data) is False
    copy = rf"^zk_plonk_witness: \d+ of {3 * layout.N} slots differ from the value of their class; the first is slot "
    (ol, nl, sb, bt), second = steps[0], steps[1]
    broken = {"leaf": (pi, [((ol + 1) % R, nl, sb, bt), second]), "sibling": (pi, [(ol, nl, [(sb[0] + 1) % R] + sb[1:], bt), second]),
              "root": (limbs([old_root, (after[-1] + 1) % R]), steps)}
    for kind, (pub, st) in broken.items():
        with pytest.raises(ValueError, match=copy):
            plonk.witness(ctx, pk, plan, pub, ps.merkle_update_inputs(layout, v, st))
