"""
The Poseidon kernels (csrc/zk_poseidon.hip) bit for bit against the independent model (poseidon_model.py): the batch permutation at sizes
around a wave and a workgroup, in place, on edge values; hash2 with an aliased output; the Merkle tree through the level launches, the
single-workgroup tail and both mixed; the refusals; and a params object with other constants.
"""
import random

import numpy as np
import pytest

import poseidon_model as pm

pytestmark = pytest.mark.gpu
R = pm.R
ALL_ONES_64 = (1 << 64) - 1


def limbs(xs) -> np.ndarray:
    """canonical integers -> [n, 4] u64 Montgomery limbs"""
    return np.frombuffer(b"".join(((x << 256) % R).to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def ints(a) -> list:
    return pm._ints(np.asarray(a).reshape(-1, 4))


RINV = pow(1 << 256, R - 2, R)
# values whose MONTGOMERY form has saturated limbs: the stored words are the pattern reduced mod r
EDGE_STORED = [((1 << 256) - 1) % R, ((1 << 255) - 1) % R, (ALL_ONES_64 << 192 | ALL_ONES_64) % R, (((1 << 32) - 1) << 224) % R, R - 1, 1, 0xFFFFFFFF, R - 0xFFFFFFFF]
EDGE_VALUES = [v % R * RINV % R for v in EDGE_STORED]


@pytest.fixture(scope="module")
def pos(ctx):
    from zkhip import poseidon as ps

    p = ps.Poseidon(ctx)
    yield p
    p.free()


@pytest.fixture(scope="module")
def states():
    """257 states: all zero, all r - 1, the edge patterns, then random ones; and the model's permutation of each (computed once)"""
    rng = random.Random(21)
    s = [(0, 0, 0), (R - 1, R - 1, R - 1)]
    s += [tuple(EDGE_VALUES[(i + j) % len(EDGE_VALUES)] for j in range(3)) for i in range(len(EDGE_VALUES))]
    s += [tuple(rng.randrange(R) for _ in range(3)) for _ in range(257 - len(s))]
    return s, [pm.permute(x) for x in s]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_permute(ctx, pos, states, n):
    s, want = states
    flat = limbs([v for st in s[:n] for v in st])
    d_in = ctx.to_device(flat)
    out = pos.permute(d_in, n).download((3 * n, 4))
    assert (out == limbs([v for st in want[:n] for v in st])).all()
    assert (d_in.download((3 * n, 4)) == flat).all()
    pos.permute(d_in, n, out=d_in)  # in place
    assert (d_in.download((3 * n, 4)) == out).all()


def test_hash2_and_aliased_output(ctx, pos, states):
    s, _ = states
    n = 65
    left, right = [st[1] for st in s[:n]], [st[2] for st in s[:n]]
    want = limbs([pm.hash2(l, r) for l, r in zip(left, right)])
    d_l, d_r = ctx.to_device(limbs(left)), ctx.to_device(limbs(right))
    assert (pos.hash2(d_l, d_r, n).download((n, 4)) == want).all()
    pos.hash2(d_l, d_r, n, out=d_l)
    assert (d_l.download((n, 4)) == want).all() and (d_r.download((n, 4)) == limbs(right)).all()
    d_l.upload(limbs(left))
    pos.hash2(d_l, d_r, n, out=d_r)
    assert (d_r.download((n, 4)) == want).all()


@pytest.fixture(scope="module")
def tree64():
    rng = random.Random(22)
    leaves = [rng.randrange(R) for _ in range(64)]
    return leaves, pm.merkle(leaves)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_merkle_small(ctx, pos, tree64, n):
    from zkhip import poseidon as ps

    leaves = tree64[0][:n]
    got = pos.merkle(ctx.to_device(limbs(leaves)), n).download((2 * n - 1, 4))
    assert ints(got) == ps.merkle_host(leaves) == pm.merkle(leaves)


def test_merkle_512_root_and_one_path(ctx, pos):
    """the default knob at n = 512 (256 nodes are not MORE than 256: one workgroup walks all nine levels, every lane busy on the first),
    checked by the root and one path"""
    n, index = 512, 300
    leaves = [pm.hash2(i, 7) for i in range(8)]  # eight model hashes, spread over the leaves by cheap field arithmetic
    leaves = [(leaves[i % 8] * (i + 1) + i) % R for i in range(n)]
    tree = ints(pos.merkle(ctx.to_device(limbs(leaves)), n).download((2 * n - 1, 4)))
    assert tree[:n] == leaves
    sibs, bits = pm.path_of(tree, n, index)
    assert pm.root_of_path(leaves[index], sibs, bits) == tree[2 * n - 2]
    # and every node of the path is the hash of its children on the device's own tree
    base, cnt, i = 0, n, index
    while cnt > 1:
        assert tree[base + cnt + i // 2] == pm.hash2(tree[base + (i & ~1)], tree[base + (i | 1)])
        base, cnt, i = base + cnt, cnt // 2, i // 2


@pytest.mark.parametrize("tail", [1, 8, 64, 16, 0])
def test_merkle_launch_paths(ctx, pos, tree64, tail):
    """n = 64 -- 32, 16, 8, 4, 2, 1 nodes.  tail 1: every level a launch of its own (the last through the one-workgroup kernel); 8: three level
    launches and one workgroup for 8 .. 1; 64: the single workgroup alone; 16: a mix; 0: level launches only"""
    leaves, want = tree64
    ctx.dbg_tune("poseidon_tail_nodes", tail)
    try:
        got = pos.merkle(ctx.to_device(limbs(leaves)), 64).download((127, 4))
    finally:
        ctx.dbg_tune("poseidon_tail_nodes", 256)
    assert ints(got) == want


def test_merkle_leaves_in_place(ctx, pos, tree64):
    leaves, want = tree64
    buf = ctx.alloc(32 * 127)
    buf.upload(limbs(leaves))
    pos.merkle(buf, 64, out=buf)
    assert ints(buf.download((127, 4))) == want


def test_refusals(ctx, pos):
    from zkhip import poseidon as ps

    buf = ctx.alloc(32 * 16)
    for bad_n in (0, 3, 6):
        with pytest.raises(ValueError, match="power of two"):
            pos.merkle(buf, bad_n, out=buf)
    pos.permute(buf, 0, out=buf)  # n = 0 is fine
    pos.hash2(buf, buf, 0, out=buf)
    rc, M = pm.constants()
    for rf, rp in ((7, 58), (0, 10), (8, 249), (-2, 4)):
        with pytest.raises(ValueError, match="rounds"):
            ps.Poseidon(ctx, ps.make_params(rf, rp, (rc * 4)[:3 * max(rf + rp, 0)], M))
    p = ps.make_params(8, 57, rc, M)
    p["rc_mont"] = p["rc_mont"].copy()
    p["rc_mont"][5] = np.frombuffer(R.to_bytes(32, "little"), dtype="<u8")  # r itself: zero mod r, not reduced
    with pytest.raises(ValueError, match="round constant 5 is not below r"):
        ps.Poseidon(ctx, p)


def test_other_constants(ctx, states):
    """rf = 2, rp = 1 with model-derived constants: the constants are data"""
    from zkhip import poseidon as ps

    rc, M = pm.derived_constants(2, 1, b"test-instance")
    s, _ = states
    n = 70
    other = ps.Poseidon(ctx, ps.make_params(2, 1, rc, M))
    got = other.permute(ctx.to_device(limbs([v for st in s[:n] for v in st])), n).download((3 * n, 4))
    other.free()
    assert ints(got) == [v for st in s[:n] for v in pm.permute(st, rf=2, rp=1, consts=(rc, M))]
