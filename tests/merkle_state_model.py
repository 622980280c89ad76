"""
An independent statement of a Poseidon Merkle tree that is opened and updated, on top of poseidon_model.py alone (nothing from zkhip): an
update is "replace the leaves, build the whole tree again", a path is pm.path_of, a root is pm.root_of_path, and the update circuit is
judged row by row with pm.evaluate.
"""
import numpy as np

import poseidon_model as pm

R = pm.R


def limbs(xs) -> np.ndarray:
    """canonical integers -> [n, 4] u64 Montgomery limbs"""
    return np.frombuffer(b"".join(((x << 256) % R).to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def ints(a) -> list:
    return pm._ints(np.asarray(a).reshape(-1, 4))


def update(tree, n, writes, **kw):
    """the tree after the writes (index, value) in order -- a later write of a leaf replaces an earlier one: the leaves replaced, ALL of it rebuilt"""
    leaves = list(tree[:n])
    for i, v in writes:
        assert 0 <= i < n
        leaves[i] = v % R
    return pm.merkle(leaves, **kw)


def update_touched(tree, n, writes, **kw):
    """the same on a list whose nodes need NOT be the hashes of their children (a buffer filled with a pattern): the leaves are written, every
    node with a written leaf below it becomes the hash of its two children, every other element stays what it was"""
    out = list(tree)
    for i, v in writes:
        out[i] = v % R
    base, width, nodes = 0, n, {i for i, _ in writes}
    while width > 1:
        nodes = {i // 2 for i in nodes}
        for q in nodes:
            out[base + width + q] = pm.hash2(out[base + 2 * q], out[base + 2 * q + 1], **kw)
        base, width = base + width, width // 2
    return out


def paths(tree, n, indices):
    """one sibling list per index, from the leaf level up"""
    return [pm.path_of(tree, n, i)[0] for i in indices]


def bits_of(index, depth):
    return [(index >> j) & 1 for j in range(depth)]


def root(leaf, sibs, index):
    return pm.root_of_path(leaf, sibs, bits_of(index, len(sibs)))


def chain(tree, n, writes):
    """the writes applied ONE AFTER ANOTHER -> (steps, trees): steps[i] = (old leaf, new leaf, siblings, bits) on the tree before write i,
    trees[i] the tree before write i, trees[-1] the last one"""
    depth = n.bit_length() - 1
    steps, trees = [], [list(tree)]
    for i, v in writes:
        cur = trees[-1]
        steps.append((cur[i], v % R, pm.path_of(cur, n, i)[0], bits_of(i, depth)))
        trees.append(update(cur, n, [(i, v)]))
    return steps, trees


def free_slots(free) -> dict:
    """a [3N, 4] `free` array -> {slot: canonical integer} for pm.evaluate"""
    used = np.flatnonzero(np.asarray(free).any(axis=1))
    return {int(s): x for s, x in zip(used, ints(np.asarray(free)[used]))}
