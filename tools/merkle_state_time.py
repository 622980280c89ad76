#!/usr/bin/env python3
"""
Times of the Merkle state tree calls -> profiles/merkle_state_time.txt.  One process, warm-up 3, median of 20 blocking calls (the call, then
a synchronisation of the ctx stream).  At n = 2^20 and n = 2^24 leaves, for count = 1, 2^8 and 2^16 seeded distinct leaves:
  * zk_poseidon_merkle_update (ascending indices, values already on the device: the library call alone, its index staging included),
    beside zk_poseidon_merkle of the same n MEASURED IN THE SAME RUN;
  * zk_poseidon_merkle_paths and zk_poseidon_merkle_roots (the roots of the gathered paths over arbitrary leaves: a timing input).

EXPECTATION, written before the first run, from profiles/poseidon_time.txt.  One lane's hash is about 0.65 ms of dependent multiplications
(2^10 permutations: 0.645 ms) and 2^16 lanes cost no more (0.670 ms), so a level of an update costs about 0.65 ms whether it hashes one
node or 2^16, and an update of any of these counts about depth x 0.65 ms: ~13 ms at 2^20 -- only modestly below the 18.3 ms rebuild there
-- and ~15.6 ms at 2^24, against a rebuild that grows with n (about 16 x 18 ms).  roots walks the same depth with one lane per path: about
the same as update.  paths is a gather of count x depth elements after one small host-to-device copy: far below both (under a tenth).
A line is marked `confirmed` when the measured time is within 0.7 .. 1.3 of the expected one (paths: when it is under a tenth of the
update of the same n and count), `refuted` otherwise.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))

import numpy as np  # noqa: E402

WARM, REPS = 3, 20
HASH_MS = 0.65  # one lane's hash (profiles/poseidon_time.txt)


def median_ms(be, call) -> float:
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        be.sync()
        if i >= WARM:
            ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def mark(ms: float, expected: float) -> str:
    return f"expected ~{expected:.1f} ms: " + ("confirmed" if 0.7 * expected <= ms <= 1.3 * expected else "refuted")


def main() -> int:
    import zkhip
    from zkhip import poseidon as ps
    from zkhip.field import splitmix_fr

    out = ["# tools/merkle_state_time.py: warm-up %d, median of %d blocking calls, one process" % (WARM, REPS)]
    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    block = splitmix_fr(1 << 20, 1)
    values = be.to_device(splitmix_fr(1 << 16, 2))
    for k in (20, 24):
        n = 1 << k
        leaves = be.to_device(np.tile(block, (n >> 20, 1)))
        tree = be.alloc(32 * (2 * n - 1))
        rebuild = median_ms(be, lambda: pos.merkle(leaves, n, out=tree))
        out.append(f"zk_poseidon_merkle         n=2^{k}: {rebuild:.3f} ms  (the rebuild, same run)")
        rng = np.random.default_rng(k)
        for c in (0, 8, 16):
            count = 1 << c
            idx = np.sort(rng.choice(n, size=count, replace=False)).astype(np.uint64)
            up = median_ms(be, lambda: pos.update(tree, n, idx, values))
            out.append(f"zk_poseidon_merkle_update  n=2^{k} count=2^{c}: {up:.3f} ms  {up / rebuild:.2f} of the rebuild  {mark(up, k * HASH_MS)}")
            sibs = be.alloc(32 * count * k)
            pa = median_ms(be, lambda: pos.paths(tree, n, idx, out=sibs))
            out.append(f"zk_poseidon_merkle_paths   n=2^{k} count=2^{c}: {pa:.3f} ms  expected under a tenth of the update: " + ("confirmed" if pa < up / 10 else "refuted"))
            roots = be.alloc(32 * count)
            ro = median_ms(be, lambda: pos.roots(values, idx, sibs, k, out=roots))
            out.append(f"zk_poseidon_merkle_roots   n=2^{k} count=2^{c}: {ro:.3f} ms  {mark(ro, k * HASH_MS)}")
        del leaves, tree
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "merkle_state_time.txt")  # (an argument: another file)
    with open(dest, "w") as f:
        f.write(text)
    pos.free()
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
