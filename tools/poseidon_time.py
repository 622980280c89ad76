#!/usr/bin/env python3
"""
Times of the Poseidon kernels and of witness generation on the deep narrow Merkle-path circuit -> profiles/poseidon_time.txt.
One process, warm-up 3, median of 20 blocking calls (the call, then a synchronisation of the ctx stream).
  * zk_poseidon_permute at 2^10, 2^16, 2^20 states; zk_poseidon_merkle at 2^10, 2^16, 2^20 leaves;
  * beside them the compiled host's serial rule (host/bin/poseidon_check --time-host K, a process of its own) at 2^10 and 2^16 -- it is
    linear in K, 2^20 would take about a minute per line and is not run;
  * zk_plonk_witness on poseidon.merkle_circuit(depth), depth 1, 8, 32, next to plonk.sample_circuit_wide of the same mu, with the levels
    and launches of zk_witness_plan_info.

EXPECTATION, written before the first run.  A permutation is 828 Fr multiplications (18 per full round, 12 per partial one) and about 590
additions.  DESIGN section 5 puts the Fr multiplier at about 130 G mul/s on a full device, so at most 157 M permutations/s; with the
additions (roughly a fifth of a multiplication each) about 125 M/s: 2^20 states in about 8 ms, 2^16 in about 0.6 ms if 256 workgroups of
256 lanes -- one per CU, one wave per SIMD -- run at a quarter of the full rate.  2^10 states are 4 workgroups: the time of ONE lane's
permutation, 828 dependent multiplications of ~460 instructions each at one wave per SIMD, about 0.7 ms.  The Merkle tree of 2^20 leaves
hashes 2^20 - 1 pairs: the large levels cost what the permutations cost (~8 ms), every level below ~2^16 nodes and each of the nine
levels of the single-workgroup tail costs one lane's permutation (~0.7 ms): about 20 ms.  Witness generation on the Merkle circuit is
~200 levels per hash in ONE workgroup, a barrier and a dependent gather per level: tens of microseconds per level is the guess, so
depth 32 (6000+ levels) is expected in the tens of milliseconds, far above the sampled circuit of the same size.
"""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))

import numpy as np  # noqa: E402

WARM, REPS = 3, 20


def median_ms(be, call) -> float:
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        be.sync()
        if i >= WARM:
            ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def main() -> int:
    import zkhip
    from zkhip import plonk
    from zkhip import poseidon as ps
    from zkhip.field import fr_from_mont, fr_mont, splitmix_fr

    out = ["# tools/poseidon_time.py: warm-up %d, median of %d blocking calls, one process" % (WARM, REPS)]
    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    data = be.to_device(splitmix_fr(3 << 20, 1))
    perm_out, tree = be.alloc(96 << 20), be.alloc(32 * ((2 << 20) - 1))
    for k in (10, 16, 20):
        n = 1 << k
        ms = median_ms(be, lambda: pos.permute(data, n, out=perm_out))
        out.append(f"zk_poseidon_permute n=2^{k}: {ms:.3f} ms  {n / ms / 1e3:.2f} M perm/s  {828 * n / ms / 1e6:.1f} G mul/s")
    for k in (10, 16, 20):
        n = 1 << k
        ms = median_ms(be, lambda: pos.merkle(data, n, out=tree))
        out.append(f"zk_poseidon_merkle  n=2^{k}: {ms:.3f} ms  {(n - 1) / ms / 1e3:.2f} M hash/s")
    check = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host", "bin", "poseidon_check")
    for k in (10, 16):
        r = subprocess.run([check, "--time-host", str(1 << k)], capture_output=True, text=True, timeout=600)
        out += ["host (serial, one core) " + re.sub(r" \((check|root) [0-9a-f]+\)", "", ln) for ln in r.stdout.splitlines()]
    for depth in (1, 8, 32):
        circuit, layout, v = ps.merkle_circuit(depth)
        mu, n = circuit["mu"], 1 << min(depth, 10)  # a tree of at most 2^10 leaves, the path padded by repeating its levels: a timing input
        leaves = [fr_from_mont(x) for x in splitmix_fr(n, 5)]
        t = ps.merkle_host(leaves)
        sibs, bits = ps.merkle_path(t, n, 5 % n)
        sibs, bits = (sibs * depth)[:depth], (bits * depth)[:depth]
        root = ps.path_root_host(leaves[5 % n], sibs, bits)
        key, plan = plonk.witness_key(be, circuit), plonk.witness_plan(be, circuit)
        free = be.to_device(ps.merkle_witness_inputs(layout, v, leaves[5 % n], sibs, bits))
        pi = fr_mont(root).reshape(1, 4)
        ms = median_ms(be, lambda: plonk.witness(be, key, plan, pi, free))
        out.append(f"zk_plonk_witness merkle_circuit(depth={depth}) mu={mu}: {ms:.3f} ms  {plan.info()}")
        sc = plonk.sample_circuit_wide(mu, 7)
        skey, splan = plonk.witness_key(be, sc), plonk.witness_plan(be, sc)
        ms = median_ms(be, lambda: plonk.witness(be, skey, splan, sc["public_inputs"]))
        out.append(f"zk_plonk_witness sample_circuit_wide mu={mu}: {ms:.3f} ms  {splan.info()}")
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "poseidon_time.txt")  # (an argument: another file)
    with open(dest, "w") as f:
        f.write(text)
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
