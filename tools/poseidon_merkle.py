#!/usr/bin/env python3
"""
"I know a leaf and a path to this public root", end to end: a tree of 2^D field.splitmix_fr(2^D, S) leaves built on the device
(zk_poseidon_merkle), the path of leaf S mod 2^D, the circuit poseidon.merkle_circuit(D), then
witness_plan -> witness -> preprocess -> prove -> proof bytes -> verify_bytes.  Prints

    circuit sha256 <circuit.circuit_digest>
    root <the root, 64 hex digits of the canonical integer>
    proof sha256 <plonk.proof_digest>
    verdict accept | reject            (or:  refused: <the library's message>  when `witness` refuses the path)

host/bin/poseidon_check takes the same flags and prints the same lines.  The SRS trapdoor is splitmix_fr(mu + 1, S + 1).
  --break bit | sibling | root    flip the leaf-level bit / add 1 to the leaf-level sibling / add 1 to the public root
  --sample-only                   the circuit digest and the root by the host rule (poseidon.merkle_host); no GPU
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))

import numpy as np  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--break", dest="brk", choices=("bit", "root", "sibling"))
    ap.add_argument("--sample-only", action="store_true")
    args = ap.parse_args()

    from zkhip import poseidon as ps
    from zkhip.circuit import circuit_digest
    from zkhip.field import R_MOD, fr_from_mont, fr_mont, splitmix_fr

    ints = lambda a: [fr_from_mont(x) for x in np.asarray(a).reshape(-1, 4)]
    depth, n = args.depth, 1 << args.depth
    index = args.seed % n
    circuit, layout, v = ps.merkle_circuit(depth)
    leaves = splitmix_fr(n, args.seed)
    print("circuit sha256", circuit_digest(circuit))
    if args.sample_only:
        print("root %064x" % ps.merkle_host(ints(leaves))[-1])
        return 0

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    tree = ints(pos.merkle(be.to_device(leaves), n).download((2 * n - 1, 4)))
    pos.free()
    root = tree[-1]
    print("root %064x" % root)
    sibs, bits = ps.merkle_path(tree, n, index)
    if args.brk == "bit":
        bits[0] ^= 1
    if args.brk == "sibling":
        sibs[0] = (sibs[0] + 1) % R_MOD
    pi = fr_mont(root + 1 if args.brk == "root" else root).reshape(1, 4)
    s = splitmix_fr(circuit["mu"] + 1, args.seed + 1)
    pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
    pk, vk = plonk.preprocess(be, pcs, circuit, pr.powers_of_g2(ints(s)))
    plan = plonk.witness_plan(be, circuit)
    try:
        a, b, c = plonk.witness(be, pk, plan, pi, ps.merkle_witness_inputs(layout, v, tree[index], sibs, bits))
    except ValueError as e:
        print("refused:", e)
        return 1
    proof = plonk.prove(be, pk, a, b, c, pi)
    print("proof sha256", plonk.proof_digest(proof))
    ok = plonk.verify_bytes(be, vk, pi, plonk.proof_to_bytes(proof))
    print("verdict", "accept" if ok else "reject")
    be.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
