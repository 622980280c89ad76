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

  --update COUNT    the state transition instead: the same tree kept on the device, COUNT writes applied ONE AFTER ANOTHER -- write k puts
                    splitmix_fr(COUNT, S + 2)[k] into leaf (S + 5k) mod 2^D with Poseidon.update, its path taken with Poseidon.paths from
                    the tree before it -- then poseidon.merkle_update_circuit(D, COUNT) through the same pipeline.  Prints
                        circuit sha256 .. / old root .. / new root .. / proof sha256 .. / verdict ..
                    --break leaf | bit | sibling | root alters the first write's old leaf, leaf-level bit or sibling, or the public new
                    root; --sample-only prints the first three lines by the host rules (merkle_host, update_host)

  --transfer [--bits B --amount A]
                    a proved transfer instead: the leaves are BALANCES, leaf k holds 2^(B-2) + (13 S + 41 k) mod 2^(B-2) (4 <= B <= 64); leaf
                    S mod 2^D pays A (default 5) to leaf (S + 1) mod 2^D -- two writes one after another with Poseidon.update, each path
                    from the tree before its write -- then poseidon.merkle_transfer_circuit(D, B), whose inverses and bits the witness
                    generator makes on the device.  Prints
                        circuit sha256 .. / roots <old> <new> / proof sha256 .. / verdict ..
                    --break sibling alters the sender's leaf-level sibling; --sample-only prints the first two lines by the host rules

  --schnorr         "I know a signature under this public key on this public message": sk = S + 1, m = S + 1000, jubjub.sign_host, the native check
                    on the device (Jubjub.schnorr_verify must say 0), then jubjub.schnorr_circuit().  Prints
                        circuit sha256 .. / signature sha256 .. / proof sha256 .. / verdict ..
                    --sample-only prints the first two lines

  --signed-transfer [--bits B --amount A --forge]
                    the same transfer on leaves hash2(hash2(PK.x, PK.y), balance): leaf k belongs to the secret key S + 1 + k (jubjub.keygen_host),
                    balances as for --transfer; the sender signs m = hash2(hash2(receiver key hash, A), old root) with jubjub.sign_host and
                    jubjub.merkle_signed_transfer_circuit(D, B) checks that signature.  --forge signs with the RECEIVER's key instead.  Prints
                        circuit sha256 .. / signature sha256 .. / roots <old> <new> / proof sha256 .. / verdict ..
                    (signature sha256: of R.x || R.y || s); --sample-only prints the first three lines by the host rules
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))

import numpy as np  # noqa: E402


def update(args) -> int:
    """--update COUNT: the proved state transition (module text)"""
    from zkhip import poseidon as ps
    from zkhip.circuit import circuit_digest
    from zkhip.field import R_MOD, fr_from_mont, fr_mont, splitmix_fr

    ints = lambda a: [fr_from_mont(x) for x in np.asarray(a).reshape(-1, 4)]
    depth, n, count = args.depth, 1 << args.depth, args.update
    circuit, layout, v = ps.merkle_update_circuit(depth, count)
    leaves = splitmix_fr(n, args.seed)
    writes = [((args.seed + 5 * k) % n, x) for k, x in enumerate(ints(splitmix_fr(count, args.seed + 2)))]
    print("circuit sha256", circuit_digest(circuit))
    if args.sample_only:
        tree = ps.merkle_host(ints(leaves))
        print("old root %064x" % tree[-1])
        for w in writes:
            tree = ps.update_host(tree, n, [w])
        print("new root %064x" % tree[-1])
        return 0

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    d_tree = pos.merkle(be.to_device(leaves), n)
    root_of = lambda: ints(d_tree.download((1, 4), offset=32 * (2 * n - 2)))[0]
    old_root = root_of()
    print("old root %064x" % old_root)
    steps = []
    for i, x in writes:  # one after another: the old leaf and the path are those of the tree before the write
        old_leaf = ints(d_tree.download((1, 4), offset=32 * i))[0]
        sibs = ints(pos.paths(d_tree, n, [i]).download((depth, 4)))
        steps.append([old_leaf, x, sibs, [(i >> j) & 1 for j in range(depth)]])
        pos.update(d_tree, n, [i], fr_mont(x).reshape(1, 4))
    new_root = root_of()
    pos.free()
    print("new root %064x" % new_root)
    if args.brk == "leaf":
        steps[0][0] = (steps[0][0] + 1) % R_MOD
    if args.brk == "bit":
        steps[0][3][0] ^= 1
    if args.brk == "sibling":
        steps[0][2][0] = (steps[0][2][0] + 1) % R_MOD
    pi = np.stack([fr_mont(old_root), fr_mont((new_root + 1) % R_MOD if args.brk == "root" else new_root)])
    s = splitmix_fr(circuit["mu"] + 1, args.seed + 1)
    pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
    pk, vk = plonk.preprocess(be, pcs, circuit, pr.powers_of_g2(ints(s)))
    plan = plonk.witness_plan(be, circuit)
    try:
        a, b, c = plonk.witness(be, pk, plan, pi, ps.merkle_update_inputs(layout, v, steps))
    except ValueError as e:
        print("refused:", e)
        return 1
    proof = plonk.prove(be, pk, a, b, c, pi)
    print("proof sha256", plonk.proof_digest(proof))
    ok = plonk.verify_bytes(be, vk, pi, plonk.proof_to_bytes(proof))
    print("verdict", "accept" if ok else "reject")
    be.close()
    return 0 if ok else 1


def transfer(args) -> int:
    """--transfer: the proved transfer (module text)"""
    from zkhip import poseidon as ps
    from zkhip.circuit import circuit_digest
    from zkhip.field import R_MOD, fr_from_mont, fr_mont, splitmix_fr

    ints = lambda a: [fr_from_mont(x) for x in np.asarray(a).reshape(-1, 4)]
    depth, n, quarter = args.depth, 1 << args.depth, 1 << (args.bits - 2)
    circuit, layout, v = ps.merkle_transfer_circuit(depth, args.bits)
    balances = [quarter + (13 * args.seed + 41 * k) % quarter for k in range(n)]
    i, j = args.seed % n, (args.seed + 1) % n
    writes = [(i, (balances[i] - args.amount) % R_MOD), (j, (balances[j] + args.amount) % R_MOD)]
    print("circuit sha256", circuit_digest(circuit))
    if args.sample_only:
        tree = ps.merkle_host(balances)
        old_root = tree[-1]
        for w in writes:
            tree = ps.update_host(tree, n, [w])
        print("roots %064x %064x" % (old_root, tree[-1]))
        return 0

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    d_tree = pos.merkle(be.to_device(np.stack([fr_mont(x) for x in balances])), n)
    root_of = lambda: ints(d_tree.download((1, 4), offset=32 * (2 * n - 2)))[0]
    old_root = root_of()
    sides = []
    for k, x in writes:  # one after another: the old leaf and the path are those of the tree before the write
        old_leaf = ints(d_tree.download((1, 4), offset=32 * k))[0]
        sibs = ints(pos.paths(d_tree, n, [k]).download((depth, 4)))
        sides.append((old_leaf, sibs, [(k >> t) & 1 for t in range(depth)]))
        pos.update(d_tree, n, [k], fr_mont(x).reshape(1, 4))
    new_root = root_of()
    pos.free()
    print("roots %064x %064x" % (old_root, new_root))
    if args.brk == "sibling":
        sides[0][1][0] = (sides[0][1][0] + 1) % R_MOD
    pi = np.stack([fr_mont(old_root), fr_mont(new_root)])
    s = splitmix_fr(circuit["mu"] + 1, args.seed + 1)
    pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
    pk, vk = plonk.preprocess(be, pcs, circuit, pr.powers_of_g2(ints(s)))
    plan = plonk.witness_plan(be, circuit)
    try:
        a, b, c = plonk.witness(be, pk, plan, pi, ps.merkle_transfer_inputs(layout, v, args.amount, *sides))
    except ValueError as e:
        print("refused:", e)
        return 1
    proof = plonk.prove(be, pk, a, b, c, pi)
    print("proof sha256", plonk.proof_digest(proof))
    ok = plonk.verify_bytes(be, vk, pi, plonk.proof_to_bytes(proof))
    print("verdict", "accept" if ok else "reject")
    be.close()
    return 0 if ok else 1


def schnorr(args) -> int:
    """--schnorr: the proved signature (module text)"""
    import hashlib

    from zkhip import jubjub as jj
    from zkhip import poseidon as ps
    from zkhip.circuit import circuit_digest
    from zkhip.field import fr_from_mont, fr_mont, splitmix_fr

    ints = lambda a: [fr_from_mont(x) for x in np.asarray(a).reshape(-1, 4)]
    circuit, layout, v = jj.schnorr_circuit()
    sk, m = args.seed + 1, args.seed + 1000
    pk, sig = jj.keygen_host(sk), jj.sign_host(sk, m)
    print("circuit sha256", circuit_digest(circuit))
    print("signature sha256", hashlib.sha256(jj.signature_bytes(sig)).hexdigest())
    if args.sample_only:
        return 0 if jj.verify_host(pk, m, sig) == 0 else 1

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    st = jj.Jubjub(be, pos).schnorr_verify(be.to_device(jj.points_limbs([pk])), be.to_device(fr_mont(m).reshape(1, 4)), be.to_device(jj.signatures_limbs([sig])), 1)
    pos.free()
    if st[0]:
        print("refused: zk_schnorr_verify: status", int(st[0]))
        return 1
    pi = np.stack([fr_mont(pk[0]), fr_mont(pk[1]), fr_mont(m), fr_mont(0)])
    s = splitmix_fr(circuit["mu"] + 1, args.seed + 1)
    pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
    ppk, vk = plonk.preprocess(be, pcs, circuit, pr.powers_of_g2(ints(s)))
    plan = plonk.witness_plan(be, circuit)
    try:
        a, b, c = plonk.witness(be, ppk, plan, pi, jj.schnorr_inputs(layout, v, sig))
    except ValueError as e:
        print("refused:", e)
        return 1
    proof = plonk.prove(be, ppk, a, b, c, pi)
    print("proof sha256", plonk.proof_digest(proof))
    ok = plonk.verify_bytes(be, vk, pi, plonk.proof_to_bytes(proof))
    print("verdict", "accept" if ok else "reject")
    be.close()
    return 0 if ok else 1


def signed_transfer(args) -> int:
    """--signed-transfer: the proved transfer with the sender's signature (module text)"""
    import hashlib

    from zkhip import jubjub as jj
    from zkhip import poseidon as ps
    from zkhip.circuit import circuit_digest
    from zkhip.field import fr_from_mont, fr_mont, splitmix_fr

    ints = lambda a: [fr_from_mont(x) for x in np.asarray(a).reshape(-1, 4)]
    depth, n, quarter = args.depth, 1 << args.depth, 1 << (args.bits - 2)
    circuit, layout, v = jj.merkle_signed_transfer_circuit(depth, args.bits)
    balances = [quarter + (13 * args.seed + 41 * k) % quarter for k in range(n)]
    sks = [args.seed + 1 + k for k in range(n)]
    pks = [jj.keygen_host(sk) for sk in sks]
    keys = [ps.hash2_host(*pk) for pk in pks]
    i, j = args.seed % n, (args.seed + 1) % n
    leaves = [ps.hash2_host(k, bal) for k, bal in zip(keys, balances)]
    writes = [(i, ps.hash2_host(keys[i], balances[i] - args.amount)), (j, ps.hash2_host(keys[j], balances[j] + args.amount))]
    print("circuit sha256", circuit_digest(circuit))
    sign = lambda old_root: jj.sign_host(sks[j] if args.forge else sks[i], jj.signed_transfer_message(keys[j], args.amount, old_root))
    if args.sample_only:
        tree = ps.merkle_host(leaves)
        old_root = tree[-1]
        print("signature sha256", hashlib.sha256(jj.signature_bytes(sign(old_root))).hexdigest())
        for w in writes:
            tree = ps.update_host(tree, n, [w])
        print("roots %064x %064x" % (old_root, tree[-1]))
        return 0

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    d_tree = pos.merkle(be.to_device(np.stack([fr_mont(x) for x in leaves])), n)
    root_of = lambda: ints(d_tree.download((1, 4), offset=32 * (2 * n - 2)))[0]
    old_root = root_of()
    sig = sign(old_root)
    print("signature sha256", hashlib.sha256(jj.signature_bytes(sig)).hexdigest())
    sides = []
    for k, x in writes:  # one after another: the path is that of the tree before the write
        sibs = ints(pos.paths(d_tree, n, [k]).download((depth, 4)))
        sides.append((balances[k], sibs, [(k >> t) & 1 for t in range(depth)]))
        pos.update(d_tree, n, [k], fr_mont(x).reshape(1, 4))
    new_root = root_of()
    pos.free()
    print("roots %064x %064x" % (old_root, new_root))
    pi = np.stack([fr_mont(old_root), fr_mont(new_root)])
    s = splitmix_fr(circuit["mu"] + 1, args.seed + 1)
    pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
    pk, vk = plonk.preprocess(be, pcs, circuit, pr.powers_of_g2(ints(s)))
    plan = plonk.witness_plan(be, circuit)
    try:
        a, b, c = plonk.witness(be, pk, plan, pi, jj.merkle_signed_transfer_inputs(layout, v, args.amount, pks[i], keys[j], sig, *sides))
    except ValueError as e:
        print("refused:", e)
        return 1
    proof = plonk.prove(be, pk, a, b, c, pi)
    print("proof sha256", plonk.proof_digest(proof))
    ok = plonk.verify_bytes(be, vk, pi, plonk.proof_to_bytes(proof))
    print("verdict", "accept" if ok else "reject")
    be.close()
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--break", dest="brk", choices=("bit", "root", "sibling", "leaf"))
    ap.add_argument("--sample-only", action="store_true")
    ap.add_argument("--update", type=int, default=0, metavar="COUNT")
    ap.add_argument("--transfer", action="store_true")
    ap.add_argument("--schnorr", action="store_true")
    ap.add_argument("--signed-transfer", action="store_true")
    ap.add_argument("--forge", action="store_true")
    ap.add_argument("--bits", type=int, default=64)
    ap.add_argument("--amount", type=int, default=5)
    args = ap.parse_args()
    if args.schnorr:
        if args.signed_transfer or args.transfer or args.update or args.brk or args.forge:
            ap.error("--schnorr goes alone (with --seed and --sample-only)")
        return schnorr(args)
    if args.signed_transfer:
        if args.transfer or args.update or args.brk or not 4 <= args.bits <= 64 or not 0 <= args.amount < 1 << 63:
            ap.error("--signed-transfer goes without --transfer, --update and --break, with 4 <= --bits <= 64 and 0 <= --amount < 2^63")
        return signed_transfer(args)
    if args.forge:
        ap.error("--forge goes with --signed-transfer")
    if args.transfer:
        if args.update or args.brk not in (None, "sibling") or not 4 <= args.bits <= 64 or not 0 <= args.amount < 1 << 63:
            ap.error("--transfer goes without --update, with --break sibling only, 4 <= --bits <= 64 and 0 <= --amount < 2^63")
        return transfer(args)
    if args.update < 0 or (args.brk == "leaf" and not args.update):
        ap.error("--update takes a COUNT >= 1, and --break leaf goes with --update")
    if args.update:
        return update(args)

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
