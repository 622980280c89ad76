#!/usr/bin/env python3
"""
Times of advice rows in witness generation -> profiles/advice_time.txt.  One process, warm-up 3, median of 20 blocking calls.
  (a) zk_plonk_witness on ONE flat level of 2^16 and 2^20 ADV_INV0 rows on free values, beside zk_fr_batch_div (numerator 1) of the same
      count in the same run;
  (b) the same level of adv_bits(60, 8) rows, beside a level of gate rows c = 3 a + 1 of the same count;
  (c) witness, prove and verify_bytes on poseidon.merkle_transfer_circuit(20, 64), beside poseidon.merkle_update_circuit(20, 2) -- the
      closest circuit without advice; the difference is the price of the range checks -- with the levels of zk_witness_plan_info.
      (The paths are timing inputs: the witness is refused at its last step, after every level ran; prove runs on the wires it left.)

EXPECTATION, written before the first run.  One ADV_INV0 lane does a Fermat exponentiation: 255 squarings and about 125 multiplications,
roughly 380 dependent Fr multiplications.  At the ~130 G mul/s of the Fr multiplier on a full device 2^20 inverses are
4 * 10^8 multiplications, about 3 ms; at 2^16 the 256 workgroups are one wave per SIMD and the call is bound by ONE lane's chain, about
0.3 ms.  zk_fr_batch_div uses Montgomery's trick, three multiplications per element plus one inversion per lane, and should be several
times cheaper per element at 2^20; the ratio is reported, not gated on.  A bit-field row is one multiplication out of Montgomery form,
shifts, and one multiplication back -- fewer than a gate row's ten: (b) should cost what the gate level costs, both bound by the 96 bytes
a row stores.  (c): the transfer circuit adds 3 * 64 bit rows that all sit on ONE early level, 3 * 63 recomposition levels of one row each
and one inversion level to a run of ~16 000 levels; at the 8.2 us per level of profiles/poseidon_time.txt the ~190 extra levels are about
1.6 ms on ~130 ms, and the inversion level costs one lane's chain, ~0.3 ms: `witness` within a few per cent of the update circuit's; prove
and verify_bytes equal (same mu).
"""
import os
import statistics
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


def flat_level(mu: int, code: int) -> dict:
    """row x >= 4 reads a free a: an advice row with `code`, or (code 0) a gate row c = 3 a + 1.  Fixed points only: sigma is the identity"""
    from zkhip.circuit import _limbs

    N, l = 1 << mu, 4
    col = lambda head, rest: np.concatenate([np.repeat(_limbs([head]), l, axis=0), np.repeat(_limbs([rest]), N - l, axis=0)])
    c = {"gate": "wide", "mu": mu, "l": l, "sigma": np.arange(3 * N, dtype=np.uint64), "public_inputs": _limbs([3, 8, 13, 18])}
    c.update(qL=col(0, 0 if code else 3), qR=col(0, 0), qM=col(0, 0), qO=col(1, 0 if code else 1), qC=col(0, 0 if code else 1), qH=col(0, 0))
    if code:
        c["advice"] = np.concatenate([np.zeros(l, dtype=np.uint32), np.full(N - l, code, dtype=np.uint32)])
    return c


def main() -> int:
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip import poseidon as ps
    from zkhip.field import fr_from_mont, fr_mont, splitmix_fr

    out = ["# tools/advice_time.py: warm-up %d, median of %d blocking calls, one process" % (WARM, REPS)]
    be = zkhip.Ctx(0)
    for mu in (16, 20):
        N = 1 << mu
        free = be.to_device(splitmix_fr(3 * N, 3))
        ms = {}
        for name, code in (("inv0", plonk.ADV_INV0), ("bits", plonk.adv_bits(60, 8)), ("gate", 0)):
            c = flat_level(mu, code)
            key, plan = plonk.witness_key(be, c), plonk.witness_plan(be, c)
            ms[name] = median_ms(be, lambda: plonk.witness(be, key, plan, c["public_inputs"], free))
            out.append(f"zk_plonk_witness flat level of 2^{mu} {name} rows: {ms[name]:.3f} ms  {plan.info()}")
        ones, quo = be.to_device(np.repeat(fr_mont(1).reshape(1, 4), N, axis=0)), be.alloc(32 * N)
        div = median_ms(be, lambda: be.fr_batch_div(ones, free, N, out=quo))
        out.append(f"zk_fr_batch_div n=2^{mu}: {div:.3f} ms  inv0 level / batch_div = {ms['inv0'] / div:.2f}x  bits level / gate level = {ms['bits'] / ms['gate']:.2f}x")
    depth, n = 20, 1 << 10  # a tree of 2^10 leaves, the paths padded by repeating their levels: timing inputs
    leaves = [fr_from_mont(x) % (1 << 62) for x in splitmix_fr(n, 5)]
    t = ps.merkle_host(leaves)
    pad = lambda k: tuple((v * depth)[:depth] for v in ps.merkle_path(t, n, k))
    for name in ("transfer", "update"):
        if name == "transfer":
            circuit, layout, v = ps.merkle_transfer_circuit(depth, 64)
            free = ps.merkle_transfer_inputs(layout, v, 5, (leaves[0], *pad(0)), (leaves[1], *pad(1)))
        else:
            circuit, layout, v = ps.merkle_update_circuit(depth, 2)
            free = ps.merkle_update_inputs(layout, v, [(leaves[0], leaves[0] - 5, *pad(0)), (leaves[1], leaves[1] + 5, *pad(1))])
        s = splitmix_fr(circuit["mu"] + 1, 8)
        pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
        pk, vk = plonk.preprocess(be, pcs, circuit, pr.powers_of_g2([fr_from_mont(x) for x in s]))
        plan, d_free, pi = plonk.witness_plan(be, circuit), be.to_device(free), np.stack([fr_mont(t[-1]), fr_mont(t[-1])])
        N = 1 << circuit["mu"]
        w = tuple(be.alloc(32 * N) for _ in range(3))
        sels, h_pi, lk = plonk._witness_args(pk, plan, pi)

        def gen():
            try:
                be.plonk_witness(plan, sels, h_pi, d_free, w, **lk)
            except ValueError:  # the padded paths do not reach the roots: refused after every level ran
                pass

        ms_w = median_ms(be, gen)
        proof = [None]
        ms_p = median_ms(be, lambda: proof.__setitem__(0, plonk.prove(be, pk, *w, pi)))
        raw = plonk.proof_to_bytes(proof[0])
        ms_v = median_ms(be, lambda: plonk.verify_bytes(be, vk, pi, raw))
        out.append(f"{name} circuit depth={depth} mu={circuit['mu']}: witness {ms_w:.3f} ms  prove {ms_p:.3f} ms  verify_bytes {ms_v:.3f} ms  {plan.info()}")
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "advice_time.txt")  # (an argument: another file)
    with open(dest, "w") as f:
        f.write(text)
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
