#!/usr/bin/env python3
"""
Times the witness generation on the device: zk_plonk_witness (zkhip.plonk.witness, check included, the plan already built) on the sampled
test circuit of 2^mu rows beside the compiled host's sampler loop -- the row loop of host/zkhost/plonk.hpp's sampler alone, the big-int
loop that copies a, b and computes c, without the draws, sigma and the trapdoor (host/bin/plonk_check --sample-only --time-sample R); it
is the only CPU baseline the project has --, its share of plonk.prove on the same circuit, and the plan build time.  One protocol for all
four figures: warm-up 3, median of R (--reps, 20) blocking calls; the three device figures in this process, the host loop in one process
of the compiled host.  The witness time does NOT include the plan build (once per circuit), which is reported beside it; the sampler's
counterpart of the plan, its sigma construction, is not in the loop time either.  Writes profiles/witness_time.txt.

    python tools/witness_time.py [--mu 16 20] [--gate wide] [--reps 20] [--out profiles/witness_time.txt]

--lookup-fn: what a lookup-computing row costs.  zk_plonk_witness_lookup on plonk.sample_circuit_lookup_fn (lookup rows with the gate
switched off: their c comes from the XOR table) beside zk_plonk_witness on plonk.sample_circuit_wide of the same size -- the plain wide
path, which a lookup plan does not touch, as the yardstick --, the plan build of each (the lookup plan's includes the key table, built on
the device), the share of lookup-computing rows and the level counts.  The same protocol.  Writes profiles/witness_lookup_time.txt.

    python tools/witness_time.py --lookup-fn [--mu 16 20] [--reps 20] [--out profiles/witness_lookup_time.txt]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scalable-collaborative-zksnark_amd")
sys.path.insert(0, PKG)
HOST = os.path.join(PKG, "host")


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def host_loop_ms(mu, seed, wide, reps):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    args = [os.path.join(HOST, "bin", "plonk_check"), "--mu", str(mu), "--seed", str(seed), "--sample-only", "--time-sample", str(reps)] + (["--gate", "wide"] if wide else [])
    r = subprocess.run(args, capture_output=True, text=True, check=True)
    return float(re.search(r"sample row loop seconds ([0-9.]+)", r.stdout).group(1)) * 1e3


def lookup_fn(ctx, o):
    import numpy as np

    from zkhip import plonk

    lines = [f"# tools/witness_time.py --lookup-fn: seed={o.seed}; ms; every figure: warm-up 3, median of {o.reps} blocking calls, one process; the witness figures "
             f"exclude the plan build; yardstick: zk_plonk_witness on sample_circuit_wide of the same size"]
    for mu in o.mu:
        N, row = 1 << mu, {}
        for name, c, lk in (("lookup-fn", plonk.sample_circuit_lookup_fn(mu, o.seed), True), ("wide", plonk.sample_circuit_wide(mu, o.seed), False)):
            pk, pi = plonk.witness_key(ctx, c), c["public_inputs"]
            ts = []
            for i in range(3 + o.reps):  # warm-up 3; every plan but the last is freed at once, outside the timed region
                t = time.perf_counter()
                plan = plonk.witness_plan(ctx, c, lookup=lk)
                ts.append((time.perf_counter() - t) * 1e3)
                if i < 2 + o.reps:
                    plan.free()
            plan_ms = statistics.median(ts[3:])
            free = ctx.to_device(np.ascontiguousarray(c["free"], dtype=np.uint64)) if lk else None
            out = []
            wit_ms = median_ms(lambda: out.append(plonk.witness(ctx, pk, plan, pi, free)) or out.__delitem__(slice(0, -1)), o.reps, 3)
            assert all((x.download((N, 4)) == c[k]).all() for x, k in zip(out[-1], "abc")), "the generated wires are not the sampler's"
            row[name] = (wit_ms, plan_ms, plan.info())
            if lk:
                share = float(((c["lookup"]["qk"] != 0).any(axis=1) & (c["qO"] == 0).all(axis=1)).mean())
        (lw, lp, li), (ww, wp, wi) = row["lookup-fn"], row["wide"]
        lines.append(f"mu={mu}: zk_plonk_witness_lookup {lw:.3f} ({100 * share:.1f} % lookup-computing rows; levels={li['levels']} max_level_rows={li['max_level_rows']} "
                     f"launches={li['launches']}; plan build {lp:.1f}) | zk_plonk_witness wide {ww:.3f} (levels={wi['levels']} max_level_rows={wi['max_level_rows']} "
                     f"launches={wi['launches']}; plan build {wp:.1f}) | ratio {lw / ww:.2f}x")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lookup-fn", action="store_true")
    ap.add_argument("--mu", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--gate", choices=["wide"], default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    o.out = o.out or os.path.join(ROOT, "profiles", "witness_lookup_time.txt" if o.lookup_fn else "witness_time.txt")
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import plonk

    ctx = zkhip.Ctx(0)
    if o.lookup_fn:
        lines = lookup_fn(ctx, o)
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        ctx.close()
        return
    lines = [f"# tools/witness_time.py: gate={o.gate or 'basic'} seed={o.seed}; ms; every figure: warm-up 3, median of {o.reps} blocking calls (device figures: one process; "
             f"host row loop: one process of the compiled host); zk_plonk_witness excludes the plan build, the host row loop excludes the draws and sigma"]
    for mu in o.mu:
        c = (plonk.sample_circuit_wide if o.gate else plonk.sample_circuit)(mu, o.seed)
        pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
        pk, _vk = plonk.preprocess(ctx, pcs, c)
        pi = c["public_inputs"]
        plans = []
        plan_ms = median_ms(lambda: plans.append(plonk.witness_plan(ctx, c)), o.reps, 3)  # (the plans are freed outside the timed calls)
        plan = plans.pop()
        del plans[:]
        out = []
        wit_ms = median_ms(lambda: out.append(plonk.witness(ctx, pk, plan, pi)) or out.__delitem__(slice(0, -1)), o.reps, 3)
        a, b, cc = out[-1]
        N = 1 << mu
        assert all((x.download((N, 4)) == c[k]).all() for x, k in zip((a, b, cc), "abc")), "the generated wires are not the sampler's"
        prove_ms = median_ms(lambda: plonk.prove(ctx, pk, a, b, cc, pi), o.reps, 3)
        cpu_ms = host_loop_ms(mu, o.seed, bool(o.gate), o.reps)
        info = plan.info()
        lines.append(f"mu={mu} levels={info['levels']} max_level_rows={info['max_level_rows']} launches={info['launches']}: zk_plonk_witness {wit_ms:.3f} | "
                     f"host sampler row loop {cpu_ms:.1f} ({cpu_ms / wit_ms:.1f}x) | plonk.prove {prove_ms:.2f} (witness = {100 * wit_ms / prove_ms:.1f} % of it) | "
                     f"plan build {plan_ms:.1f} (not in zk_plonk_witness)")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
