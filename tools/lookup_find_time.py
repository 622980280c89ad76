#!/usr/bin/env python3
"""
The device's own search for the table rows against the call it replaces -- one process, warm-up 3, median of --reps (20) blocking calls:

  find    zk_lookup_find beside zk_lookup_multiplicities, and zk_lookup3_find beside zk_lookup3_multiplicities with the sample's idx given
          (the parent's check-and-count pass), at n in --n (16, 20, 22, 24) with distinct = N / 4 and N; with --dup also distinct = 1, where
          every insert meets one slot.  The table holds `distinct` different entries padded to N by repeating the last one, the rows draw
          from them (lookup.sample_lookup's shape; the three-column form repeats it per column, every row selected).
  proof   plonk.prove with idx = FIND beside plonk.prove with the sample's idx, both gate kinds, at mu in --proof-mu (16, 20): the last of
          three runs each, as tools/plonk_time.py reports them.

Prediction, recorded before any measurement: the multiplicities call reads N rows and gathers N entries; the find reads the N entries once more
to insert them, touches about one random 4-byte slot per insert and per probe and gathers about 1.5 entries per probe at a load <= 0.5 --
2.5 to 3.5 times the bytes, most of them random: 2.5 - 4 x the multiplicities call, and under 2 % of plonk.prove at 2^20.  Every line carries
the verdict for its own ratio.

One JSON line per result goes to stdout and to --out (default profiles/lookup_find_time.txt).

    python tools/lookup_find_time.py [--n 16,20,22,24] [--proof-mu 16,20] [--dup] [--reps 20] [--seed 7] [--out FILE | -] [--append]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))

PREDICTED = [2.5, 4.0]


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts) * 1e3


def once(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def band(x):
    return "confirmed" if PREDICTED[0] <= x <= PREDICTED[1] else ("refuted: below the band" if x < PREDICTED[0] else "refuted: above the band")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16,20,22,24")
    ap.add_argument("--proof-mu", default="16,20")
    ap.add_argument("--dup", action="store_true", help="also distinct = 1: every insert on one slot")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_find_time.txt"), help="file the JSON lines are written to ('-': stdout only)")
    ap.add_argument("--append", action="store_true", help="add to --out (a measurement split over several runs)")
    a = ap.parse_args()
    import numpy as np

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip.field import fr_from_mont, fr_mont, splitmix_fr

    be = zkhip.Ctx(0)
    out = None if a.out == "-" else open(a.out, "a" if a.append else "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:  # line by line: a run that is cut short keeps what it measured
            out.write(line + "\n")
            out.flush()

    free = be.mem_info()[0]
    for n in [int(x) for x in a.n.split(",") if x]:
        N = 1 << n
        need = 32 * 7 * N + 32 * N + 4 * N + 12 * N  # six columns and qk, m, idx, counters and slots
        if need > 0.8 * free:
            emit({"find_n": n, "skipped": "needs %.1f GiB of %.1f GiB free" % (need / 2**30, free / 2**30)})
            continue
        draw = splitmix_fr(N, a.seed + 11)[:, 0]
        for distinct in [N // 4, N] + ([1] if a.dup else []):
            idx = (draw % np.uint64(distinct)).astype(np.uint32)
            ts = []
            for j in range(3):
                col = np.empty((N, 4), dtype=np.uint64)
                col[:distinct] = splitmix_fr(distinct, a.seed + 20 + j)
                col[distinct:] = col[distinct - 1]
                ts.append(col)
            d_t = [be.to_device(c) for c in ts]
            d_w = [be.to_device(c[idx]) for c in ts]
            del ts
            d_idx, d_qk = be.to_device(idx), be.to_device(np.tile(fr_mont(1), (N, 1)))
            o_idx, o_m = be.alloc(4 * N), be.alloc(32 * N)
            g = {"find_n": n, "distinct": distinct}
            g["multiplicities_ms"] = timed(lambda: be.lookup_multiplicities(d_w[0], d_t[0], d_idx, N, out=o_m), 3, a.reps)
            g["find_ms"] = timed(lambda: be.lookup_find(d_w[0], d_t[0], N, idx=o_idx, m=o_m), 3, a.reps)
            same = bool((o_idx.download((N,), np.uint32) == idx).all())
            g["multiplicities3_ms"] = timed(lambda: be.lookup3_multiplicities(d_w, d_t, d_qk, d_idx, N, out=o_m), 3, a.reps)
            g["find3_ms"] = timed(lambda: be.lookup3_find(d_w, d_t, d_qk, N, idx=o_idx, m=o_m), 3, a.reps)
            g["idx_is_the_samples"] = same and bool((o_idx.download((N,), np.uint32) == idx).all())
            g["find_over_multiplicities"], g["find3_over_multiplicities3"] = g["find_ms"] / g["multiplicities_ms"], g["find3_ms"] / g["multiplicities3_ms"]
            g.update(predicted=PREDICTED, prediction=band(g["find_over_multiplicities"]), prediction3=band(g["find3_over_multiplicities3"]))
            emit(g)
            del d_t, d_w, d_idx, d_qk, o_idx, o_m
    for mu in [int(x) for x in a.proof_mu.split(",") if x]:
        for kind in (None, "wide"):
            g = {"proof_mu": mu, "gate": kind or "basic"}
            c = plonk.sample_circuit_lookup(mu, a.seed, gate=kind)
            pcs = dp.PolynomialCommitmentCub.new(be, c["s"]).mature()
            pk, vk = plonk.preprocess(be, pcs, c, pr.powers_of_g2([fr_from_mont(x) for x in c["s"]]))
            wires, idx = [be.to_device(c[k]) for k in ("a", "b", "c")], be.to_device(c["idx"])
            digests = {}
            for name, given in (("idx", idx), ("find", plonk.FIND)):
                for rep in range(3):  # the last of three runs is reported (the first ones grow the arenas)
                    proof, g[name + "_prove_ms"] = once(lambda: plonk.prove(be, pk, *wires, c["public_inputs"], idx=given))
                digests[name] = plonk.proof_digest(proof)
            g["same_digest"] = digests["idx"] == digests["find"]
            g["verdict"] = bool(plonk.verify(be, vk, c["public_inputs"], proof))
            w_cols, t_cols = wires, [pk["tables"][k] for k in ("t0", "t1", "t2")]
            N = 1 << mu
            g["multiplicities3_ms"] = timed(lambda: be.lookup3_multiplicities(w_cols, t_cols, pk["tables"]["qk"], idx, N), 3, a.reps)
            g["find3_ms"] = timed(lambda: be.lookup3_find(w_cols, t_cols, pk["tables"]["qk"], N), 3, a.reps)
            g["find_over_prove"] = g["find3_ms"] / g["idx_prove_ms"]
            g["added_over_prove"] = (g["find3_ms"] - g["multiplicities3_ms"]) / g["idx_prove_ms"]
            g.update(predicted_share="< 0.02", prediction=("confirmed" if g["find_over_prove"] < 0.02 else "refuted"))
            emit(g)
            del pk, vk, proof, wires, idx, pcs
    if out:
        out.close()
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
