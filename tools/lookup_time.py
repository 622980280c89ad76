#!/usr/bin/env python3
"""
The lookup sumcheck and the stand-alone lookup proof against their nearest sibling -- one process, warm-up 3, median of --reps (20):

  sumcheck  zk_sumcheck_lookup and zk_sumcheck_lookup_fs beside zk_sumcheck_wiring / _fs at the same len = 2^n (six tables against
            seven of which one is the 2N-element tree; 22 multiplications per index pair against 23) at n in --n (16, 20, 22, 24),
            with the ratio and the multiplication count's prediction.
  proof     lookup.prove / lookup.verify at n in --proof-n (16, 20) on lookup.sample_lookup, with the three phase times of prove.

One JSON line per result goes to stdout and to --out (default profiles/lookup_time.txt).

    python tools/lookup_time.py [--n 16,20,22,24] [--proof-n 16,20] [--reps 20] [--seed 7] [--out FILE | -]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16,20,22,24")
    ap.add_argument("--proof-n", default="16,20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_time.txt"), help="file the JSON lines are written to ('-': stdout only)")
    a = ap.parse_args()
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import lookup as lk
    from zkhip import pairing as pr
    from zkhip.field import fr_from_mont, fr_mont, splitmix_fr
    from zkhip.transcript import Transcript

    be = zkhip.Ctx(0)
    out = None if a.out == "-" else open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:  # line by line: a run that is cut short keeps what it measured
            out.write(line + "\n")
            out.flush()

    chunk = 1 << 14
    base = be.to_device(splitmix_fr(chunk, 1))

    def filler(n, k):
        """n elements: chunk i is coef_k * base + i"""
        buf, coef = be.alloc(32 * n), splitmix_fr(1, 50 + k)[0]
        for i in range(max(n // chunk, 1)):
            be.fr_axpb(None, base, coef, fr_mont(i + 1), min(chunk, n), out=buf.at(32 * chunk * i))
        return buf

    free = be.mem_info()[0]
    for n in [int(x) for x in a.n.split(",") if x]:
        N = 1 << n
        need = 32 * (7 * N + 2 * N + 7 * 3 * N // 4)  # the larger set: eq, the 2N tree, num, den, and ping-pong scratch of 7 x (N/2 + N/4)
        if need > 0.8 * free:
            emit({"sumcheck_n": n, "skipped": "needs %.1f GiB of %.1f GiB free" % (need / 2**30, free / 2**30)})
            continue
        gamma, chal = splitmix_fr(1, 3)[0], splitmix_fr(n, 4)
        tabs = [filler(N, k) for k in range(6)]
        tr = Transcript(be, b"time")
        look = timed(lambda: be.sumcheck_lookup(tabs, N, gamma, chal), 3, a.reps)
        look_fs = timed(lambda: be.sumcheck_lookup_fs(tabs, N, gamma, tr), 3, a.reps)
        tree = filler(2 * N, 6)
        wir = timed(lambda: be.sumcheck_wiring(tabs[0], tree, tabs[1], tabs[2], N, gamma, chal), 3, a.reps)
        wir_fs = timed(lambda: be.sumcheck_wiring_fs(tabs[0], tree, tabs[1], tabs[2], N, gamma, tr), 3, a.reps)
        tr.free()
        del tabs, tree
        emit({"sumcheck_n": n, "lookup_ms": look, "lookup_fs_ms": look_fs, "wiring_ms": wir, "wiring_fs_ms": wir_fs, "lookup_over_wiring": look / wir,
              "lookup_fs_over_wiring_fs": look_fs / wir_fs, "predicted_by_multiplications": 22 / 23})
    for n in [int(x) for x in a.proof_n.split(",") if x]:
        t, f, idx = lk.sample_lookup(n, a.seed)
        s = lk.sample_srs(n, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
        pk, vk = lk.preprocess(be, pcs, t, pr.powers_of_g2([fr_from_mont(x) for x in s]))
        d_f, d_idx = be.to_device(f), be.to_device(idx)
        g = {"proof_n": n}
        reps = max(a.reps // 4, 3)
        tb = {}
        proof = lk.prove(be, pk, d_f, d_idx)
        g["prove_ms"] = timed(lambda: lk.prove(be, pk, d_f, d_idx, timing=tb), 1, reps)
        g.update(commit_ms=tb["commit_s"] * 1e3, sumcheck_ms=tb["sumcheck_s"] * 1e3, opening_ms=tb["opening_s"] * 1e3)
        ok, _ = once(lambda: lk.verify(be, vk, proof))
        g["verify_ms"] = timed(lambda: lk.verify(be, vk, proof), 1, reps)
        g["ok"] = bool(ok)
        emit(g)
    be.close()


if __name__ == "__main__":
    main()
