"""
What Fiat-Shamir on the device costs: for each of the three fused sumchecks the wall time of the transcript-driven call
(zk_sumcheck_*_fs) beside its preset-challenge parent on the same tables in the same process, and the whole non-interactive provers
(zkhip.nizk) beside the batched provers with pre-sampled challenges.  Warm-up, then --reps timed calls, median (and minimum).

    python tools/fs_time.py [--n 16 20 24] [--reps 20] [--no-provers] [--out profiles/fs_time.txt]

One JSON line per size; --out appends them to a file as well.
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
    return round(statistics.median(ts) * 1e3, 4), round(min(ts) * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--no-provers", action="store_true", help="the three sumchecks only (no SRS, no openings)")
    ap.add_argument("--prover-max-n", type=int, default=20, help="largest n at which the whole provers are timed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import nizk
    from zkhip import wiring as wr
    from zkhip import zerocheck as zc
    from zkhip.field import splitmix_fr
    from zkhip.transcript import Transcript

    be = zkhip.Ctx(0)
    for n in a.n:
        N = 1 << n
        out = {"n": n, "reps": a.reps}
        tabs, tau, chal, s = zc.satisfied_circuit(be, n, a.seed)
        eq = be.eq_table(tau)
        gate = (eq, tabs["q1"], tabs["q2"], tabs["a"], tabs["b"], tabs["c"], tabs["in"])
        tr = Transcript(be, b"time")
        out["gate_ms"], out["gate_min_ms"] = timed(lambda: be.sumcheck_gate(*gate, N, chal), 3, a.reps)
        out["gate_fs_ms"], out["gate_fs_min_ms"] = timed(lambda: be.sumcheck_gate_fs(*gate, N, tr), 3, a.reps)
        # wiring: the tables of a real instance (alpha, beta, gamma of the circuit's own streams)
        w, sid, ssigma, alpha, beta, gamma, wtau, wchal, ws = wr.permuted_circuit(be, n, a.seed)
        num, den = be.fr_axpb(w, sid, alpha, beta, N), be.fr_axpb(w, ssigma, alpha, beta, N)
        tree = be.product_tree(be.fr_batch_div(num, den, N), N)
        weq = be.eq_table(wtau)
        out["wiring_ms"], out["wiring_min_ms"] = timed(lambda: be.sumcheck_wiring(weq, tree, num, den, N, gamma, wchal), 3, a.reps)
        out["wiring_fs_ms"], out["wiring_fs_min_ms"] = timed(lambda: be.sumcheck_wiring_fs(weq, tree, num, den, N, gamma, tr), 3, a.reps)
        # multi: the six pairs of the gate's batch instance
        es = [be.eq_table(splitmix_fr(n, 900 + j)) for j in range(6)]
        fs = [tabs[k] for k in zc.OPENED]
        out["multi6_ms"], out["multi6_min_ms"] = timed(lambda: be.sumcheck_multi(es, fs, N, chal), 3, a.reps)
        out["multi6_fs_ms"], out["multi6_fs_min_ms"] = timed(lambda: be.sumcheck_multi_fs(es, fs, N, tr), 3, a.reps)
        tr.free()
        del es, eq, weq
        if not a.no_provers and n <= a.prover_max_n:
            reps = max(3, a.reps // 4)
            pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
            al, rho = splitmix_fr(1, 1)[0], splitmix_fr(n, 2)
            out["gate_prove_batched_ms"], _ = timed(lambda: zc.gate_zerocheck_prove_batched(be, pcs, tabs, tau, chal, al, rho), 1, reps)
            out["gate_prove_ni_ms"], _ = timed(lambda: nizk.gate_prove_ni(be, pcs, tabs), 1, reps)
            del pcs
            wpcs = dp.PolynomialCommitmentCub.new(be, ws).mature()
            rho1 = splitmix_fr(n + 1, 3)
            out["wiring_prove_batched_ms"], _ = timed(lambda: wr.wiring_prove_batched(be, wpcs, w, sid, ssigma, N, alpha, beta, gamma, wtau, wchal, al, rho, rho1), 1, reps)
            out["wiring_prove_ni_ms"], _ = timed(lambda: nizk.wiring_prove_ni(be, wpcs, w, sid, ssigma, N), 1, reps)
            del wpcs
        del tabs, w, sid, ssigma, num, den, tree
        be.trim() if hasattr(be, "trim") else None
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    be.close()


if __name__ == "__main__":
    main()
