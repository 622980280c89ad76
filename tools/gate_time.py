"""
Gate ZeroCheck from Python: prove + verify a satisfied circuit (the circuit of host/bin/gate_check for the same seed), and the
timing of zk_sumcheck_gate against its yardstick -- the six-call simulation it makes real: one zk_sumcheck_batch of six product
items on (eq,q1) (q1,a+b) (eq,q2) (a,b) (q2,a) (eq,c-in), same process, same tables.  Warm-up, then --reps timed calls, median.

    python tools/gate_time.py --n 20 [--seed 7] [--reps 20] [--break-gate K] [--digest] [--no-proof]
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
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--break-gate", type=int, default=None)
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--no-proof", action="store_true", help="timing only (no SRS, no openings: sizes beyond the proof's memory)")
    a = ap.parse_args()
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import zerocheck as zc
    from zkhip.field import fr_from_mont

    be = zkhip.Ctx(0)
    n, m = a.n, 1 << a.n
    tabs, tau, chal, s = zc.satisfied_circuit(be, n, a.seed, a.break_gate)
    out = {"n": n, "seed": a.seed}
    if not a.no_proof:
        cub = dp.PolynomialCommitmentCub.new(be, s)
        vk = dp.pcs_vk(be, pr.powers_of_g2([fr_from_mont(x) for x in s]))
        tm = {}
        proof = zc.gate_zerocheck_prove(be, cub.mature(), tabs, tau, chal, timing=tm)
        t = time.perf_counter()
        ok = zc.gate_zerocheck_verify(be, vk, proof, tau, chal)
        out.update(verdict="accept" if ok else "reject", eq_table_ms=tm["eq_table_s"] * 1e3, sumcheck_gate_first_call_ms=tm["sumcheck_s"] * 1e3,
                   verify_ms=(time.perf_counter() - t) * 1e3)
        if a.digest:
            out["proof_sha256"] = zc.proof_digest(proof)
        del cub, proof
    # ---- the comparison run ----
    eq = be.eq_table(tau)
    apb, cmi = be.fr_add(tabs["a"], tabs["b"], m), be.fr_sub(tabs["c"], tabs["in"], m)
    six = [(eq, tabs["q1"]), (tabs["q1"], apb), (eq, tabs["q2"]), (tabs["a"], tabs["b"]), (tabs["q2"], tabs["a"]), (eq, cmi)]

    def eqt():
        be.eq_table(tau, out=eq)
        be.sync()

    gate_med, gate_min = timed(lambda: be.sumcheck_gate(eq, tabs["q1"], tabs["q2"], tabs["a"], tabs["b"], tabs["c"], tabs["in"], m, chal), 3, a.reps)
    six_med, six_min = timed(lambda: be.sumcheck_batch([("product", f, g, m, chal) for f, g in six]), 3, a.reps)
    eq_med, eq_min = timed(eqt, 3, a.reps)
    # algorithmic bytes of the gate sumcheck: round i reads 7 tables of m / 2^i and writes 7 of m / 2^(i+1) elements
    gate_bytes = sum(7 * 32 * ((m >> i) + (m >> (i + 1))) for i in range(n))
    out.update(reps=a.reps, sumcheck_gate_ms={"median": gate_med * 1e3, "min": gate_min * 1e3},
               six_product_batch_ms={"median": six_med * 1e3, "min": six_min * 1e3}, eq_table_timed_ms={"median": eq_med * 1e3, "min": eq_min * 1e3},
               gate_over_six=gate_med / six_med, gate_algorithmic_GBps=gate_bytes / gate_med / 1e9, eq_table_GBps=32 * m / eq_med / 1e9)
    print(json.dumps(out))
    be.close()
    return 0 if out.get("verdict", "accept") == "accept" else 1


if __name__ == "__main__":
    sys.exit(main())
