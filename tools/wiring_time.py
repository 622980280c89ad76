"""
Wiring PermCheck from Python: prove + verify a satisfied copy-constraint system (the circuit of host/bin/wiring_check for the same
seed), and the timing of zk_sumcheck_wiring against its yardstick -- the form it replaces: the six product sumchecks of
hyperplonk.rs:133-140 as one zk_sumcheck_batch on (eq,v1x) (eq,vx0) (vx0,vx1) (eq,den) (h,den) (eq,num) plus the
zk_fr_deinterleave that form needs for v(x,0) / v(x,1), same process, same tables.  Warm-up, then --reps timed calls, median.

    python tools/wiring_time.py --mu 20 [--seed 7] [--reps 20] [--break-wire K] [--digest] [--no-proof]
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
    ap.add_argument("--mu", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--break-wire", type=int, default=None)
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--no-proof", action="store_true", help="timing only (no SRS, no openings: sizes beyond the proof's memory)")
    a = ap.parse_args()
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import wiring as wr
    from zkhip.field import fr_from_mont

    be = zkhip.Ctx(0)
    mu, n = a.mu, 1 << a.mu
    w, sid, ssigma, alpha, beta, gamma, tau, chal, s = wr.permuted_circuit(be, mu, a.seed, a.break_wire)
    out = {"mu": mu, "seed": a.seed}
    if not a.no_proof:
        cub = dp.PolynomialCommitmentCub.new(be, s)
        vk_mu, vk_mu1 = wr.verifying_keys(be, pr.powers_of_g2([fr_from_mont(x) for x in s]))
        tm = {}
        proof = wr.wiring_prove(be, cub.mature(), w, sid, ssigma, n, alpha, beta, gamma, tau, chal, timing=tm)
        t = time.perf_counter()
        ok = wr.wiring_verify(be, vk_mu, vk_mu1, proof, alpha, beta, gamma, tau, chal)
        out.update(verdict="accept" if ok else "reject", failed_field_checks=wr.failed_checks(proof, alpha, beta, gamma, tau, chal),
                   tables_ms=tm["tables_s"] * 1e3, sumcheck_wiring_first_call_ms=tm["sumcheck_s"] * 1e3, verify_ms=(time.perf_counter() - t) * 1e3)
        if a.digest:
            out["proof_sha256"] = wr.proof_digest(proof)
        del cub, proof
    # ---- the comparison run ----
    num, den = be.fr_axpb(w, sid, alpha, beta, n), be.fr_axpb(w, ssigma, alpha, beta, n)
    tree = be.product_tree(be.fr_batch_div(num, den, n), n)
    eq = be.eq_table(tau)
    be.sync()

    def six():
        vx0, vx1 = be.fr_deinterleave(tree, n)
        pairs = [(eq, tree.at(32 * n)), (eq, vx0), (vx0, vx1), (eq, den), (tree.at(0), den), (eq, num)]
        be.sumcheck_batch([("product", f, g, n, chal) for f, g in pairs])

    def split():
        be.fr_deinterleave(tree, n)
        be.sync()

    wir_med, wir_min = timed(lambda: be.sumcheck_wiring(eq, tree, num, den, n, gamma, chal), 3, a.reps)
    six_med, six_min = timed(six, 3, a.reps)
    spl_med, spl_min = timed(split, 3, a.reps)
    # algorithmic bytes of the wiring sumcheck: round i reads 7 tables of n / 2^i and writes 7 of n / 2^(i+1) elements
    wir_bytes = sum(7 * 32 * ((n >> i) + (n >> (i + 1))) for i in range(mu))
    out.update(reps=a.reps, sumcheck_wiring_ms={"median": wir_med * 1e3, "min": wir_min * 1e3},
               six_product_batch_with_deinterleave_ms={"median": six_med * 1e3, "min": six_min * 1e3},
               deinterleave_alone_ms={"median": spl_med * 1e3, "min": spl_min * 1e3},
               wiring_over_six=wir_med / six_med, wiring_algorithmic_GBps=wir_bytes / wir_med / 1e9)
    print(json.dumps(out))
    be.close()
    return 0 if out.get("verdict", "accept") == "accept" else 1


if __name__ == "__main__":
    sys.exit(main())
