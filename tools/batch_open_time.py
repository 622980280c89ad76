"""
Batch opening from Python: prove + verify one instance (zkhip.batch_open.random_instance: J random tables, K claims at random,
repeated and boolean points), and the measurements of DESIGN section 5 -- same process, warm-up 3, median of --reps:

  kernel    zk_sumcheck_multi against what the library offered before it: one zk_sumcheck_batch of `count` product items with the
            same challenges; the host sum of the count triples that form also needs (3 n count field additions, microseconds) is NOT timed, n in --kernel-n, count in 3, 6, 9;
  HBM       zk_fr_lincomb and zk_eq_table_acc at 2^--hbm-n: GB/s over algorithmic bytes (32 (count + 1) len; 4 x 32 len for the accumulate, see below);
  prover    gate_zerocheck_prove_batched / wiring_prove_batched against gate_zerocheck_prove / wiring_prove on the same tables at
            2^--proof-n: opening phase and total; verifier: the same pairs, verify wall time.

    python tools/batch_open_time.py [--n 10] [--seed 7] [--digest] [--kernel-n 20,22,24] [--hbm-n 24] [--proof-n 20] [--reps 20] [--out FILE]

The one JSON line goes to stdout and to --out (default profiles/batch_open_time.txt; '-' for stdout only).
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
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--tables", type=int, default=4)
    ap.add_argument("--claims", type=int, default=9)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--digest", action="store_true")
    ap.add_argument("--kernel-n", default="")
    ap.add_argument("--hbm-n", type=int, default=0)
    ap.add_argument("--proof-n", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_open_time.txt"), help="file the JSON line is written to ('-': stdout only)")
    a = ap.parse_args()
    import zkhip
    from zkhip import batch_open as bo
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import wiring as wr
    from zkhip import zerocheck as zc
    from zkhip.field import fr_from_mont, splitmix_fr

    be = zkhip.Ctx(0)
    ints = lambda s: [fr_from_mont(x) for x in s]
    n, N = a.n, 1 << a.n
    tables, pts, alpha, rho, s = bo.random_instance(be, n, a.tables, a.claims, a.seed)
    pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
    import numpy as np

    comms = np.stack([dp.commit(be, pcs, t, N) for t in tables])
    claims = bo.evaluate_claims(be, tables, N, pts)
    proof = bo.batch_open_prove(be, pcs, tables, N, claims, alpha, rho)
    ok = bo.batch_open_verify(be, dp.pcs_vk(be, pr.powers_of_g2(ints(s))), comms, claims, proof, alpha, rho)
    out = {"n": n, "tables": a.tables, "claims": a.claims, "seed": a.seed, "verdict": "accept" if ok else "reject"}
    if a.digest:
        out["proof_sha256"] = bo.proof_digest(proof)
    del tables, pcs, proof

    kernel = []
    for kn in [int(x) for x in a.kernel_n.split(",") if x]:
        m = 1 << kn
        ch = splitmix_fr(kn, 11)
        for count in (3, 6, 9):
            es = [be.to_device(splitmix_fr(m, 100 + j)) for j in range(count)]
            fs = [be.to_device(splitmix_fr(m, 200 + j)) for j in range(count)]
            multi = timed(lambda: be.sumcheck_multi(es, fs, m, ch), 3, a.reps)
            batch = timed(lambda: be.sumcheck_batch([("product", e, f, m, ch) for e, f in zip(es, fs)]), 3, a.reps)
            # algorithmic bytes: round i reads 2 count tables of m / 2^i and writes 2 count of m / 2^(i+1) elements
            nbytes = sum(2 * count * 32 * ((m >> i) + (m >> (i + 1))) for i in range(kn))
            kernel.append({"n": kn, "count": count, "sumcheck_multi_ms": multi, "product_batch_ms": batch, "multi_over_batch": multi / batch,
                           "multi_algorithmic_GBps": nbytes / multi / 1e6})
            del es, fs
    if kernel:
        out["kernel"] = kernel

    if a.hbm_n:
        m = 1 << a.hbm_n
        hbm = []
        for count in (1, 3, 6, 16):
            tabs = [be.to_device(splitmix_fr(m, 300 + j)) for j in range(count)]
            co, dst = splitmix_fr(count, 12), be.alloc(32 * m)

            def lin():
                be.fr_lincomb(tabs, co, m, out=dst)
                be.sync()

            ms = timed(lin, 3, a.reps)
            hbm.append({"fr_lincomb_count": count, "ms": ms, "GBps": 32 * (count + 1) * m / ms / 1e6})
            del tabs, dst
        acc, z, w = be.to_device(splitmix_fr(m, 13)), splitmix_fr(a.hbm_n, 14), splitmix_fr(1, 15)[0]

        def eqa():
            be.eq_table_acc(z, w, acc)
            be.sync()

        ms = timed(eqa, 3, a.reps)
        # last level: reads the half-size level (0.5) and the accumulator (1), writes the accumulator (1); the doubling levels below
        # read and write sum_k 2 * 2^-k / 2 of a table each way (1.5 in all): 4 x 32 x 2^n bytes
        hbm.append({"eq_table_acc_n": a.hbm_n, "ms": ms, "GBps": (4 * 32 * m) / ms / 1e6})
        out["hbm"] = hbm
        del acc

    if a.proof_n:
        pn, pm = a.proof_n, 1 << a.proof_n
        b_alpha, rho_n, rho_n1 = splitmix_fr(1, 21)[0], splitmix_fr(pn, 22), splitmix_fr(pn + 1, 23)
        tabs, tau, chal, s = zc.satisfied_circuit(be, pn, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
        vk = dp.pcs_vk(be, pr.powers_of_g2(ints(s)))
        cm = {k: dp.commit(be, pcs, tabs[k], pm) for k in zc.OPENED}
        g = {}
        for rep in range(3):  # the last of three runs is reported (the first ones grow the arenas)
            tb = {}
            p_plain, g["prove_ms"] = once(lambda: zc.gate_zerocheck_prove(be, pcs, tabs, tau, chal, commitments=cm))
            p_bat, g["prove_batched_ms"] = once(lambda: zc.gate_zerocheck_prove_batched(be, pcs, tabs, tau, chal, b_alpha, rho_n, commitments=cm, timing=tb))
            g["batched_opening_phase_ms"] = tb["opening_s"] * 1e3
            _, g["open_many_6_ms"] = once(lambda: dp.open_many(be, pcs, [tabs[k] for k in zc.OPENED], [pm] * 6, [chal] * 6))
        for rep in range(2):
            ok1, g["verify_ms"] = once(lambda: zc.gate_zerocheck_verify(be, vk, p_plain, tau, chal))
            ok2, g["verify_batched_ms"] = once(lambda: zc.gate_zerocheck_verify_batched(be, vk, p_bat, tau, chal, b_alpha, rho_n))
        g["verdicts"] = [bool(ok1), bool(ok2)]
        out["gate_2^%d" % pn] = g
        del tabs, pcs, p_plain, p_bat, cm
        w, sid, ssigma, al, beta, gamma, tau, chal, s = wr.permuted_circuit(be, pn, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
        vk_mu, vk_mu1 = wr.verifying_keys(be, pr.powers_of_g2(ints(s)))
        cm = {"w": dp.commit(be, pcs, w, pm), "sid": dp.commit(be, pcs, sid, pm), "ssigma": dp.commit(be, pcs, ssigma, pm)}
        g = {}
        for rep in range(3):
            tb = {}
            p_plain, g["prove_ms"] = once(lambda: wr.wiring_prove(be, pcs, w, sid, ssigma, pm, al, beta, gamma, tau, chal, commitments=cm))
            p_bat, g["prove_batched_ms"] = once(lambda: wr.wiring_prove_batched(be, pcs, w, sid, ssigma, pm, al, beta, gamma, tau, chal, b_alpha, rho_n, rho_n1, commitments=cm, timing=tb))
            g["batched_opening_phase_ms"] = tb["opening_s"] * 1e3
            g["batched_tables_and_sumcheck_ms"], g["batched_tree_commit_ms"] = tb["sumcheck_s"] * 1e3, tb["commit_s"] * 1e3
        for rep in range(2):
            ok1, g["verify_ms"] = once(lambda: wr.wiring_verify(be, vk_mu, vk_mu1, p_plain, al, beta, gamma, tau, chal))
            ok2, g["verify_batched_ms"] = once(lambda: wr.wiring_verify_batched(be, vk_mu, vk_mu1, p_bat, al, beta, gamma, tau, chal, b_alpha, rho_n, rho_n1))
        g["verdicts"] = [bool(ok1), bool(ok2)]
        out["wiring_2^%d" % pn] = g
    line = json.dumps(out)
    print(line)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    be.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
