"""
The three-column wiring sumcheck and the one-circuit proof against what the library offered before them -- one process, warm-up 3,
median of --reps:

  sumcheck  zk_sumcheck_perm3 and zk_sumcheck_perm3_fs on N = 2^mu rows against zk_sumcheck_wiring at mu + 2 (the 3N slots laid out
            as one table of 4N elements, a tree of 8N), mu in --mu; tables are device-derived filler (the time does not depend on values);
  proof     plonk.prove / plonk.verify at mu in --proof-mu against gate_prove_ni at mu plus wiring_prove_ni at mu + 2 (and the matching
            verifiers); the last of three runs is reported (the first ones grow the arenas).

    python tools/plonk_time.py [--mu 16,20,22,24] [--proof-mu 16,20] [--reps 20] [--out FILE] [--trace-mu M]

--trace-mu M runs five zk_sumcheck_perm3 calls at 2^M and nothing else (the subject of a kernel trace).  One JSON line per result goes
to stdout and to --out (default profiles/plonk_time.txt; '-' for stdout only).

--gate wide measures the wide Plonk gate instead (default --out profiles/widegate_time.txt):

  sumcheck  zk_sumcheck_gate_wide and zk_sumcheck_gate_wide_fs against zk_sumcheck_gate on tables of the same 2^mu rows, with the ratio
            the multiplication counts predict (91 / 27 per index pair);
  proof     plonk.prove / plonk.verify of the wide kind with the four phase times, and the basic kind's prove of the same run beside them.

With --gate wide, --trace-mu M runs five zk_sumcheck_gate_wide calls at 2^M.

--lookup measures Plonk with lookups instead (default --out profiles/plonk_lookup_time.txt):

  sumcheck  zk_sumcheck_lookup_sel and zk_sumcheck_lookup_sel_fs (seven tables) against zk_sumcheck_lookup and zk_sumcheck_lookup_fs on the first
            six of the same tables, with the band the multiplication count (23 / 22) and the traffic (7 / 6) predict;
  proof     plonk.prove / plonk.verify on sample_circuit_lookup (both gate kinds, with --gate wide only the wide one) against plonk.prove
            on the same circuit without its lookup part plus the stand-alone lookup.prove of the same size (and the matching verifiers):
            neither baseline is touched by the lookup path, so the same run measures both sides.

With --lookup, --trace-mu M runs five zk_sumcheck_lookup_sel calls at 2^M.
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
    ap.add_argument("--mu", default="16,20,22,24")
    ap.add_argument("--proof-mu", default="16,20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--trace-mu", type=int, default=0)
    ap.add_argument("--gate", choices=["wide"], default=None, help="measure the wide gate against the basic one instead")
    ap.add_argument("--lookup", action="store_true", help="measure Plonk with lookups against the six-table sumcheck and the two separate proofs instead")
    ap.add_argument("--out", default=None, help="file the JSON lines are written to ('-': stdout only; default profiles/plonk_time.txt, with --gate wide profiles/widegate_time.txt)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "plonk_lookup_time.txt" if a.lookup else "widegate_time.txt" if a.gate else "plonk_time.txt")
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import nizk, plonk
    from zkhip import pairing as pr
    from zkhip import wiring as wr
    from zkhip import zerocheck as zc
    from zkhip.field import fr_from_mont, fr_mont, splitmix_fr
    from zkhip.transcript import Transcript

    be = zkhip.Ctx(0)
    out = None if a.out == "-" or a.trace_mu else open(a.out, "w")

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

    def perm3_tables(mu):
        N = 1 << mu
        return filler(N, 0), filler(2 * N, 1), [filler(N, 2 + j) for j in range(3)], [filler(N, 5 + j) for j in range(3)]

    ints = lambda s: [fr_from_mont(x) for x in s]

    def wide_gate():
        if a.trace_mu:
            mu = a.trace_mu
            tabs, chal = [filler(1 << mu, k) for k in range(11)], splitmix_fr(mu, 4)
            for _ in range(5):
                be.sumcheck_gate_wide(tabs, 1 << mu, chal)
            return
        free = be.mem_info()[0]
        for mu in [int(x) for x in a.mu.split(",") if x]:
            N = 1 << mu
            need = 32 * (11 * N + 11 * 3 * N // 4)  # eleven tables and the ping-pong scratch of 11 x (N/2 + N/4)
            if need > 0.8 * free:
                emit({"sumcheck_mu": mu, "skipped": "needs %.1f GiB of %.1f GiB free" % (need / 2**30, free / 2**30)})
                continue
            tabs, chal = [filler(N, k) for k in range(11)], splitmix_fr(mu, 4)
            wide = timed(lambda: be.sumcheck_gate_wide(tabs, N, chal), 3, a.reps)
            tr = Transcript(be, b"time")
            wide_fs = timed(lambda: be.sumcheck_gate_wide_fs(tabs, N, tr), 3, a.reps)
            basic = timed(lambda: be.sumcheck_gate(*tabs[:7], N, chal), 3, a.reps)
            basic_fs = timed(lambda: be.sumcheck_gate_fs(*tabs[:7], N, tr), 3, a.reps)
            tr.free()
            del tabs
            emit({"sumcheck_mu": mu, "gate_wide_ms": wide, "gate_wide_fs_ms": wide_fs, "gate_ms": basic, "gate_fs_ms": basic_fs, "wide_over_gate": wide / basic,
                  "wide_fs_over_gate_fs": wide_fs / basic_fs, "predicted_by_multiplications": 91 / 27})
        for mu in [int(x) for x in a.proof_mu.split(",") if x]:
            g = {"proof_mu": mu}
            for kind, sample in (("wide", plonk.sample_circuit_wide), ("basic", plonk.sample_circuit)):
                c = sample(mu, a.seed)
                pcs = dp.PolynomialCommitmentCub.new(be, c["s"]).mature()
                pk, vk = plonk.preprocess(be, pcs, c, pr.powers_of_g2(ints(c["s"])))
                wires = [be.to_device(c[k]) for k in ("a", "b", "c")]
                for rep in range(3):  # the last of three runs is reported (the first ones grow the arenas)
                    tb = {}
                    proof, g[kind + "_prove_ms"] = once(lambda: plonk.prove(be, pk, *wires, c["public_inputs"], timing=tb))
                    g.update({kind + "_prove_" + k.replace("_s", "_ms"): v * 1e3 for k, v in tb.items()})
                for rep in range(2):
                    ok, g[kind + "_verify_ms"] = once(lambda: plonk.verify(be, vk, c["public_inputs"], proof))
                g[kind + "_verdict"] = bool(ok)
                del pk, vk, pcs, wires, proof
            g["wide_prove_over_basic"] = g["wide_prove_ms"] / g["basic_prove_ms"]
            emit(g)

    def with_lookup():
        from zkhip import lookup

        band = lambda ratio: "below" if ratio < 1.05 else "above" if ratio > 1.17 else "within"  # against the predicted 1.05 .. 1.17

        if a.trace_mu:
            mu = a.trace_mu
            tabs, gamma, chal = [filler(1 << mu, k) for k in range(7)], splitmix_fr(1, 3)[0], splitmix_fr(mu, 4)
            for _ in range(5):
                be.sumcheck_lookup_sel(tabs, 1 << mu, gamma, chal)
            return
        free = be.mem_info()[0]
        for mu in [int(x) for x in a.mu.split(",") if x]:
            N = 1 << mu
            need = 32 * (7 * N + 7 * 3 * N // 4)  # seven tables and the ping-pong scratch of 7 x (N/2 + N/4)
            if need > 0.8 * free:
                emit({"sumcheck_mu": mu, "skipped": "needs %.1f GiB of %.1f GiB free" % (need / 2**30, free / 2**30)})
                continue
            tabs, gamma, chal = [filler(N, k) for k in range(7)], splitmix_fr(1, 3)[0], splitmix_fr(mu, 4)
            tr = Transcript(be, b"time")
            sel = timed(lambda: be.sumcheck_lookup_sel(tabs, N, gamma, chal), 3, a.reps)
            sel_fs = timed(lambda: be.sumcheck_lookup_sel_fs(tabs, N, gamma, tr), 3, a.reps)
            six = timed(lambda: be.sumcheck_lookup(tabs[:6], N, gamma, chal), 3, a.reps)
            six_fs = timed(lambda: be.sumcheck_lookup_fs(tabs[:6], N, gamma, tr), 3, a.reps)
            tr.free()
            del tabs
            emit({"sumcheck_mu": mu, "lookup_sel_ms": sel, "lookup_sel_fs_ms": sel_fs, "lookup_ms": six, "lookup_fs_ms": six_fs, "sel_over_lookup": sel / six,
                  "sel_fs_over_lookup_fs": sel_fs / six_fs, "predicted": [1.05, 1.17], "prediction": band(sel / six), "prediction_fs": band(sel_fs / six_fs)})
        for mu in [int(x) for x in a.proof_mu.split(",") if x]:
            for kind in (["wide"] if a.gate else [None, "wide"]):
                g = {"proof_mu": mu, "gate": kind or "basic"}
                c = plonk.sample_circuit_lookup(mu, a.seed, gate=kind)
                pcs = dp.PolynomialCommitmentCub.new(be, c["s"]).mature()
                g2 = pr.powers_of_g2(ints(c["s"]))
                wires, idx = [be.to_device(c[k]) for k in ("a", "b", "c")], be.to_device(c["idx"])
                plain = {k: v for k, v in c.items() if k not in ("lookup", "idx")}
                for name, circuit, kw in (("lookup", c, {"idx": idx}), ("plain", plain, {})):
                    pk, vk = plonk.preprocess(be, pcs, circuit, g2)
                    for rep in range(3):  # the last of three runs is reported (the first ones grow the arenas)
                        tb = {}
                        proof, g[name + "_prove_ms"] = once(lambda: plonk.prove(be, pk, *wires, c["public_inputs"], timing=tb, **kw))
                        g.update({name + "_prove_" + k.replace("_s", "_ms"): v * 1e3 for k, v in tb.items()})
                    for rep in range(2):
                        ok, g[name + "_verify_ms"] = once(lambda: plonk.verify(be, vk, c["public_inputs"], proof))
                    g[name + "_verdict"] = bool(ok)
                    del pk, vk, proof
                del wires, idx, pcs
                # the stand-alone lookup of the same size: one column against one table
                t, f, li = lookup.sample_lookup(mu, a.seed)
                s = lookup.sample_srs(mu, a.seed)
                pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
                lpk, lvk = lookup.preprocess(be, pcs, t, pr.powers_of_g2(ints(s)))
                fd, lid = be.to_device(f), be.to_device(li)
                for rep in range(3):
                    lp, g["standalone_lookup_prove_ms"] = once(lambda: lookup.prove(be, lpk, fd, lid))
                for rep in range(2):
                    ok, g["standalone_lookup_verify_ms"] = once(lambda: lookup.verify(be, lvk, lp))
                g["standalone_lookup_verdict"] = bool(ok)
                del lpk, lvk, lp, fd, lid, pcs
                g["prove_over_separate"] = g["lookup_prove_ms"] / (g["plain_prove_ms"] + g["standalone_lookup_prove_ms"])
                g["verify_over_separate"] = g["lookup_verify_ms"] / (g["plain_verify_ms"] + g["standalone_lookup_verify_ms"])
                emit(g)

    if a.lookup:
        with_lookup()
        if out:
            out.close()
        be.close()
        return 0

    if a.gate == "wide":
        wide_gate()
        if out:
            out.close()
        be.close()
        return 0

    if a.trace_mu:
        mu = a.trace_mu
        eq, tree, nums, dens = perm3_tables(mu)
        gamma, chal = splitmix_fr(1, 3)[0], splitmix_fr(mu, 4)
        for _ in range(5):
            be.sumcheck_perm3(eq, tree, nums, dens, 1 << mu, gamma, chal)
        be.close()
        return 0

    free = be.mem_info()[0]
    for mu in [int(x) for x in a.mu.split(",") if x]:
        N = 1 << mu
        # the two table sets are never resident together: perm3 holds eq, a 2N tree, six tables and ping-pong scratch of 11 x (N/2 + N/4);
        # the baseline eq, num, den of 4N, a tree of 8N and scratch of 7 x (2N + N)
        need = 32 * max(N * (1 + 2 + 6) + 11 * 3 * N // 4, 4 * N * 3 + 8 * N + 21 * N)
        if need > 0.8 * free:
            emit({"sumcheck_mu": mu, "skipped": "needs %.1f GiB of %.1f GiB free" % (need / 2**30, free / 2**30)})
            continue
        gamma, chal = splitmix_fr(1, 3)[0], splitmix_fr(mu + 2, 4)
        eq, tree, nums, dens = perm3_tables(mu)
        perm3 = timed(lambda: be.sumcheck_perm3(eq, tree, nums, dens, N, gamma, chal), 3, a.reps)
        tr = Transcript(be, b"time")
        perm3_fs = timed(lambda: be.sumcheck_perm3_fs(eq, tree, nums, dens, N, gamma, tr), 3, a.reps)
        tr.free()
        del eq, tree, nums, dens
        eq4, tree4, num4, den4 = filler(4 * N, 0), filler(8 * N, 1), filler(4 * N, 2), filler(4 * N, 3)
        wiring = timed(lambda: be.sumcheck_wiring(eq4, tree4, num4, den4, 4 * N, gamma, chal), 3, a.reps)
        del eq4, tree4, num4, den4
        emit({"sumcheck_mu": mu, "perm3_ms": perm3, "perm3_fs_ms": perm3_fs, "wiring_4N_ms": wiring, "perm3_over_wiring_4N": perm3 / wiring,
              "predicted_by_multiplications": 59 / 92})

    for mu in [int(x) for x in a.proof_mu.split(",") if x]:
        N = 1 << mu
        c = plonk.sample_circuit(mu, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, c["s"]).mature()
        pk, vk = plonk.preprocess(be, pcs, c, pr.powers_of_g2(ints(c["s"])))
        wires = [be.to_device(c[k]) for k in ("a", "b", "c")]
        g = {"proof_mu": mu}
        for rep in range(3):
            tb = {}
            proof, g["prove_ms"] = once(lambda: plonk.prove(be, pk, *wires, c["public_inputs"], timing=tb))
            g.update({"prove_" + k.replace("_s", "_ms"): v * 1e3 for k, v in tb.items()})
        for rep in range(2):
            ok, g["verify_ms"] = once(lambda: plonk.verify(be, vk, c["public_inputs"], proof))
        del pk, vk, pcs, wires, proof
        # the baseline: two unrelated proofs, the gate identity at mu and the single-column wiring at mu + 2
        tabs, _tau, _chal, s = zc.satisfied_circuit(be, mu, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
        gvk = dp.pcs_vk(be, pr.powers_of_g2(ints(s)))
        for rep in range(3):
            gp, g["gate_prove_ni_ms"] = once(lambda: nizk.gate_prove_ni(be, pcs, tabs))
        for rep in range(2):
            ok_g, g["gate_verify_ni_ms"] = once(lambda: nizk.gate_verify_ni(be, gvk, gp))
        del tabs, pcs, gvk, gp
        w, sid, ssigma, *_rest, s = wr.permuted_circuit(be, mu + 2, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, s).mature()
        vk_mu, vk_mu1 = wr.verifying_keys(be, pr.powers_of_g2(ints(s)))
        for rep in range(3):
            tb = {}
            wp, g["wiring_prove_ni_4N_ms"] = once(lambda: nizk.wiring_prove_ni(be, pcs, w, sid, ssigma, 4 * N, timing=tb))
            g["wiring_4N_commit_ms"] = tb["commit_s"] * 1e3
        for rep in range(2):
            ok_w, g["wiring_verify_ni_4N_ms"] = once(lambda: nizk.wiring_verify_ni(be, vk_mu, vk_mu1, wp))
        del w, sid, ssigma, pcs, vk_mu, vk_mu1, wp
        g["verdicts"] = [bool(ok), bool(ok_g), bool(ok_w)]
        g["prove_over_baseline"] = g["prove_ms"] / (g["gate_prove_ni_ms"] + g["wiring_prove_ni_4N_ms"])
        g["verify_over_baseline"] = g["verify_ms"] / (g["gate_verify_ni_ms"] + g["wiring_verify_ni_4N_ms"])
        emit(g)
    if out:
        out.close()
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
