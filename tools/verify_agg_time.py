"""
What aggregated verification costs beside plonk.verify (profiles/verify_agg_time.txt, JSON lines).  One process; EVERY figure is the
median of --reps (20) blocking calls after a warm-up of 3, each figure from runs of its own:

  * plonk.verify and plonk.verify_agg on the same proof at 2^16 and 2^20 rows, both gate kinds, with and without a lookup.  verify is
    the parent's function, untouched: measured in the same run it is the baseline.
  * plonk.verify_many at K = 1, 16, 256 against K x verify (the lookup sample, basic gate).  The K-proof runs reuse ONE proof K times:
    the aggregate does not care (every opening gets its own weight, and nothing is cached between openings), and K distinct 2^20 proofs
    would only add proving time to the run.
  * every aggregated figure is split into the host part (plonk.agg_openings: replay, field checks, claims: "host_ms"), the weights
    ("agg_weights_ms": zk_pcs_agg_weights alone), the segmented linear combination ("lincomb_ms": zk_g1_lincomb_seg alone on the term
    list the library builds) and the pairing ("pairing_ms": zk_pairing_product_check alone on that call's sums and the key's G2
    points, one group of n_g2 pairs -- what pairing_run does inside the library).  "agg_call_ms" is the whole zk_pcs_verify_agg call;
    "rest_ms" = the call minus those three medians: the term list and the copies inside the library, and the noise of four medians.

The expectation from operation counts was verify_agg = 0.35 - 0.45 x verify for one 2^20 lookup proof and a cost nearly flat in K; the
last line of the file says CONFIRMED or REFUTED for the band and gives the figures in K, device part and whole call.
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


def term_arrays(n_g2, ops, rho):
    """the term list zk_pcs_verify_agg builds inside the library (segment 0 = L, segment j = M_j), as the arrays of zk_g1_lincomb_seg:
    only to time that call alone on the same terms"""
    import numpy as np

    from zkhip import pairing as pr
    from zkhip.field import R_MOD, fq_mont, fr_from_mont, int_to_limbs

    segs = [[] for _ in range(n_g2)]
    vsum = 0
    for (C, e, y, opening, point, skip), (lo, hi) in zip(ops, rho):
        r = int(lo) | int(hi) << 64
        segs[0] += [(c, r * fr_from_mont(x) % R_MOD) for c, x in zip(C, e)]
        segs[0] += [(p, r * fr_from_mont(u) % R_MOD) for p, u in zip(opening, point)]
        for i, p in enumerate(opening):
            segs[1 + skip + i].append((p, r))
        vsum = (vsum + r * fr_from_mont(y)) % R_MOD
    g1 = np.concatenate([fq_mont(pr.G1_GEN[0]), fq_mont(pr.G1_GEN[1]), fq_mont(1)])
    segs[0].append((g1, (-vsum) % R_MOD))
    starts = np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)
    return starts, np.stack([p for s in segs for p, _ in s]), np.stack([int_to_limbs(k, 4) for s in segs for _, k in s])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proof-mu", default="16,20")
    ap.add_argument("--many", default="1,16,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_agg_time.txt"), help="'-': stdout only")
    a = ap.parse_args()
    import numpy as np

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip.field import Q_MOD, fq_from_mont, fq_mont, fr_from_mont

    be = zkhip.Ctx(0)
    out = None if a.out == "-" else open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def split(vk, g2, items):
        """the parts of one verify_many call on `items`, each the median of its own runs"""
        alive, ops = plonk.agg_openings(vk, items)
        assert len(alive) == len(items)
        arrays = dp.agg_arrays(ops)
        rho = be.pcs_agg_weights(*arrays)
        n_g2 = vk["pcs"][1].n_g2
        starts, pts, ks = term_arrays(n_g2, ops, rho)
        sums = be.g1_lincomb_seg(starts, pts, ks)  # normalised: (x, y, 1) or (1, 1, 0)
        g1 = np.zeros((n_g2, 12), dtype=np.uint64)  # (L, -M_1, ..), infinity as zeros: a factor 1
        for j in range(n_g2):
            if sums[j, 12:].any():
                g1[j, :6], g1[j, 6:] = sums[j, :6], sums[j, 6:12] if j == 0 else fq_mont(-fq_from_mont(sums[j, 6:12]) % Q_MOD)
        assert be.pairing_product_check([0, n_g2], g1, g2).all()
        m = {"host_ms": timed(lambda: plonk.agg_openings(vk, items), 3, a.reps), "agg_weights_ms": timed(lambda: be.pcs_agg_weights(*arrays), 3, a.reps),
             "lincomb_ms": timed(lambda: be.g1_lincomb_seg(starts, pts, ks), 3, a.reps),
             "pairing_ms": timed(lambda: be.pairing_product_check([0, n_g2], g1, g2), 3, a.reps),
             "agg_call_ms": timed(lambda: be.pcs_verify_agg(vk["pcs"][1], *arrays), 3, a.reps), "terms": int(starts[-1]), "openings": len(ops)}
        m["rest_ms"] = m["agg_call_ms"] - m["lincomb_ms"] - m["agg_weights_ms"] - m["pairing_ms"]
        return m

    ratio20, flat = None, None
    for mu in [int(x) for x in a.proof_mu.split(",") if x]:
        for gate in (None, "wide"):
            for lookup in (False, True):
                if lookup:
                    c = plonk.sample_circuit_lookup(mu, a.seed, gate=gate)
                else:
                    c = (plonk.sample_circuit_wide if gate else plonk.sample_circuit)(mu, a.seed)
                pcs = dp.PolynomialCommitmentCub.new(be, c["s"]).mature()
                pg2 = pr.powers_of_g2([fr_from_mont(x) for x in c["s"]])
                g2 = np.stack([np.concatenate([fq_mont(P[0][0]), fq_mont(P[0][1]), fq_mont(P[1][0]), fq_mont(P[1][1])]) for P in pg2])
                pk, vk = plonk.preprocess(be, pcs, c, pg2)
                wires = [be.to_device(c[k]) for k in ("a", "b", "c")]
                pi = c["public_inputs"]
                proof = plonk.prove(be, pk, *wires, pi, idx=be.to_device(c["idx"]) if lookup else None)
                g = {"proof_mu": mu, "gate": gate or "basic", "lookup": lookup,
                     "verdicts": [bool(plonk.verify(be, vk, pi, proof)), bool(plonk.verify_agg(be, vk, pi, proof))]}
                g["verify_ms"] = timed(lambda: plonk.verify(be, vk, pi, proof), 3, a.reps)
                g["verify_agg_ms"] = timed(lambda: plonk.verify_agg(be, vk, pi, proof), 3, a.reps)
                g["agg_over_verify"] = g["verify_agg_ms"] / g["verify_ms"]
                g.update(split(vk, g2, [(pi, proof)]))
                emit(g)
                if mu == 20 and lookup and gate is None:
                    ratio20 = g["agg_over_verify"]
                if lookup and gate is None and mu == max(int(x) for x in a.proof_mu.split(",") if x):
                    many = {}
                    for K in [int(x) for x in a.many.split(",") if x]:
                        items = [(pi, proof)] * K  # ONE proof K times: see the module text
                        assert plonk.verify_many(be, vk, items) == [True] * K
                        m = {"proof_mu": mu, "many": K, "verify_many_ms": timed(lambda: plonk.verify_many(be, vk, items), 3, a.reps),
                             "k_times_verify_ms": K * g["verify_ms"]}
                        m["many_over_k_verify"] = m["verify_many_ms"] / m["k_times_verify_ms"]
                        m.update(split(vk, g2, items))
                        emit(m)
                        many[K] = m
                    ks = sorted(many)
                    if len(ks) > 1:
                        flat = {"device_part_ms": {K: many[K]["agg_call_ms"] for K in ks}, "whole_ms": {K: many[K]["verify_many_ms"] for K in ks}}
                del pk, vk, wires, pcs
    verdict = {"expected_agg_over_verify_2p20_lookup": [0.35, 0.45], "measured": ratio20,
               "band": None if ratio20 is None else ("CONFIRMED" if 0.35 <= ratio20 <= 0.45 else "REFUTED"), "cost_in_K": flat}
    emit(verdict)
    be.close()


if __name__ == "__main__":
    main()
