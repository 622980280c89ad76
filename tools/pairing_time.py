#!/usr/bin/env python3
"""
Wall time of the device pairing entry points (every call ends in a synchronisation of the ctx stream), after a warm-up call,
median and spread (min .. max) over --reps runs; next to the host big-int verifier of zkhip/pairing.py on the same opening.

    python tools/pairing_time.py [--reps 5] [--json out.json]

Sizes: one pairing; 4096 pairings in one call; zk_pcs_verify_batch at n = 20 for 1 and 256 openings (the one honest
opening repeated); zkhip.pairing.verify on that opening (3 runs).  Single process, no pool.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "scalable-collaborative-zksnark_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import pyoracle as po  # noqa: E402
import zkhip  # noqa: E402
from helpers import pt_mont, rand_fr  # noqa: E402
from zkhip import dist_primitive as dp  # noqa: E402
from zkhip import pairing as pr  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up (code object load, scratch growth)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def g2_rec(Q):
    return np.array(sum((po.fq_to_mont_limbs(c) for c in (Q[0][0], Q[0][1], Q[1][0], Q[1][1])), []), dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = zkhip.Ctx(0)
    rng = po.SplitMix64(2026)
    P, Q = po.g1_mul(po.G1_GEN, rng.fr()), po.g2_mul(po.G2_GEN, rng.fr())
    g1, g2 = pt_mont(P)[None], g2_rec(Q)[None]
    res = {}
    res["pairing_1"] = timed(lambda: ctx.pairing(g1, g2), a.reps)
    g1k, g2k = np.repeat(g1, 4096, 0), np.repeat(g2, 4096, 0)
    res["pairing_4096"] = timed(lambda: ctx.pairing(g1k, g2k), a.reps)
    res["pairing_4096"]["pairings_per_s"] = round(4096 / (res["pairing_4096"]["median_ms"] / 1e3), 1)
    # 4096 lanes are 64 one-wave workgroups (64 of the 256 CUs); 65536 = 1024 waves fill every SIMD once
    g1m, g2m = np.repeat(g1, 65536, 0), np.repeat(g2, 65536, 0)
    res["pairing_65536"] = timed(lambda: ctx.pairing(g1m, g2m), a.reps)
    res["pairing_65536"]["pairings_per_s"] = round(65536 / (res["pairing_65536"]["median_ms"] / 1e3), 1)
    n = 20
    s, u = rng.fr_vec(n), rng.fr_vec(n)
    mont = lambda xs: np.array([po.fr_to_mont_limbs(x) for x in xs], dtype=np.uint64).reshape(-1, 4)
    cub = dp.PolynomialCommitmentCub.new(ctx, mont(s))
    d_poly = ctx.to_device(rand_fr(1 << n, 7))
    C = np.asarray(dp.commit(ctx, cub.mature(), d_poly, 1 << n), dtype=np.uint64)
    value, proofs = dp.open_(ctx, cub.mature(), d_poly, 1 << n, mont(u))
    proofs = np.asarray(proofs, dtype=np.uint64).reshape(n, 18)
    pg2 = pr.powers_of_g2(s)
    vk = dp.pcs_vk(ctx, pg2)
    for cnt in (1, 256):
        args = (np.repeat(C[None], cnt, 0), np.repeat(np.asarray(value, dtype=np.uint64)[None], cnt, 0), np.repeat(proofs[None], cnt, 0),
                np.repeat(mont(u)[None], cnt, 0))
        assert dp.verify_batch(ctx, vk, *args).all()
        res[f"pcs_verify_n20_x{cnt}"] = timed(lambda: dp.verify_batch(ctx, vk, *args), a.reps)
    # the device share of the 256-opening batch: the same 256 x 21 pairs through zk_pairing_product_check alone (the rest of
    # zk_pcs_verify_batch is host work: input checks and the G1 combination A of every opening)
    pairs_g1, pairs_g2 = np.repeat(g1, 256 * (n + 1), 0), np.repeat(g2, 256 * (n + 1), 0)
    starts = np.arange(0, 256 * (n + 1) + 1, n + 1, dtype=np.uint64)
    res["product_check_256x21"] = timed(lambda: ctx.pairing_product_check(starts, pairs_g1, pairs_g2), a.reps)
    hs = []
    for _ in range(3):
        t0 = time.perf_counter()
        assert dp.verify(pg2, C, value, proofs, mont(u))
        hs.append((time.perf_counter() - t0) * 1e3)
    res["host_verify_n20"] = {"median_ms": round(statistics.median(hs), 1), "min_ms": round(min(hs), 1), "max_ms": round(max(hs), 1), "reps": 3}
    res["speedup_n20_single"] = round(res["host_verify_n20"]["median_ms"] / res["pcs_verify_n20_x1"]["median_ms"], 1)
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
