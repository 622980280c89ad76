#!/usr/bin/env python3
"""
Time of loading a parameter set from a file against building it from the trapdoor:

    python tools/srs_time.py [--n 21] [--out profiles/srs_io_time.txt]

One process, one run: warm-up 3, median of 20 blocking calls, ms.  srs_from_bytes is split into its steps -- the host-to-device copy
of the G1 block, zk_g1_decompress_check_device, zk_srs_wrap_device and the n zk_srs_halve calls, and zk_srs_check, of which the 2n
MSMs are also timed alone (one zk_msm_g1_batch on the same weights; the pairing step is the difference) -- beside
PolynomialCommitmentCub.new on the same trapdoor.  The file is made in this process from a seeded trapdoor (test material).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WARMUP, REPS = 3, 20


def med(fn):
    ts = []
    for i in range(WARMUP + REPS):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts[WARMUP:])


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srs_io_time.txt"))
    a = ap.parse_args()
    import numpy as np

    import zkhip
    from plonk_srs import trapdoor
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import srs_io
    from zkhip.field import fr_mont

    be = zkhip.Ctx(0)
    n = a.n
    s = trapdoor(n, 1)
    s_m = np.stack([fr_mont(x) for x in s])
    pcs = dp.PolynomialCommitmentCub.new(be, s_m).mature()
    t = time.perf_counter()
    data = srs_io.srs_to_bytes(be, pcs, pr.powers_of_g2(s))
    t_write = time.perf_counter() - t
    del pcs
    _, pts, keys = srs_io.parse_srs(data)
    seed = srs_io.file_seed(data)
    N = 1 << n
    rows = []
    rows.append(("PolynomialCommitmentCub.new (zk_srs_powers, the trapdoor in host memory)", med(lambda: dp.PolynomialCommitmentCub.new(be, s_m))))
    rows.append(("srs_from_bytes, all steps", med(lambda: srs_io.srs_from_bytes(be, data))))
    rows.append(("srs_from_bytes(check=False)", med(lambda: srs_io.srs_from_bytes(be, data, check=False))))
    rows.append(("  parse_srs + SHA-256 of the file (host)", med(lambda: (srs_io.parse_srs(data), srs_io.file_seed(data)))))
    d_in = be.to_device(pts)
    rows.append(("  copy: host-to-device of the G1 block", med(lambda: d_in.upload(pts))))
    d_rec = be.alloc(96 * N)
    rows.append(("  decompress-check: zk_g1_decompress_check_device", med(lambda: be.g1_decompress_check_device(d_in, N, out=d_rec, refuse_infinity=True))))
    rows.append(("  zk_g2_decompress_check of the keys", med(lambda: be.g2_decompress_check(keys))))
    k_pts = be.g2_decompress_check(keys)[0]

    def halvings():
        lv = [be.srs_wrap_device(d_rec, N)]
        for _ in range(n):
            lv.append(be.srs_halve(lv[-1]))
        return lv[::-1]

    rows.append(("  halvings: zk_srs_wrap_device + n zk_srs_halve", med(halvings)))
    lv = halvings()
    rows.append(("  zk_srs_check (weights, MSMs, pairing)", med(lambda: be.srs_check(lv, k_pts, seed))))
    rho = be.fr_hash_expand(seed, srs_io.RHO_DOMAIN, N // 2)
    srs_l = [lv[k + 1] if t == 0 else lv[k] for k in range(n) for t in range(2)]
    lens = [1 << k for k in range(n) for t in range(2)]
    offs = [(1 << k) if t == 0 else 0 for k in range(n) for t in range(2)]
    rows.append(("    zk_fr_hash_expand, 2^(n-1) weights", med(lambda: (be.fr_hash_expand(seed, srs_io.RHO_DOMAIN, N // 2, out=rho), be.sync()))))
    rows.append(("    MSMs: one zk_msm_g1_batch of 2n sums", med(lambda: be.msm_g1_batch(srs_l, [rho] * (2 * n), lens, offs))))
    rows.append(("    pairing: zk_srs_check minus weights and MSMs", rows[-3][1] - rows[-2][1] - rows[-1][1]))
    lines = [f"# tools/srs_time.py --n {n}: one run, one process, warm-up {WARMUP}, median of {REPS} blocking calls, ms",
             f"# file: {len(data)} bytes (2^{n} compressed G1 points, {n + 1} G2 keys); written by srs_to_bytes in {t_write:.1f} s (Python integers)"]
    lines += [f"{name:<78} {ms:10.2f}" for name, ms in rows]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
