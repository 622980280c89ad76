#!/usr/bin/env python3
"""
What the validation of a verifying key's G2 points costs (profiles/g2check_time.txt, JSON lines).  One process, warm-up 3, median of --reps
(20) blocking calls, milliseconds.

  * zk_g2_decompress_check (Ctx.g2_decompress_check) at 22 points -- the keys of a 2^20 vk -- and at 4 096, beside the Python host's rule
    (serialize.g2_decompress_check_host; at most --python-points of them are timed and the figure is scaled, it is linear in the count)
    and the compiled host's serial big-integer rule (zkhost g2_decompress_check_host, through host/bin/plonk_check --g2check-time: a
    process of its own that touches no device, its own warm-up 3 and median of --reps).
  * vk_from_bytes (both device calls, the parse and the two zk_pcs_vk_create) beside ONE plonk.verify of the same circuit at --vk-mu.

The expectation these figures are read against (operation counts): one 64-bit ladder over Fq2 against the G1 check's two over Fq, a flat
few ms, 1.5-2 x the 1.6-1.7 ms of profiles/g1check_time.txt; little or no advantage over a compiled host at 22 points, two orders of
magnitude at thousands.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="22,4096")
    ap.add_argument("--python-points", type=int, default=22)
    ap.add_argument("--vk-mu", default="12,20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g2check_time.txt"), help="'-': stdout only")
    a = ap.parse_args()
    import numpy as np

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk
    from zkhip import serialize as ser
    from zkhip.field import fr_from_mont

    be = zkhip.Ctx(0)
    out = None if a.out == "-" else open(a.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for k in [int(x) for x in a.points.split(",") if x]:
        P, encs = None, []
        for _ in range(k):  # G, 2G, ...
            P = pr.g2_add(P, pr.G2_GEN)
            encs.append(ser.g2_serialize_compressed(P))
        data = b"".join(encs)
        dev = timed(lambda: be.g2_decompress_check(data), 3, a.reps)
        kp = min(k, a.python_points)
        host = timed(lambda: ser.g2_decompress_check_host(data[:96 * kp]), 1, 3) * k / kp
        r = subprocess.run([os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host", "bin", "plonk_check"), "--g2check-time", str(k), "--reps", str(a.reps)],
                           capture_output=True, text=True, check=True)
        m = re.fullmatch(r"g2check host points \d+ ms ([0-9.]+) all_ok 1 points_sha256 ([0-9a-f]{64})\n", r.stdout)
        cpp = float(m.group(1))
        pts, st = be.g2_decompress_check(data)
        hp, hs = ser.g2_decompress_check_host(data[:96 * kp])
        same = bool((pts[:kp] == hp).all() and (st[:kp] == hs).all()) and hashlib.sha256(np.ascontiguousarray(pts, dtype="<u8").tobytes()).hexdigest() == m.group(2)
        emit({"points": k, "device_ms": dev, "python_host_ms": host, "python_points_timed": kp, "compiled_host_ms": cpp, "python_over_device": host / dev,
              "compiled_over_device": cpp / dev, "all_ok": bool(not st.any()), "same_points": same})
    for mu in [int(x) for x in a.vk_mu.split(",") if x]:
        c = plonk.sample_circuit(mu, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, c["s"]).mature()
        pk, vk = plonk.preprocess(be, pcs, c, pr.powers_of_g2([fr_from_mont(x) for x in c["s"]]))
        wires = [be.to_device(c[k]) for k in ("a", "b", "c")]
        pi = c["public_inputs"]
        proof = plonk.prove(be, pk, *wires, pi)
        data = plonk.vk_to_bytes(vk)
        vk2 = plonk.vk_from_bytes(be, data)
        g = {"vk_mu": mu, "vk_bytes": len(data), "g2_keys": mu + 2, "verdicts": [bool(plonk.verify(be, vk, pi, proof)), bool(plonk.verify(be, vk2, pi, proof))]}
        g["verify_ms"] = timed(lambda: plonk.verify(be, vk2, pi, proof), 3, a.reps)
        g["vk_from_bytes_ms"] = timed(lambda: plonk.vk_from_bytes(be, data), 3, a.reps)
        g["check_vk_ms"] = timed(lambda: plonk.check_vk(be, vk), 3, a.reps)
        g["vk_share_of_verify"] = g["vk_from_bytes_ms"] / g["verify_ms"]
        emit(g)
        del pk, vk, vk2, wires, pcs
    be.close()


if __name__ == "__main__":
    main()
