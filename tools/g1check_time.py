"""
What the validation of a proof's G1 points costs (profiles/g1check_time.txt, JSON lines).  One process, warm-up 3, median of --reps
blocking calls:

  * zk_g1_decompress_check (Ctx.g1_decompress_check) at 68 points -- a 2^20 proof with a lookup -- and at 4 096, beside the Python
    host's rule (serialize.g1_decompress_check_host) and the compiled host's serial big-integer rule (zkhost g1_decompress_check_host,
    through host/bin/plonk_check --g1check-time: a process of its own that touches no device, its own warm-up 3 and median of --reps)
    on the same points.  The points are multiples of the generator: the kernels have constant trip counts, so members cost what any
    other point costs.  The three give the same points bit for bit ("same_points").
  * plonk.verify_bytes beside plonk.verify on the same proof (the lookup sample, basic gate) at 2^16 and 2^20 rows.  verify is the
    parent's function, untouched: measured in the same run it is the baseline.  The difference is parsing (host), one
    zk_g1_decompress_check call and nothing else.
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
    ap.add_argument("--points", default="68,4096")
    ap.add_argument("--proof-mu", default="16,20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1check_time.txt"), help="'-': stdout only")
    a = ap.parse_args()
    import numpy as np

    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk, proof_io
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
            P = pr.g1_add(P, pr.G1_GEN)
            encs.append(ser.g1_serialize_compressed(P))
        data = b"".join(encs)
        dev = timed(lambda: be.g1_decompress_check(data), 3, a.reps)
        host = timed(lambda: ser.g1_decompress_check_host(data), 3, a.reps)
        r = subprocess.run([os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host", "bin", "plonk_check"), "--g1check-time", str(k), "--reps", str(a.reps)],
                           capture_output=True, text=True, check=True)
        m = re.fullmatch(r"g1check host points \d+ ms ([0-9.]+) all_ok 1 points_sha256 ([0-9a-f]{64})\n", r.stdout)
        cpp = float(m.group(1))
        pts, st = be.g1_decompress_check(data)
        hp, hs = ser.g1_decompress_check_host(data)
        same = bool((pts == hp).all() and (st == hs).all()) and hashlib.sha256(np.ascontiguousarray(pts, dtype="<u8").tobytes()).hexdigest() == m.group(2)
        emit({"points": k, "device_ms": dev, "python_host_ms": host, "compiled_host_ms": cpp, "python_over_device": host / dev, "compiled_over_device": cpp / dev,
              "all_ok": bool(not st.any()), "same_points": same})
    for mu in [int(x) for x in a.proof_mu.split(",") if x]:
        c = plonk.sample_circuit_lookup(mu, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, c["s"]).mature()
        pk, vk = plonk.preprocess(be, pcs, c, pr.powers_of_g2([fr_from_mont(x) for x in c["s"]]))
        wires, idx = [be.to_device(c[k]) for k in ("a", "b", "c")], be.to_device(c["idx"])
        pi = c["public_inputs"]
        proof = plonk.prove(be, pk, *wires, pi, idx=idx)
        data = plonk.proof_to_bytes(proof)
        hdr, comp, _ = plonk.parse_proof(data)
        ok = plonk.verify(be, vk, pi, proof), plonk.verify_bytes(be, vk, pi, data)
        g = {"proof_mu": mu, "bytes": len(data), "points": len(comp), "verdicts": [bool(x) for x in ok]}
        g["verify_ms"] = timed(lambda: plonk.verify(be, vk, pi, proof), 3, a.reps)
        g["verify_bytes_ms"] = timed(lambda: plonk.verify_bytes(be, vk, pi, data), 3, a.reps)
        g["parse_ms"] = timed(lambda: plonk.parse_proof(data), 3, a.reps)
        g["g1_decompress_check_ms"] = timed(lambda: be.g1_decompress_check(comp), 3, a.reps)
        g["check_points_ms"] = timed(lambda: plonk.check_points(be, proof), 3, a.reps)
        g["validation_share_of_verify"] = g["g1_decompress_check_ms"] / g["verify_ms"]
        emit(g)
        del pk, vk, wires, idx, pcs
    be.close()


if __name__ == "__main__":
    main()
