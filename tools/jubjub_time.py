#!/usr/bin/env python3
"""
Times of the Jubjub kernels -> profiles/jubjub_time.txt.  One process, warm-up 3, median of 20 blocking calls (the call, then a
synchronisation of the ctx stream; Jubjub.check and schnorr_verify read their statuses back, which is such a synchronisation).
  * zk_schnorr_verify at 2^10, 2^12, 2^16 and 2^18 valid signatures (four signed messages cycled: the kernel's work does not depend on the data);
  * zk_jubjub_mul with the fixed base and zk_jubjub_check at 2^10 and 2^16;
  * beside them the compiled host's serial rule on one core (host/bin/poseidon_check --time-schnorr K, a process of its own: jubjub_verify_host,
    extended coordinates on zkhost's Fr) at 2^10 signatures -- it is linear in K; the python-integer rule (jubjub.verify_host, 8 signatures,
    another process) is printed as a second line for scale.

EXPECTATION, written before the first run, by multiplication count only.  One addition in extended coordinates is 9 Fr multiplications,
a ladder step is two of them.  A lane of zk_schnorr_verify is a chain of 4 x 828 = 3.3 k (the hashes) + 255 x 18 = 4.6 k (the subgroup test,
a full pass of the joint ladder) + 4.6 k (the joint ladder) = about 12.5 k dependent multiplications.  profiles/poseidon_time.txt has one
lane's 828 at 0.645 ms, 0.78 us per dependent multiplication at one wave per SIMD, so
    up to 2^16 signatures (256 workgroups of 256 lanes: one per CU, one wave per SIMD -- the kernel holds 256 VGPRs, so that is also all a SIMD
    can hold) cost ONE lane's latency: about 9.7 ms, at 2^10 and 2^12 and 2^16 alike.  The throughput bound 2^16 x 12.5 k / 130 G mul/s = 6.3 ms
    lies below it and is not reached.  2^18 signatures are four such rounds: about 39 ms (throughput bound 25 ms).
    zk_jubjub_mul: 256 x 18 + ~380 (the inversion) = 5.0 k multiplications: about 3.9 ms up to 2^16.  zk_jubjub_check: 255 x 18 = 4.6 k: 3.6 ms.
The serial rule does the same ~12.5 k multiplications per signature plus three inversions (~380 each) on one core; at the ~50 ns per
multiplication of zkhost's Fr that is about 0.7 ms per signature, so the device at 2^16 should be about 0.7 ms x 2^16 / 9.7 ms ~ 4 700x one core.
A figure within 30 % of its expectation is "confirmed", anything else "refuted".
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scalable-collaborative-zksnark_amd")
sys.path.insert(0, PKG)

import numpy as np  # noqa: E402

WARM, REPS = 3, 20
EXPECT_MS = {("verify", 10): 9.7, ("verify", 12): 9.7, ("verify", 16): 9.7, ("verify", 18): 39.0,
             ("mul", 10): 3.9, ("mul", 16): 3.9, ("check", 10): 3.6, ("check", 16): 3.6, ("host", 10): 0.7}
HOST_SIGS = 8


def median_ms(be, call) -> float:
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        be.sync()
        if i >= WARM:
            ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def verdict(key, ms: float) -> str:
    want = EXPECT_MS[key]
    return f"expected ~{want} ms: {'confirmed' if abs(ms - want) <= 0.3 * want else 'refuted'} ({ms / want:.2f}x)"


def host_rule() -> int:
    """the process of its own: HOST_SIGS verifications in python integers, one line"""
    from zkhip import jubjub as jj

    cases = [(jj.keygen_host(sk), m, jj.sign_host(sk, m)) for sk, m in ((3 + k, 1000 + k) for k in range(HOST_SIGS))]
    t0 = time.perf_counter()
    ok = [jj.verify_host(*c) for c in cases]
    ms = 1e3 * (time.perf_counter() - t0)
    assert ok == [0] * HOST_SIGS
    print(f"host (serial, one core, PYTHON integers -- not compiled code) verify_host: {ms / HOST_SIGS:.2f} ms per signature ({HOST_SIGS} signatures)")
    return 0


def main() -> int:
    if sys.argv[1:2] == ["--host-rule"]:
        return host_rule()
    import zkhip
    from zkhip import jubjub as jj
    from zkhip import poseidon as ps
    from zkhip.field import fr_mont, splitmix_fr

    out = ["# tools/jubjub_time.py: warm-up %d, median of %d blocking calls, one process" % (WARM, REPS)]
    be = zkhip.Ctx(0)
    pos = ps.Poseidon(be)
    jub = jj.Jubjub(be, pos)
    cases = [(jj.keygen_host(sk), m, jj.sign_host(sk, m)) for sk, m in ((7, 70), (8, 80), (9, 90), (10, 100))]
    nmax = 1 << 18
    tile = lambda a: np.ascontiguousarray(np.tile(a, (nmax // len(cases),) + (1,) * (a.ndim - 1)))
    pk = be.to_device(tile(jj.points_limbs([c[0] for c in cases])))
    msg = be.to_device(tile(np.stack([fr_mont(c[1]) for c in cases])))
    sig = be.to_device(tile(jj.signatures_limbs([c[2] for c in cases])))
    dev_ms = {}
    for k in (10, 12, 16, 18):
        n = 1 << k
        assert not jub.schnorr_verify(pk, msg, sig, n).any()
        ms = median_ms(be, lambda: jub.schnorr_verify(pk, msg, sig, n))
        dev_ms[k] = ms
        out.append(f"zk_schnorr_verify n=2^{k}: {ms:.3f} ms  {n / ms:.0f} signatures/ms  {12.5e3 * n / ms / 1e6:.1f} G mul/s (12.5 k x the rate: not counted)  -- {verdict(('verify', k), ms)}")
    scalars = be.to_device(splitmix_fr(1 << 16, 3))  # any 256-bit values are scalars
    points = be.alloc(64 << 16)
    for k in (10, 16):
        n = 1 << k
        ms = median_ms(be, lambda: jub.mul(None, scalars, n, out=points))
        out.append(f"zk_jubjub_mul (fixed base) n=2^{k}: {ms:.3f} ms  -- {verdict(('mul', k), ms)}")
    for k in (10, 16):  # the points the last call left: multiples of G
        n = 1 << k
        assert not jub.check(points, n).any()
        ms = median_ms(be, lambda: jub.check(points, n))
        out.append(f"zk_jubjub_check n=2^{k}: {ms:.3f} ms  -- {verdict(('check', k), ms)}")
    check = os.path.join(PKG, "host", "bin", "poseidon_check")
    r = subprocess.run([check, "--time-schnorr", str(1 << 10)], capture_output=True, text=True, timeout=600)
    per = float(r.stdout.split("(")[1].split()[0]) if r.returncode == 0 else float("nan")
    out.append(f"host (serial, one core, compiled) {r.stdout.strip()}  -- per signature {verdict(('host', 10), per)}; "
               f"device at 2^16: {per * (1 << 16) / dev_ms[16]:.0f}x one core (expected ~4700x)")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-rule"], capture_output=True, text=True, timeout=600)
    out += r.stdout.splitlines() or ["host rule: failed: " + r.stderr.strip()[-200:]]
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "jubjub_time.txt")  # (an argument: another file)
    with open(dest, "w") as f:
        f.write(text)
    pos.free()
    be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
