#!/usr/bin/env python3
"""
Make or check a parameter-set file (the encoding of zkhip/srs_io.py):

    python tools/plonk_srs.py --make N --seed S --out FILE     the SRS of N variables of the seeded trapdoor: TEST MATERIAL, whoever
                                                               knows the seed knows the trapdoor and can forge any opening
    python tools/plonk_srs.py --check FILE [--host-checks]     load and check the file as a prover would

--check prints the SHA-256 of the file and one verdict line; exit status 0 accepted, 2 refused (the line names the cause, e.g.
"G1 point 12345: not in the subgroup" or "level 7 does not match G2 key 14").  --host-checks runs the same rule in Python integers
(tiny N only).  An accepted file is consistent: its G1 points are the SRS of the trapdoor its G2 keys define.  That says nothing about
who knows the trapdoor.
"""
import argparse
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))


def trapdoor(n: int, seed: int) -> list:
    from zkhip.field import R_MOD

    rng = random.Random(f"zkhip-srs-{seed}-{n}")
    return [rng.randrange(2, R_MOD) for _ in range(n)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--make", type=int)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--check")
    ap.add_argument("--host-checks", action="store_true")
    a = ap.parse_args()
    if (a.make is None) == (a.check is None) or (a.make is not None and not a.out):
        ap.error("either --make N --out FILE or --check FILE")
    import numpy as np

    from zkhip import srs_io

    if a.check and a.host_checks:
        with open(a.check, "rb") as f:
            data = f.read()
        print(f"srs_sha256 {hashlib.sha256(data).hexdigest()} bytes {len(data)}")
        try:
            msgs = srs_io.srs_check_host(data)
        except ValueError as e:
            msgs = [str(e)]
        print("verdict " + ("accepted" if not msgs else "refused: " + msgs[0]))
        return 0 if not msgs else 2
    import zkhip
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip.field import fr_mont

    be = zkhip.Ctx(0)
    if a.make is not None:
        s = trapdoor(a.make, a.seed)
        pcs = dp.PolynomialCommitmentCub.new(be, np.stack([fr_mont(x) for x in s])).mature()
        data = srs_io.srs_to_bytes(be, pcs, pr.powers_of_g2(s))
        with open(a.out, "wb") as f:
            f.write(data)
        print(f"srs_sha256 {hashlib.sha256(data).hexdigest()} bytes {len(data)}")
        return 0
    with open(a.check, "rb") as f:
        data = f.read()
    print(f"srs_sha256 {hashlib.sha256(data).hexdigest()} bytes {len(data)}")
    try:
        pcs, _ = srs_io.srs_from_bytes(be, data)
    except ValueError as e:
        print(f"verdict refused: {e}")
        return 2
    print(f"verdict accepted: {len(pcs) - 1} variables, consistent with its G2 keys (this does not show that nobody knows the trapdoor)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
