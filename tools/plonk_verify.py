#!/usr/bin/env python3
"""
Verify a plonk proof from three files, in a process that never ran preprocess:

    python tools/plonk_verify.py --vk FILE --proof FILE --public FILE [--aggregate] [--host-checks]

The vk is the encoding of zkhip/vk_io.py (its commitments and G2 keys are validated on the device, or with --host-checks in Python
integers), the proof that of zkhip/proof_io.py, the public inputs l canonical 32-byte little-endian Fr.  Prints the SHA-256 of each
file and one verdict line; exit status 0 accepted, 1 rejected (the proof is refused or does not verify), 2 a key or inputs that are
refused (the line names the cause, e.g. "G2 key 3: not in the subgroup").  --aggregate: one pairing check (plonk.verify_agg).
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-collaborative-zksnark_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    for name in ("vk", "proof", "public"):
        ap.add_argument("--" + name, required=True)
    ap.add_argument("--aggregate", action="store_true")
    ap.add_argument("--host-checks", action="store_true")
    a = ap.parse_args()
    data = {}
    for name in ("vk", "proof", "public"):
        with open(getattr(a, name), "rb") as f:
            data[name] = f.read()
        print(f"{name}_sha256 {hashlib.sha256(data[name]).hexdigest()} bytes {len(data[name])}")
    import zkhip
    from zkhip import plonk

    be = zkhip.Ctx(0)
    try:
        ok = plonk.verify_files(be, data["vk"], data["proof"], data["public"], aggregate=a.aggregate, host=a.host_checks)
    except ValueError as e:
        print(f"verdict refused: {e}")
        return 2
    finally:
        be.close()
    print("verdict accepted" if ok else "verdict rejected")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
