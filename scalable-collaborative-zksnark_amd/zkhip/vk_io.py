"""
Verifying-key bytes for plonk: the vk of plonk.preprocess as ONE byte string and back, with every point validated on the way in, and a
verifier that starts from three files (vk, proof, public inputs) in a process that never ran preprocess.

Layout (no length prefixes: the header fixes every length):

    header, 26 bytes:  magic "ZKPLNVK" + version byte (1) | gate kind u8 (0 basic, 1 wide) | lookup u8 (0, 1) | mu u64 LE | l u64 LE
    body: the vk's commitments in their order (the gate's vk_tables, then qk, t0, t1, t2 with a lookup) as 48-byte compressed G1,
          then the mu + 2 keys [g2, s_0 g2, .., s_mu g2] (vk["g2"]) as 96-byte compressed G2 (serialize.py)

    commitments k = 5 (basic), 9 (wide), + 4 with a lookup
    bytes         = 26 + 48 k + 96 (mu + 2)

There is ONE encoding per key: parse_vk refuses a wrong magic or version, an unknown gate kind or lookup flag and any other length.
vk_from_bytes refuses the points by the rules of zk_g1_decompress_check and zk_g2_decompress_check (non-canonical encodings, x off the
curve, points outside the prime-order subgroups) -- ONE device call each, or, host=True, in Python integers -- and a G2 key at infinity:
a zero trapdoor coordinate or a zero generator is a group element and useless as a key.

The public inputs of verify_files are l canonical 32-byte little-endian Fr.

What is NOT checked: that the keys are the powers of ONE trapdoor and belong to the SRS the prover committed with (pairing checks
between keys, validation of the G1 powers): a vk is as trustworthy as where it comes from; these checks only keep a malformed or
off-subgroup key away from the pairing.
"""
from __future__ import annotations

import numpy as np

from . import proof_io as pio
from . import serialize as ser
from .field import R_MOD, fq_from_mont, fr_mont

MAGIC = b"ZKPLNVK"
VERSION = 1
HEADER_BYTES = pio.HEADER_BYTES


def _kinds(vk: dict):
    from .plonk import gate_of, has_lookup

    return gate_of(vk), has_lookup(vk)


def commitment_count(kind, lookup: bool) -> int:
    from .plonk import GATES, LOOKUP_VK_TABLES

    return len(GATES[kind].vk_tables) + (len(LOOKUP_VK_TABLES) if lookup else 0)


def vk_size(kind, lookup: bool, mu: int) -> int:
    """the length in bytes of the encoding of a vk of this kind: the formula of the module text"""
    return HEADER_BYTES + 48 * commitment_count(kind, lookup) + 96 * (mu + 2)


def g2_records(powers_of_g2) -> np.ndarray:
    """powers_of_g2 as python-int affine points (zkhip.pairing.powers_of_g2) or [n, 24] Montgomery records -> [n, 24] records"""
    if isinstance(powers_of_g2, np.ndarray):
        return np.ascontiguousarray(powers_of_g2, dtype=np.uint64).reshape(-1, 24).copy()
    return np.stack([ser.g2_point_words(P) for P in powers_of_g2])


def _g2_point_of_words(w):
    w = np.asarray(w, dtype=np.uint64).reshape(24)
    c = [fq_from_mont(w[6 * k:6 * k + 6]) for k in range(4)]
    return None if not any(c) else ((c[0], c[1]), (c[2], c[3]))


def vk_to_bytes(vk: dict) -> bytes:
    gate, lookup = _kinds(vk)
    mu, l = int(vk["mu"]), int(vk["l"])
    if vk.get("g2") is None:
        raise ValueError("the verifying key holds no G2 keys (preprocess without powers_of_g2)")
    comms = np.ascontiguousarray(vk["commitments"], dtype=np.uint64).reshape(-1, 18)
    keys = np.ascontiguousarray(vk["g2"], dtype=np.uint64).reshape(-1, 24)
    if len(comms) != commitment_count(gate.kind, lookup) or len(keys) != mu + 2:
        raise ValueError(f"{len(comms)} commitments and {len(keys)} G2 keys: not a vk of this kind with mu = {mu}")
    out = [MAGIC + bytes([VERSION, pio.GATE_KINDS.index(gate.kind), int(lookup)]) + mu.to_bytes(8, "little") + l.to_bytes(8, "little")]
    out += [ser.g1_serialize_compressed(pio._point_of_words(w)) for w in comms]
    out += [ser.g2_serialize_compressed(_g2_point_of_words(w)) for w in keys]
    data = b"".join(out)
    assert len(data) == vk_size(gate.kind, lookup, mu)
    return data


def parse_vk(data):
    """bytes -> (header {"gate", "lookup", "mu", "l"}, commitments [k, 48] uint8, keys [mu + 2, 96] uint8); host only.  ValueError for
    whatever is not the one encoding of some vk, the points aside"""
    data = bytes(data)
    if len(data) < HEADER_BYTES:
        raise ValueError(f"{len(data)} bytes: shorter than the header")
    if data[:7] != MAGIC:
        raise ValueError("wrong magic")
    if data[7] != VERSION:
        raise ValueError(f"version {data[7]}, this reader knows {VERSION}")
    if data[8] >= len(pio.GATE_KINDS):
        raise ValueError(f"unknown gate kind {data[8]}")
    if data[9] > 1:
        raise ValueError(f"lookup flag {data[9]}")
    kind, lookup = pio.GATE_KINDS[data[8]], bool(data[9])
    mu, l = int.from_bytes(data[10:18], "little"), int.from_bytes(data[18:26], "little")
    if mu > 64:
        raise ValueError(f"mu = {mu}")
    want = vk_size(kind, lookup, mu)
    if len(data) != want:
        raise ValueError(f"{len(data)} bytes, the header's key has {want}")
    k = commitment_count(kind, lookup)
    comms = np.frombuffer(data, dtype=np.uint8, count=48 * k, offset=HEADER_BYTES).reshape(k, 48)
    keys = np.frombuffer(data, dtype=np.uint8, count=96 * (mu + 2), offset=HEADER_BYTES + 48 * k).reshape(mu + 2, 96)
    return {"gate": kind, "lookup": lookup, "mu": mu, "l": l}, comms, keys


def _first_bad(c_status, k_status, k_inf):
    """the message for the first bad point in the order of the encoding, or None"""
    for i, s in enumerate(c_status):
        if s:
            return f"commitment {i}: {ser.G1_STATUS_TEXT[int(s)]}"
    for i, (s, inf) in enumerate(zip(k_status, k_inf)):
        if s:
            return f"G2 key {i}: {ser.G2_STATUS_TEXT[int(s)]}"
        if inf:
            return f"G2 key {i}: the point at infinity"
    return None


def vk_from_bytes(be, data, host: bool = False) -> dict:
    """the vk of the bytes.  parse_vk, then ONE g1_decompress_check over the commitments and ONE g2_decompress_check over the keys
    (host=True: the same rules in Python integers); ValueError names the first bad point, e.g. "G2 key 3: not in the subgroup".  A key
    at infinity is refused.  The pairing keys "pcs" are rebuilt by wiring.verifying_keys (be None, host only: they stay None)"""
    from . import wiring as wr

    if be is None and not host:
        raise ValueError("vk_from_bytes needs a device context, or host=True")
    hdr, comms, keys = parse_vk(data)
    c_pts, c_st = ser.g1_decompress_check_host(comms) if host else be.g1_decompress_check(comms)
    k_pts, k_st = ser.g2_decompress_check_host(keys) if host else be.g2_decompress_check(keys)
    bad = _first_bad(c_st, k_st, ~k_pts.any(axis=1))
    if bad:
        raise ValueError(bad)
    vk = {"mu": hdr["mu"], "l": hdr["l"], "commitments": c_pts.copy(), "pcs": wr.verifying_keys(be, k_pts) if be is not None else None, "g2": k_pts.copy()}
    if hdr["gate"] is not None:
        vk["gate"] = hdr["gate"]
    if hdr["lookup"]:
        vk["lookup"] = True
    return vk


def check_vk(be, vk: dict) -> list:
    """the validation of vk_from_bytes for a dict that is already in memory: ONE g1_check call over its commitments and ONE g2_check
    call over vk["g2"] -> the messages of every bad point in the order of the encoding (empty: all pass)"""
    if vk.get("g2") is None:
        raise ValueError("the verifying key holds no G2 keys (preprocess without powers_of_g2)")
    keys = np.ascontiguousarray(vk["g2"], dtype=np.uint64).reshape(-1, 24)
    c_st, k_st, k_inf = be.g1_check(vk["commitments"]), be.g2_check(keys), ~keys.any(axis=1)
    out = [f"commitment {i}: {ser.G1_STATUS_TEXT[int(s)]}" for i, s in enumerate(c_st) if s]
    return out + [f"G2 key {i}: " + (ser.G2_STATUS_TEXT[int(s)] if s else "the point at infinity") for i, (s, inf) in enumerate(zip(k_st, k_inf)) if s or inf]


def public_to_bytes(public_inputs) -> bytes:
    """[l, 4] Montgomery Fr -> l canonical 32-byte little-endian elements"""
    from .field import fr_from_mont

    return b"".join(ser.fr_serialize(fr_from_mont(w)) for w in np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4))


def public_from_bytes(data, l: int) -> np.ndarray:
    """l canonical 32-byte little-endian Fr -> [l, 4] Montgomery; ValueError for any other length and for a value >= r"""
    data = bytes(data)
    if len(data) != 32 * l:
        raise ValueError(f"{len(data)} bytes of public inputs, the key has l = {l}: {32 * l}")
    out = np.empty((l, 4), dtype=np.uint64)
    for i in range(l):
        v = int.from_bytes(data[32 * i:32 * i + 32], "little")
        if v >= R_MOD:
            raise ValueError(f"public input {i}: not a canonical Fr")
        out[i] = fr_mont(v)
    return out


def verify_files(be, vk_bytes, proof_bytes, public_bytes, aggregate: bool = False, host: bool = False) -> bool:
    """the verdict on three byte strings: vk_from_bytes and public_from_bytes (ValueError for a key or inputs that are refused, naming
    the cause), then proof_io.verify_bytes (False for a proof that is refused or does not verify).  host: the vk's points are
    validated in Python integers; the proof's and the pairing stay on the device"""
    vk = vk_from_bytes(be, vk_bytes, host)
    return pio.verify_bytes(be, vk, public_from_bytes(public_bytes, vk["l"]), proof_bytes, aggregate)
