"""
Proof bytes for plonk: a record of plonk.prove as ONE byte string and back, with every G1 point validated on the way in.

Layout (no length prefixes: the header fixes every length):

    header, 26 bytes:  magic "ZKPLONK" + version byte (1) | gate kind u8 (0 basic, 1 wide) | lookup u8 (0, 1) | mu u64 LE | l u64 LE
    body: the record's parts in the order plonk.proof_digest walks them --
        commitments (3 G1), v_commitment (1 G1), p_rounds (6 mu Fr), g_rounds (E mu Fr), g_values (S + 3 Fr), p_values (6 Fr),
        v_values (5 Fr), batch.rounds (3 mu Fr), batch.opening (mu G1), v_batch.rounds (3 (mu + 1) Fr), v_batch.opening (mu + 1 G1)
        and with a lookup: lookup.commitments (3 G1), lookup.rounds (4 mu Fr), lookup.values (10 Fr), lookup.batch.rounds (3 mu Fr),
        lookup.batch.opening (mu G1)
    E, S = evaluations per gate round, selectors: 5, 2 (basic), 8, 6 (wide).

Every G1 point is the 48-byte compressed encoding of serialize.py, every Fr the canonical little-endian 32 bytes (out of Montgomery form).

    points  k  = 2 mu + 5                       (+ mu + 3 with a lookup)
    scalars f  = (12 + E) mu + S + 17           (+ 7 mu + 10 with a lookup)
    bytes      = 26 + 48 k + 32 f

There is ONE encoding per record: parse_proof refuses a wrong magic or version, an unknown gate kind or lookup flag, any length but the
header's (trailing bytes included) and any Fr >= r; the points are refused by the rule of zk_g1_decompress_check (non-canonical
encodings, x off the curve, points outside the prime-order subgroup), on the device in ONE call or, host=True, in Python integers.

What is NOT checked here: the verifying key.  A vk made by preprocess in this process is the verifier's own and stays trusted; one that
comes from outside is read by vk_io.vk_from_bytes (or checked by vk_io.check_vk), which validates its commitments by the same G1 rule and
its G2 keys by zk_g2_decompress_check / zk_g2_check.  zk_pairing and zk_pcs_vk_create themselves still test no membership.
"""
from __future__ import annotations

import numpy as np

from . import serialize as ser
from .field import R_MOD, fq_from_mont, fr_from_mont, fr_mont

MAGIC = b"ZKPLONK"
VERSION = 1
HEADER_BYTES = 26
GATE_KINDS = (None, "wide")  # the header's gate kind byte indexes this


def _gate(kind):
    from .plonk import GATES

    return GATES[kind]


def _layout(kind, lookup: bool, mu: int):
    """[(part name, "g1" | "fr", shape without the word axis)] in the order of the body"""
    g = _gate(kind)
    parts = [("commitments", "g1", (3,)), ("v_commitment", "g1", ()), ("p_rounds", "fr", (mu, 6)), ("g_rounds", "fr", (mu, g.evals)),
             ("g_values", "fr", (len(g.g_values),)), ("p_values", "fr", (6,)), ("v_values", "fr", (5,)), ("batch.rounds", "fr", (mu, 3)),
             ("batch.opening", "g1", (mu,)), ("v_batch.rounds", "fr", (mu + 1, 3)), ("v_batch.opening", "g1", (mu + 1,))]
    if lookup:
        parts += [("lookup.commitments", "g1", (3,)), ("lookup.rounds", "fr", (mu, 4)), ("lookup.values", "fr", (10,)),
                  ("lookup.batch.rounds", "fr", (mu, 3)), ("lookup.batch.opening", "g1", (mu,))]
    return parts


def _count(shape) -> int:
    return int(np.prod(shape, dtype=np.int64)) if shape else 1


def proof_size(kind, lookup: bool, mu: int) -> int:
    """the length in bytes of the encoding of a record of this kind: the formula of the module text"""
    g = _gate(kind)
    k = 2 * mu + 5 + (mu + 3 if lookup else 0)
    f = (12 + g.evals) * mu + len(g.selectors) + 17 + (7 * mu + 10 if lookup else 0)
    return HEADER_BYTES + 48 * k + 32 * f


def _get(proof: dict, name: str):
    for key in name.split("."):
        proof = proof[key]
    return proof


def _point_of_words(w) -> ser.Point:
    """18 u64 Jacobian, any representative -> the affine point in integers"""
    w = np.asarray(w, dtype=np.uint64).reshape(18)
    x, y, z = fq_from_mont(w[0:6]), fq_from_mont(w[6:12]), fq_from_mont(w[12:18])
    if z == 0:
        return None
    if z == 1:
        return (x, y)
    zi = pow(z, -1, ser.Q_MOD)
    return (x * zi * zi % ser.Q_MOD, y * zi * zi * zi % ser.Q_MOD)


def point_parts(kind, lookup: bool, mu: int):
    """[(part, index)] of the k points in the order of the encoding"""
    return [(name, i) for name, what, shape in _layout(kind, lookup, mu) if what == "g1" for i in range(_count(shape))]


def describe(part: str, index: int, status: int) -> str:
    """e.g. "opening point 7 of v_batch: not in the subgroup" """
    where = f"opening point {index} of {part[:-len('.opening')]}" if part.endswith(".opening") else f"point {index} of {part}"
    return f"{where}: {ser.G1_STATUS_TEXT[int(status)]}"


def proof_to_bytes(proof: dict) -> bytes:
    from .plonk import gate_of, has_lookup

    kind, lookup, mu, l = gate_of(proof).kind, has_lookup(proof), int(proof["mu"]), int(proof["l"])
    out = [MAGIC + bytes([VERSION, GATE_KINDS.index(kind), int(lookup)]) + mu.to_bytes(8, "little") + l.to_bytes(8, "little")]
    for name, what, shape in _layout(kind, lookup, mu):
        a = np.ascontiguousarray(_get(proof, name), dtype=np.uint64)
        if what == "g1":
            out += [ser.g1_serialize_compressed(_point_of_words(w)) for w in a.reshape(_count(shape), 18)]
        else:
            out += [ser.fr_serialize(fr_from_mont(w)) for w in a.reshape(_count(shape), 4)]
    data = b"".join(out)
    assert len(data) == proof_size(kind, lookup, mu)
    return data


def parse_header(data) -> dict:
    """the 26 bytes and the length they imply -> {"gate", "lookup", "mu", "l"}; ValueError for a wrong magic, version, gate kind, lookup
    flag or length.  No scalar is converted: verify_bytes compares this with the vk first"""
    data = bytes(data) if not isinstance(data, bytes) else data
    if len(data) < HEADER_BYTES:
        raise ValueError(f"{len(data)} bytes: shorter than the header")
    if data[:7] != MAGIC:
        raise ValueError("wrong magic")
    if data[7] != VERSION:
        raise ValueError(f"version {data[7]}, this reader knows {VERSION}")
    if data[8] >= len(GATE_KINDS):
        raise ValueError(f"unknown gate kind {data[8]}")
    if data[9] > 1:
        raise ValueError(f"lookup flag {data[9]}")
    kind, lookup = GATE_KINDS[data[8]], bool(data[9])
    mu, l = int.from_bytes(data[10:18], "little"), int.from_bytes(data[18:26], "little")
    if mu > 64:
        raise ValueError(f"mu = {mu}")
    want = proof_size(kind, lookup, mu)
    if len(data) != want:
        raise ValueError(f"{len(data)} bytes, the header's record has {want}")
    return {"gate": kind, "lookup": lookup, "mu": mu, "l": l}


def parse_proof(data, header: dict | None = None):
    """bytes -> (header {"gate", "lookup", "mu", "l"}, compressed [k, 48] uint8, {part name: Montgomery Fr array}); host only.
    ValueError for whatever is not the one encoding of some record, the points aside.  header: the result of parse_header(data), when
    the caller has it already"""
    data = bytes(data)
    hdr = parse_header(data) if header is None else header
    kind, lookup, mu = hdr["gate"], hdr["lookup"], hdr["mu"]
    pos, comp, frs = HEADER_BYTES, [], {}
    for name, what, shape in _layout(kind, lookup, mu):
        n = _count(shape)
        if what == "g1":
            comp.append(np.frombuffer(data, dtype=np.uint8, count=48 * n, offset=pos).reshape(n, 48))
            pos += 48 * n
            continue
        a = np.empty((n, 4), dtype=np.uint64)
        for i in range(n):
            v = int.from_bytes(data[pos + 32 * i : pos + 32 * i + 32], "little")
            if v >= R_MOD:
                raise ValueError(f"element {i} of {name}: not a canonical Fr")
            a[i] = fr_mont(v)
        frs[name] = a.reshape(*shape, 4)
        pos += 32 * n
    return hdr, np.concatenate(comp), frs


def _first_bad(parts, status):
    bad = np.nonzero(np.asarray(status))[0]
    return None if not len(bad) else (*parts[int(bad[0])], int(status[int(bad[0])]))


def proof_from_bytes(be, data, host: bool = False) -> dict:
    """the record of the bytes.  parse_proof, then ONE g1_decompress_check over all k points (host=True: the same rule in Python
    integers, be may be None); ValueError names the first bad point by part, index and status"""
    return _record(be, parse_proof(data), host)


def _record(be, parsed, host: bool = False) -> dict:
    hdr, comp, frs = parsed
    points, status = ser.g1_decompress_check_host(comp) if host else be.g1_decompress_check(comp)
    parts = point_parts(hdr["gate"], hdr["lookup"], hdr["mu"])
    bad = _first_bad(parts, status)
    if bad:
        raise ValueError(describe(*bad))
    proof: dict = {"mu": hdr["mu"], "l": hdr["l"]}
    pos = 0
    for name, what, shape in _layout(hdr["gate"], hdr["lookup"], hdr["mu"]):
        if what == "g1":
            n = _count(shape)
            val = points[pos:pos + n].reshape(*shape, 18).copy()
            pos += n
        else:
            val = frs[name]
        d, keys = proof, name.split(".")
        for key in keys[:-1]:
            d = d.setdefault(key, {})
        d[keys[-1]] = val
    if hdr["gate"] is not None:
        proof["gate"] = hdr["gate"]
    return proof


def check_points(be, proof: dict) -> list:
    """the validation of proof_from_bytes for a record that is already a dict: ONE g1_check call over all its points ->
    [(part, index, status)] of every bad point (empty: all are canonical, on the curve and in G1)"""
    from .plonk import gate_of, has_lookup

    kind, lookup, mu = gate_of(proof).kind, has_lookup(proof), int(proof["mu"])
    pts = np.concatenate([np.ascontiguousarray(_get(proof, name), dtype=np.uint64).reshape(_count(shape), 18)
                          for name, what, shape in _layout(kind, lookup, mu) if what == "g1"])
    status = be.g1_check(pts)
    parts = point_parts(kind, lookup, mu)
    return [(*parts[int(i)], int(status[int(i)])) for i in np.nonzero(status)[0]]


def _record_for(be, vk: dict, data):
    """the record of the bytes when its header agrees with the vk (gate kind, lookup, mu, l) and every point passes; None otherwise"""
    from .plonk import gate_of, has_lookup

    try:
        data = bytes(data)
        hdr = parse_header(data)
        if (hdr["gate"], hdr["lookup"], hdr["mu"], hdr["l"]) != (gate_of(vk).kind, has_lookup(vk), int(vk["mu"]), int(vk["l"])):
            return None
        return _record(be, parse_proof(data, hdr))  # the body is parsed once
    except (KeyError, ValueError, TypeError):
        return None


def verify_bytes(be, vk: dict, public_inputs, data, aggregate: bool = False) -> bool:
    """proof_from_bytes, the header against the vk (gate kind, lookup, mu, l), then plonk.verify (aggregate=True: plonk.verify_agg, one
    pairing call); any refusal is False"""
    from .plonk import verify, verify_agg

    proof = _record_for(be, vk, data)
    if proof is None:
        return False
    return (verify_agg if aggregate else verify)(be, vk, public_inputs, proof)


def verify_bytes_many(be, vk: dict, items) -> list:
    """verify_bytes for a list of (public_inputs, data): each encoding is validated on its own, the records that pass go through
    plonk.verify_many -- ONE aggregated pairing check for all of them"""
    from .plonk import verify_many

    records = [(pi, _record_for(be, vk, data)) for pi, data in items]
    good = [n for n, (_, rec) in enumerate(records) if rec is not None]
    verdicts = verify_many(be, vk, [records[n] for n in good])
    out = [False] * len(records)
    for n, v in zip(good, verdicts):
        out[n] = bool(v)
    return out
