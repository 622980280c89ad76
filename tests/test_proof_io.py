"""
Proof bytes without a device: the Python host's G1 rule (zkhip.serialize.g1_decompress_check_host) against the integer model
(g1check_model.py: membership by the definition [r]P = O), and zkhip.proof_io on synthetic records whose points are generator multiples:
round trip, the documented size, and every refusal with the part, index and status it must name.
"""
import numpy as np
import pytest

import g1check_model as gm
from zkhip import plonk, proof_io
from zkhip import serialize as ser
from zkhip.field import R_MOD, fr_mont

KINDS = [(None, False), (None, True), ("wide", False), ("wide", True)]
MU = 3


def test_host_rule_matches_the_model_on_every_kind_of_point():
    encs = [e for _, e in gm.cases(1)]
    want_pts, want_st = gm.expected(encs)
    assert set(want_st.tolist()) == {0, 1, 2, 3}
    pts, st = ser.g1_decompress_check_host(b"".join(encs))
    assert st.tolist() == want_st.tolist(), [(n, int(a), int(b)) for (n, _), a, b in zip(gm.cases(1), st, want_st) if a != b]
    assert (pts == want_pts).all()
    # the random curve points ARE outside G1, the members inside, by the definition
    for name, e in gm.cases(1):
        s = gm.decompress_check(e)[0]
        if name.startswith(("curve", "cofactor", "order")):
            assert s == gm.NOT_IN_G1, name
        if name.startswith(("member", "infinity")):
            assert s == gm.OK, name
    # the wrong sign bit gives -P: valid, and another point
    for name, e in gm.cases(1):
        if name == "member":
            flipped = bytes([e[0] ^ 0x20]) + e[1:]
            (s0, P), (s1, N) = gm.decompress_check(e), gm.decompress_check(flipped)
            assert s0 == s1 == 0 and N == gm.neg(P) != P
            assert (ser.g1_decompress_check_host(flipped)[0][0] == gm.words(N)).all()
    assert ser.g1_decompress_check_host(b"")[1].shape == (0,)


def test_beta_is_the_root_that_belongs_to_minus_x_squared():
    P = gm.mul(gm.G, 0xDEADBEEF)
    assert (ser.BETA * P[0] % gm.Q, P[1]) == gm.mul(P, gm.R - ser.X_ABS**2)
    assert pow(ser.BETA, 3, gm.Q) == 1 and ser.X_ABS**4 - ser.X_ABS**2 + 1 == gm.R


def synthetic_record(kind, lookup, mu, seed=5):
    """a record of the right shapes: generator multiples for points, seeded canonical elements for scalars (it proves nothing)"""
    rng = np.random.default_rng(seed)
    state = {"k": 1}

    def g1(*shape):
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        out = np.stack([gm.words(gm.mul(gm.G, state["k"] + i)) for i in range(n)])
        state["k"] += n
        return out.reshape(*shape, 18)

    def fr(*shape):
        n = int(np.prod(shape, dtype=np.int64))
        return np.stack([fr_mont(int(rng.integers(1, 1 << 62)) ** 4 % R_MOD) for _ in range(n)]).reshape(*shape, 4)

    g = plonk.GATES[kind]
    rec = {"mu": mu, "l": 2, "commitments": g1(3), "v_commitment": g1(), "p_rounds": fr(mu, 6), "g_rounds": fr(mu, g.evals),
           "g_values": fr(len(g.g_values)), "p_values": fr(6), "v_values": fr(5), "batch": {"rounds": fr(mu, 3), "opening": g1(mu)},
           "v_batch": {"rounds": fr(mu + 1, 3), "opening": g1(mu + 1)}, **g.tag()}
    if lookup:
        rec["lookup"] = {"commitments": g1(3), "rounds": fr(mu, 4), "values": fr(10), "batch": {"rounds": fr(mu, 3), "opening": g1(mu)}}
    rec["batch"]["opening"][1] = gm.words(None)  # infinity travels too
    return rec


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_round_trip_digest_bytes_and_length(kind, lookup):
    rec = synthetic_record(kind, lookup, MU)
    data = plonk.proof_to_bytes(rec)
    g = plonk.GATES[kind]
    k = 2 * MU + 5 + (MU + 3 if lookup else 0)
    f = (12 + g.evals) * MU + len(g.selectors) + 17 + (7 * MU + 10 if lookup else 0)
    assert len(data) == 26 + 48 * k + 32 * f == proof_io.proof_size(kind, lookup, MU)
    hdr, comp, frs = plonk.parse_proof(data)
    assert hdr == {"gate": kind, "lookup": lookup, "mu": MU, "l": 2} and comp.shape == (k, 48) and sum(v.size // 4 for v in frs.values()) == f
    back = plonk.proof_from_bytes(None, data, host=True)
    assert plonk.proof_digest(back) == plonk.proof_digest(rec)
    assert plonk.proof_to_bytes(back) == data
    assert plonk.gate_of(back).kind == kind and plonk.has_lookup(back) == lookup
    # a non-normalised representative of a point encodes to the same bytes: one encoding per record
    other = dict(rec, v_commitment=gm.jac_words(gm.mul(gm.G, 4), 0x1234567))
    assert plonk.proof_to_bytes(other) == data


def _data(kind=None, lookup=True):
    return bytearray(plonk.proof_to_bytes(synthetic_record(kind, lookup, MU)))


def test_refusals_of_the_framing():
    data = _data()
    for bad, what in ((data[:-1], "bytes"), (data + b"\0", "bytes"), (data[:20], "header")):
        with pytest.raises(ValueError, match=what):
            plonk.parse_proof(bytes(bad))
    v = bytearray(data)
    v[7] = 2
    with pytest.raises(ValueError, match="version"):
        plonk.parse_proof(bytes(v))
    v = bytearray(data)
    v[0] ^= 1
    with pytest.raises(ValueError, match="magic"):
        plonk.parse_proof(bytes(v))
    for off, val in ((8, 1), (8, 2), (9, 0), (9, 2), (10, MU + 1)):  # a header that disagrees with the body's kind / size
        v = bytearray(data)
        v[off] = val
        with pytest.raises(ValueError):
            plonk.parse_proof(bytes(v))
    # an Fr equal to r, and r - 1 accepted: the first scalar is p_rounds[0][0], after four points
    v = bytearray(data)
    v[26 + 4 * 48:26 + 4 * 48 + 32] = R_MOD.to_bytes(32, "little")
    with pytest.raises(ValueError, match="element 0 of p_rounds"):
        plonk.parse_proof(bytes(v))
    v[26 + 4 * 48:26 + 4 * 48 + 32] = (R_MOD - 1).to_bytes(32, "little")
    assert plonk.parse_proof(bytes(v))[2]["p_rounds"][0, 0].tolist() == fr_mont(R_MOD - 1).tolist()


def test_every_bad_point_is_refused_with_its_part_index_and_status():
    kind, lookup = "wide", True
    data = _data(kind, lookup)
    parts = proof_io.point_parts(kind, lookup, MU)
    assert [p for p, _ in parts][:4] == ["commitments"] * 3 + ["v_commitment"] and len(parts) == 3 * MU + 8
    # the byte offset of every point
    offs, pos = [], 26
    for name, what, shape in proof_io._layout(kind, lookup, MU):
        n = proof_io._count(shape)
        if what == "g1":
            offs += [pos + 48 * i for i in range(n)]
        pos += (48 if what == "g1" else 32) * n
    bad_kinds = [(name, e) for name, e in gm.cases(1) if gm.decompress_check(e)[0] != 0]
    assert {gm.decompress_check(e)[0] for _, e in bad_kinds} == {1, 2, 3}
    for j, (name, e) in enumerate(bad_kinds):
        slot = (5 * j + 1) % len(parts)
        v = bytearray(data)
        v[offs[slot]:offs[slot] + 48] = e
        part, idx = parts[slot]
        want = proof_io.describe(part, idx, gm.decompress_check(e)[0])
        with pytest.raises(ValueError) as err:
            plonk.proof_from_bytes(None, bytes(v), host=True)
        assert str(err.value) == want, (name, slot)
    assert proof_io.describe("v_batch.opening", 7, 3) == "opening point 7 of v_batch: not in the subgroup"
    assert proof_io.describe("commitments", 2, 1) == "point 2 of commitments: bad encoding"
    # two bad points: the first is named
    v = bytearray(data)
    for slot in (9, 2):
        v[offs[slot]:offs[slot] + 48] = gm.compress((0, 2))
    with pytest.raises(ValueError, match="^point 2 of commitments: not in the subgroup$"):
        plonk.proof_from_bytes(None, bytes(v), host=True)
