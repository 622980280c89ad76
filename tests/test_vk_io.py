"""
zkhip.vk_io on the host alone (host=True, no device): the size formula, the round trip of a synthetic vk (commitments k G1_GEN, keys
s_i G2_GEN), every refusal of parse_vk, a non-member key and a key at infinity named in the error, and the public-input bytes.
"""
import numpy as np
import pytest

import g1check_model as g1m
import g2check_model as gm

KINDS = [(None, False), (None, True), ("wide", False), ("wide", True)]
MU = 4


def _synthetic(kind, lookup, mu=MU, l=2):
    from zkhip import vk_io

    k = vk_io.commitment_count(kind, lookup)
    vk = {"mu": mu, "l": l, "pcs": None, "commitments": np.stack([g1m.words(g1m.mul(g1m.G, 3 + j)) for j in range(k)]),
          "g2": np.stack([gm.words(gm.mul(gm.G2, 5 + 7 * j)) for j in range(mu + 2)])}
    if kind:
        vk["gate"] = kind
    if lookup:
        vk["lookup"] = True
    return vk


@pytest.mark.parametrize("kind,lookup", KINDS)
def test_size_formula_and_round_trip(kind, lookup):
    from zkhip import plonk, vk_io

    vk = _synthetic(kind, lookup)
    data = plonk.vk_to_bytes(vk)
    k = {None: 5, "wide": 9}[kind] + (4 if lookup else 0)
    assert vk_io.commitment_count(kind, lookup) == k
    assert len(data) == 26 + 48 * k + 96 * (MU + 2) == vk_io.vk_size(kind, lookup, MU)
    assert data[:8] == b"ZKPLNVK\x01" and data[8] == (1 if kind else 0) and data[9] == int(lookup)
    hdr, comms, keys = plonk.parse_vk(data)
    assert hdr == {"gate": kind, "lookup": lookup, "mu": MU, "l": 2} and comms.shape == (k, 48) and keys.shape == (MU + 2, 96)
    assert bytes(keys[1]) == gm.compress(gm.mul(gm.G2, 12)) and bytes(comms[0]) == g1m.compress(g1m.mul(g1m.G, 3))
    back = plonk.vk_from_bytes(None, data, host=True)
    assert set(back) == set(vk) and back["pcs"] is None
    assert (back["commitments"] == vk["commitments"]).all() and (back["g2"] == vk["g2"]).all()
    assert (back["mu"], back["l"], back.get("gate"), back.get("lookup", False)) == (MU, 2, kind, lookup)
    assert plonk.vk_to_bytes(back) == data


def test_a_vk_without_keys_has_no_encoding():
    from zkhip import plonk

    vk = _synthetic(None, False)
    vk["g2"] = None
    with pytest.raises(ValueError):
        plonk.vk_to_bytes(vk)


def test_every_refusal_of_parse_vk():
    from zkhip import plonk

    data = plonk.vk_to_bytes(_synthetic(None, False))

    def refused(b, word):
        with pytest.raises(ValueError) as e:
            plonk.parse_vk(bytes(b))
        assert word in str(e.value), str(e.value)

    refused(data[:20], "shorter")
    refused(b"ZKPLONK" + data[7:], "magic")  # a proof's magic
    refused(data[:7] + b"\x02" + data[8:], "version")
    refused(data[:8] + b"\x02" + data[9:], "gate kind")
    refused(data[:9] + b"\x02" + data[10:], "lookup flag")
    refused(data + b"\0", "bytes")
    refused(data[:-1], "bytes")
    refused(data[:8] + b"\x01" + data[9:], "bytes")  # the other kind: another length
    refused(data[:9] + b"\x01" + data[10:], "bytes")
    refused(data[:10] + (MU + 1).to_bytes(8, "little") + data[18:], "bytes")
    refused(data[:10] + (2**63).to_bytes(8, "little") + data[18:], "mu")
    plonk.parse_vk(data)


def test_bad_points_are_named():
    from zkhip import plonk, vk_io

    vk = _synthetic(None, True)
    data = plonk.vk_to_bytes(vk)
    k = vk_io.commitment_count(None, True)
    key_at = lambda j: 26 + 48 * k + 96 * j
    t13 = dict(gm.points(1))["order13"]

    def message(b):
        with pytest.raises(ValueError) as e:
            plonk.vk_from_bytes(None, bytes(b), host=True)
        return str(e.value)

    for j in (0, 3, MU + 1):
        bad = bytearray(data)
        P = gm.add(gm.decompress_check(bytes(data[key_at(j):key_at(j) + 96]))[1], t13)  # key + a point of order 13
        assert gm.on_curve(P) and not gm.in_g2(P)
        bad[key_at(j):key_at(j) + 96] = gm.compress(P)
        assert message(bad) == f"G2 key {j}: not in the subgroup"
        inf = bytearray(data)
        inf[key_at(j):key_at(j) + 96] = gm.compress(None)
        assert message(inf) == f"G2 key {j}: the point at infinity"
    bad = bytearray(data)
    bad[key_at(2)] &= 0x7F
    assert message(bad) == "G2 key 2: bad encoding"
    bad = bytearray(data)
    bad[26 + 48 * 2:26 + 48 * 3] = g1m.compress(g1m.add(g1m.mul(g1m.G, 5), (0, 2)))  # + a point of order 3
    assert message(bad) == "commitment 2: not in the subgroup"
    bad[26 + 48] &= 0x7F  # the first bad point is the one named
    assert message(bad) == "commitment 1: bad encoding"


def test_public_input_bytes():
    from zkhip import vk_io
    from zkhip.field import fr_mont

    pi = np.stack([fr_mont(v) for v in (0, 1, gm.R - 1, 12345)])
    data = vk_io.public_to_bytes(pi)
    assert len(data) == 128 and data[32:64] == (1).to_bytes(32, "little")
    assert (vk_io.public_from_bytes(data, 4) == pi).all()
    for bad, l in ((data, 2), (data[:-1], 4), (data + b"\0", 4), (b"", 4)):
        with pytest.raises(ValueError):
            vk_io.public_from_bytes(bad, l)
    with pytest.raises(ValueError) as e:
        vk_io.public_from_bytes(data[:64] + gm.R.to_bytes(32, "little") + data[96:], 4)
    assert "public input 2" in str(e.value)
