"""
Parameter-set bytes on the CPU: the encoding of zkhip/srs_io.py, what parse_srs refuses, and srs_check_host against the point-by-point
verdict of tests/srs_io_model.py.  The untampered files of tests/test_gpu_srs_io.py are the ones accepted here.
"""
import hashlib

import numpy as np
import pytest

import g1check_model as gm
import srs_io_model as sm
from zkhip import pairing as pr
from zkhip import serialize as ser
from zkhip import srs_io


def good_file(n: int) -> bytes:
    _, lv, ks = sm.sample(n)
    return srs_io.encode(lv[n], ks)


def with_point(data: bytes, i: int, P) -> bytes:
    b = bytearray(data)
    b[26 + 48 * i:26 + 48 * i + 48] = gm.compress(P)
    return bytes(b)


def with_key(data: bytes, n: int, i: int, K) -> bytes:
    b = bytearray(data)
    o = 26 + (48 << n) + 96 * i
    b[o:o + 96] = ser.g2_serialize_compressed(K)
    return bytes(b)


def model_messages(data: bytes) -> list:
    """the point-by-point verdict on a file whose points and keys are all valid"""
    n, pts, keys = srs_io.parse_srs(data)
    top = [gm.decompress_check(pts[i].tobytes())[1] for i in range(1 << n)]
    ks = [ser.g2_deserialize_compressed(keys[i].tobytes()) for i in range(n + 1)]
    return [srs_io.level_message(k, n) for k in sm.failing_levels(sm.derive(top), ks)]


@pytest.mark.parametrize("n", [1, 3])
def test_round_trip(n):
    _, lv, ks = sm.sample(n)
    data = srs_io.encode(lv[n], ks)
    assert len(data) == srs_io.srs_size(n) == 26 + 48 * 2**n + 96 * (n + 1)
    assert data[:8] == b"ZKPLSRS\x01" and data[8:10] == bytes(2) and data[10:18] == n.to_bytes(8, "little") and data[18:26] == bytes(8)
    m, pts, keys = srs_io.parse_srs(data)
    assert m == n and pts.shape == (2**n, 48) and keys.shape == (n + 1, 96)
    assert [gm.decompress_check(pts[i].tobytes()) for i in range(2**n)] == [(gm.OK, P) for P in lv[n]]
    assert [ser.g2_deserialize_compressed(keys[i].tobytes()) for i in range(n + 1)] == ks
    assert srs_io.encode(lv[n], ks) == data  # one encoding


def test_levels_satisfy_relation_a_and_the_weights_are_hashlib():
    _, lv, _ = sm.sample(3)
    assert sm.derive(lv[3]) == lv
    assert [srs_io.halve_points(lv[k + 1]) == lv[k] for k in range(3)] == [True] * 3
    seed = hashlib.sha256(b"w").digest()
    assert srs_io.rho(seed, 5) == sm.rho(seed, 5) and all(v < 2**128 for v in sm.rho(seed, 5))
    assert sm.rho(seed, 3) != sm.rho(seed, 3, domain=2)
    assert sm.rho(seed, 1)[0] == int.from_bytes(hashlib.sha256(seed + bytes([1, 0, 0, 0]) + bytes(8)).digest()[:16], "little")


def test_malformed_files_are_refused_by_name():
    data = good_file(2)
    cases = [
        (data[:25], "shorter than the header"),
        (b"ZKPLNVK" + data[7:], "wrong magic"),
        (data[:7] + b"\x02" + data[8:], "version 2"),
        (data[:8] + b"\x01" + data[9:], "padding"),
        (data[:25] + b"\x01" + data[26:], "padding"),
        (data[:10] + (0).to_bytes(8, "little") + data[18:], "n = 0"),
        (data[:10] + (31).to_bytes(8, "little") + data[18:], "n = 31"),
        (data[:10] + (3).to_bytes(8, "little") + data[18:], "the header's parameter set has"),
        (data[:-1], "the header's parameter set has"),
        (data + b"\x00", "the header's parameter set has"),
    ]
    for bad, text in cases:
        with pytest.raises(ValueError, match=text):
            srs_io.parse_srs(bad)
        with pytest.raises(ValueError, match=text):
            srs_io.srs_check_host(bad)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_check_host_accepts_the_seeded_files(n):
    data = good_file(n)
    assert srs_io.srs_check_host(data) == [] == model_messages(data)


def test_check_host_names_the_level_after_one_tamper_at_each_level():
    n = 3
    data = good_file(n)
    other = gm.mul(gm.G, 0xABCDEF)
    # index 2^k of the top level is the first point of the upper half of the level k + 1 it is folded into
    for k in range(n):
        bad = with_point(data, 1 << k, other)
        want = model_messages(bad)
        assert srs_io.level_message(k, n) in want
        assert srs_io.srs_check_host(bad) == want
    bad = with_point(data, 0, other)  # folds down into L_0 = [g]: every level disagrees with its lower neighbour
    assert srs_io.srs_check_host(bad) == model_messages(bad) != []


def test_check_host_rejects_swapped_keys_and_a_compensating_tamper():
    n = 3
    s, lv, ks = sm.sample(n)
    data = good_file(n)
    swapped = with_key(with_key(data, n, 1, ks[2]), n, 2, ks[1])
    got = srs_io.srs_check_host(swapped)
    assert got == model_messages(swapped) and srs_io.level_message(n - 1, n) in got and srs_io.level_message(n - 2, n) in got
    # two points of the upper half changed by +D and -D, their images under (A) one level further down add up again: the sums of
    # every lower level are those of the good file
    D = gm.mul(gm.G, 77)
    comp = with_point(with_point(data, 4, gm.add(lv[n][4], D)), 6, gm.add(lv[n][6], gm.neg(D)))
    top = [gm.decompress_check(srs_io.parse_srs(comp)[1][i].tobytes())[1] for i in range(8)]
    assert sm.derive(top)[:n - 1] == lv[:n - 1] and sm.derive(top)[n - 1] != lv[n - 1]
    assert srs_io.srs_check_host(comp) == model_messages(comp) != []


def test_check_host_names_bad_points_and_keys():
    n = 2
    data = good_file(n)
    t3 = (0, 2)  # a point of order 3
    assert srs_io.srs_check_host(with_point(data, 3, gm.add(sm.sample(n)[1][n][3], t3))) == ["G1 point 3: not in the subgroup"]
    assert srs_io.srs_check_host(with_point(data, 1, None)) == ["G1 point 1: the point at infinity"]
    assert srs_io.srs_check_host(with_key(data, n, 2, None)) == ["G2 key 2: the point at infinity"]
    b = bytearray(data)
    b[26] &= 0x7F
    assert srs_io.srs_check_host(bytes(b)) == ["G1 point 0: bad encoding"]
    opposite = with_point(data, 2, gm.neg(sm.sample(n)[1][n][0]))
    assert srs_io.srs_check_host(opposite) == ["level 1: 1 of 2 sums are the point at infinity; the first is sum 0"]


def test_restrict_picks_the_last_coordinates():
    pcs, keys = list("abcdefgh"), np.arange(8 * 24, dtype=np.uint64).reshape(8, 24)
    lv, ks = srs_io.restrict(pcs, keys, 5)
    assert lv == list("abcdef") and (ks == keys[[0, 3, 4, 5, 6, 7]]).all()
    assert srs_io.restrict(pcs, list(range(8)), 7)[1] == list(range(8))
    with pytest.raises(ValueError):
        srs_io.restrict(pcs, keys, 8)
    # the eq basis over the last coordinates: the model's levels of s[-2:] are the first three levels of s
    s, lv3, _ = sm.sample(3)
    assert sm.levels(s[-2:]) == lv3[:3] and pr.powers_of_g2(s[-2:]) == [sm.keys(s)[i] for i in (0, 2, 3)]
