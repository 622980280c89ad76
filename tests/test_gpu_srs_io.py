"""
A parameter set from a file on the device (csrc/zk_srsio.hip, zkhip/srs_io.py): zk_g1_decompress_check_device against the host-memory
call and the integer model, zk_srs_halve against Python integer addition, zk_fr_hash_expand against hashlib, zk_srs_check /
srs_from_bytes on good and tampered files, and a proof made on a loaded set.  tests/test_srs_io.py confirms on the CPU that the
untampered files used here pass the host rule and that the model names the levels the tampers break.
"""
import hashlib
import random

import numpy as np
import pytest

import g1check_model as gm
import srs_io_model as sm
import zerocheck_model as zm
from zkhip import dist_primitive as dp
from zkhip import pairing as pr
from zkhip import plonk, serialize as ser, srs_io
from zkhip.api import ZkError
from zkhip.field import affine_ints_to_mont, affine_mont_to_ints, fr_mont

pytestmark = pytest.mark.gpu

GRID_LANES = 2048 * 64  # the validation kernels launch at most 2048 workgroups of 64 lanes


def members(ctx, count, seed=3):
    """count compressed members of G1 (none at infinity), made on the device"""
    return srs_io._compress_records(ctx.srs_generate(1000 + seed, 7 + 2 * seed, count).download())


def reference(ctx, data):
    """the host-memory call on the same bytes, in the layout of the device call: (records [k, 12], status [k])"""
    p18, st = ctx.g1_decompress_check(data)
    rec = p18[:, :12].copy()
    rec[~p18[:, 12:].any(axis=1)] = 0  # infinity (1, 1, 0) and the zero records of status 1 and 2
    return rec, st


def run_device(ctx, data, refuse_infinity=False):
    count = len(data) // 48
    out, res = ctx.g1_decompress_check_device(ctx.to_device(np.frombuffer(data, dtype=np.uint8)), count, refuse_infinity=refuse_infinity)
    return out.download((count, 12)), res


def expect(rec, st):
    bad = np.flatnonzero(st)
    return (len(bad), int(bad[0]) if len(bad) else None, int(st[bad[0]]) if len(bad) else 0)


def put(data, i, enc):
    return data[:48 * i] + enc + data[48 * i + 48:]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 1000])
def test_decompress_check_device_matches_the_host_call(ctx, count):
    good = members(ctx, count)
    pool = gm.by_status(1)
    rec, res = run_device(ctx, good)
    want_rec, want_st = reference(ctx, good)
    assert res == (0, None, 0) and not want_st.any() and (rec == want_rec).all() and rec.any(axis=1).all()
    rng = random.Random(count)
    for status in (1, 2, 3):
        for pos in sorted({0, count // 2, count - 1}):
            data = put(good, pos, rng.choice(pool[status]))
            rec, res = run_device(ctx, data)
            want_rec, want_st = reference(ctx, data)
            assert res == (1, pos, status) == expect(want_rec, want_st), (count, status, pos)
            assert (rec == want_rec).all(), (count, status, pos)
    if count > 2:  # two bad points: the count is 2 and the smaller index is the one reported, whichever lane finishes first
        for lo, hi, s_lo, s_hi in ((1, count - 1, 3, 1), (0, count // 2, 2, 3), (count // 2, count - 1, 1, 2)):
            data = put(put(good, lo, pool[s_lo][0]), hi, pool[s_hi][0])
            rec, res = run_device(ctx, data)
            assert res == (2, lo, s_lo), (count, lo, hi)
            assert (rec == reference(ctx, data)[0]).all()


def test_decompress_check_device_every_named_point_and_infinity(ctx):
    encs = [e for _, e in gm.cases(1)]
    data = b"".join(encs)
    want_pts, want_st = gm.expected(encs)  # the model
    rec, res = run_device(ctx, data)
    want_rec = want_pts[:, :12].copy()
    want_rec[~want_pts[:, 12:].any(axis=1)] = 0
    assert (rec == want_rec).all() and res == expect(want_rec, want_st)
    assert (rec == reference(ctx, data)[0]).all()
    names = [n for n, _ in gm.cases(1)]
    inf = names.index("infinity")
    assert want_st[inf] == 0
    # every case alone and as the only bad point behind 64 members
    good = members(ctx, 70)
    for i, (name, e) in enumerate(gm.cases(1)):
        if name.startswith(("cofactor", "order", "infinity")):
            s = int(want_st[i])
            assert run_device(ctx, e)[1] == ((1, 0, s) if s else (0, None, 0)), name
            assert run_device(ctx, put(good, 66, e))[1] == ((1, 66, s) if s else (0, None, 0)), name
    # infinity: a member without flag bit 0, status 4 with it; the record is zero either way
    data = put(put(good, 5, gm.compress(None)), 69, gm.compress(None))
    rec, res = run_device(ctx, data)
    assert res == (0, None, 0) and not rec[5].any() and not rec[69].any()
    rec, res = run_device(ctx, data, refuse_infinity=True)
    assert res == (2, 5, 4) and not rec[5].any() and (rec[[4, 6]] == reference(ctx, data)[0][[4, 6]]).all()
    assert run_device(ctx, put(data, 2, gm.by_status(1)[3][0]), refuse_infinity=True)[1] == (3, 2, 3)
    assert ctx.g1_decompress_check_device(ctx.alloc(16), 0)[1] == (0, None, 0)


def test_decompress_check_device_strides_past_one_grid(ctx):
    # a grid capped at two workgroups: 1000 points are eight trips of the loop
    good = members(ctx, 1000, seed=4)
    pool = gm.by_status(1)
    data = put(put(put(good, 999, pool[3][0]), 130, pool[2][0]), 640, pool[1][0])
    want_rec, want_st = reference(ctx, data)
    ctx.dbg_tune("srsio_max_blocks", 2)
    try:
        rec, res = run_device(ctx, data)
    finally:
        ctx.dbg_tune("srsio_max_blocks", 0)
    assert res == (3, 130, 2) == expect(want_rec, want_st) and (rec == want_rec).all()
    # and one point more than the largest grid: the last point is the second trip of lane 0
    count = GRID_LANES + 1
    big = members(ctx, count, seed=5)
    data = put(put(big, count - 1, pool[3][1]), 70001, pool[3][0])
    rec, res = run_device(ctx, data)
    assert res == (2, 70001, 3)
    idx = [0, 1, 63, 64, 70000, 70001, 70002, GRID_LANES - 1, GRID_LANES]
    sub = b"".join(data[48 * i:48 * i + 48] for i in idx)
    assert (rec[idx] == reference(ctx, sub)[0]).all()
    assert run_device(ctx, big)[1] == (0, None, 0)


def _ints(recs):
    return [affine_mont_to_ints(r) if r.any() else None for r in recs]


def _neg_rec(r):
    x, y = affine_mont_to_ints(r)
    return affine_ints_to_mont((x, (-y) % gm.Q))


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_srs_halve_matches_integer_addition(ctx, m):
    recs = ctx.srs_generate(31 * m + 5, 11, 2 * m).download().reshape(2 * m, 12)
    for j in sorted({0, m // 2, m - 1}):  # equal operands: a doubling
        recs[j + m] = recs[j]
    pts = _ints(recs)
    want = np.stack([affine_ints_to_mont(gm.add(pts[j], pts[j + m])) for j in range(m)])
    level = ctx.srs_register(recs)
    half = ctx.srs_halve(level)
    assert len(half) == m and (half.download().reshape(m, 12) == want).all()
    # the halved level is a level like any other: an MSM on it sees the same points
    one = np.stack([fr_mont(1)] * m)
    acc = None
    for j in range(m):
        acc = gm.add(acc, gm.add(pts[j], pts[j + m]))
    assert (ctx.msm_g1(half, ctx.to_device(one), m) == gm.words(acc)).all()
    # opposite operands: refused with the count and the smallest j
    for js in ([0], [m - 1], sorted({0, m - 1})):
        bad = recs.copy()
        for j in js:
            bad[j + m] = _neg_rec(bad[j])
        with pytest.raises(ZkError, match=f"{len(js)} of {m} sums are the point at infinity; the first is sum {js[0]}$") as e:
            ctx.srs_halve(ctx.srs_register(bad))
        assert e.value.code == -1


def test_srs_halve_refuses_odd_and_empty_levels(ctx):
    for n in (1, 3, 7):
        with pytest.raises(ZkError, match="has no halves"):
            ctx.srs_halve(ctx.srs_generate(3, 5, n))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_fr_hash_expand_matches_hashlib(ctx, n):
    seed = hashlib.sha256(b"srs-io %d" % n).digest()
    got = ctx.fr_hash_expand(seed, 1, n).download((n, 4))
    assert (got == sm.rho_mont_words(seed, n, 1)).all()
    other = ctx.fr_hash_expand(seed, 0x01020304, n).download((n, 4))
    assert (other == sm.rho_mont_words(seed, n, 0x01020304)).all() and (other != got).any(axis=1).all()


def test_fr_mul_by_r2_on_128_bit_operands(ctx):
    """zk_fr_mul -- the generated Fr multiplier on run-time operands -- takes a 128-bit integer c (upper limbs zero, as the hash gives
    it) to its Montgomery form c R^2 / R, for c through the whole range, the top tenth of it included"""
    rng = random.Random(9)
    cs = [0, 1, 2**128 - 1, 2**127, 0xE6 << 120, 0xFF << 120] + [rng.randrange(2**128) for _ in range(250)] + [rng.randrange(0xE0 << 120, 2**128) for _ in range(256)]
    a = np.array([[(c >> (64 * i)) & (2**64 - 1) for i in range(4)] for c in cs], dtype=np.uint64)
    r2 = (1 << 512) % gm.R
    b = np.array([[(r2 >> (64 * i)) & (2**64 - 1) for i in range(4)]] * len(cs), dtype=np.uint64)
    got = ctx.fr_mul(ctx.to_device(a), ctx.to_device(b), len(cs)).download((len(cs), 4))
    assert (got == np.stack([fr_mont(c) for c in cs])).all()


# ---- files ----
_FILES = {}


def srs_file(ctx, n):
    """(file, s as integers) of the seeded trapdoor of the model, built on the device from s"""
    if n not in _FILES:
        s = sm.sample(n)[0] if n <= 3 else tuple(random.Random(n).randrange(2, gm.R) for _ in range(n))
        pcs = dp.PolynomialCommitmentCub.new(ctx, np.stack([fr_mont(x) for x in s])).mature()
        _FILES[n] = (srs_io.srs_to_bytes(ctx, pcs, pr.powers_of_g2(list(s))), s, pcs)
    return _FILES[n]


def point_at(data, i):
    return gm.decompress_check(data[26 + 48 * i:26 + 48 * i + 48])[1]


def with_point(data, i, P):
    return data[:26 + 48 * i] + gm.compress(P) + data[26 + 48 * i + 48:]


def with_key(data, n, i, K):
    o = 26 + (48 << n) + 96 * i
    return data[:o] + ser.g2_serialize_compressed(K) + data[o + 96:]


@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_srs_from_bytes_accepts_the_seeded_files(ctx, n):
    data, s, built = srs_file(ctx, n)
    if n <= 3:  # the file of the model's levels, byte for byte (tests/test_srs_io.py accepts it by the host rule)
        assert data == srs_io.encode(sm.sample(n)[1][n], sm.sample(n)[2])
    pcs, keys = srs_io.srs_from_bytes(ctx, data)
    assert len(pcs) == n + 1 and keys.shape == (n + 1, 24)
    for k in range(n + 1):  # the derived levels are the levels the trapdoor gives, bit for bit
        assert (pcs[k].download() == built[k].download()).all(), k
    assert srs_io.check_srs(ctx, pcs, keys, hashlib.sha256(b"another seed").digest()) == []
    assert ctx.srs_check(pcs, keys, srs_io.file_seed(data)).tolist() == [True] * n
    assert srs_io.srs_to_bytes(ctx, pcs, keys) == data


@pytest.mark.parametrize("n", [5, 9])
def test_srs_from_bytes_refuses_tampered_files(ctx, n):
    data, s, _ = srs_file(ctx, n)
    N, other = 1 << n, gm.mul(gm.G, 0xC0FFEE)
    # a top-level point replaced by another member of G1
    for i in (0, N // 2 + 1, N - 1):
        with pytest.raises(ValueError, match=r"^level \d+ does not match G2 key \d+$"):
            srs_io.srs_from_bytes(ctx, with_point(data, i, other))
    pcs, keys = srs_io.srs_from_bytes(ctx, with_point(data, N - 1, other), check=False)  # check=False skips only the pairing step
    failed = srs_io.check_srs(ctx, pcs, keys, srs_io.file_seed(data))
    assert srs_io.level_message(n - 1, n) in failed  # index N - 1 is in the upper half of L_n: (B) between L_{n-1} and L_n
    # two points swapped
    with pytest.raises(ValueError, match="does not match G2 key"):
        srs_io.srs_from_bytes(ctx, with_point(with_point(data, 1, point_at(data, N - 2)), N - 2, point_at(data, 1)))
    # a key replaced by another member of G2: exactly the level that pairs with it is named
    for i in (1, n):
        bad = with_key(data, n, i, pr.g2_mul(pr.G2_GEN, 12345 + i))
        with pytest.raises(ValueError, match=f"^level {n - i + 1} does not match G2 key {i}$"):
            srs_io.srs_from_bytes(ctx, bad)
        pcs, keys = srs_io.srs_from_bytes(ctx, bad, check=False)
        assert srs_io.check_srs(ctx, pcs, keys, srs_io.file_seed(bad)) == [f"level {n - i + 1} does not match G2 key {i}"]
    with pytest.raises(ValueError, match=f"^G2 key {n}: the point at infinity$"):
        srs_io.srs_from_bytes(ctx, with_key(data, n, n, None))
    # a point plus a point of order 3: refused at decompression, by index
    for i in (0, N // 2, N - 1):
        with pytest.raises(ValueError, match=f"^G1 point {i}: not in the subgroup$"):
            srs_io.srs_from_bytes(ctx, with_point(data, i, gm.add(point_at(data, i), (0, 2))))
    with pytest.raises(ValueError, match=f"^G1 point 3: the point at infinity$"):
        srs_io.srs_from_bytes(ctx, with_point(data, 3, None))
    # a file cut by one byte, or longer by one
    for bad in (data[:-1], data + b"\x00"):
        with pytest.raises(ValueError, match="the header's parameter set has"):
            srs_io.srs_from_bytes(ctx, bad)
    # the compensating tamper: +D and -D on two points of the upper half whose images meet one level further down, so every level
    # below L_{n-1} is that of the good file and (A) alone would accept
    D, a, b = gm.mul(gm.G, 99), N // 2, N // 2 + N // 4
    comp = with_point(with_point(data, a, gm.add(point_at(data, a), D)), b, gm.add(point_at(data, b), gm.neg(D)))
    pcs, keys = srs_io.srs_from_bytes(ctx, comp, check=False)
    good = srs_io.srs_from_bytes(ctx, data, check=False)[0]
    assert all((pcs[k].download() == good[k].download()).all() for k in range(n - 1)) and (pcs[n - 1].download() != good[n - 1].download()).any()
    with pytest.raises(ValueError, match="does not match G2 key"):
        srs_io.srs_from_bytes(ctx, comp)
    # opposite points in the two halves: the halving refuses the sum at infinity
    with pytest.raises(ValueError, match=f"^level {n - 1}: 1 of {N // 2} sums are the point at infinity; the first is sum 2$"):
        srs_io.srs_from_bytes(ctx, with_point(data, N // 2 + 2, gm.neg(point_at(data, 2))))


def test_proof_on_a_loaded_parameter_set(ctx):
    mu = 4
    c = plonk.sample_circuit(mu, 31)
    g2 = pr.powers_of_g2(zm.ints(c["s"]))
    pcs0 = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk0, vk0 = plonk.preprocess(ctx, pcs0, c, g2)
    want = plonk.proof_digest(plonk.prove(ctx, pk0, c["a"], c["b"], c["c"], c["public_inputs"]))
    data = plonk.srs_to_bytes(ctx, pcs0, g2)
    pcs1, keys1 = plonk.srs_from_bytes(ctx, data)
    pk1, vk1 = plonk.preprocess(ctx, pcs1, c, keys1)
    proof = plonk.prove(ctx, pk1, c["a"], c["b"], c["c"], c["public_inputs"])
    assert plonk.proof_digest(proof) == want
    assert plonk.verify(ctx, vk1, c["public_inputs"], proof) is True and plonk.verify(ctx, vk0, c["public_inputs"], proof) is True
    assert plonk.vk_to_bytes(vk1) == plonk.vk_to_bytes(vk0)


def test_one_file_serves_a_smaller_circuit(ctx):
    n, nv = 7, 5
    s = np.stack([fr_mont(x) for x in [random.Random(77 + i).randrange(2, gm.R) for i in range(n)]])
    big = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    data = srs_io.srs_to_bytes(ctx, big, pr.powers_of_g2(zm.ints(s)))
    pcs, keys = plonk.restrict(*plonk.srs_from_bytes(ctx, data), nv)
    small = dp.PolynomialCommitmentCub.new(ctx, s[-nv:]).mature()
    assert len(pcs) == nv + 1 and all((pcs[k].download() == small[k].download()).all() for k in range(nv + 1))
    c = dict(plonk.sample_circuit(nv - 1, 32))
    c["s"] = s[-nv:]
    g2 = pr.powers_of_g2(zm.ints(s[-nv:]))
    assert (keys == plonk.g2_records(g2)).all()
    pk0, vk0 = plonk.preprocess(ctx, small, c, g2)
    pk1, vk1 = plonk.preprocess(ctx, pcs, c, keys)
    args = (c["a"], c["b"], c["c"], c["public_inputs"])
    proof = plonk.prove(ctx, pk1, *args)
    assert plonk.proof_digest(proof) == plonk.proof_digest(plonk.prove(ctx, pk0, *args))
    assert plonk.verify(ctx, vk1, c["public_inputs"], proof) is True
