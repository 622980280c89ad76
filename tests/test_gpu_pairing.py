"""
The device pairing (csrc/zk_pairing.hip) against the host big-int pairing of zkhip/pairing.py:
  * zk_pairing values, limb for limb, = pairing.pairing(Q, P) ** ZK_PAIRING_EXP_MULTIPLE; a point at infinity gives one;
  * bilinearity at scale through zk_pairing_product_check (4096 groups, ragged groups of 1..40 pairs);
  * zk_pcs_verify_batch = PolynomialCommitment::verify (dist-primitive/src/dpoly_comm.rs:466-484) on the library's own
    commit / open over the structured SRS (should_commit_and_open, :502-531), honest and mutated openings;
  * input checks and repeatability.
"""
import os
import re

import numpy as np
import pytest

import pyoracle as po
from helpers import jac_norm_to_affine, pt_ints, pt_mont
from zkhip import pairing as pr
from zkhip._lib import ZK_ERR_INVALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = int(re.search(r"#define ZK_PAIRING_EXP_MULTIPLE (\d+)", open(os.path.join(ROOT, "include", "zkhip.h")).read()).group(1))
R = po.R_MOD


def g2_mont(Q):
    if Q is None:
        return np.zeros(24, dtype=np.uint64)
    return np.array(po.fq_to_mont_limbs(Q[0][0]) + po.fq_to_mont_limbs(Q[0][1]) + po.fq_to_mont_limbs(Q[1][0]) + po.fq_to_mont_limbs(Q[1][1]),
                    dtype=np.uint64)


def jac_mont(P):
    """affine ints -> normalised Jacobian [18]"""
    one = po.fq_to_mont_limbs(1)
    if P is None:
        return np.array(one + one + [0] * 6, dtype=np.uint64)
    return np.array(po.fq_to_mont_limbs(P[0]) + po.fq_to_mont_limbs(P[1]) + one, dtype=np.uint64)


def _mont(xs):
    return np.array([po.fr_to_mont_limbs(x) for x in xs], dtype=np.uint64).reshape(-1, 4)


# ---- 1. values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pairing_values_equal_the_host_pairing_to_the_fixed_power(ctx):
    rng = po.SplitMix64(31)
    pairs = [(po.g1_mul(po.G1_GEN, rng.fr()), po.g2_mul(po.G2_GEN, rng.fr())) for _ in range(4)]
    pairs += [(po.G1_GEN, po.G2_GEN), (None, po.G2_GEN), (po.G1_GEN, None), (None, None)]
    g1 = np.stack([pt_mont(P) for P, _ in pairs])
    g2 = np.stack([g2_mont(Q) for _, Q in pairs])
    out = ctx.pairing(g1, g2)
    one = np.array(pr.fq12_to_ark(pr.Fq12.one()), dtype=np.uint64)
    for i, (P, Q) in enumerate(pairs):
        if P is None or Q is None:
            assert (out[i] == one).all(), i
            continue
        want = pr.pairing(Q, P) ** (M % R)
        assert (out[i] == np.array(pr.fq12_to_ark(want), dtype=np.uint64)).all(), i
        assert not (out[i] == one).all()
    # the Rust-struct stride (flag byte at offset 192) is read the same way; a set flag is infinity
    rec = np.zeros((len(pairs), 200), dtype=np.uint8)
    rec[:, :192] = g2.view(np.uint8).reshape(len(pairs), 192)
    rec[0, 192] = 1
    out2 = ctx.pairing(g1, rec, g2_stride=200)
    assert (out2[1:] == out[1:]).all() and (out2[0] == one).all()


# ---- 2. bilinearity at scale ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bilinearity_4096_groups(ctx):
    """e(a_i P, b Q) * e(-a_i b P, Q) == 1 for 4096 groups; with a_i b + 1 none is.  G1 points come from zk_srs_generate:
    point i of srs_generate(k0, k1) is (k0 + i k1) G"""
    rng = po.SplitMix64(77)
    bs = [rng.fr() for _ in range(8)]
    per = 512
    g1_t, g2_t, g1_f = [], [], []
    for b in bs:
        k0, k1 = rng.fr(), rng.fr()
        Qb = g2_mont(po.g2_mul(po.G2_GEN, b))
        aP = ctx.srs_generate(k0, k1, per).download()
        neg = ctx.srs_generate((-k0 * b) % R, (-k1 * b) % R, per).download()
        neg1 = ctx.srs_generate((-(k0 * b + 1)) % R, (-k1 * b) % R, per).download()
        for i in range(per):
            g1_t += [aP[i], neg[i]]
            g1_f += [aP[i], neg1[i]]
            g2_t += [Qb, g2_mont(po.G2_GEN)]
    starts = np.arange(0, 2 * len(bs) * per + 1, 2, dtype=np.uint64)
    g2 = np.stack(g2_t)
    ok = ctx.pairing_product_check(starts, np.stack(g1_t), g2)
    assert ok.shape == (4096,) and ok.all()
    bad = ctx.pairing_product_check(starts, np.stack(g1_f), g2)
    assert not bad.any()


@pytest.mark.gpu
def test_ragged_groups(ctx):
    """groups of 1..40 pairs (a_j G, b_j G2): prod = e(G, G2)^(sum a_j b_j), which is 1 iff sum a_j b_j = 0 mod r"""
    rng = po.SplitMix64(5)
    bs = [rng.fr() for _ in range(6)]
    g2b = [g2_mont(po.g2_mul(po.G2_GEN, b)) for b in bs]
    sizes = [1, 2, 3, 40, 7, 1, 13, 2, 29, 5, 1, 17]
    g1, g2, starts, want = [], [], [0], []
    for gi, k in enumerate(sizes):
        js = [rng.next() % len(bs) for _ in range(k)]
        a = [rng.fr() for _ in range(k - 1)]
        acc = sum(x * bs[j] for x, j in zip(a, js)) % R
        last = (-acc) * pow(bs[js[-1]], -1, R) % R
        truth = gi % 3 != 1
        if not truth:
            last = (last + 1) % R
        for x, j in zip(a + [last], js):
            g1.append(pt_mont(po.g1_mul(po.G1_GEN, x)))
            g2.append(g2b[j])
        starts.append(len(g1))
        want.append(truth)
    ok = ctx.pairing_product_check(np.array(starts, dtype=np.uint64), np.stack(g1), np.stack(g2))
    assert list(ok) == want


# ---- 3. PolynomialCommitment::verify -------------------------------------------------------------------------------------------
def _opening(ctx, n, seed):
    """(s, cub levels, [(C, value, proofs, u)] two honest openings of random polynomials) over the structured SRS"""
    from helpers import rand_fr
    from zkhip import dist_primitive as dp

    rng = po.SplitMix64(seed)
    s = rng.fr_vec(n)
    cub = dp.PolynomialCommitmentCub.new(ctx, _mont(s))
    outs = []
    for k in range(2):
        u = rng.fr_vec(n)
        d_poly = ctx.to_device(rand_fr(1 << n, seed * 10 + k))
        C = dp.commit(ctx, cub.mature(), d_poly, 1 << n)
        value, proofs = dp.open_(ctx, cub.mature(), d_poly, 1 << n, _mont(u))
        outs.append((np.asarray(C, dtype=np.uint64), np.asarray(value, dtype=np.uint64), np.asarray(proofs, dtype=np.uint64).reshape(n, 18),
                     _mont(u)))
    return s, outs


def _mutations(op, other):
    C, v, pf, u = op
    n = len(pf)
    out = {}
    out["value+1"] = (C, _mont([(po.fr_from_mont_limbs(v) + 1) % R])[0], pf, u)
    p2 = pf.copy()
    p2[n // 2] = jac_mont(po.g1_add(pt_ints(jac_norm_to_affine(pf[n // 2])), po.G1_GEN))
    out["proof+g1"] = (C, v, p2, u)
    if n > 1:
        out["point reversed"] = (C, v, pf, u[::-1].copy())
    out["other commitment"] = (other[0], v, pf, u)
    p3 = pf.copy()
    p3[0] = jac_mont(None)
    out["proof at infinity"] = (C, v, p3, u)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4, 8, 12, 20])
def test_pcs_verify_batch(ctx, n):
    from zkhip import dist_primitive as dp

    s, ops = _opening(ctx, n, 900 + n)
    pg2 = pr.powers_of_g2(s)
    vk = dp.pcs_vk(ctx, pg2)
    C = np.stack([o[0] for o in ops])
    ok = dp.verify_batch(ctx, vk, C, np.stack([o[1] for o in ops]), np.stack([o[2] for o in ops]), np.stack([o[3] for o in ops]))
    assert ok.tolist() == [True, True]
    assert dp.verify_device(ctx, pg2, *ops[0])
    if n > 8:
        return
    for k, op in enumerate(ops):
        assert dp.verify(pg2, *op) is True
        for name, mut in _mutations(op, ops[1 - k]).items():
            dev = dp.verify_device(ctx, vk, *mut)
            assert dev == dp.verify(pg2, *mut), name
            assert dev is False, name


@pytest.mark.gpu
def test_pcs_verify_batch_of_64_mixed(ctx):
    from zkhip import dist_primitive as dp

    n = 4
    s, ops = _opening(ctx, n, 4711)
    vk = dp.pcs_vk(ctx, pr.powers_of_g2(s))
    muts = [_mutations(ops[0], ops[1]), _mutations(ops[1], ops[0])]
    names = sorted(muts[0])
    rng = po.SplitMix64(64)
    items, want = [], []
    for _ in range(64):
        k = rng.next() % 2
        r = rng.next() % (len(names) + 2)
        if r < len(names):
            items.append(muts[k][names[r]])
            want.append(False)
        else:
            items.append(ops[k])
            want.append(True)
    assert any(want) and not all(want)
    got = dp.verify_batch(ctx, vk, np.stack([i[0] for i in items]), np.stack([i[1] for i in items]), np.stack([i[2] for i in items]),
                          np.stack([i[3] for i in items]))
    assert got.tolist() == want


# ---- 5. errors, empty calls, repeatability -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_input_checks_and_repeatability(ctx):
    import zkhip
    from zkhip import dist_primitive as dp

    P, Q = po.g1_mul(po.G1_GEN, 12345), po.g2_mul(po.G2_GEN, 678)
    g1, g2 = pt_mont(P)[None], g2_mont(Q)[None]
    bad1 = pt_mont((P[0], (P[1] + 1) % po.Q_MOD))[None]
    bad2 = g2_mont((Q[0], ((Q[1][0] + 1) % po.Q_MOD, Q[1][1])))[None]
    for call in (lambda: ctx.pairing(bad1, g2), lambda: ctx.pairing(g1, bad2), lambda: ctx.pairing_product_check([0, 1], bad1, g2),
                 lambda: ctx.pairing(g1, g2, g2_stride=100)):
        with pytest.raises(zkhip.ZkError) as e:
            call()
        assert e.value.code == ZK_ERR_INVALID
    assert ctx.pairing(np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)).shape == (0, 72)
    assert ctx.pairing_product_check([0], np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)).shape == (0,)
    a = ctx.pairing(g1, g2)
    assert (ctx.pairing(g1, g2) == a).all()
    # the verifier: nvars + 1 > n_g2, an off-curve commitment, an empty batch
    s, ops = _opening(ctx, 2, 33)
    vk = dp.pcs_vk(ctx, pr.powers_of_g2(s))
    C, v, pf, u = ops[0]
    with pytest.raises(zkhip.ZkError) as e:
        dp.verify_batch(ctx, vk, C[None], v[None], np.concatenate([pf, pf[:1]])[None], np.concatenate([u, u[:1]])[None])
    assert e.value.code == ZK_ERR_INVALID
    Cb = C.copy()
    Cb[6] ^= np.uint64(1)
    with pytest.raises(zkhip.ZkError) as e:
        dp.verify_batch(ctx, vk, Cb[None], v[None], pf[None], u[None])
    assert e.value.code == ZK_ERR_INVALID
    with pytest.raises(zkhip.ZkError) as e:
        dp.pcs_vk(ctx, np.zeros((0, 24), dtype=np.uint64))
    assert e.value.code == ZK_ERR_INVALID
    assert dp.verify_batch(ctx, vk, np.zeros((0, 18), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64),
                           np.zeros((0, 2, 18), dtype=np.uint64), np.zeros((0, 2, 4), dtype=np.uint64)).shape == (0,)
    first = dp.verify_batch(ctx, vk, C[None], v[None], pf[None], u[None])
    assert first.tolist() == [True] and (dp.verify_batch(ctx, vk, C[None], v[None], pf[None], u[None]) == first).all()


@pytest.mark.gpu
def test_vk_input_checks(ctx):
    """zk_pcs_vk_create: an off-curve G2 power, an off-curve g1, and the Rust-stride infinity flag"""
    import zkhip
    from zkhip import dist_primitive as dp

    s = [5, 7]
    pg2 = np.stack([g2_mont(Q) for Q in pr.powers_of_g2(s)])
    bad = pg2.copy()
    bad[1, 12] ^= np.uint64(1)
    with pytest.raises(zkhip.ZkError) as e:
        ctx.pcs_vk(bad)
    assert e.value.code == ZK_ERR_INVALID
    g1bad = pt_mont(po.G1_GEN).copy()
    g1bad[6] ^= np.uint64(1)
    with pytest.raises(zkhip.ZkError) as e:
        ctx.pcs_vk(pg2, g1_96=g1bad)
    assert e.value.code == ZK_ERR_INVALID
    # Rust stride (flag byte at offset 192): the same vk as the packed records; a set flag makes s_1 g2 infinity
    s2, ops = _opening(ctx, 2, 17)
    pg = np.stack([g2_mont(Q) for Q in pr.powers_of_g2(s2)])
    rec = np.zeros((3, 200), dtype=np.uint8)
    rec[:, :192] = pg.view(np.uint8).reshape(3, 192)
    vk_a, vk_b = ctx.pcs_vk(rec, g2_stride=200), ctx.pcs_vk(pg)
    C, v, pf, u = ops[0]
    assert dp.verify_device(ctx, vk_a, C, v, pf, u) and dp.verify_device(ctx, vk_b, C, v, pf, u)
    rec[2, 192] = 1  # s_1 g2 -> infinity: the honest opening no longer verifies
    vk_c = ctx.pcs_vk(rec, g2_stride=200)
    assert not dp.verify_device(ctx, vk_c, C, v, pf, u)


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [2, 4])
def test_distributed_opening(ctx, parties):
    """
    d_commit / d_open (dpoly_comm.rs:276-297, :355-398) over LocalTestNet: the leader's value is the unsplit polynomial's value,
    its proof vector has n entries, and the device verifier's verdicts on it -- against the unsplit commitment and against d_commit --
    equal the host big-int verifier's.  (Why these openings do not satisfy verify's equation on a structured SRS: see DESIGN.md.)
    """
    import zkhip
    from helpers import rand_fr
    from zkhip import dist_primitive as dp
    from zkhip.net import LocalTestNet

    n = 4
    plog = parties.bit_length() - 1
    m = n - plog
    rng = po.SplitMix64(533 + parties)
    s, u = rng.fr_vec(n), rng.fr_vec(n)
    poly = rand_fr(1 << n, 581 + parties)
    cub = dp.PolynomialCommitmentCub.new(ctx, _mont(s))
    C_full = np.asarray(dp.commit(ctx, cub.mature(), ctx.to_device(poly), 1 << n), dtype=np.uint64)
    v_full, _ = dp.open_(ctx, cub.mature(), ctx.to_device(poly), 1 << n, _mont(u))
    ctxs = [zkhip.Ctx(0) for _ in range(parties)]
    cubs = [dp.PolynomialCommitmentCub.new(c, _mont(s)).mature() for c in ctxs]

    def party(net):
        p = net.party_id
        c = ctxs[p]
        d = c.to_device(np.ascontiguousarray(poly[p << m:(p + 1) << m]))
        dC = dp.d_commit(c, cubs[p], d, 1 << m, net)
        val, prf = dp.d_open(c, cubs[p], d, 1 << m, _mont(u), net)
        return np.asarray(dC, dtype=np.uint64), np.asarray(val, dtype=np.uint64), np.asarray(prf, dtype=np.uint64).reshape(-1, 18)

    try:
        res = LocalTestNet.simulate_network_round(parties, party)
    finally:
        for c in ctxs:
            c.close()
    dC, v, pf = res[0]
    assert (v == np.asarray(v_full, dtype=np.uint64)).all() and pf.shape == (n, 18)
    pg2 = pr.powers_of_g2(s)
    vk = dp.pcs_vk(ctx, pg2)
    for Cx in (C_full, dC):
        assert dp.verify_device(ctx, vk, Cx, v, pf, _mont(u)) == dp.verify(pg2, Cx, v, pf, _mont(u))


@pytest.mark.gpu
def test_compiled_host_pcs_verify_matches_the_python_host(ctx):
    """bin/pcs_verify (should_commit_and_open on the C++ host) prints the verdicts the Python host gives for the same seeds"""
    import subprocess

    from zkhip import dist_primitive as dp
    from zkhip.field import int_to_limbs

    host = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
    r = subprocess.run([os.path.join(host, "bin", "pcs_verify"), "--n", "6", "--seed", "502"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = dict(re.findall(r"should_commit_and_open n=6 (\S+): (accept|reject)", r.stdout))
    # the same inputs in Python: zkhost's SplitMix64::fr() takes the raw limbs as the Montgomery form
    n, rng = 6, po.SplitMix64(502)
    raw = lambda k: np.array([int_to_limbs(rng.fr(), 4) for _ in range(k)], dtype=np.uint64).reshape(-1, 4)
    s, u, poly, poly2 = raw(n), raw(n), raw(1 << n), raw(1 << n)
    cub = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    C = np.asarray(dp.commit(ctx, cub, ctx.to_device(poly), 1 << n), dtype=np.uint64)
    C2 = np.asarray(dp.commit(ctx, cub, ctx.to_device(poly2), 1 << n), dtype=np.uint64)
    v, pf = dp.open_(ctx, cub, ctx.to_device(poly), 1 << n, u)
    op = (C, np.asarray(v, dtype=np.uint64), np.asarray(pf, dtype=np.uint64).reshape(n, 18), u)
    pg2 = pr.powers_of_g2([po.fr_from_mont_limbs(x) for x in s])
    muts = _mutations(op, (C2,))
    names = {"honest": op, "value+1": muts["value+1"], "proof+g1": muts["proof+g1"], "point_reversed": muts["point reversed"],
             "other_commitment": muts["other commitment"], "proof_at_infinity": muts["proof at infinity"]}
    assert set(got) == set(names)
    for k, args in names.items():
        host = dp.verify(pg2, *args)
        assert got[k] == ("accept" if host else "reject"), k
    assert got["honest"] == "accept" and sum(x == "reject" for x in got.values()) == 5
