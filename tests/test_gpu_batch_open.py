"""
Batch opening on the GPU: zk_eq_table_acc, zk_fr_lincomb and zk_sumcheck_multi bit-exact against the big-int model
(batch_open_model.py), the large sizes against existing device code, and the prover / verifier end to end through the device pairing.
Every comparison is bit-exact.
"""
import numpy as np
import pytest

import batch_open_model as bm
import pyoracle as po
from helpers import jac_norm_to_affine, pt_ints, rand_fr

R = po.R_MOD
pytestmark = pytest.mark.gpu
COUNTS = (1, 2, 3, 6, 16)


def _dev(ctx, ints):
    return ctx.to_device(bm.mont(ints))


def _down(buf, n):
    return bm.ints(buf.download((n, 4)))


# ---- zk_eq_table_acc ----
@pytest.mark.parametrize("n", range(0, 15))
def test_eq_table_acc_matches_model(ctx, n):
    rng = po.SplitMix64(40 + n)
    N = 1 << n
    base = rng.fr_vec(N)
    boolean = [(i + n) & 1 for i in range(n)]
    single = [1] * max(n - 1, 0) + [0] * min(n, 1)
    mixed = [rng.fr() if i % 3 else (i // 3) & 1 for i in range(n)]
    for z in (rng.fr_vec(n), boolean, single, mixed):
        for w in (0, 1, R - 1, rng.fr()):
            acc = _dev(ctx, base)
            ctx.eq_table_acc(bm.mont(z).reshape(n, 4), bm.mont([w])[0], acc)
            want = [(b + w * e) % R for b, e in zip(base, bm.eq_table(z))]
            assert _down(acc, N) == want, (n, z[:2], w)
    if n >= 1:  # (1,..,1,0) touches one entry
        acc = _dev(ctx, [0] * N)
        ctx.eq_table_acc(bm.mont(single).reshape(n, 4), bm.mont([5])[0], acc)
        assert _down(acc, N) == [0] * (N - 2) + [5, 0]


@pytest.mark.parametrize("n,J,K", [(1, 1, 3), (6, 3, 7), (11, 4, 9), (13, 2, 5)])
def test_accumulations_in_a_row_equal_the_models_combined_tables(ctx, n, J, K):
    from zkhip import batch_open as bo

    tables, claims, alpha, _ = bm.instance(n, J, K, 500 + n) if n <= 6 else (None, [(k % J, z, 0) for k, z in enumerate(bm.mixed_points(n, K, po.SplitMix64(n)))], po.SplitMix64(n + 1).fr(), None)
    got = bo.combined_eq_tables(ctx, J, n, bm.claims_mont(claims), bm.mont([alpha])[0])
    want = bm.combined_eq_tables(J, n, claims, alpha)
    for j in range(J):
        assert _down(got[j], 1 << n) == want[j], j


# ---- zk_fr_lincomb ----
@pytest.mark.parametrize("count", COUNTS)
def test_fr_lincomb_matches_model(ctx, count):
    for n, seed in ((0, 1), (5, 2), (9, 3)):
        rng = po.SplitMix64(600 + 16 * count + seed)
        N = 1 << n
        tabs = [rng.fr_vec(N) for _ in range(count)]
        if count >= 2:
            tabs[1] = [R - 1] * N
        for coeffs in (rng.fr_vec(count), [R - 1] * count, [0] * count, [1] + [0] * (count - 1)):
            d = [_dev(ctx, t) for t in tabs]
            out = ctx.fr_lincomb(d, bm.mont(coeffs), N)
            assert _down(out, N) == bm.lincomb(coeffs, tabs), (count, n)
            for b, t in zip(d, tabs):
                assert _down(b, N) == t


@pytest.mark.parametrize("count", COUNTS)
def test_fr_lincomb_in_place(ctx, count):
    """d_out may be one of the inputs: the first, a middle and the last table in turn"""
    for n in (0, 7, 12):
        N = 1 << n
        rng = po.SplitMix64(650 + 16 * count + n)
        tabs, coeffs = [rng.fr_vec(N) for _ in range(count)], rng.fr_vec(count)
        want = bm.lincomb(coeffs, tabs)
        for k in sorted({0, count // 2, count - 1}):
            d = [_dev(ctx, t) for t in tabs]
            out = ctx.fr_lincomb(d, bm.mont(coeffs), N, out=d[k])
            assert out is d[k] and _down(d[k], N) == want, (count, n, k)
            for j in range(count):
                if j != k:
                    assert _down(d[j], N) == tabs[j]


@pytest.mark.parametrize("count", COUNTS)
def test_fr_lincomb_2_20_equals_the_chain_of_scale_and_add(ctx, count):
    N = 1 << 20
    d = [ctx.to_device(rand_fr(N, 700 + j)) for j in range(count)]
    coeffs = rand_fr(count, 800 + count)
    got = ctx.fr_lincomb(d, coeffs, N).download((N, 4))
    acc = ctx.fr_scale(d[0], coeffs[0], N)
    for j in range(1, count):
        acc = ctx.fr_add(acc, ctx.fr_scale(d[j], coeffs[j], N), N)
    assert (got == acc.download((N, 4))).all()


# ---- zk_sumcheck_multi ----
def _check_multi(ctx, es, fs, rho, label=""):
    n, count = len(rho), len(es)
    N = 1 << n
    de, df = [_dev(ctx, e) for e in es], [_dev(ctx, f) for f in fs]
    want_rounds, want_le, want_lf = bm.sumcheck_multi(es, fs, rho)
    rounds, le, lf = ctx.sumcheck_multi(de, df, N, bm.mont(rho))
    assert rounds.shape == (n, 3, 4) and le.shape == (count, 4) and lf.shape == (count, 4)
    for i in range(n):
        assert bm.ints(rounds[i]) == want_rounds[i], (label, n, count, i)
    assert bm.ints(le) == want_le and bm.ints(lf) == want_lf, (label, n, count)
    for b, t in zip(de + df, es + fs):
        assert _down(b, N) == t, label  # inputs unchanged


def _rand_tabs(n, count, seed):
    rng = po.SplitMix64(seed)
    return [rng.fr_vec(1 << n) for _ in range(count)], [rng.fr_vec(1 << n) for _ in range(count)], rng.fr_vec(n)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", range(1, 15))
def test_sumcheck_multi_matches_model(ctx, n, count):
    _check_multi(ctx, *_rand_tabs(n, count, 900 + 32 * n + count))


@pytest.mark.parametrize("n", [1, 4, 10, 11])
def test_sumcheck_multi_edge_values(ctx, n):
    N = 1 << n
    for count in (1, 3, 16):
        es, fs, rho = _rand_tabs(n, count, 1300 + n + count)
        _check_multi(ctx, [[0] * N] * count, [[0] * N] * count, rho, "zero")
        _check_multi(ctx, [[R - 1] * N] * count, [[R - 1] * N] * count, rho, "r-1")
        _check_multi(ctx, [[R - 1] * N] * count, [[R - 1] * N] * count, [R - 1] * n, "everything r-1")
        _check_multi(ctx, es, fs, [0] * n, "chal 0")
        _check_multi(ctx, es, fs, [1] * n, "chal 1")
        _check_multi(ctx, es, fs, [(i & 1) for i in range(n)], "chal 0/1")
        _check_multi(ctx, es, fs, [R - 1] * n, "chal r-1")


@pytest.mark.parametrize("local_e", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512])
def test_sumcheck_multi_every_handover_point(ctx, local_e):
    """knob multi_local_e: HBM passes down to tables of local_e elements (1: to the very end; capped by what 2 count tables leave of
    the LDS), the LDS stage takes the rest; knob multi_pass_wg: one and (the default) four workgroups per CU"""
    try:
        ctx.dbg_tune("multi_local_e", local_e)
        for wg in (0, 1):
            ctx.dbg_tune("multi_pass_wg", wg)
            for n, count in ((1, 2), (3, 16), (7, 6), (10, 3), (11, 1)) if wg == 0 else ((10, 2),):
                _check_multi(ctx, *_rand_tabs(n, count, 3000 + 16 * n + local_e), f"local_e={local_e} wg={wg}")
    finally:
        ctx.dbg_tune("multi_local_e", 512)
        ctx.dbg_tune("multi_pass_wg", 0)


@pytest.mark.parametrize("n", [1, 2, 9, 10, 13, 18])
def test_count_one_is_sumcheck_product_bit_for_bit(ctx, n):
    N = 1 << n
    e, f, rho = ctx.to_device(rand_fr(N, 50 + n)), ctx.to_device(rand_fr(N, 60 + n)), rand_fr(n, 70 + n)
    tr, lf, lg = ctx.sumcheck_product(e, f, N, rho)
    rounds, le, lff = ctx.sumcheck_multi([e], [f], N, rho)
    assert (rounds == tr).all() and (le[0] == lf).all() and (lff[0] == lg).all()


def _big(ctx, n, count, seed):
    """no big-int model: the triples are the field sum over j of zk_sumcheck_product, the last values zk_fold of each table"""
    from zkhip.field import fr_sum_mont

    N = 1 << n
    rho = rand_fr(n, seed)
    de = [ctx.to_device(rand_fr(N, seed + 1 + j)) for j in range(count)]
    df = [ctx.to_device(rand_fr(N, seed + 101 + j)) for j in range(count)]
    rounds, le, lf = ctx.sumcheck_multi(de, df, N, rho)
    per = [ctx.sumcheck_product(e, f, N, rho) for e, f in zip(de, df)]
    assert (rounds == fr_sum_mont(np.stack([p[0] for p in per]))).all()
    for j in range(count):
        assert (le[j] == per[j][1]).all() and (lf[j] == per[j][2]).all()
        assert (le[j] == ctx.fold(de[j], N, rho).download((1, 4))[0]).all()
        assert (lf[j] == ctx.fold(df[j], N, rho).download((1, 4))[0]).all()


@pytest.mark.parametrize("count", [3, 6])
def test_sumcheck_multi_n20_equals_the_sum_of_product_sumchecks(ctx, count):
    _big(ctx, 20, count, 8100 + count)


@pytest.mark.parametrize("count", [3, 6])
def test_sumcheck_multi_n24_equals_the_sum_of_product_sumchecks(ctx, count):
    n = 24
    need = (2 * count * (32 << n)) * 2 + (2 << 30)  # the tables, as much again in ping-pong scratch and folds, and headroom
    free, _total = ctx.mem_info()
    if free < need:
        pytest.skip(f"needs {need >> 30} GiB of free device memory, {free >> 30} GiB free")
    _big(ctx, n, count, 8200 + count)


def test_sumcheck_multi_errors_leave_outputs_untouched(ctx):
    import ctypes

    import zkhip
    from zkhip.api import _h, _ptr

    n = 4
    d = ctx.to_device(rand_fr(1 << n, 1))
    chal = rand_fr(n, 2)
    out = np.full((n, 3, 4), 0xA5, dtype=np.uint64)
    le, lf = np.full((16, 4), 0xA5, dtype=np.uint64), np.full((16, 4), 0xA5, dtype=np.uint64)

    def arr(count, hole=None):
        a = (ctypes.c_void_p * max(count, 1))()
        for i in range(count):
            a[i] = None if i == hole else _ptr(d)
        return a

    def call(count, N, e=None, f=None, ch=chal, o=out, a=le, b=lf):
        return ctx.lib.zk_sumcheck_multi(ctx.h, count, e if e is not None else arr(min(count, 17)), f if f is not None else arr(min(count, 17)), N,
                                         None if ch is None else _h(ch), None if o is None else _h(o), None if a is None else _h(a), None if b is None else _h(b))

    assert call(0, 1 << n) == -1 and call(17, 1 << n) == -1
    for N in (0, 1, 3, 12, 17):
        assert call(2, N) == -1, N
    assert call(16, 1 << 30) == -1 and call(1, 1 << 34) == -1  # count * len > 2^33
    assert call(3, 1 << n, e=arr(3, hole=1)) == -1 and call(3, 1 << n, f=arr(3, hole=2)) == -1
    assert ctx.lib.zk_sumcheck_multi(ctx.h, 2, None, arr(2), 1 << n, _h(chal), _h(out), _h(le), _h(lf)) == -1
    assert ctx.lib.zk_sumcheck_multi(ctx.h, 2, arr(2), None, 1 << n, _h(chal), _h(out), _h(le), _h(lf)) == -1
    assert call(2, 1 << n, ch=None) == -1 and call(2, 1 << n, o=None) == -1 and call(2, 1 << n, a=None) == -1 and call(2, 1 << n, b=None) == -1
    assert (out == 0xA5).all() and (le == 0xA5).all() and (lf == 0xA5).all()
    # zk_fr_lincomb / zk_eq_table_acc
    keep = d.download((1 << n, 4))
    co = rand_fr(17, 3)
    assert ctx.lib.zk_fr_lincomb(ctx.h, 0, arr(1), _h(co), 1 << n, _ptr(d)) == -1
    assert ctx.lib.zk_fr_lincomb(ctx.h, 17, arr(17), _h(co), 1 << n, _ptr(d)) == -1
    assert ctx.lib.zk_fr_lincomb(ctx.h, 2, arr(2, hole=1), _h(co), 1 << n, _ptr(d)) == -1
    assert ctx.lib.zk_fr_lincomb(ctx.h, 2, None, _h(co), 1 << n, _ptr(d)) == -1
    assert ctx.lib.zk_fr_lincomb(ctx.h, 2, arr(2), None, 1 << n, _ptr(d)) == -1
    assert ctx.lib.zk_fr_lincomb(ctx.h, 2, arr(2), _h(co), 1 << n, None) == -1
    assert ctx.lib.zk_eq_table_acc(ctx.h, None, n, _h(co), _ptr(d)) == -1
    assert ctx.lib.zk_eq_table_acc(ctx.h, _h(chal), n, None, _ptr(d)) == -1
    assert ctx.lib.zk_eq_table_acc(ctx.h, _h(chal), n, _h(co), None) == -1
    assert ctx.lib.zk_eq_table_acc(ctx.h, _h(chal), 41, _h(co), _ptr(d)) == -1
    ctx.sync()
    assert (d.download((1 << n, 4)) == keep).all()
    with pytest.raises(zkhip.ZkError):
        ctx.sumcheck_multi([d], [d], 12, chal)


# ---- end to end ----
@pytest.mark.parametrize("n", [10, 16])
def test_end_to_end_prove_and_verify(ctx, n):
    from zkhip import batch_open as bo
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip.field import fr_mont

    J, K, N = 4, 9, 1 << n
    tables, pts, alpha, rho, s = bo.random_instance(ctx, n, J, K, 7)
    assert any((z == pts[k - 1][1]).all() for k, (_, z) in enumerate(pts) if k) and (pts[-1][1][:-1] == fr_mont(1)).all() and not pts[-1][1][-1].any()
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    comms = np.stack([dp.commit(ctx, pcs, t, N) for t in tables])
    claims = bo.evaluate_claims(ctx, tables, N, pts)
    # each v_k is the value the existing open_many returns for that claim
    opened = dp.open_many(ctx, pcs, [tables[j] for j, _ in pts], [N] * K, [z for _, z in pts])
    for (_, _, v), (ov, _) in zip(claims, opened):
        assert (np.asarray(ov, dtype=np.uint64).reshape(4) == v).all()
    proof = bo.batch_open_prove(ctx, pcs, tables, N, claims, alpha, rho)
    assert proof["rounds"].shape == (n, 3, 4) and proof["opening"].shape == (n, 18)
    pg2 = pr.powers_of_g2(bm.ints(s))
    vk = dp.pcs_vk(ctx, pg2)
    assert bo.failed_checks(J, claims, proof, alpha, rho) == []
    assert bo.batch_open_verify(ctx, vk, comms, claims, proof, alpha, rho) is True
    # g(rho) from zk_open_rounds equals the value the chain ends in
    e = bo.eq_coefficients(J, claims, alpha, rho)
    g = ctx.fr_lincomb(tables, bm.mont(e), N)
    _q, gv = ctx.open_rounds(g, N, rho)
    ok, y = bo.chain_value(proof, claims, alpha, rho)
    assert ok and bm.ints(gv)[0] == y
    cg = bo.combined_commitment(ctx, comms, claims, alpha, rho)
    assert (cg == dp.commit(ctx, pcs, g, N)).all()

    def host_verdict(cl, p, cm):
        """the same decision with the host big-int pairing on the single opening"""
        good, yy = bo.chain_value(p, cl, alpha, rho)
        return bool(good and dp.verify(pg2, bo.combined_commitment(ctx, cm, cl, alpha, rho), fr_mont(yy), p["opening"], rho))

    assert host_verdict(claims, proof, comms) is True
    clone = lambda p: {"rounds": p["rounds"].copy(), "opening": p["opening"].copy()}
    wrong_v = list(claims)
    wrong_v[4] = (claims[4][0], claims[4][1], fr_mont(bm.ints(claims[4][2])[0] + 1))
    mut_round = clone(proof)
    mut_round["rounds"][n // 2][2] = fr_mont(bm.ints(mut_round["rounds"][n // 2][2])[0] + 1)
    mut_point = clone(proof)
    other = po.g1_add(pt_ints(jac_norm_to_affine(mut_point["opening"][n // 2])), po.G1_GEN)  # another valid curve point
    mut_point["opening"][n // 2] = np.concatenate([np.array(po.fq_to_mont_limbs(other[0]) + po.fq_to_mont_limbs(other[1]), dtype=np.uint64), mut_point["opening"][n // 2][12:]])
    swapped = comms.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    for name, (cl, p, cm) in {"wrong v_k": (wrong_v, proof, comms), "mutated round": (claims, mut_round, comms),
                              "opening proof point replaced": (claims, mut_point, comms), "swapped commitment": (claims, proof, swapped)}.items():
        assert bo.batch_open_verify(ctx, vk, cm, cl, p, alpha, rho) is False, name
        assert host_verdict(cl, p, cm) is False, name
    # the proof-point mutation and the swapped commitment pass the field checks: it is the pairing that rejects them
    assert bo.failed_checks(J, claims, mut_point, alpha, rho) == []
    assert bo.failed_checks(J, wrong_v, proof, alpha, rho) == [1] and bo.failed_checks(J, claims, mut_round, alpha, rho) == [1]


@pytest.mark.parametrize("n", [10, 16])
def test_batched_gate_zerocheck(ctx, n):
    from zkhip import batch_open as bo
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import zerocheck as zc
    from zkhip.field import fr_mont, splitmix_fr

    alpha, rho = splitmix_fr(1, 91)[0], splitmix_fr(n, 92)

    def prove(break_gate=None):
        tables, tau, chal, s = zc.satisfied_circuit(ctx, n, 5, break_gate)
        pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
        return zc.gate_zerocheck_prove_batched(ctx, pcs, tables, tau, chal, alpha, rho), tau, chal, s, (tables, pcs)

    proof, tau, chal, s, (tables, pcs) = prove()
    vk = dp.pcs_vk(ctx, pr.powers_of_g2(bm.ints(s)))
    assert zc.gate_zerocheck_verify_batched(ctx, vk, proof, tau, chal, alpha, rho) is True
    # the same round transcript and commitments as the unbatched proof
    plain = zc.gate_zerocheck_prove(ctx, pcs, tables, tau, chal)
    assert (plain["rounds"] == proof["rounds"]).all()
    for (c, v, _), bc, bv in zip(plain["openings"], proof["commitments"], proof["values"]):
        assert (c == bc).all() and (v == bv).all()
    assert zc.gate_zerocheck_verify_batched(ctx, vk, prove(break_gate=3)[0], tau, chal, alpha, rho) is False
    bad = dict(proof, values=proof["values"].copy())
    bad["values"][2] = fr_mont(bm.ints(bad["values"][2])[0] + 1)
    assert zc.gate_zerocheck_verify_batched(ctx, vk, bad, tau, chal, alpha, rho) is False
    bad = dict(proof, commitments=proof["commitments"][::-1].copy())
    assert zc.gate_zerocheck_verify_batched(ctx, vk, bad, tau, chal, alpha, rho) is False


@pytest.mark.parametrize("mu", [10, 16])
def test_batched_wiring(ctx, mu):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import wiring as wr
    from zkhip.field import fr_mont, splitmix_fr

    b_alpha, rho_mu, rho_mu1 = splitmix_fr(1, 93)[0], splitmix_fr(mu, 94), splitmix_fr(mu + 1, 95)

    def prove(break_wire=None):
        w, sid, ssigma, alpha, beta, gamma, tau, chal, s = wr.permuted_circuit(ctx, mu, 7, break_wire)
        pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
        return wr.wiring_prove_batched(ctx, pcs, w, sid, ssigma, 1 << mu, alpha, beta, gamma, tau, chal, b_alpha, rho_mu, rho_mu1), (alpha, beta, gamma, tau, chal), s

    proof, sc, s = prove()
    vk_mu, vk_mu1 = wr.verifying_keys(ctx, pr.powers_of_g2(bm.ints(s)))
    rest = (b_alpha, rho_mu, rho_mu1)
    assert wr.wiring_verify_batched(ctx, vk_mu, vk_mu1, proof, *sc, *rest) is True
    assert wr.wiring_verify_batched(ctx, vk_mu, vk_mu1, prove(break_wire=5)[0], *sc, *rest) is False
    for key, k in (("values", 1), ("v_values", 2), ("v_values", 4)):
        bad = dict(proof)
        bad[key] = proof[key].copy()
        bad[key][k] = fr_mont(bm.ints(bad[key][k])[0] + 1)
        assert wr.wiring_verify_batched(ctx, vk_mu, vk_mu1, bad, *sc, *rest) is False, (key, k)
    assert wr.wiring_verify_batched(ctx, vk_mu1, vk_mu, proof, *sc, *rest) is False  # the keys the wrong way round
