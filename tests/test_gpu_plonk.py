"""
One-circuit HyperPlonk on the GPU: zk_perm3_terms and zk_sumcheck_perm3 against the big-int model (plonk_model.py), the
transcript-driven form against its preset-challenge parent and a hashlib replay, the error cases, prove / verify end to end
through the device pairing, and the compiled host (host/bin/plonk_check): one digest for one seed.  Every comparison is bit-exact.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import plonk_model as pm
import pyoracle as po
import zerocheck_model as zm
from helpers import rand_fr

R = po.R_MOD
pytestmark = pytest.mark.gpu


def _columns(ctx, mu, seed):
    """three wire columns and three columns of slot numbers on the device, and the same as ints"""
    from zkhip import plonk

    w, ss = pm.random_columns(mu, seed)
    d_w = [ctx.to_device(zm.mont(x)) for x in w]
    d_ss = [plonk.slot_table(ctx, np.array(x, dtype=np.uint64)) for x in ss]
    return w, ss, d_w, d_ss


def _down(buf, n):
    return buf.download((n, 4))


def _big_tables(ctx, mu, seed):
    """eleven random tables for the sizes the model cannot reach: eq, a 2N `tree` (any 2N elements: the identity's rounds are defined
    for any tables), three nums, three dens"""
    N = 1 << mu
    eq, tree = ctx.to_device(rand_fr(N, seed)), ctx.to_device(rand_fr(2 * N, seed + 1))
    nums = [ctx.to_device(rand_fr(N, seed + 2 + j)) for j in range(3)]
    dens = [ctx.to_device(rand_fr(N, seed + 5 + j)) for j in range(3)]
    return eq, tree, nums, dens


@pytest.mark.parametrize("mu", range(1, 11))
def test_terms_and_sumcheck_against_the_model(ctx, mu):
    N = 1 << mu
    w, ss, d_w, d_ss = _columns(ctx, mu, 60 + mu)
    alpha, beta, gamma = po.SplitMix64(mu).fr_vec(3)
    tau, chal = po.SplitMix64(100 + mu).fr_vec(mu), po.SplitMix64(200 + mu).fr_vec(mu)
    before = [_down(b, N) for b in d_w + d_ss]
    nums, dens, P, Q = ctx.perm3_terms(d_w, d_ss, N, zm.mont([alpha])[0], zm.mont([beta])[0])
    n, d, mP, mQ, h = pm.terms(w, ss, alpha, beta)
    for j in range(3):
        assert (_down(nums[j], N) == zm.mont(n[j])).all() and (_down(dens[j], N) == zm.mont(d[j])).all(), j
    assert (_down(P, N) == zm.mont(mP)).all() and (_down(Q, N) == zm.mont(mQ)).all()
    d_h = ctx.fr_batch_div(P, Q, N)
    assert (_down(d_h, N) == zm.mont(h)).all()
    tree = ctx.product_tree(d_h, N)
    tabs, m_tree = pm.tables(w, ss, alpha, beta, tau)
    assert (_down(tree, 2 * N) == zm.mont(m_tree)).all()
    eq = ctx.eq_table(zm.mont(tau))
    ins = [eq, tree] + nums + dens
    snap = [_down(b, 2 * N if b is tree else N) for b in ins]
    rounds, last = ctx.sumcheck_perm3(eq, tree, nums, dens, N, zm.mont([gamma])[0], zm.mont(chal))
    m_rounds, m_last = pm.sumcheck_perm3(tabs, gamma, chal)
    assert (rounds == np.stack([zm.mont(p) for p in m_rounds])).all()
    assert (last == zm.mont(m_last)).all()
    # inputs unchanged after the calls
    for b, s in zip(ins, snap):
        assert (_down(b, len(s)) == s).all()
    for b, s in zip(d_w + d_ss, before):
        assert (_down(b, N) == s).all()


@pytest.mark.parametrize("mu", [3, 9, 12, 15])
def test_hand_over_knob(ctx, mu):
    N = 1 << mu
    eq, tree, nums, dens = _big_tables(ctx, mu, 7 * mu)
    gamma, chal = rand_fr(1, 3)[0], rand_fr(mu, 4)
    got = {}
    try:
        for e in (1, 16, 256):
            ctx.dbg_tune("perm3_local_e", e)
            got[e] = ctx.sumcheck_perm3(eq, tree, nums, dens, N, gamma, chal)
    finally:
        ctx.dbg_tune("perm3_local_e", 256)
    for e in (1, 16):
        assert (got[e][0] == got[256][0]).all() and (got[e][1] == got[256][1]).all(), e


@pytest.mark.parametrize("mu", range(1, 21))
def test_fs_form_equals_its_parent_and_a_hashlib_replay(ctx, mu):
    from zkhip.transcript import HostTranscript, Transcript

    N = 1 << mu
    eq, tree, nums, dens = _big_tables(ctx, mu, 11 * mu)
    gamma = rand_fr(1, mu)[0]
    seed = bytes([mu]) * 5
    tr, h = Transcript(ctx, b"perm3"), HostTranscript(b"perm3")
    try:
        tr.absorb(seed), h.absorb(seed)
        rounds, last, chal = ctx.sumcheck_perm3_fs(eq, tree, nums, dens, N, gamma, tr)
        want = np.stack([h.absorb(r).challenge() for r in rounds])  # round i absorbed, challenge i drawn
        assert (chal == want).all()
        assert tr.state() == h.state()
        assert (tr.challenges(2) == h.challenges(2)).all()
    finally:
        tr.free()
    p_rounds, p_last = ctx.sumcheck_perm3(eq, tree, nums, dens, N, gamma, chal)
    assert (rounds == p_rounds).all() and (last == p_last).all()
    if mu in (9, 13):  # the hand-over knob moves no bit of the derived form either
        try:
            ctx.dbg_tune("perm3_local_e", 1)
            tr = Transcript(ctx, b"perm3")
            tr.absorb(seed)
            again = ctx.sumcheck_perm3_fs(eq, tree, nums, dens, N, gamma, tr)
            tr.free()
        finally:
            ctx.dbg_tune("perm3_local_e", 256)
        assert all((x == y).all() for x, y in zip(again, (rounds, last, chal)))


def test_error_cases(ctx):
    import zkhip
    from zkhip._lib import ZK_ERR_INVALID
    from zkhip.transcript import Transcript

    mu = 4
    N = 1 << mu
    eq, tree, nums, dens = _big_tables(ctx, mu, 5)
    gamma, chal = rand_fr(1, 3)[0], rand_fr(mu, 4)
    w = [ctx.to_device(rand_fr(N, 20 + j)) for j in range(3)]
    tr = Transcript(ctx, b"err")
    state = tr.state()

    def invalid(call):
        with pytest.raises(zkhip.ZkError) as e:
            call()
        assert e.value.code == ZK_ERR_INVALID

    for bad_n in (0, 1, 3, 12, 1 << 36):  # not a power of two >= 2; longer than the sums can hold
        invalid(lambda: ctx.sumcheck_perm3(eq, tree, nums, dens, bad_n, gamma, rand_fr(40, 1)))
        invalid(lambda: ctx.sumcheck_perm3_fs(eq, tree, nums, dens, bad_n, gamma, tr))
        if bad_n < N:
            invalid(lambda: ctx.perm3_terms(w, w, bad_n, gamma, gamma))
    arr = lambda bufs: (ctypes.c_void_p * 3)(*[b.ptr for b in bufs])  # the wrapper would allocate the outputs: 2^36 elements straight through the ABI
    assert ctx.lib.zk_perm3_terms(ctx.h, arr(w), arr(w), 1 << 36, gamma.ctypes.data, gamma.ctypes.data, arr(nums), arr(dens), eq.ptr, tree.ptr) == ZK_ERR_INVALID
    for k in range(3):  # a null pointer
        holed = list(nums)
        holed[k] = None
        invalid(lambda: ctx.sumcheck_perm3(eq, tree, holed, dens, N, gamma, chal))
        invalid(lambda: ctx.sumcheck_perm3(eq, tree, nums, holed, N, gamma, chal))
        invalid(lambda: ctx.sumcheck_perm3_fs(eq, tree, holed, dens, N, gamma, tr))
        invalid(lambda: ctx.perm3_terms(holed, w, N, gamma, gamma))
    invalid(lambda: ctx.sumcheck_perm3(None, tree, nums, dens, N, gamma, chal))
    invalid(lambda: ctx.sumcheck_perm3(eq, None, nums, dens, N, gamma, chal))
    invalid(lambda: ctx.sumcheck_perm3_fs(eq, tree, nums, dens, N, gamma, None))  # a null transcript
    try:  # a knob out of range
        for e in (0, 3, 512):
            ctx.dbg_tune("perm3_local_e", e)
            invalid(lambda: ctx.sumcheck_perm3(eq, tree, nums, dens, N, gamma, chal))
            invalid(lambda: ctx.sumcheck_perm3_fs(eq, tree, nums, dens, N, gamma, tr))
    finally:
        ctx.dbg_tune("perm3_local_e", 256)
    assert tr.state() == state  # nothing was absorbed by the failed calls
    tr.free()
    # a zero denominator: Q with a zero entry
    zq = rand_fr(N, 9)
    zq[5] = 0
    with pytest.raises(ZeroDivisionError):
        ctx.fr_batch_div(nums[0], ctx.to_device(zq), N)
    ctx.sumcheck_perm3(eq, tree, nums, dens, N, gamma, chal)  # the ctx still works


def _setup(ctx, mu, seed, **kw):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    c = plonk.sample_circuit(mu, seed, **kw)
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
    return c, pk, vk


@pytest.mark.parametrize("mu", [4, 10, 14, 20])
def test_prove_verify_end_to_end(ctx, mu):
    from zkhip import plonk

    c, pk, vk = _setup(ctx, mu, 7)
    pi = c["public_inputs"]
    proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi)
    assert plonk.field_checks(vk, pi, proof) is True
    assert plonk.verify(ctx, vk, pi, proof) is True
    if mu == 4:  # the big-int model on the same tables and commitments: the same rounds, values and (so) challenges
        m = pm.prove(pm.circuit_ints(c), mu, c["l"], vk["commitments"], proof["commitments"], lambda tree: proof["v_commitment"])
        assert pm.field_digest(pm.record(m, proof["commitments"])) == pm.field_digest(proof)
        assert plonk.field_checks(vk, pi, proof, zm.mont(m["finals"]), zm.mont(m["v_finals"])) is True
    if mu <= 14:
        assert plonk.proof_digest(plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi)) == plonk.proof_digest(proof)  # deterministic
    N = 1 << mu
    for kw in ({"break_gate": N - 3}, {"break_wire": N - 3}):
        bc = plonk.sample_circuit(mu, 7, **kw)
        bad = plonk.prove(ctx, pk, bc["a"], bc["b"], bc["c"], pi)
        assert plonk.field_checks(vk, pi, bad) is False and plonk.verify(ctx, vk, pi, bad) is False, kw
    wrong = np.array(pi, copy=True)
    wrong[1, 0] ^= np.uint64(1)
    assert plonk.field_checks(vk, wrong, proof) is False and plonk.verify(ctx, vk, wrong, proof) is False
    assert plonk.verify(ctx, vk, pi, plonk.prove(ctx, pk, c["a"], c["b"], c["c"], wrong)) is False  # the prover's `in` disagrees with the wires

    def flip(a, idx):
        a = np.array(a, dtype=np.uint64, copy=True)
        a.reshape(-1)[idx] ^= np.uint64(1)
        return a

    for key in pm.FIELD_PARTS:  # a flipped limb of each record field
        bad = dict(proof, **{key: flip(proof[key], np.asarray(proof[key]).size // 2)})
        assert plonk.field_checks(vk, pi, bad) is False and plonk.verify(ctx, vk, pi, bad) is False, key
    for b in ("batch", "v_batch"):
        bad = dict(proof, **{b: dict(proof[b], rounds=flip(proof[b]["rounds"], 5))})
        assert plonk.field_checks(vk, pi, bad) is False and plonk.verify(ctx, vk, pi, bad) is False, b
        # the opening proof: the field part cannot see it, the pairing does
        op = np.array(proof[b]["opening"], copy=True)
        op[0] = op[-1]  # (another valid point: a flipped limb would leave the curve)
        bad = dict(proof, **{b: dict(proof[b], opening=op)})
        assert plonk.field_checks(vk, pi, bad) is True and plonk.verify(ctx, vk, pi, bad) is False, b
    if mu <= 14:
        _c2, _pk2, vk2 = _setup(ctx, mu, 8)  # the vk of another seed
        assert plonk.verify(ctx, vk2, pi, proof) is False


# ---- the compiled host ----
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
PLONK_CHECK = os.path.join(HOST, "bin", "plonk_check")


def _plonk_check(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/plonk_check"])
    r = subprocess.run([PLONK_CHECK, *args], capture_output=True, text=True, timeout=600)
    m = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout)
    return r, m.group(1) if m else None


@pytest.mark.parametrize("mu,seed", [(2, 3), (4, 7), (10, 7), (14, 2)])
def test_python_and_cpp_digests_agree(ctx, mu, seed):
    from zkhip import plonk

    r, got = _plonk_check("--mu", str(mu), "--seed", str(seed))
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    c, pk, vk = _setup(ctx, mu, seed)
    proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"])
    assert plonk.proof_digest(proof) == got
    assert plonk.verify(ctx, vk, c["public_inputs"], proof) is True


def test_plonk_check_rejects_broken_circuits_and_a_bad_input(ctx):
    from zkhip import plonk

    mu, seed = 10, 7
    c, pk, _vk = _setup(ctx, mu, seed)
    for flag, kw in ((("--break-gate", "700"), {"break_gate": 700}), (("--break-wire", "700"), {"break_wire": 700}), (("--bad-input",), {})):
        r, got = _plonk_check("--mu", str(mu), "--seed", str(seed), *flag)
        assert r.returncode == 1 and "reject" in r.stdout and got, (flag, r.returncode, r.stdout, r.stderr)
        bc = plonk.sample_circuit(mu, seed, **kw)  # the broken record is the same record in both hosts
        assert plonk.proof_digest(plonk.prove(ctx, pk, bc["a"], bc["b"], bc["c"], c["public_inputs"])) == got, flag
