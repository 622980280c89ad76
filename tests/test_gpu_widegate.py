"""
The wide Plonk gate on the GPU: zk_sumcheck_gate_wide against the big-int model (widegate_model.py), the hand-over knob, the
grid-stride path against what a verifier checks, edge values, the transcript-driven form against its parent and a hashlib replay, the
error cases, prove / verify of the wide kind end to end, and the compiled host (host/bin/plonk_check --gate wide): one digest for one
seed.  Every comparison is bit-exact.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
import widegate_model as wg
import zerocheck_model as zm
from helpers import rand_fr

R = po.R_MOD
pytestmark = pytest.mark.gpu
# zkhip.plonk.proof_digest of the basic kind's proof for (mu, seed) = (4, 7), as both hosts computed it on the commit before the wide gate
BASIC_DIGEST_4_7 = "d3bcfbe650d5d85333fb1ed13a9a9bf34a311a2b31f5f671ac1be949075834cc"


@functools.lru_cache(maxsize=None)
def _model(mu):
    """random tables, challenges and the model's run, once per size"""
    tabs = wg.random_tables(mu, 60 + mu)
    chal = po.SplitMix64(200 + mu).fr_vec(mu)
    rounds, last = wg.sumcheck_gate_wide(tabs, chal)
    return tabs, chal, np.stack([zm.mont(p) for p in rounds]), zm.mont(last)


def _upload(ctx, tabs):
    return [ctx.to_device(zm.mont(tabs[k])) for k in wg.TABLES]


def _rand_tables(ctx, mu, seed):
    return [ctx.to_device(rand_fr(1 << mu, seed + k)) for k in range(11)]


@pytest.mark.parametrize("mu", range(1, 11))
def test_sumcheck_against_the_model(ctx, mu):
    """mu <= 8: the local stage alone; 9 and 10: one and two HBM passes, then the hand-over"""
    N = 1 << mu
    tabs, chal, m_rounds, m_last = _model(mu)
    d = _upload(ctx, tabs)
    snap = [b.download((N, 4)) for b in d]
    rounds, last = ctx.sumcheck_gate_wide(d, N, zm.mont(chal))
    assert rounds.shape == (mu, 8, 4) and (rounds == m_rounds).all()
    assert (last == m_last).all()
    for b, s in zip(d, snap):  # inputs unchanged
        assert (b.download((N, 4)) == s).all()


@pytest.mark.parametrize("mu", [3, 9, 12])
def test_hand_over_knob(ctx, mu):
    N = 1 << mu
    if mu <= 10:
        tabs, chal, m_rounds, m_last = _model(mu)
        d, chal = _upload(ctx, tabs), zm.mont(chal)
    else:
        d, chal = _rand_tables(ctx, mu, 7 * mu), rand_fr(mu, 4)
    got = {}
    try:
        for e in (1, 4, 256):
            ctx.dbg_tune("gatew_local_e", e)
            got[e] = ctx.sumcheck_gate_wide(d, N, chal)
    finally:
        ctx.dbg_tune("gatew_local_e", 256)
    for e in (1, 4):
        assert (got[e][0] == got[256][0]).all() and (got[e][1] == got[256][1]).all(), e
    if mu <= 10:
        assert (got[256][0] == m_rounds).all() and (got[256][1] == m_last).all()


def test_grid_stride_and_many_passes_as_a_verifier_sees_them(ctx):
    from zkhip import plonk
    from zkhip.zerocheck import _ints, wide_gate_value

    mu = 18
    N = 1 << mu
    d, chal = _rand_tables(ctx, mu, 900), rand_fr(mu, 5)
    rounds, last = ctx.sumcheck_gate_wide(d, N, chal)
    # the claimed sum from the existing element-wise calls and a host sum (Montgomery forms add like the values they stand for)
    eq, qL, qR, qM, qO, qC, qH, a, b, c, inp = d
    mul, add = (lambda x, y: ctx.fr_mul(x, y, N)), (lambda x, y: ctx.fr_add(x, y, N))
    a2 = mul(a, a)
    a5 = mul(mul(a2, a2), a)
    br = add(add(add(mul(qL, a), mul(qR, b)), add(mul(mul(qM, a), b), mul(qH, a5))), add(qC, inp))
    w = mul(eq, ctx.fr_sub(br, mul(qO, c), N))
    raw = np.ascontiguousarray(w.download((N, 4)), dtype="<u8").tobytes()
    total = sum(int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)) % R
    target = total * pow(1 << 256, -1, R) % R
    r = _ints(chal)
    for i in range(mu):  # the chain on the nodes 0 .. 7
        p = _ints(rounds[i])
        assert (p[0] + p[1]) % R == target, i
        target = plonk.round_poly_at(p, r[i])
    assert target == wide_gate_value(*_ints(last))
    for k in range(11):  # each folded-out value is the existing fold of its table by the same challenges
        assert (ctx.fold(d[k], N, chal).download((1, 4))[0] == last[k]).all(), k


@pytest.mark.parametrize("case", ["zeros", "r_minus_1", "a_and_qH_r_minus_1"])
def test_edge_values(ctx, case):
    mu = 9
    N = 1 << mu
    tabs, chal, _r, _l = _model(mu)
    if case == "zeros":
        tabs = {k: [0] * N for k in wg.TABLES}
    elif case == "r_minus_1":
        tabs = {k: [R - 1] * N for k in wg.TABLES}
    else:
        tabs = dict(tabs, a=[R - 1] * N, qH=[R - 1] * N)
    m_rounds, m_last = wg.sumcheck_gate_wide(tabs, chal)
    rounds, last = ctx.sumcheck_gate_wide(_upload(ctx, tabs), N, zm.mont(chal))
    assert (rounds == np.stack([zm.mont(p) for p in m_rounds])).all() and (last == zm.mont(m_last)).all()


@pytest.mark.parametrize("mu", list(range(1, 13)) + [18])
def test_fs_form_equals_its_parent_and_a_hashlib_replay(ctx, mu):
    from zkhip.transcript import HostTranscript, Transcript

    N = 1 << mu
    d = _upload(ctx, _model(mu)[0]) if mu <= 10 else _rand_tables(ctx, mu, 11 * mu)
    seed = bytes([mu]) * 5
    tr, h = Transcript(ctx, b"gatew"), HostTranscript(b"gatew")
    try:
        tr.absorb(seed), h.absorb(seed)
        rounds, last, chal = ctx.sumcheck_gate_wide_fs(d, N, tr)
        want = np.stack([h.absorb(r).challenge() for r in rounds])  # round i's eight evaluations absorbed as they sit in the output
        assert (chal == want).all()
        assert tr.state() == h.state()
    finally:
        tr.free()
    p_rounds, p_last = ctx.sumcheck_gate_wide(d, N, chal)
    assert (rounds == p_rounds).all() and (last == p_last).all()
    if mu <= 10:
        m_rounds, m_last = wg.sumcheck_gate_wide(_model(mu)[0], zm.ints(chal))
        assert (rounds == np.stack([zm.mont(p) for p in m_rounds])).all() and (last == zm.mont(m_last)).all()


def test_error_cases(ctx):
    import zkhip
    from zkhip._lib import ZK_ERR_INVALID
    from zkhip.transcript import Transcript

    mu = 4
    N = 1 << mu
    d, chal = _rand_tables(ctx, mu, 5), rand_fr(40, 4)
    other = zkhip.Ctx(0)
    tr, foreign = Transcript(ctx, b"err"), Transcript(other, b"err")
    state = tr.state()
    ptrs = lambda bufs: (ctypes.c_void_p * 11)(*[None if b is None else b.ptr for b in bufs])
    PAT = np.uint64(0xA5A5A5A5A5A5A5A5)

    def invalid(tabs, n, chal_ptr=chal.ctypes.data, transcript=tr):
        """both entry points straight through the ABI: ZK_ERR_INVALID, the outputs untouched"""
        for fs in (False, True):
            out, last, cout = np.full((40, 8, 4), PAT), np.full((11, 4), PAT), np.full((40, 4), PAT)
            if fs:
                rc = ctx.lib.zk_sumcheck_gate_wide_fs(ctx.h, tabs, n, getattr(transcript, "h", None), out.ctypes.data, last.ctypes.data, cout.ctypes.data)
            else:
                rc = ctx.lib.zk_sumcheck_gate_wide(ctx.h, tabs, n, chal_ptr, out.ctypes.data, last.ctypes.data)
            assert rc == ZK_ERR_INVALID, (fs, n)
            assert (out == PAT).all() and (last == PAT).all() and (cout == PAT).all()

    for bad_n in (0, 1, 3, 12, 1 << 36):  # < 2, not a power of two, longer than the sums can hold
        invalid(ptrs(d), bad_n)
    for k in range(11):  # a null table
        invalid(ptrs(d[:k] + [None] + d[k + 1:]), N)
    invalid(None, N)
    out, last = np.full((mu, 8, 4), PAT), np.full((11, 4), PAT)
    assert ctx.lib.zk_sumcheck_gate_wide(ctx.h, ptrs(d), N, None, out.ctypes.data, last.ctypes.data) == ZK_ERR_INVALID  # null challenges
    assert ctx.lib.zk_sumcheck_gate_wide(ctx.h, ptrs(d), N, chal.ctypes.data, None, last.ctypes.data) == ZK_ERR_INVALID
    assert ctx.lib.zk_sumcheck_gate_wide(ctx.h, ptrs(d), N, chal.ctypes.data, out.ctypes.data, None) == ZK_ERR_INVALID
    assert ctx.lib.zk_sumcheck_gate_wide_fs(ctx.h, ptrs(d), N, tr.h, out.ctypes.data, last.ctypes.data, None) == ZK_ERR_INVALID
    assert (out == PAT).all() and (last == PAT).all()
    for t in (None, foreign):  # a null transcript, the transcript of another ctx
        with pytest.raises(zkhip.ZkError) as e:
            ctx.sumcheck_gate_wide_fs(d, N, t)
        assert e.value.code == ZK_ERR_INVALID
    try:  # a knob out of range
        for e in (0, 3, 512):
            ctx.dbg_tune("gatew_local_e", e)
            invalid(ptrs(d), N)
    finally:
        ctx.dbg_tune("gatew_local_e", 256)
    assert tr.state() == state  # nothing was absorbed by the failed calls
    with pytest.raises(ValueError):
        ctx.sumcheck_gate_wide(d[:10], N, chal)
    # the ctx is usable afterwards
    rounds, last, got = ctx.sumcheck_gate_wide_fs(d, N, tr)
    p_rounds, p_last = ctx.sumcheck_gate_wide(d, N, got)
    assert (rounds == p_rounds).all() and (last == p_last).all()
    tr.free(), foreign.free()
    other.close()


def _setup(ctx, mu, seed, wide=True, **kw):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import plonk

    c = (plonk.sample_circuit_wide if wide else plonk.sample_circuit)(mu, seed, **kw)
    pcs = dp.PolynomialCommitmentCub.new(ctx, c["s"]).mature()
    pk, vk = plonk.preprocess(ctx, pcs, c, pr.powers_of_g2(zm.ints(c["s"])))
    return c, pk, vk


@pytest.mark.parametrize("mu", [4, 10, 14])
def test_prove_verify_end_to_end(ctx, mu):
    from zkhip import plonk

    c, pk, vk = _setup(ctx, mu, 7)
    pi = c["public_inputs"]
    assert vk["gate"] == "wide" and vk["commitments"].shape == (9, 18)
    proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], pi)
    assert proof["gate"] == "wide" and proof["g_rounds"].shape == (mu, 8, 4) and np.asarray(proof["g_values"]).shape == (9, 4)
    assert plonk.field_checks(vk, pi, proof) is True
    assert plonk.verify(ctx, vk, pi, proof) is True
    if mu == 4:  # the big-int model on the same tables and commitments: the same rounds, values and (so) challenges
        import plonk_model as pm

        m = wg.prove(wg.circuit_ints(c), mu, c["l"], vk["commitments"], proof["commitments"], lambda tree: proof["v_commitment"])
        assert pm.field_digest(wg.record(m, proof["commitments"])) == pm.field_digest(proof)
        finals, v_finals = zm.mont(m["finals"]), zm.mont(m["v_finals"])
        assert plonk.field_checks(vk, pi, proof, finals, v_finals) is True  # field_checks with finals agrees with verify
        bad_finals = np.array(finals, copy=True)
        bad_finals[5, 0] ^= np.uint64(1)
        assert plonk.field_checks(vk, pi, proof, bad_finals, v_finals) is False
    N = 1 << mu
    for kw in ({"break_gate": N - 3}, {"break_wire": N - 3}):
        bc = plonk.sample_circuit_wide(mu, 7, **kw)
        bad = plonk.prove(ctx, pk, bc["a"], bc["b"], bc["c"], pi)
        assert plonk.field_checks(vk, pi, bad) is False and plonk.verify(ctx, vk, pi, bad) is False, kw
    wrong = np.array(pi, copy=True)
    wrong[1, 0] ^= np.uint64(1)
    assert plonk.field_checks(vk, wrong, proof) is False and plonk.verify(ctx, vk, wrong, proof) is False

    def flip(a, idx):
        a = np.array(a, dtype=np.uint64, copy=True)
        a.reshape(-1)[idx] ^= np.uint64(1)
        return a

    for key, idx in (("g_rounds", ((mu - 1) * 8 + 7) * 4), ("g_values", 5 * 4)):  # one limb of g_rounds[mu - 1][7], of g_values[5] = qH
        bad = dict(proof, **{key: flip(proof[key], idx)})
        assert plonk.field_checks(vk, pi, bad) is False and plonk.verify(ctx, vk, pi, bad) is False, key
    _bc, _bpk, b_vk = _setup(ctx, mu, 7, wide=False)  # a basic vk
    assert plonk.failed_checks(b_vk, pi, proof) == [0] and plonk.verify(ctx, b_vk, pi, proof) is False


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

    r, got = _plonk_check("--mu", str(mu), "--seed", str(seed), "--gate", "wide")
    assert r.returncode == 0 and "gate=wide: accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    c, pk, vk = _setup(ctx, mu, seed)
    proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"])
    assert plonk.proof_digest(proof) == got
    assert plonk.verify(ctx, vk, c["public_inputs"], proof) is True


def test_plonk_check_rejects_broken_circuits_and_a_bad_input(ctx):
    from zkhip import plonk

    mu, seed = 10, 7
    c, pk, _vk = _setup(ctx, mu, seed)
    for flag, kw in ((("--break-gate", "5"), {"break_gate": 5}), (("--break-wire", "9"), {"break_wire": 9}), (("--bad-input",), {})):
        r, got = _plonk_check("--mu", str(mu), "--seed", str(seed), "--gate", "wide", *flag)
        assert r.returncode == 1 and "reject" in r.stdout and got, (flag, r.returncode, r.stdout, r.stderr)
        bc = plonk.sample_circuit_wide(mu, seed, **kw)  # the broken record is the same record in both hosts
        assert plonk.proof_digest(plonk.prove(ctx, pk, bc["a"], bc["b"], bc["c"], c["public_inputs"])) == got, flag


def test_basic_kind_digest_is_pinned_in_both_hosts(ctx):
    from zkhip import plonk

    r, got = _plonk_check("--mu", "4", "--seed", "7")
    assert r.returncode == 0 and r.stdout.endswith("plonk_check mu=4 N=16 l=4 seed=7: accept\n"), (r.returncode, r.stdout, r.stderr)
    c, pk, vk = _setup(ctx, 4, 7, wide=False)
    proof = plonk.prove(ctx, pk, c["a"], c["b"], c["c"], c["public_inputs"])
    assert "gate" not in proof and "gate" not in vk
    assert plonk.proof_digest(proof) == got == BASIC_DIGEST_4_7
