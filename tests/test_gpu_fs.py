"""
Fiat-Shamir on the GPU: the device transcript against hashlib, the three transcript-driven sumchecks against their preset-challenge
parents (the challenges a call derived, fed to the parent, give the same rounds and last values), and the non-interactive provers and
verifiers end to end through the device pairing and against the compiled host.  Every comparison is bit-exact.  The model states
everything of a record but the commitments and the opening proofs (no curve arithmetic there): it is given the commitments and the
records are compared through fs_model.field_digest; the opening proofs are covered by the pairing and by the other host's digest.
"""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import fs_model as fm
import pyoracle as po
import zerocheck_model as zm
from helpers import rand_fr

R = po.R_MOD
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scalable-collaborative-zksnark_amd", "host")
NI_CHECK = os.path.join(HOST, "bin", "ni_check")
pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 22, 23, 54, 55, 56, 63, 64, 119, 120)
SIZES = (1, 2, 8, 9, 10, 11, 13, 16, 20)


def _data(n, salt=0):
    return bytes((11 * i + 5 + salt) & 0xFF for i in range(n))


# ---- the device transcript ----
def test_device_transcript_host_absorbs(ctx):
    from zkhip.transcript import HostTranscript, Transcript

    for label in (b"", b"gate", b"a label of more than fifty-five bytes, so that init takes two compressions"):
        d, h = Transcript(ctx, label), HostTranscript(label)
        assert d.state() == h.state() == hashlib.sha256(b"zkhip-fs-v1" + label).digest()
        for n in LENGTHS + (2048, 2049, 5000):  # 2049 on: the staged path
            data = _data(n, len(label))
            d.absorb(data), h.absorb(data)
            assert d.state() == h.state(), (label, n)
        assert (d.challenges(5) == h.challenges(5)).all() and d.state() == h.state()
        d.free()


def test_device_transcript_device_absorbs_and_interleaving(ctx):
    from zkhip.transcript import HostTranscript, Transcript

    d, h = Transcript(ctx, b"dev"), HostTranscript(b"dev")
    blob = np.frombuffer(_data(4096), dtype=np.uint8)
    buf = ctx.to_device(blob)
    for k, n in enumerate(LENGTHS + (4096,)):
        d.absorb_device(buf, n), h.absorb(blob[:n].tobytes())
        got, want = d.challenges(k % 3), h.challenges(k % 3)  # interleaved absorbs and challenges (sometimes none)
        assert (got == want).all() and d.state() == h.state(), n
        d.absorb_u64(n), h.absorb_u64(n)
    elems = rand_fr(7, 3)
    d.absorb(elems), h.absorb(elems)
    c = d.challenges(40)
    assert (c == h.challenges(40)).all()
    assert all(x < 1 << 254 for x in zm.ints(c))
    d.free()


def test_two_transcripts_on_one_ctx(ctx):
    from zkhip.transcript import HostTranscript, Transcript

    d1, d2, h1, h2 = Transcript(ctx, b"one"), Transcript(ctx, b"two"), HostTranscript(b"one"), HostTranscript(b"two")
    for i in range(6):
        (d1 if i & 1 else d2).absorb(_data(30 + i))
        (h1 if i & 1 else h2).absorb(_data(30 + i))
        assert (d1.challenge() == h1.challenge()).all() and (d2.challenge() == h2.challenge()).all()
    assert d1.state() == h1.state() != d2.state() == h2.state()
    d1.free(), d2.free()


# ---- the differential test against the parents ----
def _replay(label_state_of, rounds):
    from zkhip.transcript import HostTranscript

    tr = HostTranscript(b"diff")
    tr.absorb(label_state_of)
    return np.stack([tr.absorb(r).challenge() for r in rounds]), tr


def _fresh(ctx, seed_bytes):
    from zkhip.transcript import Transcript

    return Transcript(ctx, b"diff").absorb(seed_bytes)


def _gate_tabs(ctx, n, seed):
    return [ctx.to_device(rand_fr(1 << n, seed + k)) for k in range(7)]


def _same(bufs, before, n):
    for b, t in zip(bufs, before):
        assert (b.download(t.shape) == t).all(), "an input table was written"


def _diff_gate(ctx, n, seed):
    tabs = _gate_tabs(ctx, n, seed)
    before = [t.download((1 << n, 4)) for t in tabs] if n <= 13 else None
    tr = _fresh(ctx, b"g%d" % n)
    rounds, last, chal = ctx.sumcheck_gate_fs(*tabs, 1 << n, tr)
    want, host = _replay(b"g%d" % n, rounds)
    assert (chal == want).all(), n
    assert tr.state() == host.state()  # the device transcript has absorbed every round
    p_rounds, p_last = ctx.sumcheck_gate(*tabs, 1 << n, chal)
    assert (rounds == p_rounds).all() and (last == p_last).all(), n
    if before is not None:
        _same(tabs, before, n)
    tr.free()


def _diff_wiring(ctx, n, seed):
    N = 1 << n
    eq, num, den = (ctx.to_device(rand_fr(N, seed + k)) for k in range(3))
    tree = ctx.product_tree(ctx.to_device(rand_fr(N, seed + 3)), N)
    gamma = rand_fr(1, seed + 4)[0]
    before = [eq.download((N, 4)), tree.download((2 * N, 4)), num.download((N, 4)), den.download((N, 4))] if n <= 13 else None
    tr = _fresh(ctx, b"w%d" % n)
    rounds, last, chal = ctx.sumcheck_wiring_fs(eq, tree, num, den, N, gamma, tr)
    want, host = _replay(b"w%d" % n, rounds)
    assert (chal == want).all() and tr.state() == host.state(), n
    p_rounds, p_last = ctx.sumcheck_wiring(eq, tree, num, den, N, gamma, chal)
    assert (rounds == p_rounds).all() and (last == p_last).all(), n
    if before is not None:
        _same([eq, tree, num, den], before, n)
    tr.free()


def _diff_multi(ctx, n, count, seed):
    N = 1 << n
    es = [ctx.to_device(rand_fr(N, seed + 2 * j)) for j in range(count)]
    fs = [ctx.to_device(rand_fr(N, seed + 2 * j + 1)) for j in range(count)]
    before = [t.download((N, 4)) for t in es + fs] if n <= 13 else None
    tr = _fresh(ctx, b"m%d" % n)
    rounds, le, lf, chal = ctx.sumcheck_multi_fs(es, fs, N, tr)
    want, host = _replay(b"m%d" % n, rounds)
    assert (chal == want).all() and tr.state() == host.state(), (n, count)
    p_rounds, p_le, p_lf = ctx.sumcheck_multi(es, fs, N, chal)
    assert (rounds == p_rounds).all() and (le == p_le).all() and (lf == p_lf).all(), (n, count)
    if before is not None:
        _same(es + fs, before, n)
    tr.free()


@pytest.mark.parametrize("n", SIZES)
def test_gate_fs_equals_parent_on_its_own_challenges(ctx, n):
    _diff_gate(ctx, n, 1000 + 10 * n)


@pytest.mark.parametrize("n", SIZES)
def test_wiring_fs_equals_parent_on_its_own_challenges(ctx, n):
    _diff_wiring(ctx, n, 2000 + 10 * n)


@pytest.mark.parametrize("n", SIZES)
def test_multi_fs_equals_parent_on_its_own_challenges(ctx, n):
    for count in (1, 3, 6, 16):
        if count * (1 << n) * 64 > (3 << 30):  # 2 count tables of 2^n Fr: keep the test's own footprint below 3 GiB
            continue
        _diff_multi(ctx, n, count, 3000 + 100 * n + count)


def test_hbm_passes_down_to_the_last_element(ctx):
    """gate_local_e / wiring_local_e / multi_local_e = 1: every round is an HBM pass, the local stage only applies the pending fold"""
    from zkhip._lib import test_hooks

    lib = test_hooks()
    keys = (b"gate_local_e", b"wiring_local_e", b"multi_local_e")
    found = {}
    for k in keys:  # what the knobs hold now goes back at the end, whatever the defaults are
        v = ctypes.c_long(0)
        assert lib.zk_dbg_tune_get(k, ctypes.byref(v)) == 0
        found[k] = v.value
    try:
        for k in keys:
            assert lib.zk_dbg_tune(k, 1) == 0
        for n in (1, 2, 9, 11):
            _diff_gate(ctx, n, 4000 + n)
            _diff_wiring(ctx, n, 4100 + n)
            for count in (1, 3, 16):
                _diff_multi(ctx, n, count, 4200 + 20 * n + count)
    finally:
        for k in keys:
            lib.zk_dbg_tune(k, found[k])


def test_gate_fs_small_sizes_match_the_model(ctx):
    """n = 1 .. 6 against the big-int model driven by the model transcript (no parent code involved)"""
    for n in range(1, 7):
        rng = po.SplitMix64(50 + n)
        tabs = {k: rng.fr_vec(1 << n) for k in zm.TABLES}
        tr_m = fm.Model(b"diff").absorb(b"x")
        rounds, at, chal = fm._stepwise(tr_m, tabs, lambda cur, ch: zm.sumcheck_gate(cur, ch)[0])
        last = [at[k] for k in zm.TABLES]
        tr = _fresh(ctx, b"x")
        got_r, got_l, got_c = ctx.sumcheck_gate_fs(*[ctx.to_device(zm.mont(tabs[k])) for k in zm.TABLES], 1 << n, tr)
        assert [zm.ints(r) for r in got_r] == rounds and zm.ints(got_l) == last and zm.ints(got_c) == chal, n
        assert tr.state() == tr_m.state
        tr.free()


# ---- error paths ----
def test_fs_errors_return_invalid_without_launching(ctx):
    import zkhip
    from zkhip._lib import ZK_ERR_INVALID
    from zkhip.transcript import Transcript

    tabs = _gate_tabs(ctx, 4, 1)
    tr = Transcript(ctx, b"err")
    state = tr.state()
    for bad_tr, length in ((None, 16), (tr, 12), (tr, 0), (tr, 1)):
        with pytest.raises(zkhip.ZkError) as e:
            ctx.sumcheck_gate_fs(*tabs, length, bad_tr)
        assert e.value.code == ZK_ERR_INVALID
        with pytest.raises(zkhip.ZkError) as e:
            ctx.sumcheck_wiring_fs(tabs[0], tabs[1], tabs[2], tabs[3], length // 2 if length == 16 else length, rand_fr(1, 1)[0], bad_tr)
        assert e.value.code == ZK_ERR_INVALID
        with pytest.raises(zkhip.ZkError) as e:
            ctx.sumcheck_multi_fs(tabs[:2], tabs[2:4], length, bad_tr)
        assert e.value.code == ZK_ERR_INVALID
    other = zkhip.Ctx(0)
    try:
        foreign = Transcript(other, b"err")
        for call in (lambda: ctx.sumcheck_gate_fs(*tabs, 16, foreign), lambda: ctx.sumcheck_multi_fs(tabs[:2], tabs[2:4], 16, foreign),
                     lambda: ctx.sumcheck_wiring_fs(tabs[0], tabs[1], tabs[2], tabs[3], 8, rand_fr(1, 1)[0], foreign)):
            with pytest.raises(zkhip.ZkError) as e:
                call()
            assert e.value.code == ZK_ERR_INVALID
        rc = ctx.lib.zk_transcript_absorb(ctx.h, foreign.h, b"x", 1)
        assert rc == ZK_ERR_INVALID
        foreign.free()
    finally:
        other.close()
    assert tr.state() == state  # nothing was absorbed by the failed calls
    tr.free()


# ---- end to end ----
def _field_digest_of(proof):
    return fm.field_digest(proof)


@pytest.mark.parametrize("n", [4, 10, 14, 20])
def test_gate_ni_end_to_end(ctx, n):
    from zkhip import dist_primitive as dp
    from zkhip import nizk
    from zkhip import pairing as pr
    from zkhip import zerocheck as zc

    tables, _tau, _chal, s = zc.satisfied_circuit(ctx, n, 5)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    proof = nizk.gate_prove_ni(ctx, pcs, tables)
    vk = dp.pcs_vk(ctx, pr.powers_of_g2(zm.ints(s)))
    assert nizk.gate_field_checks_ni(proof) is True
    assert nizk.gate_verify_ni(ctx, vk, proof) is True
    assert nizk.proof_digest(nizk.gate_prove_ni(ctx, pcs, tables)) == nizk.proof_digest(proof)  # deterministic
    if n <= 14:  # the big-int model on the same tables and commitments: the same rounds, values and (so) challenges
        ints = {k: zm.ints(tables[k].download((1 << n, 4))) for k in fm.OPENED_GATE}
        m = fm.gate_prove(ints, proof["commitments"])
        assert fm.field_digest(fm.gate_record(m, proof["commitments"])) == fm.field_digest(proof)
    if n <= 14:
        # a tampered record: one round evaluation, one claimed value, one limb of a commitment, one limb of the opening proof
        for key, idx in (("rounds", (n - 1, 0)), ("values", 2)):
            bad = dict(proof)
            a = np.array(proof[key], copy=True)
            a[idx] = zm.mont([(zm.ints(a[idx])[0] + 1) % R])[0]
            bad[key] = a
            assert nizk.gate_verify_ni(ctx, vk, bad) is False, key
        bad = dict(proof, batch=dict(proof["batch"], opening=np.array(proof["batch"]["opening"], copy=True)))
        bad["batch"]["opening"][0] = proof["batch"]["opening"][n - 1] if n > 1 else proof["commitments"][0]
        assert nizk.gate_field_checks_ni(bad) is True and nizk.gate_verify_ni(ctx, vk, bad) is False  # only the pairing sees it
        broken, _, _, _ = zc.satisfied_circuit(ctx, n, 5, break_gate=3)
        assert nizk.gate_verify_ni(ctx, vk, nizk.gate_prove_ni(ctx, pcs, broken)) is False


@pytest.mark.parametrize("mu", [4, 10, 14, 20])
def test_wiring_ni_end_to_end(ctx, mu):
    from zkhip import dist_primitive as dp
    from zkhip import nizk
    from zkhip import pairing as pr
    from zkhip import wiring as wr

    w, sid, ssigma, *_rest, s = wr.permuted_circuit(ctx, mu, 7)
    pcs = dp.PolynomialCommitmentCub.new(ctx, s).mature()
    proof = nizk.wiring_prove_ni(ctx, pcs, w, sid, ssigma, 1 << mu)
    vk_mu, vk_mu1 = wr.verifying_keys(ctx, pr.powers_of_g2(zm.ints(s)))
    assert nizk.wiring_field_checks_ni(proof) is True
    assert nizk.wiring_verify_ni(ctx, vk_mu, vk_mu1, proof) is True
    if mu <= 14:  # the big-int model on the same tables and commitments
        ints = [zm.ints(b.download((1 << mu, 4))) for b in (w, sid, ssigma)]
        m = fm.wiring_prove(*ints, proof["commitments"], lambda tree: proof["v_commitment"])
        assert fm.field_digest(fm.wiring_record(m, proof["commitments"])) == fm.field_digest(proof)
    if mu <= 14:
        for key, idx in (("rounds", (0, 3)), ("v_values", 4), ("values", 0)):
            bad = dict(proof)
            a = np.array(proof[key], copy=True)
            a[idx] = zm.mont([(zm.ints(a[idx])[0] + 1) % R])[0]
            bad[key] = a
            assert nizk.wiring_verify_ni(ctx, vk_mu, vk_mu1, bad) is False, key
        bw, bsid, bss, *_r = wr.permuted_circuit(ctx, mu, 7, break_wire=5)
        assert nizk.wiring_verify_ni(ctx, vk_mu, vk_mu1, nizk.wiring_prove_ni(ctx, pcs, bw, bsid, bss, 1 << mu)) is False


# ---- the compiled host ----
def _ni_check(*args):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/ni_check"])
    r = subprocess.run([NI_CHECK, *args], capture_output=True, text=True, timeout=600)
    m = re.search(r"proof sha256 ([0-9a-f]{64})", r.stdout)
    return r, m.group(1) if m else None


@pytest.mark.parametrize("n,seed", [(1, 3), (4, 7), (10, 7), (14, 2)])
def test_gate_ni_python_and_cpp_digests_agree(ctx, n, seed):
    from zkhip import dist_primitive as dp
    from zkhip import nizk
    from zkhip import zerocheck as zc

    r, got = _ni_check("--which", "gate", "--n", str(n), "--seed", str(seed))
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    tables, _tau, _chal, s = zc.satisfied_circuit(ctx, n, seed)
    proof = nizk.gate_prove_ni(ctx, dp.PolynomialCommitmentCub.new(ctx, s).mature(), tables)
    assert nizk.proof_digest(proof) == got


@pytest.mark.parametrize("mu,seed", [(1, 3), (4, 7), (10, 7), (14, 2)])
def test_wiring_ni_python_and_cpp_digests_agree(ctx, mu, seed):
    from zkhip import dist_primitive as dp
    from zkhip import nizk
    from zkhip import wiring as wr

    r, got = _ni_check("--which", "wiring", "--n", str(mu), "--seed", str(seed))
    assert r.returncode == 0 and "accept" in r.stdout, (r.returncode, r.stdout, r.stderr)
    w, sid, ssigma, *_rest, s = wr.permuted_circuit(ctx, mu, seed)
    proof = nizk.wiring_prove_ni(ctx, dp.PolynomialCommitmentCub.new(ctx, s).mature(), w, sid, ssigma, 1 << mu)
    assert nizk.proof_digest(proof) == got


def test_ni_check_rejects_broken_circuits():
    for which in ("gate", "wiring"):
        r, got = _ni_check("--which", which, "--n", "10", "--seed", "7", "--break", "5")
        assert r.returncode == 1 and "reject" in r.stdout and got, (which, r.returncode, r.stdout, r.stderr)


def test_absorbs_beyond_the_limit_are_refused(ctx):
    import zkhip
    from zkhip._lib import ZK_ERR_INVALID
    from zkhip.transcript import Transcript

    tr = Transcript(ctx, b"limit")
    state = tr.state()
    buf = ctx.alloc((1 << 20) + 1)
    for call in (lambda: tr.absorb_device(buf, (1 << 20) + 1), lambda: tr.absorb(bytes((1 << 20) + 1))):
        with pytest.raises(zkhip.ZkError) as e:
            call()
        assert e.value.code == ZK_ERR_INVALID
    assert tr.state() == state
    tr.free()
