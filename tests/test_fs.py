"""
Fiat-Shamir without a GPU: zkhip.transcript.HostTranscript against the model (fs_model.py) and against hand-stated hashlib expressions,
and the host verifiers' replay and field checks (zkhip.nizk) on the model prover's records.  The pairing step needs the device, so the
acceptance tests here stop at the field checks plus the derived challenges; tests/test_gpu_fs.py goes through the pairing.
"""
import copy
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import batch_open_model as bm
import fs_model as fm
import pyoracle as po
import wiring_model as wm
import zerocheck_model as zm

R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 22, 23, 54, 55, 56, 63, 64, 119, 120)  # the padding boundaries after the 33-byte prefix


def _data(n, salt=0):
    return bytes((7 * i + 3 + salt) & 0xFF for i in range(n))


def _vectors():
    """label -> absorb lengths in turn, two challenges after each: the lines host/bin/ni_check --vectors prints"""
    from zkhip.transcript import HostTranscript

    lines = []
    for label in (b"", b"gate", b"wiring"):
        tr = HostTranscript(label)
        lines.append(f"init {label.decode() or '-'} {tr.state().hex()}")
        for n in LENGTHS:
            tr.absorb(_data(n, len(label)))
            lines.append(f"absorb {n} {tr.state().hex()}")
            for c in tr.challenges(2):
                lines.append("challenge " + "".join(f"{int(w):016x}" for w in c))
    return lines


@pytest.mark.parametrize("n", LENGTHS)
def test_host_transcript_matches_hashlib_and_model(n):
    from zkhip.field import fr_from_mont
    from zkhip.transcript import HostTranscript

    d = _data(n)
    tr, m = HostTranscript(b"lbl"), fm.Model(b"lbl")
    s0 = hashlib.sha256(b"zkhip-fs-v1lbl").digest()
    assert tr.state() == s0 == m.state
    tr.absorb(d), m.absorb(d)
    s1 = hashlib.sha256(s0 + b"\x00" + d).digest()
    assert tr.state() == s1 == m.state
    state = s1
    for _ in range(4):  # successive challenges
        state = hashlib.sha256(state + b"\x01").digest()
        want = int.from_bytes(state, "little") & ((1 << 254) - 1)
        got = tr.challenges(1)
        assert got.shape == (1, 4) and fr_from_mont(got[0]) == want == m.challenge()
        assert want < 1 << 254 < R and tr.state() == state


def test_words_and_integers_enter_little_endian():
    from zkhip.transcript import HostTranscript

    words = np.array([[1, 2, 3, 0x8877665544332211]], dtype=np.uint64)
    a, b = HostTranscript(b"x").absorb(words), HostTranscript(b"x").absorb(words.astype("<u8").tobytes())
    assert a.state() == b.state() == fm.Model(b"x").absorb(fm.words_bytes(words)).state
    assert words.astype("<u8").tobytes()[-8:] == bytes.fromhex("1122334455667788")
    assert HostTranscript(b"x").absorb_u64(20).state() == hashlib.sha256(hashlib.sha256(b"zkhip-fs-v1x").digest() + b"\x00" + bytes([20, 0, 0, 0, 0, 0, 0, 0])).digest()
    assert fm.fr_bytes([5]) == zm.mont([5]).astype("<u8").tobytes()  # the model's element bytes are the record's


def test_clearing_the_two_top_bits_is_observable():
    """a chosen transcript whose challenge digest has a top bit set: the challenge differs from the raw integer by exactly those bits"""
    from zkhip.field import fr_from_mont
    from zkhip.transcript import HostTranscript

    for k in range(64):
        label = b"top" + bytes([k])
        d = hashlib.sha256(hashlib.sha256(b"zkhip-fs-v1" + label).digest() + b"\x01").digest()
        if d[31] & 0xC0 == 0xC0:
            break
    else:
        pytest.fail("no vector with both top bits set among 64 labels")
    raw = int.from_bytes(d, "little")
    got = fr_from_mont(HostTranscript(label).challenge())
    assert raw >> 254 == 3 and got == raw - (3 << 254) and got < 1 << 254


def _fake_comms(count, seed):
    return np.array([x & ((1 << 64) - 1) for x in po.SplitMix64(seed).fr_vec(count * 18)], dtype=np.uint64).reshape(count, 18)


def _gate(n, seed, **kw):
    comms = np.asarray(_fake_comms(6, seed), dtype=np.uint64)
    tabs = zm.circuit(n, seed, **kw)
    m = fm.gate_prove(tabs, comms)
    return m, fm.gate_record(m, comms), tabs


def _wiring(mu, seed, **kw):
    comms = np.asarray(_fake_comms(3, seed), dtype=np.uint64)
    w, sid, ssigma = wm.shuffled_circuit(mu, seed, **kw)
    v_of = lambda tree: np.asarray([sum(tree) % (1 << 64)] * 18, dtype=np.uint64)  # stands for a commitment: any function of the tree
    m = fm.wiring_prove(w, sid, ssigma, comms, v_of)
    return m, fm.wiring_record(m, comms), (w, sid, ssigma)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_gate_model_prover_to_host_verifier(n):
    from zkhip import nizk

    m, rec, _ = _gate(n, 300 + n)
    c = nizk.gate_challenges(rec)
    for key in ("tau", "chal", "rho"):
        assert zm.ints(c[key]) == m[key], key
    assert zm.ints(c["alpha"]) == [m["alpha"]]
    assert all(x < 1 << 254 for key in ("tau", "chal", "rho") for x in m[key])
    assert nizk.gate_field_checks_ni(rec) is True
    # the chain of the batch instance ends in sum_j e_j f_j(rho): what the pairing would certify
    from zkhip import batch_open as bo

    claims = [(i, c["chal"], rec["values"][i]) for i in range(6)]
    assert bo.failed_checks(6, claims, rec["batch"], c["alpha"], c["rho"], finals=zm.mont(m["finals"])) == []
    assert nizk.gate_field_checks_ni(_gate(n, 300 + n, break_gate=(1 << n) - 1)[1]) is False


@pytest.mark.parametrize("mu", [1, 2, 5])
def test_wiring_model_prover_to_host_verifier(mu):
    from zkhip import nizk

    m, rec, _ = _wiring(mu, 400 + mu)
    c = nizk.wiring_challenges(rec)
    for key in ("tau", "chal", "rho_mu", "rho_mu1"):
        assert zm.ints(c[key]) == m[key], key
    for key in ("alpha", "beta", "gamma", "b_alpha"):
        assert zm.ints(c[key]) == [m[key]], key
    assert nizk.wiring_field_checks_ni(rec) is True
    assert nizk.wiring_field_checks_ni(_wiring(mu, 400 + mu, break_wire=1)[1]) is False


def _bump(arr, idx):
    """add 1 to the field element / word at idx"""
    a = np.array(arr, dtype=np.uint64, copy=True)
    if a.shape[-1] == 4:
        a[idx] = zm.mont([(zm.ints(a[idx])[0] + 1) % R])[0]
    else:
        a[idx] ^= np.uint64(1)
    return a


def test_gate_verifier_rejects_every_single_change():
    from zkhip import nizk

    n = 3
    m, rec, tabs = _gate(n, 77)
    assert nizk.gate_field_checks_ni(rec, finals=zm.mont(m["finals"])) is True

    def finals_at(bad):  # the tables at the point the changed record leads to: what the pairing would compare the chain's end with
        rho = zm.ints(nizk.gate_challenges(bad)["rho"])
        return zm.mont([bm.evaluate(tabs[k], rho) for k in fm.OPENED_GATE])

    for i in range(n):
        for t in range(5):
            bad = dict(rec, rounds=_bump(rec["rounds"], (i, t)))
            assert nizk.gate_field_checks_ni(bad) is False, ("round", i, t)
        for t in range(3):
            bad = copy.deepcopy(rec)
            bad["batch"]["rounds"] = _bump(rec["batch"]["rounds"], (i, t))
            assert nizk.gate_field_checks_ni(bad, finals=finals_at(bad)) is False, ("batch round", i, t)
    for k in range(6):
        assert nizk.gate_field_checks_ni(dict(rec, values=_bump(rec["values"], k))) is False, ("value", k)
        for limb in range(18):
            assert nizk.gate_field_checks_ni(dict(rec, commitments=_bump(rec["commitments"], (k, limb)))) is False, ("commitment", k, limb)
    assert nizk.gate_field_checks_ni(dict(rec, n=n + 1)) is False
    assert nizk.gate_field_checks_ni(dict(rec, n=n - 1)) is False
    assert nizk.gate_field_checks_ni(rec, label=b"wiring") is False  # a valid record under the other label


def test_wiring_verifier_rejects_every_single_change():
    from zkhip import nizk

    mu = 3
    m, rec, (w, sid, ssigma) = _wiring(mu, 78)
    assert nizk.wiring_field_checks_ni(rec, finals=zm.mont(m["finals"]), v_finals=zm.mont(m["v_finals"])) is True
    tree = wm.tree_of(wm.fractions(w, sid, ssigma, m["alpha"], m["beta"])[2])

    def finals_at(bad):
        c = nizk.wiring_challenges(bad)
        return {"finals": zm.mont([bm.evaluate(t, zm.ints(c["rho_mu"])) for t in (w, sid, ssigma)]), "v_finals": zm.mont([bm.evaluate(tree, zm.ints(c["rho_mu1"]))])}

    for i in range(mu):
        for t in range(4):
            assert nizk.wiring_field_checks_ni(dict(rec, rounds=_bump(rec["rounds"], (i, t)))) is False, ("round", i, t)
    for which, count in (("batch", mu), ("v_batch", mu + 1)):
        for i in range(count):
            for t in range(3):
                bad = copy.deepcopy(rec)
                bad[which]["rounds"] = _bump(rec[which]["rounds"], (i, t))
                assert nizk.wiring_field_checks_ni(bad, **finals_at(bad)) is False, (which, i, t)
    for k in range(3):
        assert nizk.wiring_field_checks_ni(dict(rec, values=_bump(rec["values"], k))) is False
        for limb in range(18):
            assert nizk.wiring_field_checks_ni(dict(rec, commitments=_bump(rec["commitments"], (k, limb)))) is False
    for k in range(5):
        assert nizk.wiring_field_checks_ni(dict(rec, v_values=_bump(rec["v_values"], k))) is False
    for limb in range(18):
        assert nizk.wiring_field_checks_ni(dict(rec, v_commitment=_bump(rec["v_commitment"], limb))) is False
    assert nizk.wiring_field_checks_ni(dict(rec, mu=mu + 1)) is False
    assert nizk.wiring_field_checks_ni(rec, label=b"gate") is False


def test_a_change_in_round_i_changes_every_later_challenge():
    from zkhip import nizk

    n = 4
    _, rec, _ = _gate(n, 91)
    base = nizk.gate_challenges(rec)
    flat = lambda c: [tuple(x) for x in c["chal"]] + [tuple(c["alpha"])] + [tuple(x) for x in c["rho"]]
    for i in range(n):
        c = nizk.gate_challenges(dict(rec, rounds=_bump(rec["rounds"], (i, 2))))
        assert (c["tau"] == base["tau"]).all()
        got, want = flat(c), flat(base)
        assert got[:i] == want[:i]
        assert all(g != w for g, w in zip(got[i:], want[i:])), i


def test_cpp_host_prints_the_same_transcript_vectors():
    """host/bin/ni_check --vectors needs no GPU: the C++ HostTranscript (zkhost/transcript.hpp) against the Python one, line by line"""
    host = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "bin/ni_check"])
    out = subprocess.run([os.path.join(host, "bin", "ni_check"), "--vectors"], capture_output=True, text=True, check=True).stdout.split("\n")
    got = [l for l in out if re.match(r"(init|absorb|challenge) ", l)]
    assert got == _vectors()


def test_ni_check_refuses_without_a_gpu():
    host = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "bin/ni_check"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    for which in ("gate", "wiring"):
        r = subprocess.run([os.path.join(host, "bin", "ni_check"), "--which", which, "--n", "4"], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "no CPU fallback" in r.stderr, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run([os.path.join(host, "bin", "ni_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "usage" in r.stderr
