"""
Lookups without caller indices, the part that needs no device: zkhip.lookup.find_indices_host (the CPU statement of the rule of
zk_lookup_find / zk_lookup3_find: the smallest index of an equal entry) against the plain-Python model (lookup_find_model.py) and on the
samples of both provers, the FIND sentinel's argument checks, and the compiled hosts' --find beside --sample-only.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lookup_find_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")


def _distincts(N):
    return sorted({1, min(2, N), max(N // 2, 1), N})


def _scattered(n, seed, distinct, cols=1):
    """a table whose duplicates lie anywhere (entry y = value draw[y] mod distinct), rows drawn from it, and a selector with some zeros"""
    from zkhip.field import fr_mont, splitmix_fr

    N = 1 << n
    vals = [splitmix_fr(distinct, seed + j) for j in range(cols)]
    draw = splitmix_fr(N, seed + 7)
    ty, fy = (draw[:, 0] % np.uint64(distinct)).astype(np.int64), (draw[:, 1] % np.uint64(distinct)).astype(np.int64)
    fy = np.where(np.isin(fy, ty), fy, ty[0])  # only values that the table holds
    t, f = [v[ty] for v in vals], [v[fy] for v in vals]
    qk = np.zeros((N, 4), dtype=np.uint64)
    qk[(draw[:, 2] & np.uint64(3)) != 0] = fr_mont(1)
    return t, f, qk


def test_the_model_knows_the_montgomery_one():
    from zkhip.field import fr_mont

    assert tuple(int(v) for v in fr_mont(1)) == fm.ONE


@pytest.mark.parametrize("n", range(1, 8))
def test_find_indices_host_matches_the_model(n):
    from zkhip import lookup as lk

    N = 1 << n
    for distinct in _distincts(N):
        t, f, qk = _scattered(n, 100 * n + distinct, distinct)
        want, bad, _ = fm.find(t, f)
        assert bad == 0 and lk.find_indices_host(t[0], f[0]).tolist() == want
        t3, f3, qk = _scattered(n, 300 * n + distinct, distinct, cols=3)
        for j in range(3):  # rows that claim nothing hold anything
            f3[j][(qk == 0).all(axis=1)] ^= np.uint64(5)
        want, bad, _ = fm.find(t3, f3, qk)
        got = lk.find_indices_host(t3, f3, qk)
        assert bad == 0 and got.dtype == np.uint32 and got.tolist() == want
        assert all(fm.keys(t3)[y] == fm.keys(f3)[x] for x, y in enumerate(got) if tuple(qk[x]) == fm.ONE)


def test_find_indices_host_reports_missing_and_bad_rows_like_the_model():
    from zkhip import lookup as lk
    from zkhip.field import fr_mont

    n, N = 5, 32
    t, f, qk = _scattered(n, 77, 9, cols=3)
    sel = np.flatnonzero((qk == fr_mont(1)).all(axis=1))
    f[2][sel[3], 3] ^= np.uint64(1 << 60)  # differs from every entry in one top limb
    _, bad, first = fm.find(t, f, qk)
    assert (bad, first) == (1, int(sel[3]))
    with pytest.raises(ValueError, match=f"1 of {N} rows.*first is row {first}$"):
        lk.find_indices_host(t, f, qk)
    qk[sel[1]] = fr_mont(2)  # neither 0 nor 1
    _, bad, first = fm.find(t, f, qk)
    assert (bad, first) == (2, int(sel[1]))
    with pytest.raises(ValueError, match=f"2 of {N} rows.*first is row {first}$"):
        lk.find_indices_host(t, f, qk)
    f1 = f[0].copy()
    f1[7, 0] ^= np.uint64(1)
    with pytest.raises(ValueError, match=f"1 of {N} rows.*first is row 7$"):
        lk.find_indices_host(t[0], f1)


@pytest.mark.parametrize("n", range(1, 9))
def test_the_lookup_sample_names_first_occurrences(n):
    from zkhip import lookup as lk

    N = 1 << n
    for distinct in _distincts(N):
        t, f, idx = lk.sample_lookup(n, 3 + n, distinct)
        assert (lk.find_indices_host(t, f) == idx).all(), (n, distinct)
        assert fm.find(t, f) == (idx.tolist(), 0, None)


@pytest.mark.parametrize("gate", [None, "wide"])
@pytest.mark.parametrize("mu", range(3, 7))
def test_the_circuit_sample_names_first_occurrences(mu, gate):
    from zkhip import lookup as lk
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(mu, 7, gate=gate)
    L = c["lookup"]
    got = lk.find_indices_host([L["t0"], L["t1"], L["t2"]], [c["a"], c["b"], c["c"]], L["qk"])
    assert (got == c["idx"]).all()  # the zeros of the unselected rows among them
    assert fm.find([L["t0"], L["t1"], L["t2"]], [c["a"], c["b"], c["c"]], L["qk"]) == (c["idx"].tolist(), 0, None)


def test_indices_moved_into_the_padding_are_valid_but_not_what_the_find_returns():
    """entry D - 1 is repeated up to N - 1: naming N - 1 instead is a valid claim with other multiplicities; the find names D - 1"""
    from zkhip import lookup as lk
    from zkhip import plonk

    n, D = 6, 16
    t, f, idx = lk.sample_lookup(n, 9, D)
    moved = np.where(idx == D - 1, (1 << n) - 1, idx).astype(np.uint32)
    assert (moved != idx).any() and (t[moved] == f).all()
    assert fm.multiplicities(moved.tolist()) != fm.multiplicities(idx.tolist())
    assert (lk.find_indices_host(t, f) == idx).all()
    c = plonk.sample_circuit_lookup(6, 7)
    L, N, D = c["lookup"], 64, 16
    sel = (L["qk"] != 0).any(axis=1)
    moved = np.where(sel & (c["idx"] == D - 1), N - 1, c["idx"]).astype(np.uint32)
    assert (moved != c["idx"]).any()
    assert all((L[k][moved[sel]] == c[w][sel]).all() for k, w in (("t0", "a"), ("t1", "b"), ("t2", "c")))
    assert fm.multiplicities(moved.tolist(), L["qk"]) != fm.multiplicities(c["idx"].tolist(), L["qk"])
    got = lk.find_indices_host([L["t0"], L["t1"], L["t2"]], [c["a"], c["b"], c["c"]], L["qk"])
    assert (got == c["idx"]).all() and (got[sel & (moved == N - 1)] == D - 1).all()


def test_prove_checks_the_sentinel_before_touching_a_device():
    from zkhip import lookup as lk
    from zkhip import plonk

    assert lk.FIND == "find" and plonk.FIND == lk.FIND
    z = np.zeros((8, 4), dtype=np.uint64)
    pk = {"mu": 3, "l": 4, "pcs": None, "tables": {}, "commitments": None}
    with pytest.raises(ValueError, match="idx"):  # FIND with a key without a lookup
        plonk.prove(None, pk, z, z, z, z[:4], idx=plonk.FIND)
    with pytest.raises(ValueError, match="idx"):  # an unknown string
        plonk.prove(None, dict(pk, lookup=True), z, z, z, z[:4], idx="search")
    with pytest.raises(ValueError, match="idx"):
        lk.prove(None, {"n": 3, "t": None, "pcs": None}, z, "search")


def test_symbols_in_the_library_the_header_and_the_binding():
    import ctypes

    import zkhip

    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    lib = ctypes.CDLL(zkhip.LIB_PATH)
    for s in ("zk_lookup_find", "zk_lookup3_find"):
        assert f"int {s}(" in header and f"pub fn {s}(" in rust and getattr(lib, s) is not None, s
    assert hasattr(zkhip.Ctx, "lookup_find") and hasattr(zkhip.Ctx, "lookup3_find")
    assert zkhip._lib.ZK_ERR_INTERNAL == -8 and "ZK_ERR_INTERNAL = -8" in header and "ZK_ERR_INTERNAL: i32 = -8" in rust
    val = ctypes.c_long(0)
    assert lib.zk_dbg_tune_get(b"find_force_slot", ctypes.byref(val)) == 0 and val.value == -1


# ---- the compiled hosts (no GPU): --find changes what is proved from, not the sample ----
def _digest(tool, *args):
    subprocess.check_call(["make", "-C", HOST, "-s", f"bin/{tool}"])
    r = subprocess.run([os.path.join(HOST, "bin", tool), *args, "--sample-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return re.search(r"sha256 ([0-9a-f]{64})", r.stdout).group(1)


def test_sample_only_with_find_leaves_the_digests_unchanged():
    from zkhip import lookup as lk
    from zkhip import plonk

    want = lk.sample_digest(*lk.sample_lookup(7, 3))
    assert _digest("lookup_check", "--n", "7", "--seed", "3") == want == _digest("lookup_check", "--n", "7", "--seed", "3", "--find")
    for gate, kind in ((None, ()), ("wide", ("--gate", "wide"))):
        want = plonk.circuit_digest(plonk.sample_circuit_lookup(5, 7, gate=gate))
        assert _digest("plonk_check", "--mu", "5", "--seed", "7", "--lookup", *kind) == want
        assert _digest("plonk_check", "--mu", "5", "--seed", "7", "--lookup", "--find", *kind) == want
    r = subprocess.run([os.path.join(HOST, "bin", "plonk_check"), "--mu", "5", "--find"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.stdout, r.stderr)  # --find needs --lookup
