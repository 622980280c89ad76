"""
Witness generation through lookups without a GPU: sample_circuit_lookup_fn satisfies every gate, copy and lookup; the model of the rules
(witness_lookup_model.py) reproduces its wires from the public inputs and the free values alone; the sampled circuits have the shapes the
GPU tests rely on (enough lookup-computing rows, chains through lookup rows, both launch paths); the model's refusals; and the library,
the binding and the Rust FFI carry the new symbols; the compiled host's sampler gives the Python sampler's digest.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import witness_lookup_model as wlm
import witness_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_witness_plan_create_lookup", "zk_plonk_witness_lookup", "zk_plonk_witness_check_lookup")
OK = {"bad_rows": 0, "first_bad_row": None, "bad_copies": 0, "first_bad_copy": None, "bad_lookups": 0, "first_bad_lookup": None}
# two seeds whose circuits meet test_sampled_circuits_are_not_vacuous at every size: at mu = 3 only four rows are drawn, and most seeds
# miss one of the three feeding patterns there (from mu = 5 on every seed tried has them all)
MUS, SEEDS = (3, 5, 9, 12), (4, 5)
_cache = {}


def sampled(mu: int, seed: int):
    """(circuit, model plan, free as canonical ints), computed once and shared; nobody writes to them"""
    from zkhip import plonk

    if (mu, seed) not in _cache:
        c = plonk.sample_circuit_lookup_fn(mu, seed)
        _cache[mu, seed] = (c, wlm.plan(c), wm.ints(c["free"]))
    return _cache[mu, seed]


def a_break_row(c: dict) -> int:
    """the last lookup row whose a slot is free (a fixed point of sigma)"""
    N = 1 << c["mu"]
    qk = wm.ints(c["lookup"]["qk"])
    return max(x for x in range(N) if qk[x] and int(c["sigma"][x]) == x)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mu", MUS)
def test_sampler_is_satisfied_and_the_model_reproduces_it(mu, seed):
    from zkhip import lookup

    c, p, free = sampled(mu, seed)
    N = 1 << mu
    a, b, cc = (wm.ints(c[k]) for k in "abc")
    assert wlm.check(c, p, a, b, cc, c["public_inputs"]) == OK  # every gate, copy and lookup
    got = wlm.generate(c, p, c["public_inputs"], free)
    for name, g in zip("abc", got):
        assert (wm.limbs(g) == c[name]).all(), name
    lk = c["lookup"]
    idx = lookup.find_indices_host([lk[k] for k in ("t0", "t1", "t2")], [c[k] for k in "abc"], lk["qk"])
    assert (idx == c["idx"]).all() and c["idx"].dtype == np.uint32
    assert wlm.find_indices(p, a, b, cc) == c["idx"].tolist()
    # the gate of a lookup row is switched off, and the table is the XOR table on k bits
    k = min(4, mu // 2)
    sel = wm.selectors(c)
    for x in range(N):
        if p["kind"][x] == wlm.LOOKUP:
            assert all(sel[q][x] == 0 for q in wm.WIDE) and cc[x] == a[x] ^ b[x] < 1 << k
    assert p["table"]["t"] == list(zip(*(wlm.xor_table(N, k)[q] for q in ("t0", "t1", "t2"))))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mu", MUS)
def test_sampled_circuits_are_not_vacuous(mu, seed):
    c, p, _ = sampled(mu, seed)
    N = 1 << mu
    lk_rows = [x for x in range(N) if p["kind"][x] == wlm.LOOKUP]
    assert 4 * len(lk_rows) >= N
    fed = lambda x: [v for free, v in (p["src"][x], p["src"][N + x]) if not free]  # the source rows of a row's a and b
    assert any(p["kind"][y] == wlm.LOOKUP for x in lk_rows for y in fed(x))
    assert any(p["kind"][y] == wlm.LOOKUP for x in range(N) if p["kind"][x] == wlm.GATE for y in fed(x))
    if mu >= 9:
        assert any(len(r) > 256 for r in p["levels"]) and any(e - v >= 2 for v, e in wlm.launches(p))


def test_break_row_is_one_bad_lookup_and_the_generator_leaves_zero():
    from zkhip import plonk

    mu, seed = 5, SEEDS[1]
    good, p, _ = sampled(mu, seed)
    K = a_break_row(good)
    c = plonk.sample_circuit_lookup_fn(mu, seed, break_row=K)
    a, b, cc = wlm.generate(c, p, c["public_inputs"], wm.ints(c["free"]))
    for name, g in zip("abc", (a, b, cc)):
        assert (wm.limbs(g) == c[name]).all(), name
    assert a[K] >= 1 << 2 and cc[K] == 0
    assert wlm.check(c, p, a, b, cc, c["public_inputs"]) == dict(OK, bad_lookups=1, first_bad_lookup=K)
    with pytest.raises(ValueError, match="lookup row with a free a"):
        plonk.sample_circuit_lookup_fn(mu, seed, break_row=0)


def test_the_function_rule_and_qk_refusals_of_the_model():
    c = wlm.flat(3, 2, 1)  # N = 8, the table has 4 entries and is padded with entry 3
    t2 = wm.ints(c["lookup"]["t2"])
    bad = dict(c, lookup=dict(c["lookup"], t2=wm.limbs(t2[:6] + [t2[6] + 1] + t2[7:])))
    with pytest.raises(ValueError, match=r"^1 of 8 table entries repeat the pair \(t0, t1\) of an earlier entry with another t2; the first is entry 6$"):
        wlm.plan(bad)
    # entries 3 .. 7 are one pair: with the FIRST one changed the four later ones differ from it
    bad = dict(c, lookup=dict(c["lookup"], t2=wm.limbs(t2[:3] + [t2[3] + 1] + t2[4:])))
    with pytest.raises(ValueError, match=r"^4 of 8 table entries repeat .* the first is entry 4$"):
        wlm.plan(bad)
    wlm.plan(c)  # the padding repeats a whole entry: accepted
    qk = wm.ints(c["lookup"]["qk"])
    bad = dict(c, lookup=dict(c["lookup"], qk=wm.limbs(qk[:5] + [2] + qk[6:])))
    with pytest.raises(ValueError, match=r"^1 of 8 entries of qk are neither 0 nor 1; the first is row 5$"):
        wlm.plan(bad)


def test_hand_built_plans():
    mu, l = 10, 4
    N = 1 << mu
    p = wlm.plan(wlm.chain(mu, l))
    assert [len(r) for r in p["levels"]] == [l + 1] + [1] * (N - l - 1)
    assert wlm.info(p) == {"levels": N - l, "max_level_rows": l + 1, "launches": 1}
    p = wlm.plan(wlm.flat(mu, l))
    assert wlm.info(p) == {"levels": 1, "max_level_rows": N, "launches": 1} and wlm.launches(p) == [(0, 1)]
    with pytest.raises(ValueError, match=r"^2 of 64 rows depend on their own output; the first is row 33$"):
        wlm.plan(wlm.self_dependent())
    # a gate-computing row with qk = 1 stays gate-computing
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(5, 7, gate="wide")
    assert wlm.LOOKUP not in wlm.plan(c)["kind"]


def test_new_symbols_exist():
    import zkhip
    from zkhip import _lib, plonk

    lib = ctypes.CDLL(zkhip.LIB_PATH)
    bound = {s[0] for s in _lib.SYMBOLS}
    rust = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in bound and f"pub fn {s}(" in rust and f"{s}(" in header, s
    assert callable(plonk.sample_circuit_lookup_fn) and callable(zkhip.Ctx.witness_plan_lookup)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mu", MUS)
def test_plonk_check_sample_only_prints_the_python_samplers_digest(mu, seed):
    from zkhip import plonk

    tool = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host", "bin", "plonk_check")
    flags = [tool, "--mu", str(mu), "--seed", str(seed), "--gate", "wide", "--lookup-fn", "--sample-only"]
    r = subprocess.run(flags, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == f"circuit sha256 {plonk.circuit_digest(sampled(mu, seed)[0])}\n"
    if mu == 5:  # and with a broken row; a row that is no lookup row with a free a, and the flag without the wide gate, are refused
        K = a_break_row(sampled(mu, seed)[0])
        r = subprocess.run(flags + ["--break-lookup", str(K)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == f"circuit sha256 {plonk.circuit_digest(plonk.sample_circuit_lookup_fn(mu, seed, break_row=K))}\n"
        assert subprocess.run(flags + ["--break-lookup", "0"], capture_output=True, text=True, timeout=120).returncode == 2
        assert subprocess.run([tool, "--mu", "5", "--lookup-fn", "--sample-only"], capture_output=True, text=True, timeout=120).returncode == 2
