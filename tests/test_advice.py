"""
Advice rows without a device: the builder's gadgets (zkhip.circuit) against the model of the rules (advice_model.py).  Every gadget's
generated witness passes the check on the inputs it accepts and is reported as a bad gate row or a bad copy on those it refuses; a generated
witness with ONE advice output overwritten by another value is reported too -- the soundness of the constraints, not of the advice; the
circuit digests of circuits without advice stand; both hosts print one digest for the transfer circuit.
"""
import os
import subprocess
import sys

import pytest

import advice_model as am
import witness_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
R = wm.R
OK = {"bad_rows": 0, "first_bad_row": None, "bad_copies": 0, "first_bad_copy": None}


def run(make, inputs: dict):
    """make(builder, {name: variable}) -> {name: output variable or list of them}; inputs: {name: integer} of private variables, each read
    through a lin copy row (to_bits wants computed values).  -> (the check's report, {name: value of the output}, layout, outs)"""
    from zkhip.circuit import Builder

    b = Builder()
    priv = {k: b.private() for k in inputs}
    outs = make(b, {k: b.lin(1, v, 0, None, 0) for k, v in priv.items()}) or {}
    circuit, layout = b.build()
    free = [0] * (3 * layout.N)
    for k, v in inputs.items():
        free[layout.slot(priv[k])] = v % R
    p = am.plan(circuit)
    pi = wm.limbs([0] * circuit["l"])
    a, b_, c = am.generate(circuit, p, pi, free)
    value = lambda v: c[layout.row(v)]
    return am.check(circuit, p, a, b_, c, pi), {k: ([value(x) for x in v] if isinstance(v, list) else value(v)) for k, v in outs.items()}, layout, outs


@pytest.mark.parametrize("x", [0, 1, 2, R - 1, 1 << 200])
def test_is_zero_and_is_equal(x):
    rep, out, _, _ = run(lambda b, v: {"z": b.is_zero(v["x"]), "e": b.is_equal(v["x"], v["y"]), "n": b.is_equal(v["x"], v["x"])}, {"x": x, "y": 1})
    assert rep == OK
    assert out == {"z": int(x == 0), "e": int(x == 1), "n": 1}


@pytest.mark.parametrize("x", [1, 5, R - 1])
def test_inverse_div_select(x):
    def make(b, v):
        b.assert_nonzero(v["x"])
        return {"i": b.inverse(v["x"]), "q": b.div(v["n"], v["x"]), "s1": b.select(v["one"], v["x"], v["n"]), "s0": b.select(v["zero"], v["x"], v["n"])}

    rep, out, _, _ = run(make, {"x": x, "n": 77, "one": 1, "zero": 0})
    assert rep == OK
    assert out == {"i": pow(x, -1, R), "q": 77 * pow(x, -1, R) % R, "s1": x, "s0": 77}


@pytest.mark.parametrize("gadget", ["inverse", "div", "assert_nonzero"])
def test_zero_has_no_inverse(gadget):
    """on 0 the advice is 0 and the assertion x i = 1 is a bad gate row: the row after the inv0 row"""
    make = {"inverse": lambda b, v: {"i": b.inverse(v["x"])}, "div": lambda b, v: {"q": b.div(v["n"], v["x"])}, "assert_nonzero": lambda b, v: b.assert_nonzero(v["x"])}[gadget]
    rep, _, layout, _ = run(make, {"x": 0, "n": 3})
    assert rep["bad_rows"] == 1 and rep["first_bad_row"] == layout.l + 2 + 1 and rep["bad_copies"] == 0  # two copy rows, the inv0 row, the assertion


@pytest.mark.parametrize("n", [1, 64, 253])
def test_to_bits(n):
    for x in (0, 1, (1 << n) - 1):
        rep, out, _, _ = run(lambda b, v: {"bits": b.to_bits(v["x"], n)}, {"x": x})
        assert rep == OK
        assert out["bits"] == [(x >> k) & 1 for k in range(n)]
    # 2^n has no n-bit decomposition: its low n bits recompose to 0, a second computing c slot that differs from its class
    rep, out, layout, outs = run(lambda b, v: {"bits": b.to_bits(v["x"], n)}, {"x": 1 << n})
    # (n = 1: the one bit IS the sum and sits in x's class, so its assert_bool row reads the class's value 2 and fails as well)
    assert rep["bad_rows"] == int(n == 1) and rep["bad_copies"] == 1
    last = layout.l + 1 + 2 * n + (n - 1) - 1 if n > 1 else layout.row(outs["bits"][0])  # the last row of the recomposition chain
    assert rep["first_bad_copy"] == 2 * layout.N + last


def test_to_bits_limits():
    from zkhip.circuit import Builder

    b = Builder()
    x = b.lin(1, b.private(), 0, None, 0)
    for n in (0, 254, 255):
        with pytest.raises(ValueError):
            b.to_bits(x, n)
    with pytest.raises(ValueError):
        b.less_than(x, x, 253)
    with pytest.raises(ValueError):
        b.bits_of(x, 250, 6)


def test_to_bits_of_a_private_variable_is_self_dependent():
    """tied to a private variable alone the sum becomes the source of its class: the plan refuses it (the builder's text says so)"""
    from zkhip.circuit import Builder

    b = Builder()
    b.to_bits(b.private(), 4)
    circuit, _ = b.build()
    with pytest.raises(ValueError, match="depend on their own output"):
        am.plan(circuit)


@pytest.mark.parametrize("n", [1, 8, 252])
def test_less_than(n):
    top = (1 << n) - 1
    for x, y in [(0, 0), (top, top), (3 % (top + 1), 3 % (top + 1)), (0, 1), (1, 0), (top - 1, top), (top, top - 1), (0, top), (top, 0)]:
        rep, out, _, _ = run(lambda b, v: {"lt": b.less_than(v["x"], v["y"], n)}, {"x": x, "y": y})
        assert rep == OK and out["lt"] == int(x < y), (x, y)


def test_assert_range():
    assert run(lambda b, v: b.assert_range(v["x"], 8), {"x": 255})[0] == OK
    rep = run(lambda b, v: b.assert_range(v["x"], 8), {"x": 256})[0]
    assert rep["bad_copies"] == 1 and rep["bad_rows"] == 0
    rep = run(lambda b, v: b.assert_range(v["x"], 8), {"x": R - 1})[0]  # "minus one" is far above 2^8
    assert rep["bad_copies"] == 1 and rep["bad_rows"] == 0


# ---- soundness of the constraints: another value in the place of an advice output ----
def _tampered(make, inputs, new):
    """make returns the variable of ONE advice row.  Generate, then put new(old) into that row's c AND into every slot of its class -- the
    copies agree, the rows computed from the old value stand as they were -- and check"""
    from zkhip.circuit import Builder

    b = Builder()
    priv = {k: b.private() for k in inputs}
    adv_var = make(b, {k: b.lin(1, v, 0, None, 0) for k, v in priv.items()})
    circuit, layout = b.build()
    free = [0] * (3 * layout.N)
    for k, v in inputs.items():
        free[layout.slot(priv[k])] = v % R
    p = am.plan(circuit)
    pi = wm.limbs([0] * circuit["l"])
    w = list(am.generate(circuit, p, pi, free))
    x, N = layout.row(adv_var), layout.N
    assert p["kind"][x] == am.ADVICE
    flat = w[0] + w[1] + w[2]
    value = new(flat[2 * N + x]) % R
    for s in range(3 * N):
        if p["src"][s] == (False, x):
            flat[s] = value
    a, b_, c = flat[:N], flat[N:2 * N], flat[2 * N:]
    return am.check(circuit, p, a, b_, c, pi), layout, x


def test_a_false_is_zero_is_reported():
    """claim is_zero = 1 for a non-zero x: the prover hands in i = 0, z = 1 -- the assertion x z = 0 fails"""
    def make(b, v):
        make.i = b.inv0(v["x"])
        make.z = b.mul(v["x"], make.i, -1, 1)
        b.assert_zero_of(0, v["x"], 0, make.z, 1, 0)
        return make.i

    rep, layout, x = _tampered(make, {"x": 5}, lambda old: 0)
    # with i = 0 the honest z row would give 1; the stale z = 0 is a bad gate row at the mul row -- whichever z the prover writes, one of
    # the two rows after the advice fails
    assert rep["bad_rows"] >= 1 and rep["first_bad_row"] in (x + 1, x + 2)


def test_a_false_is_zero_with_a_consistent_z_is_reported():
    from zkhip.circuit import Builder

    b = Builder()
    xp = b.private()
    x = b.lin(1, xp, 0, None, 0)
    z = b.is_zero(x)
    circuit, layout = b.build()
    free = [0] * (3 * layout.N)
    free[layout.slot(xp)] = 5
    p = am.plan(circuit)
    pi = wm.limbs([0] * circuit["l"])
    a, b_, c = am.generate(circuit, p, pi, free)
    N, rz = layout.N, layout.row(z)
    ri = rz - 1
    c[ri] = 0                 # the advice: "no inverse"
    b_[rz] = 0                # its copy on the z row
    c[rz] = 1                 # z = 1 - x * 0: the z row holds
    b_[rz + 1] = 1            # z's copy on the assertion row: x * 1 != 0
    rep = am.check(circuit, p, a, b_, c, pi)
    assert rep["bad_copies"] == 0 and rep["bad_rows"] == 1 and rep["first_bad_row"] == rz + 1


@pytest.mark.parametrize("k", [0, 3, 7])
def test_a_flipped_bit_is_reported(k):
    def make(b, v):
        bits = b.to_bits(v["x"], 8)
        return bits[k]

    rep, layout, x = _tampered(make, {"x": 0xA5}, lambda old: old ^ 1)
    assert rep["bad_rows"] + rep["bad_copies"] >= 1  # the recomposition no longer holds: the first lin row that read the bit
    rep2, _, _ = _tampered(make, {"x": 0xA5}, lambda old: old + 2)  # not a bit at all: its assert_bool row as well
    assert rep2["bad_rows"] >= 1


# ---- what does not change ----
def test_circuits_without_advice_are_what_they_were():
    from zkhip import poseidon as ps
    from zkhip.circuit import Builder, circuit_digest

    circuit, _, _ = ps.merkle_update_circuit(1, 1)
    assert "advice" not in circuit
    # the digest test_host_merkle_state's cases print for (1, 1): recorded from the commit before advice existed
    assert circuit_digest(circuit) == "290ed8986488c464fcc9ea771174ce7e944e0637b9d2615d13a27874f4d0bd66"
    b = Builder()
    b.mul(b.private(), b.private())
    assert "advice" not in b.build()[0]
    b.inv0(b.private())
    c2 = b.build()[0]
    assert list(c2["advice"]) == [0, 0, 1, 0] and circuit_digest(c2) != circuit_digest({k: v for k, v in c2.items() if k != "advice"})


def test_model_codes():
    assert am.bits(3, 5) == 2 | 3 << 8 | 5 << 16
    for code in (0, 1, am.bits(0, 1), am.bits(0, 64), am.bits(191, 64), am.bits(254, 1)):
        assert am.known(code)
    for code in (3, am.bits(0, 0), am.bits(0, 65), am.bits(192, 64), am.bits(255, 1), 1 | 1 << 24, 2 | 1 << 16 | 1 << 31, 1 | 1 << 8, 1 << 8):
        assert not am.known(code)
    assert am.value(am.bits(60, 8), 0xAB << 60) == 0xAB and am.value(1, 0) == 0 and am.value(1, 2) * 2 % R == 1


def test_plonk_code_helpers():
    from zkhip import plonk

    assert plonk.ADV_INV0 == am.INV0 and plonk.adv_bits(60, 8) == am.bits(60, 8)
    for shift, width in ((0, 0), (0, 65), (192, 64), (-1, 3)):
        with pytest.raises(ValueError):
            plonk.adv_bits(shift, width)


@pytest.mark.parametrize("depth,bits", [(1, 8), (2, 16)])
def test_transfer_digest_agrees_between_the_hosts(depth, bits):
    subprocess.check_call(["make", "-C", HOST, "-s", "bin/poseidon_check"])
    args = ["--depth", str(depth), "--transfer", "--bits", str(bits), "--sample-only"]
    cpp = subprocess.run([os.path.join(HOST, "bin", "poseidon_check"), *args], capture_output=True, text=True, timeout=600)
    py = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "poseidon_merkle.py"), *args], capture_output=True, text=True, timeout=600)
    assert cpp.returncode == 0 and py.returncode == 0, (cpp.stderr, py.stderr)
    lines = cpp.stdout.splitlines()
    assert lines == py.stdout.splitlines() and len(lines) == 2
    assert lines[0].startswith("circuit sha256 ") and lines[1].startswith("roots ") and len(lines[1].split()) == 3


def test_transfer_circuit_in_the_model():
    """the transfer circuit's witness by the model: accepted on a good transfer; amount 0 a bad gate row; an amount above the balance, an
    overflowing receiver and a wrong sibling bad copies"""
    import transfer_cases as tc

    case = tc.case(1, 8)
    for name, want in tc.EXPECTED.items():
        rep = tc.model_report(case, name)
        assert (rep["bad_rows"] > 0, rep["bad_copies"] > 0) == want, (name, rep)
