"""
A small circuit builder for the WIDE gate

    qL a + qR b + qM a b + qH a^5 - qO c + qC + in = 0

that emits the circuit dict `plonk.preprocess` and `plonk.witness_plan` take (the same in host/zkhost/circuit.hpp).  Variables are integers
handed out by the builder.  Every call below appends ONE row and returns the variable that names the row's c:

    public()                                an input row: qO = 1, all else 0, c = the public input.  Must precede every other row
    lin(ka, x, kb, y, kc)                   c = ka x + kb y + kc              (qL = ka, qR = kb, qC = kc, qO = 1)
    mul(x, y, k=1, kc=0)                    c = k x y + kc                    (qM = k, qC = kc, qO = 1)
    pow5(x, kc=0)                           c = x^5 + kc                      (qH = 1, qC = kc, qO = 1)
    assert_zero_of(ka, x, kb, y, km, kc)    ka x + kb y + km x y + kc = 0: a NON-COMPUTING row, qO = 0; its c is unused and tied to nothing
    assert_bool(x)                          x x - x = 0, one assert_zero_of row

    inv0(x)                                 an ADVICE row (plonk module text, WITNESS): every selector 0, code ADV_INV0, c = 1 / x, or 0 for x = 0
    bits_of(x, shift, width)                an advice row, code adv_bits(shift, width): c = bits shift .. shift + width - 1 of x's canonical integer

An advice row constrains NOTHING: the witness generator fills its c, and a prover may put any value there.  The gadgets below add the gate
rows that make the value mean something.  They are plain calls of the rows above (rows appended in brackets):

    inverse(x) -> i            [2]          i = inv0(x) and the assertion x i = 1: no witness exists for x = 0
    div(n, d) -> q             [3]          inverse(d), q = n i
    assert_nonzero(x)          [2]          inverse(x), its output dropped
    is_zero(x) -> z            [3]          i = inv0(x), z = 1 - x i, the assertion x z = 0: z = 1 for x = 0 and z = 0 otherwise, whatever i holds
    is_equal(x, y) -> z        [4]          is_zero(x - y)
    select(bit, x, y) -> v     [3]          v = y + bit (x - y): x when bit = 1, y when bit = 0 (the bit is not asserted boolean here)
    to_bits(x, n) -> [n bits]  [3n - 1]     n rows bits_of(x, k, 1), n assert_bool rows, n - 1 lin rows b_0 + 2 b_1 + ... + 2^(n-1) b_(n-1), and
                                            assert_equal(sum, x).  1 <= n <= 253: the sum stays below r, so the bits are unique (ValueError above).
                                            x must name a COMPUTED value (a row's c, a public input): tied to a private variable alone, the
                                            sum would become the source of x's class and the bits_of rows would depend on their own output
                                            -- the witness plan refuses that.  Pass lin(1, x, 0, None) for a private x.
    to_bits_strict(x) -> [255 bits]  [1018] the bits of x's CANONICAL integer and of no other: 255 rows bits_of(x, k, 1), 255 assert_bool rows, 254 lin
                                            rows of the sum, assert_equal(sum, x) -- which alone would also admit the bits of x + r (2^255 > r) --
                                            and 254 rows that compare the bit vector with the constant r - 1 from the top bit down: with e = "every
                                            higher bit equals that of r - 1" (e starts as bit 254, which r - 1 has set), a position where r - 1 has
                                            a 1 is the row e <- e b_k, a position where it has a 0 is the assertion e b_k = 0.  The bits of x + r
                                            exceed r - 1, so they meet such an assertion with e = 1: NO witness.  x must name a computed value,
                                            as for to_bits.
    assert_bits_at_most(bits, c)  [n - 1]   for n boolean variables (the caller's assertion), least significant first, and a constant c of exactly n
                                            bits: the integer of the bits is <= c, by the comparison to_bits_strict describes
    assert_range(x, n)         [3n - 1]     to_bits(x, n), its bits dropped: x < 2^n
    less_than(x, y, n) -> bit  [3n + 4]     for x, y < 2^n (the caller's assertion), n <= 252: d = x - y + 2^n, to_bits(d, n + 1), bit = 1 - its
                                            top bit: 1 iff x < y

and two calls append nothing:

    private()                               a free variable: its value comes from free[s] at the smallest slot s of its class
    assert_equal(x, y)                      puts both variables into one copy class

Coefficients are python integers, taken mod r.  An operand whose coefficient is 0 may be None: its slot then belongs to no class.

build() -> (circuit, layout).  The public rows come first, padded with input rows of value 0 to l = a power of two (l = 1 without any);
the other rows follow in the order of the calls; mu is the smallest value with N = 2^mu >= rows and N >= 2 l (and mu >= 1); the unused rows
have all-zero selectors (qO = 0: they compute nothing).  circuit = {"gate": "wide", "mu", "l", "qL", "qR", "qM", "qO", "qC", "qH": [N, 4]
Montgomery Fr, "sigma": [3N] u64} and, only when an advice row was used, "advice": [N] u32 codes (0 on every other row).  SIGMA: the slots of a class are the a / b / c slots (slot = column * N + row) of every variable in
it; sigma is ONE cycle per class over its slots in increasing slot order (the largest slot maps to the smallest) and every slot that
belongs to no class is a fixed point -- so the result is deterministic and equal in both hosts.

The builder does not decide satisfiability: plonk.witness / check_witness do, by the witness rules of the plonk module.  A class with
a computing c slot takes its value from the smallest such row; a second computing c slot in the class is an equality assertion, which
is how assert_equal(output, public input) works.  A class of private variables only is free and takes free[smallest slot]:
layout.free({variable: value}) builds that array.  Out of scope: the basic gate, lookups (lookup-based range checks among them),
optimisation passes.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .field import R_MOD

SELECTORS = ("qL", "qR", "qM", "qO", "qC", "qH")
ADV_INV0 = 1  # the advice codes of the plonk module text (plonk.ADV_INV0, plonk.adv_bits)


def adv_bits(shift: int, width: int) -> int:
    if not (0 <= shift and 1 <= width <= 64 and shift + width <= 255):
        raise ValueError(f"no advice code for shift {shift}, width {width}: 0 <= shift, 1 <= width <= 64 and shift + width <= 255 are needed")
    return 2 | shift << 8 | width << 16


def _limbs(xs) -> np.ndarray:
    """canonical integers -> [n, 4] u64 Montgomery limbs"""
    return np.frombuffer(b"".join(((x << 256) % R_MOD).to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


class Layout:
    """where a built circuit keeps its variables: N, l, mu, rows (used ones), and per variable the smallest slot of its class"""

    def __init__(self, mu: int, l: int, rows: int, slot: dict, row: dict):
        self.mu, self.N, self.l, self.rows, self._slot, self._row = mu, 1 << mu, l, rows, slot, row

    def slot(self, var: int) -> int:
        """the smallest slot of the variable's class: where `free` is read for a free class"""
        return self._slot[var]

    def row(self, var: int) -> int:
        """the row whose c the variable names (KeyError for a private variable)"""
        return self._row[var]

    def free(self, values: dict) -> np.ndarray:
        """{private variable: integer} -> the [3N, 4] `free` array of plonk.witness (zero wherever nothing is given)"""
        out = np.zeros((3 * self.N, 4), dtype=np.uint64)
        for var, v in values.items():
            out[self._slot[var]] = _limbs([int(v) % R_MOD])[0]
        return out


class Builder:
    def __init__(self):
        self._publics = 0
        self._rows = []      # (selectors: six ints in SELECTORS order, a, b: variable or None, c: variable or None, advice code), the rows after the input rows
        self._parent = []    # union-find over the variables
        self._c_row = {}     # variable -> ("pub", i) / ("row", i)

    # ---- variables ----
    def _new(self) -> int:
        self._parent.append(len(self._parent))
        return len(self._parent) - 1

    def _find(self, v: int) -> int:
        while self._parent[v] != v:
            self._parent[v] = self._parent[self._parent[v]]
            v = self._parent[v]
        return v

    def _var(self, v, k: int):
        if v is None:
            if k % R_MOD:
                raise ValueError("an operand with a non-zero coefficient is needed")
            return None
        if not (isinstance(v, int) and 0 <= v < len(self._parent)):
            raise ValueError(f"not a variable of this builder: {v!r}")
        return v

    def _row(self, sel: dict, a, b, computing: bool, advice: int = 0):
        c = self._new() if computing else None
        if computing:
            self._c_row[c] = ("row", len(self._rows))
        self._rows.append(([int(sel.get(k, 0)) % R_MOD for k in SELECTORS], a, b, c, advice))
        return c

    # ---- rows ----
    def public(self) -> int:
        if self._rows:
            raise ValueError("public() must precede every other row")
        v = self._new()
        self._c_row[v] = ("pub", self._publics)
        self._publics += 1
        return v

    def private(self) -> int:
        return self._new()

    def lin(self, ka: int, x, kb: int, y, kc: int = 0) -> int:
        return self._row({"qL": ka, "qR": kb, "qC": kc, "qO": 1}, self._var(x, ka), self._var(y, kb), True)

    def mul(self, x, y, k: int = 1, kc: int = 0) -> int:
        return self._row({"qM": k, "qC": kc, "qO": 1}, self._var(x, 1), self._var(y, 1), True)

    def pow5(self, x, kc: int = 0) -> int:
        return self._row({"qH": 1, "qC": kc, "qO": 1}, self._var(x, 1), None, True)

    def assert_zero_of(self, ka: int, x, kb: int, y, km: int, kc: int) -> None:
        self._row({"qL": ka, "qR": kb, "qM": km, "qC": kc}, self._var(x, (ka % R_MOD) or (km % R_MOD)), self._var(y, (kb % R_MOD) or (km % R_MOD)), False)

    def assert_bool(self, x) -> None:
        self.assert_zero_of(-1, x, 0, x, 1, 0)

    # ---- advice rows and the gadgets on them (module text) ----
    def inv0(self, x) -> int:
        return self._row({}, self._var(x, 1), None, True, ADV_INV0)

    def bits_of(self, x, shift: int, width: int) -> int:
        return self._row({}, self._var(x, 1), None, True, adv_bits(shift, width))

    def inverse(self, x) -> int:
        i = self.inv0(x)
        self.assert_zero_of(0, x, 0, i, 1, -1)
        return i

    def div(self, n, d) -> int:
        return self.mul(n, self.inverse(d))

    def assert_nonzero(self, x) -> None:
        self.inverse(x)

    def is_zero(self, x) -> int:
        z = self.mul(x, self.inv0(x), -1, 1)
        self.assert_zero_of(0, x, 0, z, 1, 0)
        return z

    def is_equal(self, x, y) -> int:
        return self.is_zero(self.lin(1, x, -1, y, 0))

    def select(self, bit, x, y) -> int:
        return self.lin(1, y, 1, self.mul(bit, self.lin(1, x, -1, y, 0)), 0)

    def to_bits(self, x, n: int) -> list:
        if not 1 <= n <= 253:
            raise ValueError(f"to_bits takes 1 <= n <= 253 bits, not {n}: above that the decomposition would not be unique")
        bits = [self.bits_of(x, k, 1) for k in range(n)]
        for v in bits:
            self.assert_bool(v)
        acc = bits[0]
        for k in range(1, n):
            acc = self.lin(1, acc, 1 << k, bits[k], 0)
        self.assert_equal(acc, x)
        return bits

    def to_bits_strict(self, x) -> list:
        bits = [self.bits_of(x, k, 1) for k in range(255)]
        for v in bits:
            self.assert_bool(v)
        acc = bits[0]
        for k in range(1, 255):
            acc = self.lin(1, acc, 1 << k, bits[k], 0)
        self.assert_equal(acc, x)
        self.assert_bits_at_most(bits, R_MOD - 1)
        return bits

    def assert_bits_at_most(self, bits, c: int) -> None:
        n = len(bits)
        if n < 2 or not (1 << (n - 1)) <= c < (1 << n):
            raise ValueError("assert_bits_at_most takes n >= 2 bits and a constant of exactly n bits")
        e = bits[n - 1]  # c has its top bit set
        for k in range(n - 2, -1, -1):
            if (c >> k) & 1:
                e = self.mul(e, bits[k])
            else:
                self.assert_zero_of(0, e, 0, bits[k], 1, 0)

    def assert_range(self, x, n: int) -> None:
        self.to_bits(x, n)

    def less_than(self, x, y, n: int) -> int:
        if not 1 <= n <= 252:
            raise ValueError(f"less_than takes 1 <= n <= 252 bits, not {n}")
        top = self.to_bits(self.lin(1, x, -1, y, 1 << n), n + 1)[n]
        return self.lin(-1, top, 0, None, 1)

    def assert_equal(self, x, y) -> None:
        rx, ry = self._find(self._var(x, 1)), self._find(self._var(y, 1))
        if rx != ry:
            self._parent[max(rx, ry)] = min(rx, ry)

    # ---- the circuit ----
    def build(self):
        l = 1
        while l < self._publics:
            l *= 2
        rows = l + len(self._rows)
        mu = 1
        while (1 << mu) < rows or (1 << mu) < 2 * l:
            mu += 1
        N = 1 << mu
        sel = {k: [0] * N for k in SELECTORS}
        sel["qO"][:l] = [1] * l
        slots = {}  # class -> its slots
        row_of = {}
        for v, (kind, i) in self._c_row.items():
            x = i if kind == "pub" else l + i
            row_of[v] = x
            slots.setdefault(self._find(v), []).append(2 * N + x)
        advice = np.zeros(N, dtype=np.uint32)
        for i, (s, a, b, c, adv) in enumerate(self._rows):
            x = l + i
            advice[x] = adv
            for k, val in zip(SELECTORS, s):
                sel[k][x] = val
            if a is not None:
                slots.setdefault(self._find(a), []).append(x)
            if b is not None:
                slots.setdefault(self._find(b), []).append(N + x)
        sigma = np.arange(3 * N, dtype=np.uint64)
        smallest = {}
        for cls, ss in slots.items():
            ss.sort()
            smallest[cls] = ss[0]
            for s, t in zip(ss, ss[1:] + ss[:1]):
                sigma[s] = t
        slot = {v: smallest[self._find(v)] for v in range(len(self._parent)) if self._find(v) in smallest}
        circuit = {"gate": "wide", "mu": mu, "l": l, "sigma": sigma}
        circuit.update({k: _limbs(v) for k, v in sel.items()})
        if advice.any():
            circuit["advice"] = advice
        return circuit, Layout(mu, l, rows, slot, row_of)


def circuit_digest(circuit: dict) -> str:
    """SHA-256 of a built circuit: mu and l (one u64 each), the six selectors in SELECTORS order, sigma (u64) and, only when the
    circuit has them, the advice codes (u32), little-endian -- what host/bin/poseidon_check --sample-only prints.  (plonk.circuit_digest is the digest of a SAMPLED circuit, wires and trapdoor included.)"""
    h = hashlib.sha256()
    h.update(int(circuit["mu"]).to_bytes(8, "little") + int(circuit["l"]).to_bytes(8, "little"))
    for k in SELECTORS + ("sigma",):
        h.update(np.ascontiguousarray(circuit[k], dtype="<u8").tobytes())
    if "advice" in circuit:
        h.update(np.ascontiguousarray(circuit["advice"], dtype="<u4").tobytes())
    return h.hexdigest()
