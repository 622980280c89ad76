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

and two calls append nothing:

    private()                               a free variable: its value comes from free[s] at the smallest slot s of its class
    assert_equal(x, y)                      puts both variables into one copy class

Coefficients are python integers, taken mod r.  An operand whose coefficient is 0 may be None: its slot then belongs to no class.

build() -> (circuit, layout).  The public rows come first, padded with input rows of value 0 to l = a power of two (l = 1 without any);
the other rows follow in the order of the calls; mu is the smallest value with N = 2^mu >= rows and N >= 2 l (and mu >= 1); the unused rows
have all-zero selectors (qO = 0: they compute nothing).  circuit = {"gate": "wide", "mu", "l", "qL", "qR", "qM", "qO", "qC", "qH": [N, 4]
Montgomery Fr, "sigma": [3N] u64}.  SIGMA: the slots of a class are the a / b / c slots (slot = column * N + row) of every variable in
it; sigma is ONE cycle per class over its slots in increasing slot order (the largest slot maps to the smallest) and every slot that
belongs to no class is a fixed point -- so the result is deterministic and equal in both hosts.

The builder does not decide satisfiability: plonk.witness / check_witness do, by the witness rules of the plonk module.  A class with
a computing c slot takes its value from the smallest such row; a second computing c slot in the class is an equality assertion, which
is how assert_equal(output, public input) works.  A class of private variables only is free and takes free[smallest slot]:
layout.free({variable: value}) builds that array.  Out of scope: the basic gate, lookups, optimisation passes.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .field import R_MOD

SELECTORS = ("qL", "qR", "qM", "qO", "qC", "qH")


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
        self._rows = []      # (selectors: six ints in SELECTORS order, a, b: variable or None, c: variable or None), the rows after the input rows
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

    def _row(self, sel: dict, a, b, computing: bool):
        c = self._new() if computing else None
        if computing:
            self._c_row[c] = ("row", len(self._rows))
        self._rows.append(([int(sel.get(k, 0)) % R_MOD for k in SELECTORS], a, b, c))
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
        for i, (s, a, b, c) in enumerate(self._rows):
            x = l + i
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
        return circuit, Layout(mu, l, rows, slot, row_of)


def circuit_digest(circuit: dict) -> str:
    """SHA-256 of a built circuit: mu and l (one u64 each), the six selectors in SELECTORS order, sigma (u64), little-endian -- what
    host/bin/poseidon_check --sample-only prints.  (plonk.circuit_digest is the digest of a SAMPLED circuit, wires and trapdoor included.)"""
    h = hashlib.sha256()
    h.update(int(circuit["mu"]).to_bytes(8, "little") + int(circuit["l"]).to_bytes(8, "little"))
    for k in SELECTORS + ("sigma",):
        h.update(np.ascontiguousarray(circuit[k], dtype="<u8").tobytes())
    return h.hexdigest()
