"""
HyperPlonk for ONE circuit: the gate ZeroCheck and the wiring PermCheck over the three wire columns on the SAME committed wires,
under one Fiat-Shamir transcript, closed by two opening proofs.

A circuit has N = 2^mu rows (gates) with selectors q1, q2 and wires a, b, c:

    q1(x) (a(x) + b(x)) + q2(x) a(x) b(x) - c(x) + in(x) = 0          in: rows 0 .. l - 1 hold the public inputs, the rest is zero

and a permutation sigma of the 3N wire slots (slot j N + x = wire j of row x; a, b, c = columns 0, 1, 2) whose cycles carry one value
each.  ssigma_j(x) = sigma(j N + x) as a field element.  With

    n_j = w_j + alpha (j N + x) + beta,   d_j = w_j + alpha ssigma_j + beta,   h = n_0 n_1 n_2 / (d_0 d_1 d_2),   v = product_tree(h)

the copy constraints hold iff v(1,..,1,0) = 1, and v is tied to the wires by ONE degree-5 sumcheck on N rows (zk_sumcheck_perm3_fs):

    sum_x eq(tau_p, x) [ v(1,x) - v(x,0) v(x,1) + gamma ( h(x) d_0 d_1 d_2 - n_0 n_1 n_2 ) ] = 0

Nothing but q1, q2, ssigma_0..2 is preprocessed: the verifier evaluates `in` and the slot polynomial itself (in_eval, slot_eval).

Schedule (label "plonk"; the same in host/zkhost/plonk.hpp):
  1. absorb mu, l (one u64 each), the five vk commitments (q1, q2, ssigma_0, ssigma_1, ssigma_2), the l public inputs;
  2. absorb the commitments of a, b, c;  alpha, beta <- challenges;
  3. the derived tables and the tree; absorb the tree's commitment;  gamma <- challenge;
  4. tau_p <- mu challenges; the wiring sumcheck: per round absorb its six evaluations, r_p[i] <- challenge;
  5. tau_g <- mu challenges; the gate sumcheck on (eq, q1, q2, a, b, c, in): per round absorb its five evaluations, r_g[i] <- challenge;
  6. absorb the claimed values: q1, q2, a, b, c at r_g ("g_values"); a, b, c, ssigma_0..2 at r_p ("p_values"); the tree at the five
     wiring.V_POINTS of r_p ("v_values");  b_alpha <- challenge;
  7. the mu-variate batch instance (eleven claims on the eight tables q1, q2, a, b, c, ssigma_0..2 at the two points), then the
     (mu + 1)-variate one (five claims on the tree): per round absorb (t0, t1, t2), rho[i] <- challenge.  Two opening proofs.

A SECOND arithmetisation lives beside this one: a circuit that carries "gate": "wide" and the selectors qL, qR, qM, qO, qC, qH in the place
of q1, q2 is proved against the wide gate

    qL a + qR b + qM a b + qH a^5 - qO c + qC + in = 0

under the label "plonk-wide": nine vk commitments (the six selectors, ssigma_0..2), the gate sumcheck zk_sumcheck_gate_wide_fs with EIGHT
evaluations per round, nine values at r_g (the selectors, a, b, c), a mu-variate batch instance of twelve tables and fifteen claims.
Everything else -- the schedule, the permutation half, the (mu + 1)-variate instance -- is the same code: GATES holds one description per
gate kind (label, selector names, evaluations per round, the device sumcheck, the verifier's closed form).  The wide record and vk carry
"gate": "wide"; a circuit, key or record without the key is of the basic kind and behaves exactly as before.

LOOKUPS.  A circuit may carry "lookup": {"qk", "t0", "t1", "t2": [N, 4]}: qk is a selector (0 or 1) and the table holds N triples (pad it by
repeating an entry).  Row x with qk(x) = 1 claims (a, b, c)(x) = (t0, t1, t2)(idx[x]) for the prover's row-to-table indices idx (u32[N]); a
row with qk(x) = 0 claims nothing.  With challenges zeta, beta_l, gamma_l, lambda and a point tau_l (LogUp with a selector):

    f = a + zeta b + zeta^2 c,  t = t0 + zeta t1 + zeta^2 t2,  df = beta_l + f,  dt = beta_l + t,  hf = qk / df,  ht = m / dt,
    m[y] = #{x : qk(x) = 1, idx[x] = y}            (idx = FIND: the device finds the first occurrence of every selected triple itself,
                                                     zk_lookup3_find, and the record is the one of prove with those indices),
    sum_x hf(x) - ht(x) + E(x) [ hf(x) df(x) - qk(x) + gamma_l ( ht(x) dt(x) - m(x) ) ] = 0,      E = lambda eq(tau_l, .)

one degree-3 sumcheck over the seven tables E, df, dt, m, hf, ht, qk (zk_sumcheck_lookup_sel_fs).  f is not committed: df(r) is linear in
a(r), b(r), c(r), which the wire commitments carry.  The lookup is orthogonal to the gate kind; the label is the gate's + "-lookup".  pk,
vk and the record carry "lookup"; the vk commitments are the gate's followed by those of qk, t0, t1, t2.  Insertions into the schedule:
  2L. after alpha, beta: m; absorb its commitment;  zeta, beta_l <- challenges;
  3L. after gamma: df, dt, hf, ht; absorb the commitments of hf and ht;  gamma_l, lambda <- challenges;
  5L. after the gate sumcheck: tau_l <- mu challenges; the lookup sumcheck: per round absorb its four evaluations, r_l[i] <- challenge;
  6.  after v_values absorb "l_values": a, b, c, qk, t0, t1, t2, m, hf, ht at r_l;
  7.  the mu-variate instance gains three claims (a, b, c at r_l) after the existing ones; after the (mu + 1)-variate instance comes a THIRD
      one: the seven tables qk, t0, t1, t2, m, hf, ht with seven claims at r_l (zk_sumcheck_multi takes at most 16 tables: the wide kind's
      twelve and these seven do not fit one instance).  Three opening proofs.
The record gains "lookup": {"commitments": [3, 18] (m, hf, ht), "rounds": [mu, 4, 4], "values": [10, 4], "batch": {"rounds": [mu, 3, 4],
"opening": [mu, 18]}}.  A circuit, key or record without "lookup" behaves exactly as before.

WITNESS.  witness_plan / witness / check_witness make and check the wires a, b, c of a circuit on the device (zk_witness_plan_create,
zk_plonk_witness, zk_plonk_witness_check); preprocess and prove are not involved.  The rules (the same in include/zkhip.h):
  * the classes are the cycles of sigma; every class carries one value;
  * row x is COMPUTING when its output coefficient is non-zero.  Basic gate: every row, c = q1 (a + b) + q2 a b + in(x).  Wide gate: the
    rows with qO(x) != 0, c = (qL a + qR b + qM a b + qH a^5 + qC + in(x)) / qO(x).  in holds the public inputs on rows 0 .. l - 1 and
    zero elsewhere: an input row is the same rule, no special case;
  * the SOURCE of a class is the smallest c slot of a computing row in it.  A class without one is FREE: its value is free[s] for its
    smallest slot s (free: 3N Fr, read only at those slots; absent: 0).  Every slot of the class that is not itself the c slot of a
    computing row takes the class's value; every computing row computes its own c, so a second computing c slot in one class is an
    equality assertion -- checked, not assigned;
  * the LEVEL of a computing row is 0 when the classes of both its a and b slots are free, otherwise 1 + the largest level of the source
    rows of those classes.  A row that depends on itself, directly or through other rows, has no level: the plan is refused ("K of N
    rows depend on their own output" and the smallest such row);
  * the check: row x is a bad gate row when the gate identity does not hold on it (after generation only a non-computing row can be);
    slot s is a bad copy when its value differs from its class's value (after generation only a further computing c slot can be).  On
    caller-given a, b, c every row and slot can fail.
A plan built with lookup=True also knows the circuit's lookup (zk_witness_plan_create_lookup; additive -- without it the rules above hold
and nothing else):
  * the table must be a FUNCTION of its first two columns: two entries with equal (t0, t1) have equal t2 (repeating a whole entry is
    allowed); otherwise the plan is refused ("K of N table entries repeat the pair (t0, t1) of an earlier entry with another t2" and the
    smallest such entry), as it is for a qk entry that is neither 0 nor 1;
  * row x is LOOKUP-COMPUTING when qk(x) = 1 and it is not gate-computing (wide gate: qO(x) = 0; basic gate: never).  Its c is t2[y] for
    the smallest y with (t0, t1)[y] = (a, b)(x); without such a y its c is 0 and the check reports the row.  A row with qk = 1 that is
    gate-computing stays gate-computing: the table only checks it.  "Computing" in the rules above means either kind;
  * the check gains the BAD LOOKUPS: the rows with qk = 1 whose (a, b, c) is no table entry, of either kind; `witness` refuses them ("K
    of N rows with qk = 1 hold a triple that is no table entry" and the smallest such row);
  * on generated wires the index zk_lookup3_find gives for a lookup-computing row is the y the generator used, so
    prove(..., idx=FIND) on them needs nothing from the generator.
A circuit may carry ADVICE, "advice": N u32 codes, one per row, 0 meaning none (zk_witness_plan_create_advice; additive -- a circuit
without it follows the rules above and nothing else).  Advice is prover-side only: not preprocessed, not committed, in no vk, proof or
existing digest.
  * ADV_INV0 = 1: c = 1 / a mod r, and c = 0 when a = 0; b is gathered and stored as usual, not used.  adv_bits(shift, width) =
    2 | shift << 8 | width << 16: c = (A >> shift) mod 2^width for the canonical integer A in [0, r) of a; 0 <= shift,
    1 <= width <= 64, shift + width <= 255.  Bits 24 .. 31 are 0; anything else is an unknown code and the plan is refused ("K of N
    advice codes are unknown" and the smallest such row);
  * a row with a code is ADVICE-COMPUTING: a computing row like the other two kinds for sources, levels and the refusal of rows that depend
    on their own output.  It must not also compute by the gate (wide gate: qO(x) = 0; the basic gate computes on every row, so every
    non-zero code is refused) or by the table (qk(x) = 0): "K of N advice rows also compute by the gate or the table";
  * it constrains nothing by itself -- soundness comes from ordinary gate rows next to it (circuit.Builder's gadgets) -- and the check
    does not test advice values: it keeps its four (lookup plans: six) numbers, and a witness may hold other advice where the
    constraints allow it (any c for ADV_INV0 of 0);
  * the outputs are fully reduced Montgomery forms like every generated wire; a free value or public input at or above r is reduced
    before the advice acts on it.

Record: {"mu", "l", "commitments": [3, 18] (a, b, c), "v_commitment": [18], "p_rounds": [mu, 6, 4], "g_rounds": [mu, 5, 4],
         "g_values": [5, 4], "p_values": [6, 4], "v_values": [5, 4], "batch": {"rounds": [mu, 3, 4], "opening": [mu, 18]},
         "v_batch": {"rounds": [mu + 1, 3, 4], "opening": [mu + 1, 18]}}.
The SRS has mu + 1 variables and the mu-variate tables use the last mu of them (wiring.verifying_keys).  Single party only.
"""
from __future__ import annotations

import hashlib

import numpy as np

from . import batch_open as bo
from . import wiring as wr
from .field import R_MOD, fr_from_mont, fr_mont
from .proof_io import check_points, parse_proof, proof_from_bytes, proof_to_bytes, verify_bytes, verify_bytes_many  # noqa: F401  (proof bytes, re-exported)
from .srs_io import check_srs, parse_srs, restrict, srs_check_host, srs_from_bytes, srs_to_bytes  # noqa: F401  (parameter-set bytes, re-exported)
from .transcript import HostTranscript, Transcript
from .vk_io import check_vk, g2_records, parse_vk, verify_files, vk_from_bytes, vk_to_bytes  # noqa: F401  (vk bytes and the file verifier, re-exported)
from .verify import _ints, _u64, eq_eval, round_chain, round_poly_at  # noqa: F401  (round_poly_at: importable from here as before)
from .zerocheck import gate_value, wide_gate_value

LABEL = b"plonk"
VK_TABLES = ("q1", "q2", "ssigma0", "ssigma1", "ssigma2")
G_VALUES = ("q1", "q2", "a", "b", "c")                              # at r_g
P_VALUES = ("a", "b", "c", "ssigma0", "ssigma1", "ssigma2")          # at r_p
BATCH_TABLES = ("q1", "q2", "a", "b", "c", "ssigma0", "ssigma1", "ssigma2")  # the tables of the mu-variate batch instance
_SSIGMA = ("ssigma0", "ssigma1", "ssigma2")
LOOKUP_SUFFIX = b"-lookup"
FIND = "find"                                                        # in the place of idx: the device finds the indices (zk_lookup3_find)
LOOKUP_VK_TABLES = ("qk", "t0", "t1", "t2")                          # preprocessed; their commitments follow the gate's in the vk
LOOKUP_COMMITTED = ("m", "hf", "ht")                                  # the prover's commitments of the record's "lookup" part
L_VALUES = ("a", "b", "c", "qk", "t0", "t1", "t2", "m", "hf", "ht")  # at r_l
L_BATCH_TABLES = L_VALUES[3:]                                         # the tables of the third batch instance


class Gate:
    """One gate kind: what prove / challenges / failed_checks / verify need to know about the gate identity"""

    def __init__(self, kind, label: bytes, selectors: tuple, evals: int, sumcheck, value):
        self.kind, self.label, self.selectors, self.evals = kind, label, selectors, evals
        self.vk_tables = selectors + _SSIGMA                      # the preprocessed tables, in the order of the vk commitments
        self.g_values = selectors + ("a", "b", "c")               # the claimed values at r_g = the folded-out g_last[1 : 1 + len]
        self.batch_tables = self.g_values + _SSIGMA               # the tables of the mu-variate batch instance
        self.sumcheck = sumcheck                                  # (be, eq, tabs, inp, N, tr) -> (rounds [mu, evals, 4], last, r_g)
        self.value = value                                        # (eq, gv: name -> int, in) -> the identity at one point

    def tag(self) -> dict:
        """what a key or a record of this kind carries"""
        return {} if self.kind is None else {"gate": self.kind}


GATES = {
    None: Gate(None, LABEL, ("q1", "q2"), 5,
               lambda be, eq, t, inp, N, tr: be.sumcheck_gate_fs(eq, t["q1"], t["q2"], t["a"], t["b"], t["c"], inp, N, tr),
               lambda eq, g, inp: gate_value(eq, g["q1"], g["q2"], g["a"], g["b"], g["c"], inp)),
    "wide": Gate("wide", b"plonk-wide", ("qL", "qR", "qM", "qO", "qC", "qH"), 8,
                 lambda be, eq, t, inp, N, tr: be.sumcheck_gate_wide_fs([eq] + [t[k] for k in ("qL", "qR", "qM", "qO", "qC", "qH", "a", "b", "c")] + [inp], N, tr),
                 lambda eq, g, inp: wide_gate_value(eq, g["qL"], g["qR"], g["qM"], g["qO"], g["qC"], g["qH"], g["a"], g["b"], g["c"], inp)),
}


def gate_of(d: dict) -> Gate:
    """the gate kind of a circuit, key or record: the value under "gate" (absent: the basic kind); ValueError for an unknown one"""
    kind = d.get("gate")
    if kind not in GATES:
        raise ValueError(f"unknown gate kind {kind!r}")
    return GATES[kind]


# ---- the verifier's closed forms ----
def in_eval(public_inputs, r) -> int:
    """in(r) for the table whose rows 0 .. l - 1 hold the public inputs (l = 2^k) and whose other rows are zero; index bit 0 is the TOP bit:
    prod_{i < mu - k} (1 - r_i) * sum_y pi[y] eq(y, r_{mu-k..}).  public_inputs, r: python ints"""
    l, mu = len(public_inputs), len(r)
    k = l.bit_length() - 1
    if l != 1 << k or k > mu:
        raise ValueError("the public-input count must be a power of two <= 2^mu")
    head = 1
    for x in r[: mu - k]:
        head = head * (1 - x) % R_MOD
    acc = 0
    for y, p in enumerate(public_inputs):
        bits = [(y >> (k - 1 - i)) & 1 for i in range(k)]
        acc = (acc + p * eq_eval(bits, r[mu - k:])) % R_MOD
    return head * acc % R_MOD


def slot_eval(r) -> int:
    """the multilinear extension of x -> x at r: sum_i 2^(mu-1-i) r_i (index bit 0 is the TOP bit)"""
    mu = len(r)
    return sum(x << (mu - 1 - i) for i, x in enumerate(r)) % R_MOD


def lookup3_value(E: int, a: int, b: int, c: int, qk: int, t0: int, t1: int, t2: int, m: int, hf: int, ht: int, zeta: int, beta: int, gamma: int) -> int:
    """hf - ht + E [ hf (beta + a + zeta b + zeta^2 c) - qk + gamma ( ht (beta + t0 + zeta t1 + zeta^2 t2) - m ) ]"""
    df, dt = beta + a + zeta * b + zeta * zeta * c, beta + t0 + zeta * t1 + zeta * zeta * t2
    return (hf - ht + E * (hf * df - qk + gamma * (ht * dt - m))) % R_MOD


def has_lookup(d: dict) -> bool:
    """whether a circuit, key or record carries the lookup part"""
    return d.get("lookup") is not None and d.get("lookup") is not False


def label_of(gate: Gate, lookup: bool) -> bytes:
    return gate.label + LOOKUP_SUFFIX if lookup else gate.label


def perm3_value(eq: int, v1x: int, vx0: int, vx1: int, h: int, n, d, gamma: int) -> int:
    return eq * (v1x - vx0 * vx1 + gamma * (h * d[0] * d[1] * d[2] - n[0] * n[1] * n[2])) % R_MOD


# ---- keys ----
def slot_table(be, slots: np.ndarray):
    """integers < 2^64 -> device table of their Montgomery forms (uploaded as integers, multiplied by R^2 on the device)"""
    n = len(slots)
    raw = np.zeros((n, 4), dtype=np.uint64)
    raw[:, 0] = slots
    return be.fr_scale(be.to_device(raw), fr_mont(1 << 256), n)


def preprocess(be, pcs, circuit: dict, powers_of_g2=None):
    """
    circuit: {"mu", "l", "q1": [N, 4], "q2": [N, 4] Montgomery Fr, "sigma": [3N] slot numbers} -- or, with "gate": "wide", the six selectors
    qL, qR, qM, qO, qC, qH in the place of q1, q2 (the commitments then in GATES["wide"].vk_tables order, and pk, vk carry "gate"); pcs: the levels of a PolynomialCommitment
    over mu + 1 variables; powers_of_g2 (optional): the SRS's [g2, s_0 g2, .., s_mu g2], from which the pairing keys of `verify` are made.
    -> (pk, vk): vk = {"mu", "l", "commitments": [5, 18] in VK_TABLES order, "pcs": (vk_mu, vk_mu1) or None, "g2": the [mu + 2, 24]
    Montgomery records of powers_of_g2 or None -- read by vk_io.vk_to_bytes / check_vk only}; pk keeps the device tables.
    A circuit with "lookup" (module text): qk is checked to hold only 0 and 1, qk, t0, t1, t2 are committed after the gate's tables, and pk, vk
    carry "lookup": True.
    """
    from . import dist_primitive as dp

    gate = gate_of(circuit)
    mu, l = int(circuit["mu"]), int(circuit["l"])
    N = 1 << mu
    sigma = np.ascontiguousarray(circuit["sigma"], dtype=np.uint64).reshape(-1)
    if mu < 1 or l < 1 or l & (l - 1) or 2 * l > N:
        raise ValueError("mu >= 1 and l = 2^k <= N / 2 are needed")
    if len(sigma) != 3 * N or not np.array_equal(np.sort(sigma), np.arange(3 * N, dtype=np.uint64)):
        raise ValueError("sigma is not a permutation of the 3N wire slots")
    tabs = {k: be.to_device(_u64(circuit[k], N, 4)) for k in gate.selectors}
    for j in range(3):
        tabs[f"ssigma{j}"] = slot_table(be, sigma[j * N:(j + 1) * N])
    names, tag = gate.vk_tables, gate.tag()
    if has_lookup(circuit):
        lk = {k: _u64(circuit["lookup"][k], N, 4) for k in LOOKUP_VK_TABLES}
        one = fr_mont(1)
        if not ((lk["qk"] == 0).all(axis=1) | (lk["qk"] == one).all(axis=1)).all():
            raise ValueError("every entry of the lookup selector qk must be 0 or 1")
        tabs.update({k: be.to_device(v) for k, v in lk.items()})
        names, tag = names + LOOKUP_VK_TABLES, dict(tag, lookup=True)
    comms = np.stack([_u64(dp.commit(be, pcs, tabs[k], N), 18) for k in names])
    vk = {"mu": mu, "l": l, "commitments": comms, "pcs": wr.verifying_keys(be, powers_of_g2) if powers_of_g2 is not None else None,
          "g2": g2_records(powers_of_g2) if powers_of_g2 is not None else None, **tag}
    return {"mu": mu, "l": l, "tables": tabs, "commitments": comms, "pcs": pcs, **tag}, vk


# ---- prover ----
def prove(be, pk: dict, a, b, c, public_inputs, idx=None, timing: dict | None = None) -> dict:
    """a, b, c: device buffers of N Fr (or [N, 4] arrays); public_inputs: [l, 4] Montgomery Fr -> the record of the module text.
    idx: the N row-to-table indices (array or device buffer of u32) or FIND (the device finds them), required exactly when the key has a
    lookup (else ValueError; any other string: ValueError); a selected row whose triple is not the table entry it names -- with FIND: no entry
    at all -- raises ValueError.
    A zero denominator raises ZeroDivisionError (ZK_ERR_DIV_ZERO); a zero challenge alpha (probability 2^-254), from which ssigma_j(r_p)
    cannot be recovered, ValueError.  timing (optional dict) receives the wall seconds of the phases."""
    import time

    from . import dist_primitive as dp
    from .nizk import _batch_prove

    gate = gate_of(pk)
    lookup = has_lookup(pk)
    mu, l, pcs = pk["mu"], pk["l"], pk["pcs"]
    N = 1 << mu
    pi = _u64(public_inputs, -1, 4)
    if len(pi) != l:
        raise ValueError(f"{l} public inputs needed, {len(pi)} given")
    if lookup != (idx is not None):
        raise ValueError("idx is needed exactly when the key has a lookup")
    find = isinstance(idx, str)
    if find and idx != FIND:
        raise ValueError(f"idx must be the indices or FIND, not {idx!r}")
    if lookup and not (find or isinstance(idx, int) or hasattr(idx, "ptr") or hasattr(idx, "data_ptr")):  # not on the device: an array or a sequence
        idx = np.asarray(idx)
        if idx.size != N or idx.dtype.kind not in "ui":
            raise ValueError(f"idx must hold {N} unsigned integers")
        idx = be.to_device(np.ascontiguousarray(idx, dtype=np.uint32).reshape(N))
    wires = {k: (be.to_device(_u64(v, N, 4)) if isinstance(v, np.ndarray) else v) for k, v in (("a", a), ("b", b), ("c", c))}
    tabs = dict(pk["tables"], **wires)
    t0 = time.perf_counter()
    comms = np.stack([_u64(dp.commit(be, pcs, wires[k], N), 18) for k in ("a", "b", "c")])
    tr = Transcript(be, label_of(gate, lookup))
    lk_part = {}
    try:
        tr.absorb_u64(mu).absorb_u64(l).absorb(pk["commitments"]).absorb(pi)
        alpha, beta = tr.absorb(comms).challenges(2)
        if not fr_from_mont(alpha):
            raise ValueError("the challenge alpha is zero")
        if lookup:  # 2L
            w_cols, t_cols = [wires[k] for k in ("a", "b", "c")], [tabs[k] for k in ("t0", "t1", "t2")]
            m = be.lookup3_find(w_cols, t_cols, tabs["qk"], N)[1] if find else be.lookup3_multiplicities(w_cols, t_cols, tabs["qk"], idx, N)
            c_m = _u64(dp.commit(be, pcs, m, N), 18)
            zeta, beta_l = tr.absorb(c_m).challenges(2)
        nums, dens, P, Q = be.perm3_terms([wires[k] for k in ("a", "b", "c")], [tabs[f"ssigma{j}"] for j in range(3)], N, alpha, beta)
        tree = be.product_tree(be.fr_batch_div(P, Q, N), N)
        v_comm = _u64(dp.commit(be, pcs, tree, 2 * N), 18)
        t1 = time.perf_counter()
        gamma = tr.absorb(v_comm).challenge()
        if lookup:  # 3L
            df, dt = be.lookup3_terms(w_cols, t_cols, N, zeta, beta_l)
            hf, ht = be.fr_batch_div(tabs["qk"], df, N), be.fr_batch_div(m, dt, N)
            c_hf, c_ht = (_u64(dp.commit(be, pcs, x, N), 18) for x in (hf, ht))
            gamma_l, lam = tr.absorb(np.stack([c_hf, c_ht])).challenges(2)
        p_rounds, p_last, r_p = be.sumcheck_perm3_fs(be.eq_table(tr.challenges(mu)), tree, nums, dens, N, gamma, tr)
        t2 = time.perf_counter()
        inp = np.zeros((N, 4), dtype=np.uint64)
        inp[:l] = pi
        g_rounds, g_last, r_g = gate.sumcheck(be, be.eq_table(tr.challenges(mu)), tabs, be.to_device(inp), N, tr)
        t3 = time.perf_counter()
        if lookup:  # 5L
            E = be.fr_scale(be.eq_table(tr.challenges(mu)), lam, N)
            l_rounds, l_last, r_l = be.sumcheck_lookup_sel_fs([E, df, dt, m, hf, ht, tabs["qk"]], N, gamma_l, tr)
            # a, b, c, t0, t1, t2 at r_l: six folds in one zk_sumcheck_batch, into one buffer, one download
            six, at = ("a", "b", "c", "t0", "t1", "t2"), be.alloc(32 * 6)
            be.sumcheck_batch([("fold", tabs[k], N, r_l, at.at(32 * j)) for j, k in enumerate(six)])
            at_rl = dict(zip(six, at.download((6, 4))))
            at_rl.update(qk=l_last[6], m=l_last[3], hf=l_last[4], ht=l_last[5])  # the folded-out last values
            l_values = np.stack([at_rl[k] for k in L_VALUES])
        t3l = time.perf_counter()
        g_values = g_last[1:1 + len(gate.g_values)]  # the folded-out values ARE the selectors and a, b, c at r_g
        # the folded-out n_j, d_j at r_p give the wires and the permutation columns there: both are linear in them
        al, bt, ids = fr_from_mont(alpha), fr_from_mont(beta), slot_eval(_ints(r_p))
        n_r, d_r = _ints(p_last[5:8]), _ints(p_last[8:11])
        w_r = [(n_r[j] - al * (j * N + ids) - bt) % R_MOD for j in range(3)]
        s_r = [(d_r[j] - w_r[j] - bt) * pow(al, -1, R_MOD) % R_MOD for j in range(3)]
        p_values = np.stack([fr_mont(x) for x in w_r + s_r])
        # the tree at (0,r) = h, (1,r) = v1x, (r,0) = vx0, (r,1) = vx1 are folded-out values too; (1,..,1,0) is tree[2N - 2]
        v_values = np.stack([p_last[4], p_last[1], p_last[2], p_last[3], tree.download((1, 4), offset=32 * (2 * N - 2))[0]])
        tr.absorb(g_values).absorb(p_values).absorb(v_values)
        if lookup:
            tr.absorb(l_values)
        b_alpha = tr.challenge()
        bt_names = gate.batch_tables
        claims = [(bt_names.index(k), r_g, v) for k, v in zip(gate.g_values, g_values)] + [(bt_names.index(k), r_p, v) for k, v in zip(P_VALUES, p_values)]
        if lookup:
            claims += [(bt_names.index(k), r_l, at_rl[k]) for k in ("a", "b", "c")]
        batch, _ = _batch_prove(be, pcs, [tabs[k] for k in bt_names], N, claims, b_alpha, tr)
        v_batch, _ = _batch_prove(be, pcs, [tree], 2 * N, [(0, z, v) for z, v in zip(wr.v_points(r_p), v_values)], b_alpha, tr)
        if lookup:
            l_tabs = dict(tabs, m=m, hf=hf, ht=ht)
            l_batch, _ = _batch_prove(be, pcs, [l_tabs[k] for k in L_BATCH_TABLES], N, [(j, r_l, at_rl[k]) for j, k in enumerate(L_BATCH_TABLES)], b_alpha, tr)
            lk_part = {"lookup": {"commitments": np.stack([c_m, c_hf, c_ht]), "rounds": l_rounds, "values": l_values, "batch": l_batch}}
    finally:
        tr.free()
    t4 = time.perf_counter()
    if timing is not None:
        timing["commit_s"], timing["perm3_s"], timing["gate_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2, t4 - t3l
        if lookup:
            timing["lookup_s"] = t3l - t3
    return {"mu": mu, "l": l, "commitments": comms, "v_commitment": v_comm, "p_rounds": p_rounds, "g_rounds": g_rounds, "g_values": np.array(g_values),
            "p_values": p_values, "v_values": v_values, "batch": batch, "v_batch": v_batch, **gate.tag(), **lk_part}


# ---- witness ----
ADV_INV0 = 1


def adv_bits(shift: int, width: int) -> int:
    """the advice code "bits shift .. shift + width - 1 of a's canonical integer" (module text, WITNESS)"""
    if not (0 <= shift and 1 <= width <= 64 and shift + width <= 255):
        raise ValueError(f"no advice code for shift {shift}, width {width}: 0 <= shift, 1 <= width <= 64 and shift + width <= 255 are needed")
    return 2 | shift << 8 | width << 16


def witness_plan(be, circuit: dict, lookup: bool = False, advice: bool | None = None):
    """the witness plan of a circuit {"mu", "sigma", and with "gate": "wide" the output selector "qO"} (module text, WITNESS): built once per
    circuit on the host inside the library (Ctx.witness_plan).  A sigma that is not a permutation, or rows that depend on their own
    output: ValueError.  lookup=True: the plan of the circuit WITH its "lookup" (required then; Ctx.witness_plan_lookup builds the key
    table of (t0, t1) on the device) -- a qk that is not 0 / 1 or a table that is no function of (t0, t1): ValueError.  The default
    ignores a lookup the circuit may carry.  advice: None uses the circuit's "advice" codes when it has them (Ctx.witness_plan_advice;
    unknown codes, or advice rows that also compute by the gate or the table: ValueError), False ignores them, True requires them."""
    gate = gate_of(circuit)
    N = 1 << int(circuit["mu"])
    if advice and "advice" not in circuit:
        raise ValueError("advice=True needs a circuit with advice codes")
    adv = circuit["advice"] if advice is not False and "advice" in circuit else None
    qo = be.to_device(_u64(circuit["qO"], N, 4)) if gate.kind == "wide" else None
    sigma = np.ascontiguousarray(circuit["sigma"], dtype=np.uint64).reshape(-1)
    if not lookup:
        return be.witness_plan(sigma, N, qo) if adv is None else be.witness_plan_advice(sigma, N, qo, adv)
    if not has_lookup(circuit):
        raise ValueError("lookup=True needs a circuit with a lookup")
    lk = {k: be.to_device(_u64(circuit["lookup"][k], N, 4)) for k in LOOKUP_VK_TABLES}
    if adv is not None:
        return be.witness_plan_advice(sigma, N, qo, adv, lk["qk"], [lk[k] for k in LOOKUP_VK_TABLES[1:]])
    return be.witness_plan_lookup(sigma, N, qo, lk["qk"], [lk[k] for k in LOOKUP_VK_TABLES[1:]])


def witness_key(be, circuit: dict) -> dict:
    """what witness / check_witness read of a proving key, without an SRS or commitments: mu, l, the gate kind and, on the device, the
    selectors and -- for a circuit with a lookup -- qk, t0, t1, t2.  For callers that generate or check wires without proving."""
    gate = gate_of(circuit)
    N = 1 << int(circuit["mu"])
    tabs = {k: be.to_device(_u64(circuit[k], N, 4)) for k in gate.selectors}
    tag = gate.tag()
    if has_lookup(circuit):
        tabs.update({k: be.to_device(_u64(circuit["lookup"][k], N, 4)) for k in LOOKUP_VK_TABLES})
        tag = dict(tag, lookup=True)
    return {"mu": int(circuit["mu"]), "l": int(circuit["l"]), "tables": tabs, **tag}


def _witness_args(pk: dict, plan, public_inputs):
    """-> (selectors, public inputs, the keyword arguments of a lookup plan: qk and ts from the key's tables)"""
    gate = gate_of(pk)
    pi = _u64(public_inputs, -1, 4)
    if len(pi) != pk["l"]:
        raise ValueError(f"{pk['l']} public inputs needed, {len(pi)} given")
    if plan.N != 1 << pk["mu"] or plan.wide != (gate.kind == "wide"):
        raise ValueError("the plan is not one of this key's circuit")
    lk = {}
    if getattr(plan, "lookup", False):
        if any(k not in pk["tables"] for k in LOOKUP_VK_TABLES):
            raise ValueError("a lookup plan needs a key with the lookup's tables")
        lk = {"qk": pk["tables"]["qk"], "ts": [pk["tables"][k] for k in LOOKUP_VK_TABLES[1:]]}
    return [pk["tables"][k] for k in gate.selectors], pi, lk


def witness(be, pk: dict, plan, public_inputs, free=None):
    """the wires of pk's circuit from its public inputs ([l, 4] Montgomery Fr) and the values of its free classes (free: [3N, 4] array or
    device buffer, read at the smallest slot of every free class; None: zeros) -> (a, b, c), device buffers of N Fr that go straight into
    `prove`.  A witness that breaks a gate or a copy constraint: ValueError ("K of N rows ..." / "K of 3N slots ...").  On a lookup plan
    (witness_plan(..., lookup=True)) the lookup-computing rows take their c from pk's table, and a row with qk = 1 whose triple is no
    table entry is refused too."""
    sels, pi, lk = _witness_args(pk, plan, public_inputs)
    if isinstance(free, np.ndarray):
        free = be.to_device(_u64(free, 3 * plan.N, 4))
    return be.plonk_witness(plan, sels, pi, free, **lk)


def check_witness(be, pk: dict, plan, a, b, c, public_inputs) -> dict:
    """any a, b, c (device buffers or [N, 4] arrays) against the gate identity and the copy constraints of pk's circuit ->
    {"bad_rows", "first_bad_row", "bad_copies", "first_bad_copy"}: the counts and the smallest row / slot (None: none); on a lookup plan
    also {"bad_lookups", "first_bad_lookup"}"""
    sels, pi, lk = _witness_args(pk, plan, public_inputs)
    a, b, c = ((be.to_device(_u64(v, plan.N, 4)) if isinstance(v, np.ndarray) else v) for v in (a, b, c))
    return be.plonk_witness_check(plan, sels, pi, a, b, c, **lk)


# ---- verifier ----
def challenges(vk: dict, public_inputs, proof: dict, label: bytes | None = None) -> dict:
    """the verifier's replay of the schedule on hashlib (label: the gate kind's, unless given) -> {"alpha", "beta", "gamma", "tau_p", "r_p",
    "tau_g", "r_g", "b_alpha", "rho_mu", "rho_mu1"} and, with a lookup, {"zeta", "beta_l", "gamma_l", "lambda", "tau_l", "r_l", "rho_l"};
    ValueError / KeyError on a malformed record or statement, a record of another gate kind than the key's or a record / key pair that
    disagrees on having a lookup among them"""
    gate = gate_of(vk)
    if gate_of(proof) is not gate:
        raise ValueError("the record and the key are of different gate kinds")
    lookup = has_lookup(vk)
    if has_lookup(proof) != lookup:
        raise ValueError("the record and the key disagree on having a lookup")
    label = label_of(gate, lookup) if label is None else label
    mu, l = int(vk["mu"]), int(vk["l"])
    pi = _u64(public_inputs, -1, 4)
    p_rounds, g_rounds = _u64(proof["p_rounds"], -1, 6, 4), _u64(proof["g_rounds"], -1, gate.evals, 4)
    b_rounds, v_rounds = _u64(proof["batch"]["rounds"], -1, 3, 4), _u64(proof["v_batch"]["rounds"], -1, 3, 4)
    if int(proof["mu"]) != mu or int(proof["l"]) != l or len(pi) != l:
        raise ValueError("the record, the key and the public inputs disagree on mu / l")
    if mu < 1 or len(p_rounds) != mu or len(g_rounds) != mu or len(b_rounds) != mu or len(v_rounds) != mu + 1:
        raise ValueError("the record does not hold mu / mu + 1 rounds")
    rr = lambda tr, rounds: np.stack([tr.absorb(r).challenge() for r in rounds])
    c = {}
    if lookup:
        lp = proof["lookup"]
        l_comms, l_rounds, lb_rounds = _u64(lp["commitments"], len(LOOKUP_COMMITTED), 18), _u64(lp["rounds"], -1, 4, 4), _u64(lp["batch"]["rounds"], -1, 3, 4)
        l_values = _u64(lp["values"], len(L_VALUES), 4)
        if len(l_rounds) != mu or len(lb_rounds) != mu:
            raise ValueError("the lookup part does not hold mu rounds")
    tr = HostTranscript(label)
    tr.absorb_u64(mu).absorb_u64(l).absorb(_u64(vk["commitments"], len(gate.vk_tables) + (len(LOOKUP_VK_TABLES) if lookup else 0), 18)).absorb(pi)
    alpha, beta = tr.absorb(_u64(proof["commitments"], 3, 18)).challenges(2)
    if lookup:
        c["zeta"], c["beta_l"] = tr.absorb(l_comms[0]).challenges(2)
    gamma = tr.absorb(_u64(proof["v_commitment"], 18)).challenge()
    if lookup:
        c["gamma_l"], c["lambda"] = tr.absorb(l_comms[1:]).challenges(2)
    tau_p = tr.challenges(mu)
    r_p = rr(tr, p_rounds)
    tau_g = tr.challenges(mu)
    r_g = rr(tr, g_rounds)
    if lookup:
        c["tau_l"] = tr.challenges(mu)
        c["r_l"] = rr(tr, l_rounds)
    tr.absorb(_u64(proof["g_values"], len(gate.g_values), 4)).absorb(_u64(proof["p_values"], len(P_VALUES), 4)).absorb(_u64(proof["v_values"], len(wr.V_POINTS), 4))
    if lookup:
        tr.absorb(l_values)
    b_alpha = tr.challenge()
    rho_mu = rr(tr, b_rounds)
    c.update({"alpha": alpha, "beta": beta, "gamma": gamma, "tau_p": tau_p, "r_p": r_p, "tau_g": tau_g, "r_g": r_g, "b_alpha": b_alpha, "rho_mu": rho_mu,
              "rho_mu1": rr(tr, v_rounds)})
    if lookup:
        c["rho_l"] = rr(tr, lb_rounds)
    return c


def _claims(c: dict, proof: dict):
    gate = gate_of(proof)
    g_values, p_values = _u64(proof["g_values"], len(gate.g_values), 4), _u64(proof["p_values"], len(P_VALUES), 4)
    v_values = _u64(proof["v_values"], len(wr.V_POINTS), 4)
    bt_names = gate.batch_tables
    claims = [(bt_names.index(k), c["r_g"], v) for k, v in zip(gate.g_values, g_values)] + [(bt_names.index(k), c["r_p"], v) for k, v in zip(P_VALUES, p_values)]
    if has_lookup(proof):
        l_values = _u64(proof["lookup"]["values"], len(L_VALUES), 4)
        claims += [(bt_names.index(k), c["r_l"], l_values[j]) for j, k in enumerate(("a", "b", "c"))]
    return claims, [(0, z, v) for z, v in zip(wr.v_points(c["r_p"]), v_values)]


def _lookup_claims(c: dict, proof: dict):
    """the seven claims of the third batch instance: L_BATCH_TABLES at r_l"""
    l_values = _u64(proof["lookup"]["values"], len(L_VALUES), 4)
    return [(j, c["r_l"], l_values[3 + j]) for j in range(len(L_BATCH_TABLES))]


def failed_checks(vk: dict, public_inputs, proof: dict, finals=None, v_finals=None, c: dict | None = None, l_finals=None) -> list:
    """
    The verifier's field arithmetic (no GPU, no pairing) -> the numbers of the checks that fail ([] = all hold; [0]: malformed):
      1. the wiring chain: p_0(0) + p_0(1) == 0, p_i(0) + p_i(1) == p_{i-1}(r_{i-1}) by interpolation on the nodes 0 .. 5;
      2. the gate chain, on the nodes 0 .. 4 (the wide kind: 0 .. 7);
      3. the gate's last value == eq(tau_g, r_g) [ q1 (a + b) + q2 a b - c + in(r_g) ] with in(r_g) = in_eval(public inputs) (the wide kind:
         zerocheck.wide_gate_value on its nine values);
      4. the wiring's last value == eq(tau_p, r_p) [ v(1,r) - v(r,0) v(r,1) + gamma ( v(0,r) d_0 d_1 d_2 - n_0 n_1 n_2 ) ] with
         n_j = a_j(r_p) + alpha (j N + slot_eval(r_p)) + beta and d_j = a_j(r_p) + alpha ssigma_j(r_p) + beta;
      5. v(1,..,1,0) == 1;
      6. the two batch instances' chains (and, given finals / v_finals = the tables at rho_mu / the tree at rho_mu1, their last values).
    With a lookup:
      7. the lookup chain: p_0(0) + p_0(1) == 0, then interpolation on the nodes 0 .. 3;
      8. its last value == lookup3_value on the ten values of "lookup.values" with E = lambda eq(tau_l, r_l);
      9. the third batch instance's chain (and, given l_finals = L_BATCH_TABLES at rho_l, its last value).
    A record of another gate kind than the key's, or a record / key pair that disagrees on having a lookup, is malformed.
    """
    try:
        gate = gate_of(vk)
        if gate_of(proof) is not gate:
            return [0]
        c = c or challenges(vk, public_inputs, proof)
        mu, N = int(vk["mu"]), 1 << int(vk["mu"])
        pi = _ints(_u64(public_inputs, -1, 4))
        gv = dict(zip(gate.g_values, _ints(_u64(proof["g_values"], len(gate.g_values), 4))))
        pv = _ints(_u64(proof["p_values"], len(P_VALUES), 4))
        v0r, v1r, vr0, vr1, prod = _ints(_u64(proof["v_values"], len(wr.V_POINTS), 4))
        p_rounds, g_rounds = _u64(proof["p_rounds"], mu, 6, 4), _u64(proof["g_rounds"], mu, gate.evals, 4)
        claims, v_claims = _claims(c, proof)
        lookup = has_lookup(vk)
        if lookup:
            l_rounds, lv = _u64(proof["lookup"]["rounds"], mu, 4, 4), _ints(_u64(proof["lookup"]["values"], len(L_VALUES), 4))
            l_claims = _lookup_claims(c, proof)
            if np.asarray(proof["lookup"]["batch"]["opening"], dtype=np.uint64).size != mu * 18:
                return [0]
    except (KeyError, ValueError, TypeError):
        return [0]
    al, bt, gm = (fr_from_mont(c[k]) for k in ("alpha", "beta", "gamma"))
    r_p, r_g = _ints(c["r_p"]), _ints(c["r_g"])
    p_target, g_target = round_chain(p_rounds, r_p), round_chain(g_rounds, r_g)
    bad = [k for k, target in ((1, p_target), (2, g_target)) if target is None]
    if 2 not in bad and g_target != gate.value(eq_eval(_ints(c["tau_g"]), r_g), gv, in_eval(pi, r_g)):
        bad.append(3)
    ids = slot_eval(r_p)
    n = [(pv[j] + al * (j * N + ids) + bt) % R_MOD for j in range(3)]
    d = [(pv[j] + al * pv[3 + j] + bt) % R_MOD for j in range(3)]
    if 1 not in bad and p_target != perm3_value(eq_eval(_ints(c["tau_p"]), r_p), v1r, vr0, vr1, v0r, n, d, gm):
        bad.append(4)
    if prod != 1:
        bad.append(5)
    if bo.failed_checks(len(gate.batch_tables), claims, proof["batch"], c["b_alpha"], c["rho_mu"], finals) or \
            bo.failed_checks(1, v_claims, proof["v_batch"], c["b_alpha"], c["rho_mu1"], v_finals):
        bad.append(6)
    if lookup:
        r_l = _ints(c["r_l"])
        target = round_chain(l_rounds, r_l)
        if target is None:
            bad.append(7)
        ze, bl, gl, lam = (fr_from_mont(c[k]) for k in ("zeta", "beta_l", "gamma_l", "lambda"))
        if 7 not in bad and target != lookup3_value(lam * eq_eval(_ints(c["tau_l"]), r_l) % R_MOD, *lv, ze, bl, gl):
            bad.append(8)
        if bo.failed_checks(len(L_BATCH_TABLES), l_claims, proof["lookup"]["batch"], c["b_alpha"], c["rho_l"], l_finals):
            bad.append(9)
    return sorted(bad)


def field_checks(vk: dict, public_inputs, proof: dict, finals=None, v_finals=None, l_finals=None) -> bool:
    """everything of `verify` but the pairings, without a GPU.  finals (tests that hold the tables): the gate kind's batch_tables at rho_mu;
    v_finals: [the tree at rho_mu1]; they stand in for the pairings' check of the values the batch chains end in"""
    return not failed_checks(vk, public_inputs, proof, finals, v_finals, l_finals=l_finals)


def verify(be, vk: dict, public_inputs, proof: dict) -> bool:
    """the replay, the checks of failed_checks, then one zk_pcs_verify_batch per batch instance: two, with a lookup three (vk["pcs"]:
    wiring.verifying_keys).  The record's G1 points are taken as given (on the curve is checked, the subgroup is not): a record from
    outside goes through proof_io.verify_bytes / check_points first."""
    if vk.get("pcs") is None:
        raise ValueError("the verifying key holds no pairing keys (preprocess without powers_of_g2)")
    try:
        c = challenges(vk, public_inputs, proof)
        if failed_checks(vk, public_inputs, proof, c=c):
            return False
        claims, v_claims = _claims(c, proof)
        ns = len(gate_of(vk).selectors)
        lookup = has_lookup(vk)
        vkc, pc = _u64(vk["commitments"], ns + 3 + (len(LOOKUP_VK_TABLES) if lookup else 0), 18), _u64(proof["commitments"], 3, 18)
        comms = np.concatenate([vkc[:ns], pc, vkc[ns:ns + 3]])  # batch_tables order
        vk_mu, vk_mu1 = vk["pcs"]
        if not bo.batch_open_verify(be, vk_mu, comms, claims, proof["batch"], c["b_alpha"], c["rho_mu"]):
            return False
        if not bo.batch_open_verify(be, vk_mu1, _u64(proof["v_commitment"], 1, 18), v_claims, proof["v_batch"], c["b_alpha"], c["rho_mu1"]):
            return False
        if not lookup:
            return True
        l_comms = np.concatenate([vkc[ns + 3:], _u64(proof["lookup"]["commitments"], len(LOOKUP_COMMITTED), 18)])  # L_BATCH_TABLES order
        return bo.batch_open_verify(be, vk_mu, l_comms, _lookup_claims(c, proof), proof["lookup"]["batch"], c["b_alpha"], c["rho_l"])
    except (KeyError, ValueError, TypeError):
        return False


def _agg_openings(vk: dict, c: dict, proof: dict) -> list | None:
    """the batch instances of one proof -- two, with a lookup three -- as openings of dist_primitive.verify_agg over the full key
    vk["pcs"][1]: skip = 1 for the mu-variate instances, 0 for the tree's.  None when a chain breaks"""
    claims, v_claims = _claims(c, proof)
    ns = len(gate_of(vk).selectors)
    lookup = has_lookup(vk)
    vkc, pc = _u64(vk["commitments"], ns + 3 + (len(LOOKUP_VK_TABLES) if lookup else 0), 18), _u64(proof["commitments"], 3, 18)
    comms = np.concatenate([vkc[:ns], pc, vkc[ns:ns + 3]])  # batch_tables order
    parts = [(bo.opening_claim(comms, claims, proof["batch"], c["b_alpha"], c["rho_mu"]), 1),
             (bo.opening_claim(_u64(proof["v_commitment"], 1, 18), v_claims, proof["v_batch"], c["b_alpha"], c["rho_mu1"]), 0)]
    if lookup:
        l_comms = np.concatenate([vkc[ns + 3:], _u64(proof["lookup"]["commitments"], len(LOOKUP_COMMITTED), 18)])  # L_BATCH_TABLES order
        parts.append((bo.opening_claim(l_comms, _lookup_claims(c, proof), proof["lookup"]["batch"], c["b_alpha"], c["rho_l"]), 1))
    if any(p is None for p, _ in parts):
        return None
    return [p + (skip,) for p, skip in parts]


def agg_openings(vk: dict, items) -> tuple:
    """the host half of verify_many, without a GPU: every (public_inputs, proof) gets the replay and the checks of failed_checks; the
    batch instances of the survivors become openings of dist_primitive.verify_agg -> (alive: the survivors' indices, openings)"""
    alive, openings = [], []
    for n, (public_inputs, proof) in enumerate(items):
        try:
            c = challenges(vk, public_inputs, proof)
            if failed_checks(vk, public_inputs, proof, c=c):
                continue
            ops = _agg_openings(vk, c, proof)
        except (KeyError, ValueError, TypeError):
            continue
        if ops is not None:
            alive.append(n)
            openings += ops
    return alive, openings


def verify_many(be, vk: dict, items) -> list:
    """`verify` for a list of (public_inputs, proof): every proof gets the replay and the checks of failed_checks (agg_openings), then
    the batch instances of all surviving proofs go into ONE zk_pcs_verify_agg call over the full key vk["pcs"][1].  When the aggregate
    accepts every survivor is True; when it rejects -- or refuses a point that is not on the curve -- the survivors go one by one
    through `verify`, so the bad one is named.  The verdicts are those of [verify(be, vk, pi, proof) for pi, proof in items] up to the
    aggregate's soundness error (openings / 2^128)."""
    from . import dist_primitive as dp

    if vk.get("pcs") is None:
        raise ValueError("the verifying key holds no pairing keys (preprocess without powers_of_g2)")
    from .api import ZK_ERR_INVALID, ZkError

    def refused_is_false(call):  # a point that is not on the curve is a refusal of the library (ZK_ERR_INVALID): a record to reject
        try:
            return bool(call())
        except ZkError as e:
            if e.code != ZK_ERR_INVALID:
                raise
            return False

    items = list(items)
    alive, openings = agg_openings(vk, items)
    ok = refused_is_false(lambda: dp.verify_agg(be, vk["pcs"][1], openings)) if alive else True
    out = [False] * len(items)
    for n in alive:
        out[n] = True if ok else refused_is_false(lambda: verify(be, vk, *items[n]))
    return out


def verify_agg(be, vk: dict, public_inputs, proof: dict) -> bool:
    """`verify` with ONE pairing call instead of two or three: verify_many of one proof"""
    return verify_many(be, vk, [(public_inputs, proof)])[0]


def proof_digest(proof: dict) -> str:
    """SHA-256 over the record's little-endian words in the order of the schedule"""
    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(proof["mu"]).to_bytes(8, "little") + int(proof["l"]).to_bytes(8, "little"))
    for k in ("commitments", "v_commitment", "p_rounds", "g_rounds", "g_values", "p_values", "v_values"):
        put(proof[k])
    for b in ("batch", "v_batch"):
        put(proof[b]["rounds"]), put(proof[b]["opening"])
    if has_lookup(proof):
        lp = proof["lookup"]
        put(lp["commitments"]), put(lp["rounds"]), put(lp["values"]), put(lp["batch"]["rounds"]), put(lp["batch"]["opening"])
    return h.hexdigest()


def circuit_digest(circuit: dict) -> str:
    """SHA-256 of a sampled circuit's tables: the selectors, a, b, c, the public inputs, the trapdoor, sigma (u64) and, with a lookup, qk, t0, t1,
    t2 and idx (u32), little-endian in that order -- what host/bin/plonk_check --sample-only prints"""
    h = hashlib.sha256()
    for k in gate_of(circuit).selectors + ("a", "b", "c", "public_inputs", "s", "sigma"):
        h.update(np.ascontiguousarray(circuit[k], dtype="<u8").tobytes())
    if has_lookup(circuit):
        for k in LOOKUP_VK_TABLES:
            h.update(np.ascontiguousarray(circuit["lookup"][k], dtype="<u8").tobytes())
        h.update(np.ascontiguousarray(circuit["idx"], dtype="<u4").tobytes())
    return h.hexdigest()


# ---- the test circuit ----
CIRCUIT_SEED = 0x91A70000  # stream k of seed S is SplitMix64(CIRCUIT_SEED + 1000 S + k)


def _mont_ints(a) -> list:
    """[n, 4] limbs -> the n integers AS THEY STAND (Montgomery forms are field elements too: the gate arithmetic below stays in that form)"""
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def sample_circuit(mu: int, seed: int, break_gate: int | None = None, break_wire: int | None = None, _lookup: dict | None = None) -> dict:
    """
    A satisfied circuit (numpy and python ints only; the same in host/zkhost/plonk.hpp): N = 2^mu rows, mu >= 2, l = min(4, N / 2).
    Streams of field.splitmix_fr: 1 = the l public inputs, 2 = q1, 3 = q2, 4 = the picks, 5 = the SRS trapdoor (mu + 1 elements).
      rows 0 .. l - 1   input rows: q1 = q2 = 0, a = b = 0, c = the public input;
      row x >= l        a = c[i], b = c[k] with i = limb 0 of pick x mod x, k = limb 1 of pick x mod x; q1, q2 from their streams;
                        c = q1 (a + b) + q2 a b, so in = 0 there.
    sigma: one cycle per value -- the c slot of row y, then the a / b slots that copy it in ascending slot order, back to the c slot;
    every other slot is a fixed point.  break_gate K adds 1 to c[K] after the fact; break_wire K (K >= l) adds 1 to a[K] and recomputes
    c[K]: every gate still holds and only the copy constraint fails.  (_lookup: the lookup rows of sample_circuit_lookup -- see _lookup_rows.)
    -> {"mu", "l", "q1", "q2", "a", "b", "c": [N, 4] Montgomery Fr, "sigma": [3N] u64, "public_inputs": [l, 4], "s": [mu + 1, 4]}
    """
    from .field import splitmix_fr

    if mu < 2:
        raise ValueError("mu >= 2 is needed")
    N, base = 1 << mu, CIRCUIT_SEED + 1000 * seed
    l = min(4, N // 2)
    pi = splitmix_fr(l, base + 1)
    q1, q2, pick = splitmix_fr(N, base + 2), splitmix_fr(N, base + 3), splitmix_fr(N, base + 4)
    q1[:l], q2[:l] = 0, 0
    lk = _lookup
    if lk:  # a lookup row is a product row: q1 = 0, q2 = 1
        q1[lk["mask"]], q2[lk["mask"]] = 0, fr_mont(1)
    rows = np.arange(N, dtype=np.uint64)
    rows[0] = 1  # (row 0 is an input row: its picks are not used)
    ia, ib = pick[:, 0] % rows, pick[:, 1] % rows
    rinv = pow(1 << 256, -1, R_MOD)  # on Montgomery forms x' = x R: (x y)' = x' y' / R
    q1i, q2i = _mont_ints(q1), _mont_ints(q2)
    a, b, c = [0] * N, [0] * N, _mont_ints(pi) + [0] * (N - l)
    gate = lambda x: (q1i[x] * (a[x] + b[x]) + q2i[x] * a[x] % R_MOD * b[x] % R_MOD * rinv) % R_MOD * rinv % R_MOD
    ial, ibl = ia.tolist(), ib.tolist()
    one = (1 << 256) % R_MOD
    for x in range(l, N):
        if lk and lk["mask"][x]:
            a[x], b[x] = lk["u"][lk["y"][x]], lk["v"][lk["y"][x]]
            if x == lk["break"]:
                a[x] = (a[x] + one) % R_MOD
        else:
            a[x], b[x] = c[ial[x]], c[ibl[x]]
        c[x] = gate(x)
    if break_wire is not None:
        if not l <= break_wire < N:
            raise ValueError("break_wire must name a row past the input rows: the a slot of an input row is a fixed point")
        a[break_wire] = (a[break_wire] + one) % R_MOD
        c[break_wire] = gate(break_wire)
    if break_gate is not None:
        c[break_gate] = (c[break_gate] + one) % R_MOD
    return {"mu": mu, "l": l, "q1": q1, "q2": q2, "a": _limbs(a), "b": _limbs(b), "c": _limbs(c), "sigma": _copy_sigma(ia, ib, l, N, lk["mask"] if lk else None),
            "public_inputs": pi, "s": splitmix_fr(mu + 1, base + 5)}


def _limbs(xs) -> np.ndarray:
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def _copy_sigma(ia: np.ndarray, ib: np.ndarray, l: int, N: int, fixed: np.ndarray | None = None) -> np.ndarray:
    """one cycle per value: the users of c[y] are the a slots x with ia[x] = y and the b slots N + x with ib[x] = y, x >= l.  fixed (bool[N]):
    rows whose a and b slots copy nothing and stay fixed points (the lookup rows)"""
    src = np.concatenate([ia[l:], ib[l:]])
    slot = np.concatenate([np.arange(l, N, dtype=np.uint64), np.arange(N + l, 2 * N, dtype=np.uint64)])
    if fixed is not None:
        keep = ~np.concatenate([fixed[l:], fixed[l:]])
        src, slot = src[keep], slot[keep]
    order = np.lexsort((slot, src))
    src, slot = src[order], slot[order]
    sigma = np.arange(3 * N, dtype=np.uint64)
    same = src[1:] == src[:-1]
    first, last = np.concatenate([[True], ~same]), np.concatenate([~same, [True]])
    sigma[slot[:-1][same]] = slot[1:][same]
    sigma[slot[last]] = np.uint64(2 * N) + src[last]
    sigma[np.uint64(2 * N) + src[first]] = slot[first]
    return sigma


WIDE_SELECTORS = GATES["wide"].selectors


def sample_circuit_wide(mu: int, seed: int, break_gate: int | None = None, break_wire: int | None = None, _lookup: dict | None = None) -> dict:
    """
    A satisfied circuit of the WIDE gate qL a + qR b + qM a b + qH a^5 - qO c + qC + in = 0 (numpy and python ints only; the same in
    host/zkhost/plonk.hpp): N = 2^mu rows, mu >= 2, l = min(4, N / 2).  Streams of field.splitmix_fr as in sample_circuit -- 1 = the l public
    inputs, 4 = the picks, 5 = the SRS trapdoor -- and for the selectors 6 = qL, 7 = qR, 8 = qM, 9 = qO, 10 = qC, 11 = qH (2 and 3 stay q1, q2's).
      rows 0 .. l - 1   input rows: qO = 1, every other selector 0, a = b = 0, c = the public input;
      row x >= l        a = c[i], b = c[k] with i = limb 0 of pick x mod x, k = limb 1 of pick x mod x; the row kind is limb 2 of pick x mod 4:
                          0 linear   qL, qR, qC from their streams, qO = 1         c = qL a + qR b + qC
                          1 product  qM, qC from their streams, qO = 1             c = qM a b + qC
                          2 S-box    qH = 1, qC from its stream, qO = 1            c = a^5 + qC
                          3 full     all six from their streams (a zero qO -- none occurs for the seeds in use -- is replaced by 1)
                                                                                   c = (qL a + qR b + qM a b + qH a^5 + qC) / qO
                        a selector the kind does not name is 0, and in = 0 there.
    sigma, break_gate K, break_wire K (K >= l: a[K] + 1, c[K] recomputed by the row's rule) and "s" as in sample_circuit.
    (_lookup: the lookup rows of sample_circuit_lookup -- see _lookup_rows.)
    -> {"gate": "wide", "mu", "l", "qL", "qR", "qM", "qO", "qC", "qH", "a", "b", "c": [N, 4] Montgomery Fr, "sigma": [3N] u64,
        "public_inputs": [l, 4], "s": [mu + 1, 4]}
    """
    from .field import splitmix_fr

    if mu < 2:
        raise ValueError("mu >= 2 is needed")
    N, base = 1 << mu, CIRCUIT_SEED + 1000 * seed
    l = min(4, N // 2)
    pi, pick = splitmix_fr(l, base + 1), splitmix_fr(N, base + 4)
    drawn = {k: _ints(splitmix_fr(N, base + 6 + i)) for i, k in enumerate(WIDE_SELECTORS)}  # canonical integers: the rows are built on them
    named = (("qL", "qR", "qC"), ("qM", "qC"), ("qC",), WIDE_SELECTORS)
    sel = {k: [0] * N for k in WIDE_SELECTORS}
    sel["qO"] = [1] * N
    kinds = (pick[:, 2] % np.uint64(4)).tolist()
    for x in range(l, N):
        for k in named[kinds[x]]:
            sel[k][x] = drawn[k][x]
        if kinds[x] == 2:
            sel["qH"][x] = 1
        if kinds[x] == 3 and sel["qO"][x] == 0:
            sel["qO"][x] = 1
    lk = _lookup
    if lk:  # a lookup row is a pure product row: qM = qO = 1, every other selector 0
        for x in np.flatnonzero(lk["mask"]).tolist():
            for k in WIDE_SELECTORS:
                sel[k][x] = 1 if k in ("qM", "qO") else 0
    rows = np.arange(N, dtype=np.uint64)
    rows[0] = 1  # (row 0 is an input row: its picks are not used)
    ia, ib = pick[:, 0] % rows, pick[:, 1] % rows
    a, b, c = [0] * N, [0] * N, _ints(pi) + [0] * (N - l)

    def out(x):  # the c that satisfies row x
        s = sel["qL"][x] * a[x] + sel["qR"][x] * b[x] + sel["qM"][x] * a[x] * b[x] + sel["qH"][x] * pow(a[x], 5, R_MOD) + sel["qC"][x]
        return s % R_MOD if sel["qO"][x] == 1 else s * pow(sel["qO"][x], -1, R_MOD) % R_MOD

    ial, ibl = ia.tolist(), ib.tolist()
    for x in range(l, N):
        if lk and lk["mask"][x]:
            a[x], b[x] = lk["u"][lk["y"][x]], lk["v"][lk["y"][x]]
            if x == lk["break"]:
                a[x] = (a[x] + 1) % R_MOD
        else:
            a[x], b[x] = c[ial[x]], c[ibl[x]]
        c[x] = out(x)
    if break_wire is not None:
        if not l <= break_wire < N:
            raise ValueError("break_wire must name a row past the input rows: the a slot of an input row is a fixed point")
        a[break_wire] = (a[break_wire] + 1) % R_MOD
        c[break_wire] = out(break_wire)
    if break_gate is not None:
        c[break_gate] = (c[break_gate] + 1) % R_MOD
    mont = lambda xs: _limbs([(x << 256) % R_MOD for x in xs])
    circuit = {"gate": "wide", "mu": mu, "l": l, "a": mont(a), "b": mont(b), "c": mont(c), "sigma": _copy_sigma(ia, ib, l, N, lk["mask"] if lk else None), "public_inputs": pi,
               "s": splitmix_fr(mu + 1, base + 5)}
    circuit.update({k: mont(v) for k, v in sel.items()})
    return circuit


def _lookup_rows(mask, y, u, v, break_row) -> dict:
    """What sample_circuit_lookup hands to the two generators (struct LookupRows in host/zkhost/plonk.hpp): row x with mask[x] takes
    a = u[y[x]], b = v[y[x]] in the place of copies and a product gate (c = a b); its a and b slots stay fixed points of sigma; row
    break_row (None: none) gets a + 1 before its c is computed.  u, v: python ints in the domain the generator builds its rows in
    (sample_circuit: Montgomery forms as they stand; sample_circuit_wide: canonical)"""
    return {"mask": mask, "y": y, "u": u, "v": v, "break": break_row}


def sample_circuit_lookup(mu: int, seed: int, gate: str | None = None, break_lookup: int | None = None) -> dict:
    """
    sample_circuit(mu, seed) -- with gate="wide": sample_circuit_wide -- plus lookup rows against a fixed multiplication table (numpy and python
    ints only): N = 2^mu rows, mu >= 3.  Streams of field.splitmix_fr beside those of the two generators: 12 = u, 13 = v (D = N / 4 elements
    each).  The table does not depend on the witness: entry y < D is (u_y, v_y, u_y v_y), padded to N by repeating entry D - 1.
      row x >= l whose pick (stream 4) has an odd limb 3 is a lookup row: y = (limb 3 >> 1) mod D, a = u_y, b = v_y; its selectors make
      c = a b (basic: q1 = 0, q2 = 1; wide: qM = qO = 1, the rest 0); qk = 1 and idx = y.  Its a and b slots are fixed points of sigma; its c
      may be copied by later rows as usual.  Every other row is the generator's, with qk = 0 and idx = 0.
    break_lookup K (a lookup row): a[K] + 1 and c[K] recomputed before any later row copies it -- every gate and the wiring still hold, and
    the triple of row K is outside the table.
    -> the generator's dict plus "lookup": {"qk", "t0", "t1", "t2": [N, 4] Montgomery Fr} and "idx": u32[N]
    """
    from .field import splitmix_fr

    if mu < 3:
        raise ValueError("mu >= 3 is needed")
    if gate not in GATES:
        raise ValueError(f"unknown gate kind {gate!r}")
    N, base = 1 << mu, CIRCUIT_SEED + 1000 * seed
    l, D = min(4, N // 2), N // 4
    pick = splitmix_fr(N, base + 4)
    mask = ((pick[:, 3] & np.uint64(1)) == 1) & (np.arange(N) >= l)
    y = ((pick[:, 3] >> np.uint64(1)) % np.uint64(D)).astype(np.int64)
    if break_lookup is not None and not (0 <= break_lookup < N and mask[break_lookup]):
        raise ValueError("break_lookup must name a lookup row")
    u, v = splitmix_fr(D, base + 12), splitmix_fr(D, base + 13)
    as_ints = _ints if gate == "wide" else _mont_ints  # the domain the generator builds its rows in
    plan = _lookup_rows(mask, y.tolist(), as_ints(u), as_ints(v), break_lookup)
    circuit = (sample_circuit_wide if gate == "wide" else sample_circuit)(mu, seed, _lookup=plan)
    rinv = pow(1 << 256, -1, R_MOD)
    uv = _limbs([p * q % R_MOD * rinv % R_MOD for p, q in zip(_mont_ints(u), _mont_ints(v))])  # the Montgomery form of u_y v_y
    pad = lambda t: np.concatenate([t, np.repeat(t[-1:], N - D, axis=0)])
    qk = np.zeros((N, 4), dtype=np.uint64)
    qk[mask] = fr_mont(1)
    circuit["lookup"] = {"qk": qk, "t0": pad(u), "t1": pad(v), "t2": pad(uv)}
    circuit["idx"] = np.where(mask, y, 0).astype(np.uint32)
    return circuit


def sample_circuit_lookup_fn(mu: int, seed: int, break_row: int | None = None) -> dict:
    """
    A satisfied WIDE-gate circuit whose lookup rows have the gate switched off: the table, not the gate, gives their c (numpy and python
    ints only): N = 2^mu rows, mu >= 3, l = min(4, N / 2).
    Table: XOR on k = min(4, mu // 2) bits -- entry y < 4^k is (y >> k, y & (2^k - 1), their XOR), padded to N by repeating the last entry.
    Streams of field.splitmix_fr: 1 = the l public inputs and 5 = the SRS trapdoor as in sample_circuit, 14 = the picks of this sampler.
      rows 0 .. l - 1   input rows: qO = 1, every other selector 0, a = b = 0, c = the public input;
      row x >= l        its kind is limb 2 of pick x mod 8:
                          0 .. 5  LOOKUP  every gate selector 0, qk = 1, c = a XOR b.  a is a copy of the c of an earlier lookup row when
                                  bits 3 .. 5 of limb 2 are all 0 and there is one -- the (limb 0 mod E)-th of the E earlier lookup rows --
                                  and otherwise FREE: the slot is a fixed point of sigma and holds limb 3 & (2^k - 1).  b likewise with
                                  bits 6 .. 8, limb 1 and (limb 3 >> 8) & (2^k - 1).  XOR outputs stay below 2^k, so chains arise;
                          6       linear   qL = qR = qO = 1: c = a + b      with a = c[limb 0 mod x], b = c[limb 1 mod x] (any earlier row);
                          7       product  qM = qO = 1:      c = a b        likewise.
    sigma: one cycle per copied c -- its c slot, then the slots that copy it in ascending order; every other slot is a fixed point.
    break_row K (a lookup row with a free a) adds 2^k to that free value: the pair is in no entry, the row's c is 0 as the witness
    generator leaves it, and idx[K] = 0.
    -> the dict of sample_circuit_wide plus "lookup": {"qk", "t0", "t1", "t2": [N, 4] Montgomery Fr}, "free": [3N, 4] (the free values at
       their slots, 0 elsewhere) and "idx": u32[N], the first-occurrence indices as lookup.find_indices_host gives them
    """
    from .field import splitmix_fr

    if mu < 3:
        raise ValueError("mu >= 3 is needed")
    N, base = 1 << mu, CIRCUIT_SEED + 1000 * seed
    l, k = min(4, N // 2), min(4, mu // 2)
    D, low = 1 << (2 * k), (1 << k) - 1
    pi, pick = splitmix_fr(l, base + 1), splitmix_fr(N, base + 14).tolist()
    sel = {q: [0] * N for q in WIDE_SELECTORS}
    qk, idx, free = [0] * N, [0] * N, [0] * (3 * N)
    a, b, c = [0] * N, [0] * N, _ints(pi) + [0] * (N - l)
    users = {}       # row y -> the slots that copy c[y], in ascending order per column
    lookups = []     # the lookup rows so far
    for x in range(l):
        sel["qO"][x] = 1
    for x in range(l, N):
        p0, p1, p2, p3 = pick[x]
        kind = p2 % 8
        if kind < 6:
            qk[x] = 1
            for j, (w, bits, p, small) in enumerate(((a, (p2 >> 3) & 7, p0, p3 & low), (b, (p2 >> 6) & 7, p1, (p3 >> 8) & low))):
                if bits == 0 and lookups:
                    y = lookups[p % len(lookups)]
                    w[x] = c[y]
                    users.setdefault(y, []).append(j * N + x)
                else:
                    if j == 0 and x == break_row:
                        small += 1 << k
                    w[x] = free[j * N + x] = small
            if x == break_row and free[x] < (1 << k):
                raise ValueError("break_row must name a lookup row with a free a")
            hit = a[x] <= low and b[x] <= low
            c[x] = a[x] ^ b[x] if hit else 0
            idx[x] = (a[x] << k) | b[x] if hit else 0
            lookups.append(x)
        else:
            ya, yb = p0 % x, p1 % x
            a[x], b[x] = c[ya], c[yb]
            users.setdefault(ya, []).append(x)
            users.setdefault(yb, []).append(N + x)
            sel["qO"][x] = 1
            if kind == 6:
                sel["qL"][x] = sel["qR"][x] = 1
                c[x] = (a[x] + b[x]) % R_MOD
            else:
                sel["qM"][x] = 1
                c[x] = a[x] * b[x] % R_MOD
    if break_row is not None and not (l <= break_row < N and qk[break_row]):
        raise ValueError("break_row must name a lookup row with a free a")
    sigma = np.arange(3 * N, dtype=np.uint64)
    for y, slots in users.items():
        cyc = [2 * N + y] + sorted(slots)
        for s, t in zip(cyc, cyc[1:] + cyc[:1]):
            sigma[s] = t
    mont = lambda xs: _limbs([(x << 256) % R_MOD for x in xs])
    ys = [min(y, D - 1) for y in range(N)]
    circuit = {"gate": "wide", "mu": mu, "l": l, "a": mont(a), "b": mont(b), "c": mont(c), "sigma": sigma, "public_inputs": pi, "s": splitmix_fr(mu + 1, base + 5)}
    circuit.update({q: mont(v) for q, v in sel.items()})
    circuit["lookup"] = {"qk": mont(qk), "t0": mont([y >> k for y in ys]), "t1": mont([y & low for y in ys]), "t2": mont([(y >> k) ^ (y & low) for y in ys])}
    circuit["free"] = mont(free)
    circuit["idx"] = np.array(idx, dtype=np.uint32)
    return circuit
