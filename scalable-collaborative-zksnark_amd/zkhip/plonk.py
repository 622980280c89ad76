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
from .transcript import HostTranscript, Transcript
from .zerocheck import _ints, eq_eval, gate_value, wide_gate_value

LABEL = b"plonk"
VK_TABLES = ("q1", "q2", "ssigma0", "ssigma1", "ssigma2")
G_VALUES = ("q1", "q2", "a", "b", "c")                              # at r_g
P_VALUES = ("a", "b", "c", "ssigma0", "ssigma1", "ssigma2")          # at r_p
BATCH_TABLES = ("q1", "q2", "a", "b", "c", "ssigma0", "ssigma1", "ssigma2")  # the tables of the mu-variate batch instance
_SSIGMA = ("ssigma0", "ssigma1", "ssigma2")


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


def _u64(a, *shape) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(*shape)


# ---- the verifier's closed forms ----
def round_poly_at(evals, x: int) -> int:
    """the polynomial of degree len(evals) - 1 through (k, evals[k]) at x"""
    n, acc = len(evals), 0
    for k in range(n):
        num, den = 1, 1
        for m in range(n):
            if m != k:
                num, den = num * (x - m) % R_MOD, den * (k - m) % R_MOD
        acc = (acc + evals[k] * num % R_MOD * pow(den, -1, R_MOD)) % R_MOD
    return acc


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
    -> (pk, vk): vk = {"mu", "l", "commitments": [5, 18] in VK_TABLES order, "pcs": (vk_mu, vk_mu1) or None}; pk keeps the device tables.
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
    comms = np.stack([_u64(dp.commit(be, pcs, tabs[k], N), 18) for k in gate.vk_tables])
    vk = {"mu": mu, "l": l, "commitments": comms, "pcs": wr.verifying_keys(be, powers_of_g2) if powers_of_g2 is not None else None, **gate.tag()}
    return {"mu": mu, "l": l, "tables": tabs, "commitments": comms, "pcs": pcs, **gate.tag()}, vk


# ---- prover ----
def prove(be, pk: dict, a, b, c, public_inputs, timing: dict | None = None) -> dict:
    """a, b, c: device buffers of N Fr (or [N, 4] arrays); public_inputs: [l, 4] Montgomery Fr -> the record of the module text.
    A zero denominator raises ZeroDivisionError (ZK_ERR_DIV_ZERO); a zero challenge alpha (probability 2^-254), from which ssigma_j(r_p)
    cannot be recovered, ValueError.  timing (optional dict) receives the wall seconds of the phases."""
    import time

    from . import dist_primitive as dp
    from .nizk import _batch_prove

    gate = gate_of(pk)
    mu, l, pcs = pk["mu"], pk["l"], pk["pcs"]
    N = 1 << mu
    pi = _u64(public_inputs, -1, 4)
    if len(pi) != l:
        raise ValueError(f"{l} public inputs needed, {len(pi)} given")
    wires = {k: (be.to_device(_u64(v, N, 4)) if isinstance(v, np.ndarray) else v) for k, v in (("a", a), ("b", b), ("c", c))}
    tabs = dict(pk["tables"], **wires)
    t0 = time.perf_counter()
    comms = np.stack([_u64(dp.commit(be, pcs, wires[k], N), 18) for k in ("a", "b", "c")])
    tr = Transcript(be, gate.label)
    try:
        tr.absorb_u64(mu).absorb_u64(l).absorb(pk["commitments"]).absorb(pi)
        alpha, beta = tr.absorb(comms).challenges(2)
        if not fr_from_mont(alpha):
            raise ValueError("the challenge alpha is zero")
        nums, dens, P, Q = be.perm3_terms([wires[k] for k in ("a", "b", "c")], [tabs[f"ssigma{j}"] for j in range(3)], N, alpha, beta)
        tree = be.product_tree(be.fr_batch_div(P, Q, N), N)
        v_comm = _u64(dp.commit(be, pcs, tree, 2 * N), 18)
        t1 = time.perf_counter()
        gamma = tr.absorb(v_comm).challenge()
        p_rounds, p_last, r_p = be.sumcheck_perm3_fs(be.eq_table(tr.challenges(mu)), tree, nums, dens, N, gamma, tr)
        t2 = time.perf_counter()
        inp = np.zeros((N, 4), dtype=np.uint64)
        inp[:l] = pi
        g_rounds, g_last, r_g = gate.sumcheck(be, be.eq_table(tr.challenges(mu)), tabs, be.to_device(inp), N, tr)
        t3 = time.perf_counter()
        g_values = g_last[1:1 + len(gate.g_values)]  # the folded-out values ARE the selectors and a, b, c at r_g
        # the folded-out n_j, d_j at r_p give the wires and the permutation columns there: both are linear in them
        al, bt, ids = fr_from_mont(alpha), fr_from_mont(beta), slot_eval(_ints(r_p))
        n_r, d_r = _ints(p_last[5:8]), _ints(p_last[8:11])
        w_r = [(n_r[j] - al * (j * N + ids) - bt) % R_MOD for j in range(3)]
        s_r = [(d_r[j] - w_r[j] - bt) * pow(al, -1, R_MOD) % R_MOD for j in range(3)]
        p_values = np.stack([fr_mont(x) for x in w_r + s_r])
        # the tree at (0,r) = h, (1,r) = v1x, (r,0) = vx0, (r,1) = vx1 are folded-out values too; (1,..,1,0) is tree[2N - 2]
        v_values = np.stack([p_last[4], p_last[1], p_last[2], p_last[3], tree.download((1, 4), offset=32 * (2 * N - 2))[0]])
        b_alpha = tr.absorb(g_values).absorb(p_values).absorb(v_values).challenge()
        bt_names = gate.batch_tables
        claims = [(bt_names.index(k), r_g, v) for k, v in zip(gate.g_values, g_values)] + [(bt_names.index(k), r_p, v) for k, v in zip(P_VALUES, p_values)]
        batch, _ = _batch_prove(be, pcs, [tabs[k] for k in bt_names], N, claims, b_alpha, tr)
        v_batch, _ = _batch_prove(be, pcs, [tree], 2 * N, [(0, z, v) for z, v in zip(wr.v_points(r_p), v_values)], b_alpha, tr)
    finally:
        tr.free()
    t4 = time.perf_counter()
    if timing is not None:
        timing["commit_s"], timing["perm3_s"], timing["gate_s"], timing["opening_s"] = t1 - t0, t2 - t1, t3 - t2, t4 - t3
    return {"mu": mu, "l": l, "commitments": comms, "v_commitment": v_comm, "p_rounds": p_rounds, "g_rounds": g_rounds, "g_values": np.array(g_values),
            "p_values": p_values, "v_values": v_values, "batch": batch, "v_batch": v_batch, **gate.tag()}


# ---- verifier ----
def challenges(vk: dict, public_inputs, proof: dict, label: bytes | None = None) -> dict:
    """the verifier's replay of the schedule on hashlib (label: the gate kind's, unless given) -> {"alpha", "beta", "gamma", "tau_p", "r_p",
    "tau_g", "r_g", "b_alpha", "rho_mu", "rho_mu1"}; ValueError / KeyError on a malformed record or statement, a record of another gate
    kind than the key's among them"""
    gate = gate_of(vk)
    if gate_of(proof) is not gate:
        raise ValueError("the record and the key are of different gate kinds")
    label = gate.label if label is None else label
    mu, l = int(vk["mu"]), int(vk["l"])
    pi = _u64(public_inputs, -1, 4)
    p_rounds, g_rounds = _u64(proof["p_rounds"], -1, 6, 4), _u64(proof["g_rounds"], -1, gate.evals, 4)
    b_rounds, v_rounds = _u64(proof["batch"]["rounds"], -1, 3, 4), _u64(proof["v_batch"]["rounds"], -1, 3, 4)
    if int(proof["mu"]) != mu or int(proof["l"]) != l or len(pi) != l:
        raise ValueError("the record, the key and the public inputs disagree on mu / l")
    if mu < 1 or len(p_rounds) != mu or len(g_rounds) != mu or len(b_rounds) != mu or len(v_rounds) != mu + 1:
        raise ValueError("the record does not hold mu / mu + 1 rounds")
    rr = lambda tr, rounds: np.stack([tr.absorb(r).challenge() for r in rounds])
    tr = HostTranscript(label)
    tr.absorb_u64(mu).absorb_u64(l).absorb(_u64(vk["commitments"], len(gate.vk_tables), 18)).absorb(pi)
    alpha, beta = tr.absorb(_u64(proof["commitments"], 3, 18)).challenges(2)
    gamma = tr.absorb(_u64(proof["v_commitment"], 18)).challenge()
    tau_p = tr.challenges(mu)
    r_p = rr(tr, p_rounds)
    tau_g = tr.challenges(mu)
    r_g = rr(tr, g_rounds)
    tr.absorb(_u64(proof["g_values"], len(gate.g_values), 4)).absorb(_u64(proof["p_values"], len(P_VALUES), 4)).absorb(_u64(proof["v_values"], len(wr.V_POINTS), 4))
    b_alpha = tr.challenge()
    rho_mu = rr(tr, b_rounds)
    return {"alpha": alpha, "beta": beta, "gamma": gamma, "tau_p": tau_p, "r_p": r_p, "tau_g": tau_g, "r_g": r_g, "b_alpha": b_alpha, "rho_mu": rho_mu,
            "rho_mu1": rr(tr, v_rounds)}


def _claims(c: dict, proof: dict):
    gate = gate_of(proof)
    g_values, p_values = _u64(proof["g_values"], len(gate.g_values), 4), _u64(proof["p_values"], len(P_VALUES), 4)
    v_values = _u64(proof["v_values"], len(wr.V_POINTS), 4)
    bt_names = gate.batch_tables
    claims = [(bt_names.index(k), c["r_g"], v) for k, v in zip(gate.g_values, g_values)] + [(bt_names.index(k), c["r_p"], v) for k, v in zip(P_VALUES, p_values)]
    return claims, [(0, z, v) for z, v in zip(wr.v_points(c["r_p"]), v_values)]


def failed_checks(vk: dict, public_inputs, proof: dict, finals=None, v_finals=None, c: dict | None = None) -> list:
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
    A record of another gate kind than the key's is malformed.
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
    except (KeyError, ValueError, TypeError):
        return [0]
    al, bt, gm = (fr_from_mont(c[k]) for k in ("alpha", "beta", "gamma"))
    r_p, r_g = _ints(c["r_p"]), _ints(c["r_g"])
    bad = []
    for number, rounds, r in ((1, p_rounds, r_p), (2, g_rounds, r_g)):
        target = 0
        for i in range(mu):
            p = _ints(rounds[i])
            if (p[0] + p[1]) % R_MOD != target:
                bad.append(number)
                break
            target = round_poly_at(p, r[i])
        if number == 1:
            p_target = target
        else:
            g_target = target
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
    return sorted(bad)


def field_checks(vk: dict, public_inputs, proof: dict, finals=None, v_finals=None) -> bool:
    """everything of `verify` but the pairings, without a GPU.  finals (tests that hold the tables): the gate kind's batch_tables at rho_mu;
    v_finals: [the tree at rho_mu1]; they stand in for the pairings' check of the values the batch chains end in"""
    return not failed_checks(vk, public_inputs, proof, finals, v_finals)


def verify(be, vk: dict, public_inputs, proof: dict) -> bool:
    """the replay, checks 1-6 of failed_checks, then one zk_pcs_verify_batch per batch instance (vk["pcs"]: wiring.verifying_keys)"""
    if vk.get("pcs") is None:
        raise ValueError("the verifying key holds no pairing keys (preprocess without powers_of_g2)")
    try:
        c = challenges(vk, public_inputs, proof)
        if failed_checks(vk, public_inputs, proof, c=c):
            return False
        claims, v_claims = _claims(c, proof)
        ns = len(gate_of(vk).selectors)
        vkc, pc = _u64(vk["commitments"], ns + 3, 18), _u64(proof["commitments"], 3, 18)
        comms = np.concatenate([vkc[:ns], pc, vkc[ns:]])  # batch_tables order
        vk_mu, vk_mu1 = vk["pcs"]
        if not bo.batch_open_verify(be, vk_mu, comms, claims, proof["batch"], c["b_alpha"], c["rho_mu"]):
            return False
        return bo.batch_open_verify(be, vk_mu1, _u64(proof["v_commitment"], 1, 18), v_claims, proof["v_batch"], c["b_alpha"], c["rho_mu1"])
    except (KeyError, ValueError, TypeError):
        return False


def proof_digest(proof: dict) -> str:
    """SHA-256 over the record's little-endian words in the order of the schedule"""
    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(proof["mu"]).to_bytes(8, "little") + int(proof["l"]).to_bytes(8, "little"))
    for k in ("commitments", "v_commitment", "p_rounds", "g_rounds", "g_values", "p_values", "v_values"):
        put(proof[k])
    for b in ("batch", "v_batch"):
        put(proof[b]["rounds"]), put(proof[b]["opening"])
    return h.hexdigest()


# ---- the test circuit ----
CIRCUIT_SEED = 0x91A70000  # stream k of seed S is SplitMix64(CIRCUIT_SEED + 1000 S + k)


def _mont_ints(a) -> list:
    """[n, 4] limbs -> the n integers AS THEY STAND (Montgomery forms are field elements too: the gate arithmetic below stays in that form)"""
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def sample_circuit(mu: int, seed: int, break_gate: int | None = None, break_wire: int | None = None) -> dict:
    """
    A satisfied circuit (numpy and python ints only; the same in host/zkhost/plonk.hpp): N = 2^mu rows, mu >= 2, l = min(4, N / 2).
    Streams of field.splitmix_fr: 1 = the l public inputs, 2 = q1, 3 = q2, 4 = the picks, 5 = the SRS trapdoor (mu + 1 elements).
      rows 0 .. l - 1   input rows: q1 = q2 = 0, a = b = 0, c = the public input;
      row x >= l        a = c[i], b = c[k] with i = limb 0 of pick x mod x, k = limb 1 of pick x mod x; q1, q2 from their streams;
                        c = q1 (a + b) + q2 a b, so in = 0 there.
    sigma: one cycle per value -- the c slot of row y, then the a / b slots that copy it in ascending slot order, back to the c slot;
    every other slot is a fixed point.  break_gate K adds 1 to c[K] after the fact; break_wire K (K >= l) adds 1 to a[K] and recomputes
    c[K]: every gate still holds and only the copy constraint fails.
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
    rows = np.arange(N, dtype=np.uint64)
    rows[0] = 1  # (row 0 is an input row: its picks are not used)
    ia, ib = pick[:, 0] % rows, pick[:, 1] % rows
    rinv = pow(1 << 256, -1, R_MOD)  # on Montgomery forms x' = x R: (x y)' = x' y' / R
    q1i, q2i = _mont_ints(q1), _mont_ints(q2)
    a, b, c = [0] * N, [0] * N, _mont_ints(pi) + [0] * (N - l)
    gate = lambda x: (q1i[x] * (a[x] + b[x]) + q2i[x] * a[x] % R_MOD * b[x] % R_MOD * rinv) % R_MOD * rinv % R_MOD
    ial, ibl = ia.tolist(), ib.tolist()
    for x in range(l, N):
        a[x], b[x] = c[ial[x]], c[ibl[x]]
        c[x] = gate(x)
    one = (1 << 256) % R_MOD
    if break_wire is not None:
        if not l <= break_wire < N:
            raise ValueError("break_wire must name a row past the input rows: the a slot of an input row is a fixed point")
        a[break_wire] = (a[break_wire] + one) % R_MOD
        c[break_wire] = gate(break_wire)
    if break_gate is not None:
        c[break_gate] = (c[break_gate] + one) % R_MOD
    return {"mu": mu, "l": l, "q1": q1, "q2": q2, "a": _limbs(a), "b": _limbs(b), "c": _limbs(c), "sigma": _copy_sigma(ia, ib, l, N), "public_inputs": pi,
            "s": splitmix_fr(mu + 1, base + 5)}


def _limbs(xs) -> np.ndarray:
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def _copy_sigma(ia: np.ndarray, ib: np.ndarray, l: int, N: int) -> np.ndarray:
    """one cycle per value: the users of c[y] are the a slots x with ia[x] = y and the b slots N + x with ib[x] = y, x >= l"""
    src = np.concatenate([ia[l:], ib[l:]])
    slot = np.concatenate([np.arange(l, N, dtype=np.uint64), np.arange(N + l, 2 * N, dtype=np.uint64)])
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


def sample_circuit_wide(mu: int, seed: int, break_gate: int | None = None, break_wire: int | None = None) -> dict:
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
    rows = np.arange(N, dtype=np.uint64)
    rows[0] = 1  # (row 0 is an input row: its picks are not used)
    ia, ib = pick[:, 0] % rows, pick[:, 1] % rows
    a, b, c = [0] * N, [0] * N, _ints(pi) + [0] * (N - l)

    def out(x):  # the c that satisfies row x
        s = sel["qL"][x] * a[x] + sel["qR"][x] * b[x] + sel["qM"][x] * a[x] * b[x] + sel["qH"][x] * pow(a[x], 5, R_MOD) + sel["qC"][x]
        return s % R_MOD if sel["qO"][x] == 1 else s * pow(sel["qO"][x], -1, R_MOD) % R_MOD

    ial, ibl = ia.tolist(), ib.tolist()
    for x in range(l, N):
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
    circuit = {"gate": "wide", "mu": mu, "l": l, "a": mont(a), "b": mont(b), "c": mont(c), "sigma": _copy_sigma(ia, ib, l, N), "public_inputs": pi,
               "s": splitmix_fr(mu + 1, base + 5)}
    circuit.update({k: mont(v) for k, v in sel.items()})
    return circuit

