"""
Big-int statement of the Fiat-Shamir transcript and of the two non-interactive schedules (a helper of test_fs.py / test_gpu_fs.py,
not a test), written from the definition

    init(label):   state = SHA256("zkhip-fs-v1" || label)
    absorb(data):  state = SHA256(state || 0x00 || data)
    challenge():   d = SHA256(state || 0x01), state = d, challenge = int(d, little-endian) mod 2^254

on top of zerocheck_model / wiring_model / batch_open_model -- not from the product code.  Values are canonical python ints mod r;
field elements enter the transcript as 32 little-endian bytes of their Montgomery form, integers as 8 little-endian bytes.
Commitments cannot be modelled here (no curve arithmetic): the schedules take them as given words.
"""
import hashlib

import numpy as np

import batch_open_model as bm
import pyoracle as po
import wiring_model as wm
import zerocheck_model as zm

R = po.R_MOD
MONT_R = 1 << 256
OPENED_GATE = ("a", "b", "c", "in", "q1", "q2")
OPENED_WIRING = ("w", "sid", "ssigma")


def fr_bytes(xs) -> bytes:
    return b"".join((x % R * MONT_R % R).to_bytes(32, "little") for x in xs)


def words_bytes(words) -> bytes:
    return b"".join(int(w).to_bytes(8, "little") for w in np.asarray(words, dtype=np.uint64).reshape(-1))


class Model:
    def __init__(self, label: bytes):
        self.state = hashlib.sha256(b"zkhip-fs-v1" + label).digest()

    def absorb(self, data: bytes):
        self.state = hashlib.sha256(self.state + bytes([0]) + data).digest()
        return self

    def absorb_u64(self, v: int):
        return self.absorb(v.to_bytes(8, "little"))

    def absorb_fr(self, xs):
        return self.absorb(fr_bytes(xs))

    def challenge(self) -> int:
        self.state = hashlib.sha256(self.state + bytes([1])).digest()
        return int.from_bytes(self.state, "little") % (1 << 254)

    def challenges(self, count):
        return [self.challenge() for _ in range(count)]


def _stepwise(tr, tabs, run):
    """
    A sumcheck whose challenge i is drawn after round i's evaluations were absorbed.  The models take every challenge up front, so round
    i is the FIRST round of a run of the model on the tables as folded so far (with zeros standing for the challenges it does not
    depend on), and the fold itself is batch_open_model.fold: the cost of two plain runs.
    tabs: dict name -> table; run(tabs, chal) -> the model's rounds.  -> (rounds, last values by name, challenges)
    """
    cur = {k: list(v) for k, v in tabs.items()}
    n = len(next(iter(cur.values()))).bit_length() - 1
    rounds, chal = [], []
    for i in range(n):
        rounds.append(run(cur, [0] * (n - i))[0])
        chal.append(tr.absorb_fr(rounds[-1]).challenge())
        cur = {k: bm.fold(v, chal[-1]) for k, v in cur.items()}
    return rounds, {k: v[0] for k, v in cur.items()}, chal


def batch_prove(tr, tables, claims, alpha):
    """-> (rounds n x 3, rho, finals f_j(rho))"""
    n, J = len(tables[0]).bit_length() - 1, len(tables)
    es = bm.combined_eq_tables(J, n, claims, alpha)
    tabs = {("e", j): es[j] for j in range(J)}
    tabs.update({("f", j): tables[j] for j in range(J)})
    run = lambda cur, ch: bm.sumcheck_multi([cur[("e", j)] for j in range(J)], [cur[("f", j)] for j in range(J)], ch)[0]
    rounds, last, rho = _stepwise(tr, tabs, run)
    return rounds, rho, [last[("f", j)] for j in range(J)]


def gate_prove(tables, commitments, label=b"gate"):
    """tables: dict of the six tables of 2^n ints; commitments: [6, 18] words as given -> dict of ints: n, tau, rounds, chal, values (OPENED
    order), alpha, b_rounds, rho, finals"""
    n = len(tables["a"]).bit_length() - 1
    tr = Model(label)
    tr.absorb_u64(n).absorb(words_bytes(commitments))
    tau = tr.challenges(n)
    tabs = dict(tables, eq=zm.eq_table(tau))
    rounds, at, chal = _stepwise(tr, tabs, lambda cur, ch: zm.sumcheck_gate(cur, ch)[0])
    values = [at[k] for k in OPENED_GATE]
    alpha = tr.absorb_fr(values).challenge()
    claims = [(i, chal, values[i]) for i in range(6)]
    b_rounds, rho, finals = batch_prove(tr, [tables[k] for k in OPENED_GATE], claims, alpha)
    return {"n": n, "tau": tau, "rounds": rounds, "chal": chal, "values": values, "alpha": alpha, "b_rounds": b_rounds, "rho": rho, "finals": finals}


def wiring_prove(w, sid, ssigma, commitments, v_commitment_of, label=b"wiring"):
    """v_commitment_of(tree ints) -> [18] words (the caller's commitment to the tree: it depends on alpha and beta)"""
    mu = len(w).bit_length() - 1
    tr = Model(label)
    tr.absorb_u64(mu).absorb(words_bytes(commitments))
    alpha, beta = tr.challenges(2)
    num, den, h = wm.fractions(w, sid, ssigma, alpha, beta)
    tree = wm.tree_of(h)
    v_comm = v_commitment_of(tree)
    gamma = tr.absorb(words_bytes(v_comm)).challenge()
    tau = tr.challenges(mu)
    tabs = wm.views(tree)
    tabs.update(eq=zm.eq_table(tau), num=num, den=den)
    rounds, _last, chal = _stepwise(tr, tabs, lambda cur, ch: wm.sumcheck_wiring(cur, gamma, ch)[0])
    src = {"w": w, "sid": sid, "ssigma": ssigma}
    values = [bm.evaluate(src[k], chal) for k in OPENED_WIRING]
    v_values = [bm.evaluate(tree, z) for z in wm.v_points(chal)]
    b_alpha = tr.absorb_fr(values).absorb_fr(v_values).challenge()
    b_rounds, rho_mu, finals = batch_prove(tr, [src[k] for k in OPENED_WIRING], [(i, chal, values[i]) for i in range(3)], b_alpha)
    v_rounds, rho_mu1, v_finals = batch_prove(tr, [tree], [(0, z, v) for z, v in zip(wm.v_points(chal), v_values)], b_alpha)
    return {"mu": mu, "alpha": alpha, "beta": beta, "gamma": gamma, "tau": tau, "rounds": rounds, "chal": chal, "values": values, "v_values": v_values,
            "v_commitment": v_comm, "b_alpha": b_alpha, "b_rounds": b_rounds, "rho_mu": rho_mu, "finals": finals, "v_rounds": v_rounds, "rho_mu1": rho_mu1,
            "v_finals": v_finals}


def _batch_record(rounds, n):
    return {"rounds": np.stack([zm.mont(tr) for tr in rounds]), "opening": np.zeros((n, 18), dtype=np.uint64)}


def gate_record(m, commitments):
    """the model's run in the product's record layout (zero opening proof)"""
    return {"n": m["n"], "rounds": np.stack([zm.mont(p) for p in m["rounds"]]), "commitments": np.asarray(commitments, dtype=np.uint64).reshape(6, 18),
            "values": zm.mont(m["values"]), "batch": _batch_record(m["b_rounds"], m["n"])}


def wiring_record(m, commitments):
    return {"mu": m["mu"], "rounds": np.stack([zm.mont(p) for p in m["rounds"]]), "commitments": np.asarray(commitments, dtype=np.uint64).reshape(3, 18),
            "values": zm.mont(m["values"]), "v_commitment": np.asarray(m["v_commitment"], dtype=np.uint64).reshape(18), "v_values": zm.mont(m["v_values"]),
            "batch": _batch_record(m["b_rounds"], m["mu"]), "v_batch": _batch_record(m["v_rounds"], m["mu"] + 1)}


def field_digest(rec) -> str:
    """SHA-256 over the parts of a record the model can state: everything but the opening proofs"""
    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(rec["n"] if "n" in rec else rec["mu"]).to_bytes(8, "little"))
    put(rec["commitments"])
    if "v_commitment" in rec:
        put(rec["v_commitment"])
    put(rec["rounds"]), put(rec["values"])
    if "v_values" in rec:
        put(rec["v_values"])
    for b in ("batch", "v_batch"):
        if b in rec:
            put(rec[b]["rounds"])
    return h.hexdigest()
