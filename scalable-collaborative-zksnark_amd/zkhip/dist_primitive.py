"""
Host-side mirror of the reference's `dist-primitive` functions (same names, argument meaning,
output shape and ordering -- SURVEY.md Appendix A), with every loop body executed by
libzkhip.so on the GPU.  `be` is the compute backend: a `zkhip.Ctx` in production.  (The CPU
multi-process tests inject an oracle-backed stand-in with the same methods to exercise the
exchange logic without a GPU; this module never imports the oracle.)

Field elements cross this API as numpy uint64 Montgomery limbs ([4] per Fr), points as
normalised Jacobian [18]; tables and SRS levels stay resident in HBM (DeviceBuffer / Srs).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .field import R_MOD, fr_from_mont, fr_mont, fr_sum_mont, int_to_limbs
from .net import Net, _at
from .pss import PackedSharingParams

ZERO = np.zeros(4, dtype=np.uint64)
NTT_FROM_N = 64  # party counts from which the PSS maps on Fr run as transforms (zk_fr_ntt_map) instead of the dense matrix


def _fr_vec_to_ints(a) -> List[int]:
    return [fr_from_mont(x) for x in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def _ints_to_fr(xs) -> np.ndarray:
    return np.array([fr_mont(x) for x in xs], dtype=np.uint64).reshape(-1, 4)


# ---------------------------------------------------------------------------------------
# pss2ss (unpack.rs:72-97): gather 1 Fr, unpack, pack_single each secret, scatter
# ---------------------------------------------------------------------------------------
def pss2ss(share: np.ndarray, pp: PackedSharingParams, net: Net) -> np.ndarray:
    """returns this party's Vec<F> of length l as [l,4] limbs"""
    shares = _fr_vec_to_ints(np.stack(net.all_gather(np.asarray(share, dtype=np.uint64).reshape(4))))
    secrets = pp.unpack(shares)
    w = pp.pack_single_of_one()[net.party_id]  # pack_single(s)[p] = s * pack_single(1)[p]
    return _ints_to_fr([v * w % R_MOD for v in secrets])


# ---------------------------------------------------------------------------------------
# d_msm (dmsm.rs:9-43)
# ---------------------------------------------------------------------------------------
DEDUP_MSM = True  # default of MsmQueue(dedup=...): tools switch it off to measure what the sharing is worth
PIPELINE_MSM = True  # MsmQueue.start() really starts an asynchronous pass; False: start() runs the pass to completion (serial steps)


def _addr(buf) -> int:
    """identity of a device buffer / view / raw address (the key of MsmQueue's duplicate detection)"""
    if isinstance(buf, int):
        return buf
    if hasattr(buf, "ptr"):
        return int(buf.ptr)
    if hasattr(buf, "data_ptr"):
        return int(buf.data_ptr())
    if hasattr(buf, "a"):  # the numpy-backed stand-in of the CPU tests
        return int(buf.a.__array_interface__["data"][0])
    return id(buf)


class MsmQueue:
    """
    Collects the local MSMs of SEVERAL protocol calls and runs them in ONE pipeline pass (zk_msm_g1_batch).
    Nothing on the path consumes an MSM result on the device (challenges are pre-sampled), so every
    commit / open of a protocol step can queue its MSMs, run them together and finish (exchange + public map)
    afterwards: a batch costs ~1 ms of latency chain whatever its size, a step of the driver had 2-9 of them.
    The `*_q` functions below queue their work and return a closure that produces the reference's return value
    once `run()` has been called; every party must call them, `run()` and the closures in the same order.
    """

    def __init__(self, be, dedup: bool = None):
        self.be, self.srs, self.bufs, self.lens, self.keep, self.res = be, [], [], [], [], None
        # identical items -- same SRS level, same scalar buffer, same length -- are computed ONCE (the two opens of V in step 2.d,
        # dhyperplonk.rs:307-320, commit the same first quotient q_0 = V_hi - V_lo: it does not depend on the opening point)
        self.dedup = DEDUP_MSM if dedup is None else dedup
        self.index, self.scaled = {}, {}

    def add(self, srs_list, bufs, lens, keep=()):
        """-> indices of the items' results in `res` (an index array: `q.res[idx]`)"""
        idx = []
        for s_, b_, n_ in zip(srs_list, bufs, lens):
            # Only items whose OWNER the queue holds can be merged: a buffer / view object in self.bufs keeps its allocation
            # alive until the pass is over, so one address cannot name two tables while the queue collects.  A raw integer
            # address carries no owner (it may be freed and handed out again): never merged.
            key = None if isinstance(b_, int) else (getattr(s_, "h", None) or id(s_), _addr(b_), int(n_))
            j = self.index.get(key) if (self.dedup and key is not None) else None
            if j is None:
                j = len(self.lens)
                self.srs.append(s_)
                self.bufs.append(b_)
                self.lens.append(int(n_))
                if key is not None:
                    self.index[key] = j
            idx.append(j)
        self.keep += list(keep)  # buffers that must outlive the batched pass
        return np.array(idx, dtype=np.int64)

    def scale(self, buf, lam_m, n: int):
        """lambda * buf for the pre-scaled d_msm, once per distinct scalar buffer"""
        key = None if isinstance(buf, int) else (_addr(buf), int(n), bytes(np.asarray(lam_m, dtype=np.uint64)))
        out = self.scaled.get(key) if (self.dedup and key is not None) else None
        if out is None:
            out = self.be.fr_scale(buf, lam_m, n)
            if key is not None:
                self.scaled[key] = out
                self.keep.append(buf)  # (the key names its address: hold the owner as long as the key lives)
            self.keep.append(out)
        return out

    def _close(self):
        """the pass is over: drop the owners and, with them, the keys that named their addresses"""
        self.keep, self.index, self.scaled = [], {}, {}
        self.srs, self.bufs, self.lens = [], [], []  # (views in `bufs` reference their parents: let the quotient buffers go now)

    def run(self):
        self.res = self.be.msm_g1_batch(self.srs, self.bufs, self.lens) if self.lens else np.zeros((0, 18), dtype=np.uint64)
        self._close()
        return self.res

    # the same in two halves: start() enqueues the pass on the GPU and returns (zk_msm_g1_batch_async), finish() collects the
    # points (zk_msm_wait).  Between the two the caller can enqueue the NEXT step's kernels and do its own host work -- the
    # exchange closures of a step are host arithmetic on a few hundred points, during which the GPU would otherwise idle.
    def start(self):
        self.job = None
        if self.lens and PIPELINE_MSM and hasattr(self.be, "msm_g1_batch_async"):
            self.job = self.be.msm_g1_batch_async(self.srs, self.bufs, self.lens)
        else:
            self.run()

    def finish(self):
        if getattr(self, "job", None) is not None:
            self.res = self.job.wait()
            self.job = None
            self._close()
        return self.res


def d_msm_q(be, q: MsmQueue, bases: Sequence, scalars: Sequence, lens: Sequence[int], pp: PackedSharingParams, net: Net, prescale: bool = True):
    """d_msm (dmsm.rs:9-43) with its local MSMs queued; -> closure returning [batch, 18]"""
    assert len(bases) == len(scalars) == len(lens)  # dmsm.rs:16
    p, n = net.party_id, net.n_parties
    if not len(lens):
        return lambda: np.zeros((0, 18), dtype=np.uint64)
    # the no-`comm` echo net fabricates the other parties' messages from the local one, so the map must
    # be applied exactly where the reference applies it
    if not prescale or getattr(net, "echo", False):
        sl = q.add(bases, scalars, lens)

        def fin_plain():
            gathered = net.all_gather(q.res[sl])  # [party][batch,18]
            coeff = np.array([int_to_limbs(c, 4) for c in pp.dmsm_coeffs(p)], dtype=np.uint64)
            return be.g1_lincomb_batch(np.stack([np.asarray(g).reshape(-1, 18) for g in gathered], axis=1), coeff)

        return fin_plain
    lam = sum(pp.unpack2_matrix[j][p] for j in range(pp.l)) % R_MOD
    c_p = sum(pp.pack_matrix[p][j] for j in range(pp.l)) % R_MOD
    lam_m = fr_mont(lam)
    scaled = [q.scale(s, lam_m, m) for s, m in zip(scalars, lens)]
    sl = q.add(bases, scaled, lens)

    def fin():
        gathered = net.all_gather(q.res[sl])
        ones = np.tile(int_to_limbs(1, 4), (n, 1))
        sums = be.g1_lincomb_batch(np.stack([np.asarray(g).reshape(-1, 18) for g in gathered], axis=1), ones)
        return be.g1_lincomb_batch(sums.reshape(len(lens), 1, 18), np.array([int_to_limbs(c_p, 4)], dtype=np.uint64))

    return fin


def d_msm(be, bases: Sequence, scalars: Sequence, lens: Sequence[int], pp: PackedSharingParams, net: Net, prescale: bool = True) -> np.ndarray:
    """
    bases[k]: Srs (device-resident level), scalars[k]: device buffer of lens[k] Fr shares.
    Returns this party's share of every MSM result: [batch, 18] normalised Jacobian.
    Local: G::msm per batch item (dmsm.rs:19-24).  Exchange: the leader closure
    unpack2 -> sum -> pack_from_public([sum; l]) (:29-40) is the public linear map
        out_p = c_p * sum_i lambda_i * C_i,   lambda_i = sum_j unpack2[j][i],  c_p = sum_j pack[p][j].
    prescale=True folds lambda_p into this party's SCALARS before its MSM (one element-wise Fr
    multiplication on the GPU: MSM(b, lambda*s) = lambda*MSM(b, s)), so the exchange is an
    all-gather, 7 point additions and ONE scalar multiplication by c_p instead of an 8-term
    255-bit combination on the host.  Same group element, hence the same output bits.
    """
    if len(lens) and prescale and not getattr(net, "echo", False) and getattr(net, "ctx", None) is be and hasattr(be, "d_msm"):
        # the communicator lives in the same ctx: the whole of d_msm is ONE C-ABI call (zk_d_msm)
        p, n = net.party_id, net.n_parties
        lam = sum(pp.unpack2_matrix[j][p] for j in range(pp.l)) % R_MOD
        c_p = sum(pp.pack_matrix[p][j] for j in range(pp.l)) % R_MOD
        net._count(144 * len(lens))
        return be.d_msm(list(bases), list(scalars), list(lens), np.tile(int_to_limbs(c_p, 4), (n, 1)), lam_mont=fr_mont(lam))
    q = MsmQueue(be)
    fin = d_msm_q(be, q, bases, scalars, lens, pp, net, prescale)
    q.run()
    return fin()


# ---------------------------------------------------------------------------------------
# sumcheck family (dsumcheck.rs)
# ---------------------------------------------------------------------------------------
def _round_plain(f: List[int], r: int):
    h = len(f) // 2
    s = (sum(f[:h]) % R_MOD, sum(f[h:]) % R_MOD)
    return s, [(f[j] * (1 - r) + f[j + h] * r) % R_MOD for j in range(h)]


def _round_product(f: List[int], g: List[int], r: int):
    h = len(f) // 2
    t0 = sum(f[j] * g[j] for j in range(h)) % R_MOD
    t1 = sum(f[j + h] * g[j + h] for j in range(h)) % R_MOD
    t2 = sum((2 * f[j + h] - f[j]) * (2 * g[j + h] - g[j]) for j in range(h)) % R_MOD
    fold = lambda v: [(v[j] * (1 - r) + v[j + h] * r) % R_MOD for j in range(h)]
    return (t0, t1, t2), fold(f), fold(g)


def _trace(be, kind: str, f, g, length: int, challenge):
    """test hook: a backend carrying a list `sc_trace` gets the operands of every product sumcheck appended
    (tests/test_gpu_e2e_fullsize.py anchors every transcript of a protocol run on them through independent kernels)"""
    t = getattr(be, "sc_trace", None)
    if t is not None:
        t.append((kind, f, g, length, np.array(challenge, copy=True)))


def _sc_batch(be, reqs):
    """several independent sumcheck-family calls: ONE C-ABI call (zk_sumcheck_batch) where the backend has it"""
    if hasattr(be, "sumcheck_batch") and len(reqs) > 1:
        return be.sumcheck_batch(reqs)
    out = []
    for r in reqs:
        if r[0] == "product":
            out.append(be.sumcheck_product(r[1], r[2], r[3], r[4]))
        elif r[0] == "plain":
            out.append(be.sumcheck(r[1], r[2], r[3]))
        elif r[0] == "fold":
            out.append(be.fold(r[1], r[2], r[3]))
        else:
            out.append(be.open_rounds(r[1], r[2], r[3], q_out=r[4]) if len(r) > 4 else be.open_rounds(r[1], r[2], r[3]))
    return out


def sumcheck(be, evaluation, length: int, challenge: np.ndarray) -> np.ndarray:
    """dsumcheck.rs:6-26 -> [n+1, 2, 4]; last entry (0, last)"""
    n = length.bit_length() - 1
    pairs, last = be.sumcheck(evaluation, length, challenge[:n])
    return np.concatenate([pairs, np.stack([ZERO, last])[None]])


def c_sumcheck(be, shares, length: int, challenge: np.ndarray, pp: PackedSharingParams, net: Net) -> np.ndarray:
    """dsumcheck.rs:92-146 -> [n + log2(l) + 1, 2, 4]"""
    n = length.bit_length() - 1
    pairs, last = be.sumcheck(shares, length, challenge[:n])
    v = _fr_vec_to_ints(pss2ss(last, pp, net))
    ch = _fr_vec_to_ints(challenge)
    extra = []
    for i in range(pp.l.bit_length() - 1):  # phase 2 re-uses challenge[0..log2 l] (:129)
        s, v = _round_plain(v, ch[i])
        extra.append(s)
    extra.append((0, v[0]))
    return np.concatenate([pairs, _ints_to_fr([x for p in extra for x in p]).reshape(-1, 2, 4)])


def d_sumcheck(be, partial_poly, length: int, challenge: np.ndarray, net: Net) -> np.ndarray:
    """dsumcheck.rs:287-357.  Leader: [n'+s, 2, 4]; workers: empty"""
    n = length.bit_length() - 1
    s = net.n_parties.bit_length() - 1
    pairs, last = be.sumcheck(partial_poly, length, challenge[:n])
    local = np.concatenate([pairs, np.stack([ZERO, last])[None]])
    allp = net.all_gather(local)
    if not net.is_leader:
        return np.zeros((0, 2, 4), dtype=np.uint64)
    head = fr_sum_mont([np.asarray(allp[p])[:n] for p in range(net.n_parties)])  # [n, 2, 4]: per-round sums (:440-447)
    res = []
    v = [fr_from_mont(allp[p][n][1]) for p in range(net.n_parties)]
    ch = _fr_vec_to_ints(challenge[n : n + s])
    for i in range(s):
        sm, v = _round_plain(v, ch[i])
        res.append(sm)
    return np.concatenate([head.reshape(-1, 2, 4), _ints_to_fr([x for p in res for x in p]).reshape(-1, 2, 4)])


def _d_sumcheck_leader_rounds(phase1, chals, ns, s, net):
    """the exchange (:437, one all-gather of the concatenated payloads) and the leader rounds (:440-507) of several d_sumcheck_product"""
    locals_ = [np.concatenate([tr, np.stack([lg, lf, ZERO])[None]]) for tr, lf, lg in phase1]  # marker (g, f, 0)  :433
    cuts = np.cumsum([0] + [len(x) for x in locals_])
    allp = net.all_gather(np.concatenate(locals_))  # [party][sum(n_i + 1), 3, 4]
    if not net.is_leader:
        return [np.zeros((0, 3, 4), dtype=np.uint64) for _ in chals]
    out = []
    for k, (challenge, n) in enumerate(zip(chals, ns)):
        mine = [np.asarray(allp[p])[cuts[k] : cuts[k + 1]] for p in range(net.n_parties)]
        head = fr_sum_mont([m[:n] for m in mine])  # per-round sums (:440-447)
        f = [fr_from_mont(m[n][1]) for m in mine]  # :448
        g = [fr_from_mont(m[n][0]) for m in mine]  # :449
        ch = _fr_vec_to_ints(challenge[n : n + s])
        res = []
        for i in range(s):
            t, f, g = _round_product(f, g, ch[i])
            res.append(t)
        out.append(np.concatenate([head.reshape(-1, 3, 4), _ints_to_fr([x for t in res for x in t]).reshape(-1, 3, 4)]))
    return out


# =======================================================================================
# The product sumchecks and the opens are written ONCE, against a queue of sumcheck-family kernels (ScQueue, the mirror of
# zkhost/pipeline.hpp): every *_sq form is phase A -- add the requests (the opens' quotient buffers are allocated at once, so their
# commitments can be queued) -- and returns phase B, called after ScQueue.run(), which performs the exchanges that need a kernel
# result (pss2ss of the last values, the gather of the local open values, the leader's root opens), queues the MSM items that depend
# on them and returns the finishing closure.  A protocol step adds all its primitives to ONE queue: nothing in them needs another's
# result ON THE DEVICE, and as a blocking launch chain per call they leave the chip nearly empty.  The per-call names (sumcheck_product,
# c_sumcheck_product_many, d_sumcheck_product_many_q, open_many_q, d_open_many_q, c_open_many_q and their wrappers) are the same
# forms on a queue of their own (own_batch): add, run, phase B.
# =======================================================================================
class ScQueue:
    def __init__(self, be):
        self.be, self.reqs, self.res = be, [], None

    def add(self, req) -> int:
        if req[0] == "open" and len(req) < 5:  # the quotient buffer exists before the batch runs: a later MSM item may name it
            req = tuple(req) + (self.be.alloc(max(32 * (req[2] - 1), 1)),)
        self.reqs.append(tuple(req))
        return len(self.reqs) - 1

    def out_of(self, i: int):
        return self.reqs[i][4]

    def run(self):
        self.res = _sc_batch(self.be, self.reqs) if self.reqs else []
        self.reqs = []

    def at(self, i: int):
        if self.res is None:
            raise RuntimeError("ScQueue: a result was read before the batch ran")
        return self.res[i]


def own_batch(be, add):
    """a primitive's kernels as a batch of their own: `add(queue)` is its *_sq form; the queue runs at once; -> what the form returned"""
    sq = ScQueue(be)
    out = add(sq)
    sq.run()
    return out


def c_sumcheck_product_many_sq(be, sq: ScQueue, pairs: Sequence, length: int, challenge: np.ndarray, pp: PackedSharingParams, net: Net):
    """c_sumcheck_product_many: A adds the phase-1 loops, B = the pss2ss hand-offs (:224-225) and phase 2, item by item"""
    n = length.bit_length() - 1
    idx = []
    for f, g in pairs:
        _trace(be, "c", f, g, length, challenge[:n])
        idx.append(sq.add(("product", f, g, length, challenge[:n])))
    ch = _fr_vec_to_ints(challenge)

    def phase_b():
        out = []
        for i in idx:
            tr, lf, lg = sq.at(i)
            vf = _fr_vec_to_ints(pss2ss(lf, pp, net))  # :224
            vg = _fr_vec_to_ints(pss2ss(lg, pp, net))  # :225
            extra = []
            for r in range(pp.l.bit_length() - 1):
                t, vf, vg = _round_product(vf, vg, ch[r])
                extra.append(t)
            extra.append((0, vf[0] * vg[0] % R_MOD, 0))  # :282
            out.append(np.concatenate([tr, _ints_to_fr([x for t in extra for x in t]).reshape(-1, 3, 4)]))
        return out

    return phase_b


def sumcheck_product_sq(be, sq: ScQueue, ef, eg, length: int, challenge: np.ndarray):
    """sumcheck_product (dsumcheck.rs:28-90) with its kernels in the batch; -> closure (call after the batch)"""
    n = length.bit_length() - 1
    _trace(be, "plain", ef, eg, length, challenge[:n])
    i = sq.add(("product", ef, eg, length, challenge[:n]))

    def fin():
        tr, lf, lg = sq.at(i)
        prod = fr_mont(fr_from_mont(lf) * fr_from_mont(lg) % R_MOD)
        return np.concatenate([tr, np.stack([ZERO, prod, ZERO])[None]])

    return fin


def open_many_sq(be, sq: ScQueue, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray]):
    """several independent opens (dpoly_comm.rs:299-325 each): their fold rounds (:309-323) are added to the batch, the commitments of
    all q_i are queued; nothing to exchange, so there is no phase B -- the values are read when the finishing closure runs"""
    pts = [np.asarray(pt, dtype=np.uint64).reshape(-1, 4) for pt in points]
    idx = [sq.add(("open", pe, length, pt[: length.bit_length() - 1])) for pe, length, pt in zip(pevals, lens, pts)]
    qbufs = [sq.out_of(i) for i in idx]
    q0s = _first_quotient_sources(pevals, lens, qbufs)
    cuts = []
    for qb, length, q0 in zip(qbufs, lens, q0s):
        s_, b_, l_ = _open_msm_items(powers_of_g, qb, length, q0)
        cuts.append(q.add(s_, b_, l_, keep=[qb]))

    def fin():
        return [(sq.at(i)[1], q.res[c]) for i, c in zip(idx, cuts)]

    fin.idx = idx
    return fin


def d_open_many_sq(be, sq: ScQueue, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray], net: Net):
    """several d_open (dpoly_comm.rs:355-398): A = the local opens' kernels and quotient commitments; B = the gather of the local values
    and, on the leader, the root opens (:372-378: tables of N_p values -- their fold rounds run on the host, only the quotients go to
    the device for their commitments); B -> the finishing closure: the exchange of the proofs, root proofs ++ summed local proofs"""
    k = len(lens)
    if not k:
        return lambda: (lambda: [])
    plog = net.n_parties.bit_length() - 1
    npar = net.n_parties
    pts = [np.asarray(p, dtype=np.uint64).reshape(-1, 4) for p in points]
    f_local = open_many_sq(be, sq, q, powers_of_g, pevals, lens, [p[plog:] for p in pts])

    def phase_b():
        vals_mine = np.stack([np.asarray(sq.at(i)[1], dtype=np.uint64).reshape(4) for i in f_local.idx])
        vals = net.all_gather(vals_mine)  # [party][k, 4]
        roots = None
        if net.is_leader:
            cols = np.stack([np.asarray(v).reshape(-1, 4) for v in vals], axis=1)  # [k][party][4]
            rvals, qall = [], []
            for i in range(k):
                cur = _fr_vec_to_ints(cols[i])
                lo = _fr_vec_to_ints(pts[i][:plog])
                for r in range(plog):
                    h = len(cur) // 2
                    qall += [(cur[j + h] - cur[j]) % R_MOD for j in range(h)]
                    cur = [(cur[j] + lo[r] * (cur[j + h] - cur[j])) % R_MOD for j in range(h)]
                rvals.append(fr_mont(cur[0]))
            rcuts = [np.zeros(0, dtype=np.int64)] * k
            if npar > 1:
                dq = be.to_device(_ints_to_fr(qall))  # [k][N_p - 1]
                rcuts = []
                for i in range(k):
                    s_, b_, l_ = _open_msm_items(powers_of_g, dq.at(32 * (npar - 1) * i), npar)
                    rcuts.append(q.add(s_, b_, l_, keep=[dq]))
            roots = (rvals, rcuts)

        def fin():
            local = f_local()
            cuts = [0]
            for _, prf in local:
                cuts.append(cuts[-1] + len(prf))
            prfs = net.all_gather(np.concatenate([prf for _, prf in local]) if cuts[-1] else np.zeros((0, 18), dtype=np.uint64))
            if not net.is_leader:
                return [(ZERO.copy(), np.zeros((0, 18), dtype=np.uint64)) for _ in range(k)]
            ones = np.tile(int_to_limbs(1, 4), (npar, 1))
            total = cuts[-1]
            pi = be.g1_lincomb_batch(np.stack([np.asarray(g).reshape(-1, 18) for g in prfs], axis=1), ones) if total else np.zeros((0, 18), dtype=np.uint64)
            out = []
            for i in range(k):
                allp = list(q.res[roots[1][i]]) + list(pi[cuts[i] : cuts[i + 1]])  # root proofs FIRST (:379-384)
                out.append((roots[0][i], np.stack(allp) if allp else np.zeros((0, 18), dtype=np.uint64)))
            return out

        return fin

    return phase_b


def c_open_many_sq(be, sq: ScQueue, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray], pp: PackedSharingParams, net: Net):
    """several c_open (dpoly_comm.rs:401-464) whose q_i commitments share ONE queued d_msm.  A = the fold rounds (:418-432); B = that
    d_msm over all quotients (:436; with real parties d_msm_q pre-scales its scalars on the device when it is called, and the quotient
    buffers are filled by the batch), pss2ss of the last values (:440) and the log2(l) extra rounds, whose small MSMs are queued too;
    B -> the finishing closure"""
    k = len(lens)
    pts = [np.asarray(p, dtype=np.uint64).reshape(-1, 4) for p in points]
    # the same table at the same point again (cpermcheck opens num / den twice, dhyperplonk.rs:1324 and :1371) is the same request: its
    # kernels run once and its MSM items name the same quotient buffers, which the MsmQueue computes once
    keys = [(_addr(pe), length, pt[: length.bit_length() - 1].tobytes()) for pe, length, pt in zip(pevals, lens, pts)]
    seen, idx = {}, []
    for i, key in enumerate(keys):
        if key not in seen:
            seen[key] = sq.add(("open", pevals[i], lens[i], pts[i][: lens[i].bit_length() - 1]))
        idx.append(seen[key])
    qbufs = [sq.out_of(i) for i in idx]
    q0s = _first_quotient_sources(pevals, lens, qbufs)
    srs, bufs, ms, cuts = [], [], [], [0]
    for qb, length, q0 in zip(qbufs, lens, q0s):
        s_, b_, l_ = _open_msm_items(powers_of_g, qb, length, q0, pp.l)
        srs, bufs, ms = srs + s_, bufs + b_, ms + l_
        q.keep.append(qb)
        cuts.append(len(ms))

    def phase_b():
        f_com = d_msm_q(be, q, srs, bufs, ms, pp, net)
        tails = []
        for i in range(k):
            cur = _fr_vec_to_ints(pss2ss(sq.at(idx[i])[1], pp, net))
            pt = _fr_vec_to_ints(pts[i])
            fins = []
            for r in range(pp.l.bit_length() - 1):
                h = len(cur) // 2
                qi = [(cur[j + h] - cur[j]) % R_MOD for j in range(h)]
                level = (len(qi) * pp.l).bit_length() - 1
                d_qi = be.to_device(_ints_to_fr(qi))
                fins.append(q.add([powers_of_g[level]], [d_qi], [len(qi)], keep=[d_qi]))
                cur = [(cur[j] * (1 - pt[r]) + cur[j + h] * pt[r]) % R_MOD for j in range(h)]
            tails.append((fr_mont(cur[0]), fins))

        def fin():
            com = f_com()
            out = []
            for i in range(k):
                res = list(com[cuts[i] : cuts[i + 1]]) + [q.res[sl][0] for sl in tails[i][1]]
                out.append((tails[i][0], np.stack(res) if res else np.zeros((0, 18), dtype=np.uint64)))
            return out

        return fin

    return phase_b


def d_sumcheck_product_many_sq(be, sq: ScQueue, items: Sequence, net: Net):
    """several independent d_sumcheck_product (dsumcheck.rs:359-512); items = [(partial_f, partial_g, length, challenge)].  Their local
    phases are added to the batch; -> closure (exchange + leader rounds, _d_sumcheck_leader_rounds), called when the transcript is
    assembled, after ScQueue.run(): a protocol step calls it after it has started its MSM pass, the host work then runs beside the GPU's"""
    if not len(items):
        return lambda: []
    s = net.n_parties.bit_length() - 1
    ns = [length.bit_length() - 1 for _, _, length, _ in items]
    idx = []
    for (f, g, length, ch), n in zip(items, ns):
        _trace(be, "d", f, g, length, ch[: n + s])
        idx.append(sq.add(("product", f, g, length, ch[:n])))
    chals = [np.array(ch, copy=True) for _, _, _, ch in items]

    def fin():
        phase1 = [sq.at(i) for i in idx]
        return _d_sumcheck_leader_rounds(phase1, chals, ns, s, net)

    return fin


# the per-call forms of the product sumchecks: each a batch of its own, phase B at once
def sumcheck_product(be, ef, eg, length: int, challenge: np.ndarray) -> np.ndarray:
    """dsumcheck.rs:28-90 -> [n+1, 3, 4]; last entry (0, f*g, 0)"""
    return own_batch(be, lambda sq: sumcheck_product_sq(be, sq, ef, eg, length, challenge))()


def c_sumcheck_product_many(be, pairs: Sequence, length: int, challenge: np.ndarray, pp: PackedSharingParams, net: Net) -> List[np.ndarray]:
    """several independent c_sumcheck_product on tables of one length: their phase-1 loops as ONE batched call, then the hand-offs"""
    return own_batch(be, lambda sq: c_sumcheck_product_many_sq(be, sq, pairs, length, challenge, pp, net))()


def c_sumcheck_product(be, shares_f, shares_g, length: int, challenge: np.ndarray, pp: PackedSharingParams, net: Net) -> np.ndarray:
    """dsumcheck.rs:148-285 -> [n + log2(l) + 1, 3, 4]"""
    return c_sumcheck_product_many(be, [(shares_f, shares_g)], length, challenge, pp, net)[0]


def d_sumcheck_product_many_q(be, items: Sequence, net: Net):
    """the local phases of several d_sumcheck_product run NOW as one batched call; -> closure: the exchange and the leader part"""
    return own_batch(be, lambda sq: d_sumcheck_product_many_sq(be, sq, items, net))


def d_sumcheck_product_many(be, items: Sequence, net: Net) -> List[np.ndarray]:
    """several independent d_sumcheck_product (dsumcheck.rs:359-512) at once: the local phases as one batched call, one exchange"""
    return d_sumcheck_product_many_q(be, items, net)()


def d_sumcheck_product(be, partial_f, partial_g, length: int, challenge: np.ndarray, net: Net) -> np.ndarray:
    """dsumcheck.rs:359-512.  Leader: [n'+s, 3, 4]; workers: empty.  Marker tuple is (g, f, 0) (:433)"""
    return d_sumcheck_product_many(be, [(partial_f, partial_g, length, challenge)], net)[0]


# ---------------------------------------------------------------------------------------
# product accumulation (dacc_product.rs)
# ---------------------------------------------------------------------------------------
def sub_index(i: int) -> Tuple[int, int]:
    """dacc_product.rs:18-23"""
    x = (i & ~(1 << (i.bit_length() - 1))) << 1
    return x, x + 1


def acc_product(be, x, N: int):
    """dacc_product.rs:30-57 -> device tree (2N Fr); views v(x,0)=tree[0::2], v(x,1)=tree[1::2], v(1,x)=tree[N:]"""
    return be.product_tree(x, N)


def d_acc_product(be, inputs, N: int, net: Net):
    """dacc_product.rs:365-414 -> (subtree device buffer, leader tree [2*N_p,4] or None)"""
    subtree = be.product_tree(inputs, N)
    root = subtree.download((1, 4), offset=32 * (2 * N - 1))[0]  # the forced 0 (:381,:390)
    roots = net.all_gather(root)
    if not net.is_leader:
        return subtree, None
    t = [fr_from_mont(r) for r in roots]
    npar = net.n_parties
    for i in range(npar, 2 * npar - 1):
        a, b = sub_index(i)
        t.append(t[a] * t[b] % R_MOD)
    t.append(0)
    return subtree, _ints_to_fr(t)


# ---------------------------------------------------------------------------------------
# polynomial commitment (dpoly_comm.rs:236-464).  powers_of_g: list of Srs, level k has 2^k points
# ---------------------------------------------------------------------------------------
class PolynomialCommitmentCub:
    """
    dpoly_comm.rs:18-28,36-234: the un-matured parameter set (`powers_of_g[k]` = one Srs level of 2^k points,
    resident in HBM).  `mature()` (:141-151, projective -> affine) has nothing left to do here: levels are
    built and kept as affine records.  powers_of_g2 is not carried (G2 only serves the pairing check `verify`).
    """

    def __init__(self, powers_of_g: List):
        self.powers_of_g = powers_of_g

    @staticmethod
    def new(be, s: np.ndarray, g: np.ndarray = None) -> "PolynomialCommitmentCub":
        """:37-67: s = [n,4] Montgomery Fr; level k = g^{eq-basis over s_{n-k}..s_{n-1}} (one device pass per level)"""
        return PolynomialCommitmentCub(be.srs_powers(s, g))

    @staticmethod
    def new_single(be, len_log_2: int, pp: PackedSharingParams, seed: int = 1) -> "PolynomialCommitmentCub":
        """:197-219: a toy single-party parameter set, level i holds max(1, 2^i / l) synthetic points"""
        return PolynomialCommitmentCub([be.srs_generate(seed * 7919 + 2 * i + 1, seed * 104729 + 2 * i + 3, max(1, (1 << i) // pp.l)) for i in range(len_log_2 + 1)])

    @staticmethod
    def new_random(be, len_log_2: int, party_count: int, seed: int = 1) -> "PolynomialCommitmentCub":
        """:220-233: levels 0 .. len_log_2 - log2(party_count) of 2^i synthetic points"""
        top = len_log_2 - (party_count.bit_length() - 1)
        return PolynomialCommitmentCub([be.srs_generate(seed * 6007 + 2 * i + 5, seed * 15485863 + 2 * i + 7, 1 << i) for i in range(top + 1)])

    def to_packed(self, be, pp: PackedSharingParams, party: int) -> "PolynomialCommitmentCub":
        """:164-194 for ONE party (every GPU builds its own share): level i -> pack_from_public of every l-chunk"""
        row = np.array([int_to_limbs(pp.pack_matrix[party][j], 4) for j in range(pp.l)], dtype=np.uint64)
        return PolynomialCommitmentCub([be.srs_to_packed(lv, row, pp.l) for lv in self.powers_of_g])

    def mature(self) -> List:
        return self.powers_of_g


def commit_q(q: MsmQueue, powers_of_g, peval, length: int):
    level = length.bit_length() - 1
    assert level < len(powers_of_g) and length == 1 << level
    sl = q.add([powers_of_g[level]], [peval], [length])
    return lambda: q.res[sl][0]


def commit(be, powers_of_g, peval, length: int) -> np.ndarray:
    """dpoly_comm.rs:237-243 (= d_local_commit :269-275)"""
    level = length.bit_length() - 1
    assert level < len(powers_of_g) and length == 1 << level
    return be.msm_g1(powers_of_g[level], peval, length)


def _first_quotient_sources(pevals, lens, qbufs):
    """opens of the SAME table share their first quotient q_0 = hi - lo (it does not depend on the point): for every open the
    buffer whose first len/2 elements serve as its q_0 -- the first open's of that table.  With MsmQueue's duplicate
    detection the commitment of q_0 is then one MSM for all of them."""
    first, out = {}, []
    for pe, length, qb in zip(pevals, lens, qbufs):
        out.append(first.setdefault((_addr(pe), int(length)), qb))
    return out


def _open_msm_items(powers_of_g, q, length: int, q0=None, l: int = 1):
    """the n commitments of one open (:318-321) as MSM items over the quotient buffer q: (srs list, scalar views, lens); l: the packing
    factor of a c_open, whose h shares are committed on the level of h l points (:256-257)"""
    n = length.bit_length() - 1
    srs, bufs, lens, off, m = [], [], [], 0, length
    for i in range(n):
        h = m // 2
        srs.append(powers_of_g[(h * l).bit_length() - 1])
        bufs.append((q0 if (i == 0 and q0 is not None) else q).at(32 * off))
        lens.append(h)
        off += h
        m = h
    return srs, bufs, lens


def open_many_q(be, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray]):
    """open_many_sq with the fold rounds run now; -> closure"""
    return own_batch(be, lambda sq: open_many_sq(be, sq, q, powers_of_g, pevals, lens, points))


def open_many(be, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray]):
    """
    several independent opens (dpoly_comm.rs:299-325 each) with ALL their commitments in one batched MSM
    pass: -> list of (value [4], proofs [n_k, 18]).  Same outputs as calling open_ once per polynomial.
    """
    q = MsmQueue(be)
    fin = open_many_q(be, q, powers_of_g, pevals, lens, points)
    q.run()
    return fin()


def open_(be, powers_of_g, peval, length: int, point: np.ndarray):
    """dpoly_comm.rs:299-325 (= d_local_open :327-353) -> (value [4], proofs [n,18])"""
    # the n commitments of one open are independent: one batched pass (the reference commits them one by one)
    return open_many(be, powers_of_g, [peval], [length], [point])[0]


def d_commit_many_q(be, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], net: Net):
    k = len(lens)
    if not k:
        return lambda: np.zeros((0, 18), dtype=np.uint64)
    srs = []
    for length in lens:
        level = length.bit_length() - 1
        assert level < len(powers_of_g) and length == 1 << level
        srs.append(powers_of_g[level])
    sl = q.add(srs, pevals, lens)

    def fin():
        got = net.all_gather(q.res[sl])  # [party][k, 18]
        ones = np.tile(int_to_limbs(1, 4), (net.n_parties, 1))
        return be.g1_lincomb_batch(np.stack([np.asarray(g).reshape(-1, 18) for g in got], axis=1), ones)  # [k][party][18]

    return fin


def d_commit_many(be, powers_of_g, pevals: Sequence, lens: Sequence[int], net: Net) -> np.ndarray:
    """several d_commit (dpoly_comm.rs:276-297) in one MSM pass and one exchange -> [k, 18]"""
    q = MsmQueue(be)
    fin = d_commit_many_q(be, q, powers_of_g, pevals, lens, net)
    q.run()
    return fin()


def d_commit(be, powers_of_g, peval, length: int, net: Net) -> np.ndarray:
    """dpoly_comm.rs:276-297: every party ends with the sum of the local commitments"""
    return d_commit_many(be, powers_of_g, [peval], [length], net)[0]


def _c_commit_bases(powers_of_g, lens, pp):
    bases = []
    for n in lens:
        level = (n * pp.l).bit_length() - 1
        assert level < len(powers_of_g) and n * pp.l == 1 << level  # :256-257
        bases.append(powers_of_g[level])
    return bases


def c_commit_q(be, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], pp: PackedSharingParams, net: Net):
    return d_msm_q(be, q, _c_commit_bases(powers_of_g, lens, pp), pevals, lens, pp, net)


def c_commit(be, powers_of_g, pevals: Sequence, lens: Sequence[int], pp: PackedSharingParams, net: Net) -> np.ndarray:
    """dpoly_comm.rs:244-267: d_msm with bases_k = powers_of_g[log2(len_k * l)] -> [batch, 18]"""
    return d_msm(be, _c_commit_bases(powers_of_g, lens, pp), pevals, lens, pp, net)


def d_open_many_q(be, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray], net: Net):
    """d_open_many_sq with the local fold rounds, the exchange of the local VALUES and the leader's root opens done now; -> closure"""
    return own_batch(be, lambda sq: d_open_many_sq(be, sq, q, powers_of_g, pevals, lens, points, net))()


def d_open_many(be, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray], net: Net):
    """
    several d_open (dpoly_comm.rs:355-398) at once: the local opens and the leader's root opens share one batched
    MSM pass, the values and proofs travel in one exchange each.
    -> list of (root value [4], root proofs ++ summed local proofs) for the leader, (0, []) for workers.
    """
    q = MsmQueue(be)
    fin = d_open_many_q(be, q, powers_of_g, pevals, lens, points, net)
    q.run()
    return fin()


def d_open(be, powers_of_g, peval, length: int, point: np.ndarray, net: Net):
    """
    dpoly_comm.rs:355-398.  Leader: (root value [4], root proofs (s entries) ++ summed local proofs
    (n' entries)) -- root proofs FIRST (:379-384); workers: (0, []).
    """
    return d_open_many(be, powers_of_g, [peval], [length], [point], net)[0]


def c_open_many_q(be, q: MsmQueue, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray], pp: PackedSharingParams, net: Net):
    """c_open_many_sq with the fold rounds and the pss2ss hand-offs done now, the d_msm and the tail's MSMs queued; -> closure"""
    return own_batch(be, lambda sq: c_open_many_sq(be, sq, q, powers_of_g, pevals, lens, points, pp, net))()


def c_open_many(be, powers_of_g, pevals: Sequence, lens: Sequence[int], points: Sequence[np.ndarray], pp: PackedSharingParams, net: Net):
    """several c_open (dpoly_comm.rs:401-464) whose q_i commitments share ONE d_msm -> list of (value, proofs)"""
    q = MsmQueue(be)
    fin = c_open_many_q(be, q, powers_of_g, pevals, lens, points, pp, net)
    q.run()
    return fin()


def c_open(be, powers_of_g, peval, length: int, point: np.ndarray, pp: PackedSharingParams, net: Net):
    """
    dpoly_comm.rs:401-464: n fold rounds producing every q_i, ONE batched d_msm over them (:436),
    pss2ss of the last value, then log2(l) more rounds on the l-vector re-using point[0..] (:452).
    Returns (value [4], proofs [n + log2 l, 18]).
    """
    return c_open_many(be, powers_of_g, [peval], [length], [point], pp, net)[0]


def verify(powers_of_g2, commitment: np.ndarray, value: np.ndarray, proof: np.ndarray, point: np.ndarray, g1=None) -> bool:
    """
    PolynomialCommitment::verify (dpoly_comm.rs:466-484): e(C - value g1, g2) == sum_i e(proof_i, powers_of_g2[i+1] - point_i g2).
    commitment [18] / proof [n, 18]: normalised Jacobian as the library returns them; value [4], point [n, 4]: Montgomery Fr;
    powers_of_g2: affine G2 points as python ints (zkhip.pairing.powers_of_g2); g1 = powers_of_g[0][0] (default: the generator).
    Host big-int pairing (zkhip/pairing.py): off the hot path, seconds per call.
    """
    from . import pairing as pr
    from .field import jacobian_to_affine_ints

    pts = [jacobian_to_affine_ints(p) for p in np.asarray(proof, dtype=np.uint64).reshape(-1, 18)]
    return pr.verify(g1 or pr.G1_GEN, powers_of_g2, jacobian_to_affine_ints(commitment), fr_from_mont(value), pts, _fr_vec_to_ints(point))


def pcs_vk(be, powers_of_g2, g1=None):
    """the verifying key of a PolynomialCommitment on the device (zk_pcs_vk): powers_of_g2 as python-int affine points
    (zkhip.pairing.powers_of_g2) or [n, 24] Montgomery records; g1 = powers_of_g[0][0] (python ints or [12]; None: the generator)"""
    from .field import affine_ints_to_mont, fq_mont

    pg2 = powers_of_g2
    if not isinstance(pg2, np.ndarray):
        pg2 = np.stack([np.zeros(24, dtype=np.uint64) if P is None else
                        np.concatenate([fq_mont(P[0][0]), fq_mont(P[0][1]), fq_mont(P[1][0]), fq_mont(P[1][1])]) for P in pg2])
    if g1 is not None and not isinstance(g1, np.ndarray):
        g1 = affine_ints_to_mont(g1)
    return be.pcs_vk(pg2, g1)


def verify_batch(be, vk, commitments, values, proofs, points) -> np.ndarray:
    """
    PolynomialCommitment::verify (dpoly_comm.rs:466-484) for a batch of openings on the device (zk_pcs_verify_batch): commitments
    [count, 18] Jacobian, values [count, 4] Montgomery Fr, proofs [count, nvars, 18], points [count, nvars, 4]; vk from pcs_vk.
    Returns one verdict per opening -- the same as `verify` on every input whose points lie in their subgroups.
    """
    return be.pcs_verify_batch(vk, commitments, values, proofs, points)


def agg_arrays(openings):
    """[(C [J, 18], e [J, 4] Montgomery, value [4], proofs [nvars, 18], point [nvars, 4], skip)] -> the flat arrays of
    zk_pcs_verify_agg / zk_pcs_agg_weights: (nvars, skip, cstart, cpoints, cscalars, values, proofs, points)"""
    u = lambda a, w: np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, w)
    cs = [u(o[0], 18) for o in openings]
    cat = lambda parts, w: np.concatenate(parts) if parts else np.zeros((0, w), dtype=np.uint64)
    pfs = [u(o[3], 18) for o in openings]
    return (np.array([len(p) for p in pfs], dtype=np.uint64), np.array([int(o[5]) for o in openings], dtype=np.uint64),
            np.cumsum([0] + [len(c) for c in cs]).astype(np.uint64), cat(cs, 18), cat([u(o[1], 4) for o in openings], 4),
            cat([u(o[2], 4) for o in openings], 4), cat(pfs, 18), cat([u(o[4], 4) for o in openings], 4))


def verify_agg(be, vk, openings, rho=None) -> bool:
    """
    Any number of openings of mixed variable counts in ONE pairing check (zk_pcs_verify_agg): True when every opening holds, False
    when one does not (up to the soundness error count / 2^128 of the derived weights).  openings: the tuples of agg_arrays -- the
    commitment of an opening is sum_j e_j C_j, proof point i pairs with powers_of_g2[1 + skip + i] of the FULL key vk.
    rho: [count, 2] u64 explicit weights (tests), None: derived from the openings.
    """
    return be.pcs_verify_agg(vk, *agg_arrays(openings), rho=rho)


def verify_device(be, powers_of_g2, commitment: np.ndarray, value: np.ndarray, proof: np.ndarray, point: np.ndarray, g1=None) -> bool:
    """`verify` with the reference's arguments, on the device: one opening through verify_batch"""
    vk = powers_of_g2 if hasattr(powers_of_g2, "n_g2") else pcs_vk(be, powers_of_g2, g1)
    pf = np.asarray(proof, dtype=np.uint64).reshape(1, -1, 18)
    return bool(verify_batch(be, vk, np.asarray(commitment, dtype=np.uint64).reshape(1, 18), np.asarray(value, dtype=np.uint64).reshape(1, 4),
                             pf, np.asarray(point, dtype=np.uint64).reshape(1, pf.shape[1], 4))[0])


def fix_variable(be, evaluations, length: int, points: np.ndarray):
    """mle.rs:88-105 -> device buffer of length >> min(n, len(points))"""
    return be.fold(evaluations, length, points)


def d_fix_variable(be, shares, length: int, points: np.ndarray, pp: PackedSharingParams, net: Net):
    """mle.rs:51-86: returns a device buffer (points <= n) or a [1,4] host array (points > n)"""
    n = length.bit_length() - 1
    points = np.asarray(points, dtype=np.uint64).reshape(-1, 4)
    cnt = len(points)
    folded = be.fold(shares, length, points[: min(n, cnt)])
    if cnt <= n:
        return folded
    last = folded.download((1, 4))[0]
    cur = _fr_vec_to_ints(pss2ss(last, pp, net))
    pt = _fr_vec_to_ints(points)
    for i in range(min(cnt - n, pp.l.bit_length() - 1)):  # re-uses points[0..] (:78)
        h = len(cur) // 2
        cur = [(cur[j] * (1 - pt[i]) + cur[j + h] * pt[i]) % R_MOD for j in range(h)]
    return _ints_to_fr([cur[0]])


def _mont_matrix(rows: Sequence[Sequence[int]]) -> np.ndarray:
    """python-int matrix -> [rows, cols, 4] Montgomery limbs for zk_fr_apply_matrix"""
    return np.array([[fr_mont(v) for v in r] for r in rows], dtype=np.uint64).reshape(len(rows), -1, 4)


def _unpack2_many_device(be, gathered: Sequence[np.ndarray], pp: PackedSharingParams) -> np.ndarray:
    """gathered[i] = party i's [k,4] vector -> transpose(.).flat_map(unpack2): [k*l, 4] (unpack.rs:55-70)"""
    k = len(gathered[0])
    if k == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    d_in = be.to_device(np.concatenate([np.asarray(g, dtype=np.uint64).reshape(-1, 4) for g in gathered]))  # [n][k]
    if pp.n >= NTT_FROM_N and hasattr(be, "fr_ntt_map"):  # the reference's own form: ifft on the share domain, fft on the secret2 coset
        out = be.fr_ntt_map(pp.ntt_tables("unpack2"), d_in, 1, k, k, pp.l, 1)
    else:
        out = be.fr_apply_matrix(_mont_matrix(pp.unpack2_matrix), d_in, 1, k, k, pp.l, 1)  # out[j*l + r]
    return out.download((k * pp.l, 4))


# ---------------------------------------------------------------------------------------
# small exchanges: degree reduction and unpacking (degree_reduce.rs, unpack.rs)
# ---------------------------------------------------------------------------------------
def _apply_rows(rows: Sequence[Sequence[int]], columns: Sequence[np.ndarray]) -> np.ndarray:
    """out[r][k] = sum_i rows[r][i] * columns[i][k]; columns[i]: [k,4] limbs -> [len(rows), k, 4]"""
    cols = [_fr_vec_to_ints(c) for c in columns]
    k = len(cols[0])
    out = [[sum(row[i] * cols[i][j] for i in range(len(cols))) % R_MOD for j in range(k)] for row in rows]
    return np.stack([_ints_to_fr(o) for o in out]) if k else np.zeros((len(rows), 0, 4), dtype=np.uint64)


def degree_reduce_many(shares: np.ndarray, pp: PackedSharingParams, net: Net, be=None) -> np.ndarray:
    """
    degree_reduce.rs:10-26: element-wise pack_from_public(unpack2(.))[party] over the batch ([k,4] -> [k,4]).
    The composite D = pack o unpack2 is one public n x n matrix; this party needs only its row.
    With a backend the row is applied on the GPU (zk_fr_apply_matrix), otherwise with host big-ints.
    """
    shares = np.asarray(shares, dtype=np.uint64).reshape(-1, 4)
    allp = net.all_gather(shares)
    p, l, n = net.party_id, pp.l, pp.n
    row = [sum(pp.pack_matrix[p][j] * pp.unpack2_matrix[j][i] for j in range(l)) % R_MOD for i in range(n)]
    k = len(shares)
    if be is not None and k:
        d_in = be.to_device(np.concatenate(allp))  # [n][k]
        return be.fr_apply_matrix(_mont_matrix([row]), d_in, 1, k, k, 1, k).download((k, 4))
    return _apply_rows([row], allp)[0]


def degree_reduce(share: np.ndarray, pp: PackedSharingParams, net: Net) -> np.ndarray:
    """degree_reduce.rs:29-41"""
    vals = _fr_vec_to_ints(np.stack(net.all_gather(np.asarray(share, dtype=np.uint64).reshape(4))))
    return fr_mont(pp.pack_from_public(pp.unpack2(vals))[net.party_id])


def d_unpack_0(share: np.ndarray, pp: PackedSharingParams, net: Net) -> np.ndarray:
    """unpack.rs:8-18: every party receives unpack(shares)[0]"""
    vals = _fr_vec_to_ints(np.stack(net.all_gather(np.asarray(share, dtype=np.uint64).reshape(4))))
    return fr_mont(pp.unpack(vals)[0])


def d_unpack(share: np.ndarray, receiver: int, pp: PackedSharingParams, net: Net) -> np.ndarray:
    """unpack.rs:20-35: only `receiver` obtains unpack(shares) ([l,4]); others an empty Vec"""
    vals = net.all_gather(np.asarray(share, dtype=np.uint64).reshape(4))
    if net.party_id != receiver:
        return np.zeros((0, 4), dtype=np.uint64)
    return _ints_to_fr(pp.unpack(_fr_vec_to_ints(np.stack(vals))))


def d_unpack2(share: np.ndarray, receiver: int, pp: PackedSharingParams, net: Net) -> np.ndarray:
    """unpack.rs:37-52"""
    vals = net.all_gather(np.asarray(share, dtype=np.uint64).reshape(4))
    if net.party_id != receiver:
        return np.zeros((0, 4), dtype=np.uint64)
    return _ints_to_fr(pp.unpack2(_fr_vec_to_ints(np.stack(vals))))


def d_unpack2_many(share: np.ndarray, receiver: int, pp: PackedSharingParams, net: Net, be=None) -> np.ndarray:
    """unpack.rs:55-70: receiver gets transpose(shares).flat_map(unpack2) = [k*l, 4]"""
    share = np.asarray(share, dtype=np.uint64).reshape(-1, 4)
    allp = net.all_gather(share)
    if net.party_id != receiver:
        return np.zeros((0, 4), dtype=np.uint64)
    if be is not None:
        return _unpack2_many_device(be, allp, pp)
    cols = [_fr_vec_to_ints(a) for a in allp]
    out = []
    for k in range(len(share)):
        out.extend(pp.unpack2([cols[i][k] for i in range(pp.n)]))
    return _ints_to_fr(out)


def c_acc_product(be, inputs, N: int, pp: PackedSharingParams, net: Net):
    """
    dacc_product.rs:296-363: local subtree; every party sends its LAST min(N_p, 2N) entries (:321-329);
    the leader interleaves them level by level (:339-349) and appends N_p - 1 products and a 0.
    Returns (subtree device buffer, leader tree [.,4] or None).
    """
    subtree = be.product_tree(inputs, N)
    npar = pp.n
    num_to_send = min(npar, 2 * N)
    tail = subtree.download((num_to_send, 4), offset=32 * (2 * N - num_to_send))
    recv = net.all_gather(tail)
    if not net.is_leader:
        return subtree, None
    r = [_fr_vec_to_ints(a) for a in recv]
    tree, layer, start = [], 1 << (num_to_send.bit_length() - 1 - 1), 0
    while layer > 0:
        for j in range(npar):
            tree.extend(r[j][start : start + layer])
        start += layer
        layer >>= 1
    total = num_to_send * npar
    for i in range(total - npar, total - 1):
        a, b = sub_index(i)
        tree.append(tree[a] * tree[b] % R_MOD)
    tree.append(0)
    return subtree, _ints_to_fr(tree)


def merge(results: Sequence[np.ndarray]) -> np.ndarray:
    """dacc_product.rs:416-428: interleave per-party vectors level by level ([k,4] each)"""
    n = len(results[0])
    num = 1
    while num < n + 1:
        num <<= 1
    num >>= 1
    parts, start = [], 0
    while num > 0 and start + num <= n:  # num == 0 would spin forever in the reference (len = 2^k - 1)
        for r in results:
            parts.append(r[start : start + num])
        start += num
        num >>= 1
    return np.concatenate(parts) if parts else np.zeros((0, 4), dtype=np.uint64)


def _pack_chunks(be, vals: np.ndarray, pp: PackedSharingParams) -> List[np.ndarray]:
    """
    `vals.chunks(l).map(pack_from_public)` transposed: out[p] = party p's share of every chunk (host arrays; the small
    leader-tree payloads).  A short last chunk is zero-padded exactly as pack_from_public pads.
    """
    vals = np.asarray(vals, dtype=np.uint64).reshape(-1, 4)
    if len(vals) == 0:
        return [np.zeros((0, 4), dtype=np.uint64) for _ in range(pp.n)]
    k = (len(vals) + pp.l - 1) // pp.l
    out = _pack_chunks_device(be, be.to_device(vals), len(vals), pp).download((pp.n * k, 4))  # out[p*k + j]
    return [np.ascontiguousarray(out[p * k : (p + 1) * k]) for p in range(pp.n)]


def _pack_chunks_device(be, d_vals, count: int, pp: PackedSharingParams):
    """
    the same on a device buffer of `count` Fr -> device buffer [n][k] (party-major: the send buffer of an all-to-all),
    k = ceil(count / l).  One application of the n x l public pack matrix (or its transform form) to all chunks.
    """
    l = pp.l
    k = (count + l - 1) // l
    if count != k * l:  # zero-extend the last chunk
        padded = be.alloc(32 * k * l)
        be.copy_d2d(padded, d_vals, 32 * count)
        be.upload_ptr(_at(padded, 32 * count), np.zeros((k * l - count, 4), dtype=np.uint64))
        d_vals = padded
    if pp.n >= NTT_FROM_N and hasattr(be, "fr_ntt_map"):
        return be.fr_ntt_map(pp.ntt_tables("pack"), d_vals, l, 1, k, 1, k)
    return be.fr_apply_matrix(_mont_matrix([row[:l] for row in pp.pack_matrix]), d_vals, l, 1, k, 1, k)


def _merge_device(be, d_in, k: int, nparties: int):
    """`merge` (dacc_product.rs:416-428) on a device buffer [n][k] (what every party sent me): level by level, the parties'
    pieces side by side.  A handful of device-to-device copies per level -> (buffer, merged length)"""
    num = 1
    while num < k + 1:
        num <<= 1
    num >>= 1
    out = be.alloc(32 * max(k * nparties, 1))
    start, pos = 0, 0
    while num > 0 and start + num <= k:
        for q in range(nparties):
            be.copy_d2d(_at(out, 32 * pos), _at(d_in, 32 * (q * k + start)), 32 * num)
            pos += num
        start += num
        num >>= 1
    return out, pos


def c_acc_product_and_share(be, shares, masks, unmask0, unmask1, unmask2, S: int, pp: PackedSharingParams, net: Net):
    """
    dacc_product.rs:66-292 -> three (device buffer, length) pairs: the shares of v(x,0), v(x,1), v(1,x), un-reduced exactly
    as the reference returns them (its three trailing degree_reduce_many calls discard their results).
    DEVICE-RESIDENT: mask -> all-to-all of the masked blocks -> unpack2 of every column -> product tree -> strided views ->
    pack_from_public of every l-chunk -> all-to-all of the share vectors -> merge -> unmask, with no table leaving HBM
    (over RcclNet the two all-to-alls are zk_alltoall on HBM buffers; the thread / gloo / echo nets of the tests stage the
    exchange itself through the host, the compute chain is the same).  Only the N_p-sized tails of the trees (the
    leader's top tree, :213-263) travel as host arrays.
    """
    N = pp.n
    assert S > N  # :82
    bs = S // N
    fr = 32
    masked = be.fr_mul(shares, masks, S)  # :88-92
    # every party receives everyone's i-th block (:94-104) ...
    recv = net.all_to_all_device(masked, bs * fr, be=be, echo="slot0")  # [N][bs], party-major
    # ... and unpack2s it element-wise: transpose(.).flat_map(unpack2) -> mx[j * l + r]   (unpack.rs:55-70)
    if pp.n >= NTT_FROM_N and hasattr(be, "fr_ntt_map"):
        mx = be.fr_ntt_map(pp.ntt_tables("unpack2"), recv, 1, bs, bs, pp.l, 1)
    else:
        mx = be.fr_apply_matrix(_mont_matrix(pp.unpack2_matrix), recv, 1, bs, bs, pp.l, 1)
    mlen = bs * pp.l
    subtree, leader_tree = c_acc_product(be, mx, mlen, pp, net)
    num_to_send = min(N, 2 * mlen)
    # to_share = subtree[.. 2 mlen - num_to_send]; its three views (:118-150) as device buffers
    half = (2 * mlen - num_to_send) // 2
    vx0, vx1 = be.fr_deinterleave(subtree, half)  # to_share[0::2], to_share[1::2]
    # v(x,0), v(x,1), v(1,x) = to_share[mlen..]: `.skip(subtree.len() / 2)` past the end of to_share yields nothing (:146-150) -- tables
    # with S l / N_p <= N_p leave v(1,x) entirely to the leader tree (the reference's `transpose` then asserts on the empty matrix,
    # operator.rs:24; here the view is simply empty)
    views = ((vx0, half), (vx1, half), (_at(subtree, fr * min(mlen, 2 * mlen - num_to_send)), max(0, mlen - num_to_send)))
    outs = []
    for d_sel, cnt in views:
        k = (cnt + pp.l - 1) // pp.l
        mine = _pack_chunks_device(be, d_sel, cnt, pp)  # [N][k]: party q's share of every chunk
        got = net.all_to_all_device(mine, k * fr, be=be, echo="identity")  # (:155-203)
        outs.append(_merge_device(be, got, k, N))
    # leader-tree shares (:213-263): note the v(1,x) share packs the WHOLE leader tree (:243-250).  N_p-sized: host arrays
    if net.is_leader:
        lt = np.asarray(leader_tree, dtype=np.uint64).reshape(-1, 4)
        rows = [_pack_chunks(be, np.ascontiguousarray(v), pp) for v in (lt[0::2], lt[1::2], lt)]
        payload = [np.concatenate([rows[0][p], rows[1][p], rows[2][p]]) for p in range(N)]
        k0, k1 = len(rows[0][0]), len(rows[1][0])
    else:
        ltlen = num_to_send * N
        k0 = k1 = (ltlen // 2 + pp.l - 1) // pp.l
        k2 = (ltlen + pp.l - 1) // pp.l
        payload = [np.zeros((k0 + k1 + k2, 4), dtype=np.uint64) for _ in range(N)]
    mine = net.all_to_all(payload, echo="identity")[0]  # what the leader (party 0) sent to me
    lead = (mine[:k0], mine[k0 : k0 + k1], mine[k0 + k1 :])
    res = []
    for (sh, shlen), le, um in zip(outs, lead, (unmask0, unmask1, unmask2)):
        k = shlen + len(le)
        full = be.alloc(fr * max(k, 1))
        be.copy_d2d(full, sh, fr * shlen)
        be.upload_ptr(_at(full, fr * shlen), np.ascontiguousarray(le))
        res.append((be.fr_mul(full, um, k), k))  # unmask (:266-275)
    for buf, k in res:  # :278-285 -- communication only; the results are dropped by the reference too
        degree_reduce_many_device(be, buf, k // N * 2, pp, net)
    return tuple(res)


def degree_reduce_many_device(be, d_shares, k: int, pp: PackedSharingParams, net: Net):
    """degree_reduce_many (degree_reduce.rs:10-26) on a device vector of k shares: HBM all-gather + this party's row of
    the public map pack o unpack2 -> device buffer of k Fr"""
    if k == 0:
        return be.alloc(32)
    allp = net.all_gather_device(d_shares, 32 * k, be=be)  # [n][k]
    p = net.party_id
    row = [sum(pp.pack_matrix[p][j] * pp.unpack2_matrix[j][i] for j in range(pp.l)) % R_MOD for i in range(pp.n)]
    return be.fr_apply_matrix(_mont_matrix([row]), allp, 1, k, k, 1, k)
