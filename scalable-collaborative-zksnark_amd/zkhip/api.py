"""
Thin object wrapper over the C ABI: `Ctx` = one GPU (zk_ctx), `DeviceBuffer`, `Srs`.
Arguments that name device memory accept a DeviceBuffer, a torch CUDA tensor (data_ptr) or a
raw integer address.  Host-side results come back as numpy uint64 limb arrays.
"""
from __future__ import annotations

import ctypes
import os
from typing import Tuple

import numpy as np

from . import _lib
from ._lib import ZK_ERR_DIV_ZERO, ZK_ERR_INVALID, ZK_ERR_LENGTH, test_hooks


_TRACE_MSM = bool(os.environ.get("ZKHIP_TRACE_MSM"))


class ZkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"zkhip error {code}: {msg}")
        self.code = code


class MsmLengthError(ZkError):
    """`G::msm` -> Err(min_len) (ark-ec 0.4.2), which dmsm.rs:23 unwrap()s"""

    def __init__(self, code, msg, min_len):
        super().__init__(code, msg)
        self.min_len = min_len


def _ptr(x) -> int:
    if x is None:
        return 0
    if isinstance(x, (DeviceBuffer, DeviceView)):
        return x.ptr
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):  # torch tensor
        return int(x.data_ptr())
    raise TypeError(f"not a device buffer: {type(x)}")


def _h(a: np.ndarray) -> int:
    return a.ctypes.data


class DeviceBuffer:
    def __init__(self, ctx: "Ctx", nbytes: int):
        self.ctx = ctx
        self.nbytes = nbytes
        p = ctypes.c_void_p()
        ctx._check(ctx.lib.zk_malloc(ctx.h, nbytes, ctypes.byref(p)))
        self.ptr = p.value or 0

    def free(self):
        if self.ptr:
            self.ctx.lib.zk_free(self.ctx.h, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.zk_memcpy_h2d(self.ctx.h, self.ptr + offset, _h(a), a.nbytes))
        return self

    def download(self, shape, dtype=np.uint64, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        self.ctx._check(self.ctx.lib.zk_memcpy_d2h(self.ctx.h, _h(out), self.ptr + offset, out.nbytes))
        return out

    def at(self, byte_offset: int) -> "DeviceView":
        """a view of this buffer from byte_offset on.  The view REFERENCES its parent: whoever holds the view (a queued MSM
        item, a traced sumcheck operand) keeps the allocation alive, so its address cannot be handed to another buffer."""
        return DeviceView(self, byte_offset)


class DeviceView:
    """an address inside a DeviceBuffer that keeps the buffer alive; accepted wherever a device buffer is"""

    __slots__ = ("parent", "offset", "ptr")

    def __init__(self, parent: DeviceBuffer, byte_offset: int):
        assert 0 <= byte_offset <= parent.nbytes, "view outside its buffer"
        self.parent, self.offset, self.ptr = parent, byte_offset, parent.ptr + byte_offset

    @property
    def ctx(self):
        return self.parent.ctx

    @property
    def nbytes(self) -> int:
        return self.parent.nbytes - self.offset

    def at(self, byte_offset: int) -> "DeviceView":
        return DeviceView(self.parent, self.offset + byte_offset)

    def download(self, shape, dtype=np.uint64, offset: int = 0) -> np.ndarray:
        return self.parent.download(shape, dtype, self.offset + offset)

    def upload(self, a: np.ndarray, offset: int = 0):
        self.parent.upload(a, self.offset + offset)
        return self

    def __int__(self) -> int:
        return self.ptr


class Srs:
    def __init__(self, ctx: "Ctx", handle: int):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        return self.ctx.lib.zk_srs_len(self.h)

    @property
    def device_ptr(self) -> int:
        return self.ctx.lib.zk_srs_device_ptr(self.h) or 0

    def precompute(self, window_bits: int = 0, record_bytes: int = 0):
        """build the per-window tables (setup): MSMs on this SRS then share one bucket set.  record_bytes (G1): 96 packed (the default),
        128 = one record per 128-byte line (faster gathers, 4/3 of the table memory)"""
        if record_bytes:
            self.ctx._check(self.ctx.lib.zk_srs_precompute_layout(self.ctx.h, self.h, window_bits, record_bytes))
        else:
            self.ctx._check(self.ctx.lib.zk_srs_precompute(self.ctx.h, self.h, window_bits))
        return self

    @property
    def table_record(self) -> int:
        """bytes per record of the precomputed table, 0 if none"""
        return self.ctx.lib.zk_srs_table_record(self.h)

    @property
    def table_window(self) -> int:
        """window bits of the precomputed table, 0 if none"""
        return self.ctx.lib.zk_srs_table_window(self.h)

    def download(self) -> np.ndarray:
        n = len(self)
        out = np.empty((n, 24 if getattr(self, "g2", False) else 12), dtype=np.uint64)
        if n:
            self.ctx._check(self.ctx.lib.zk_srs_download(self.ctx.h, self.h, _h(out)))
        return out

    def free(self):
        if self.h:
            self.ctx.lib.zk_srs_free(self.ctx.h, self.h)
            self.h = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PcsVk:
    """zk_pcs_vk: g1 and powers_of_g2 of a PolynomialCommitment, held by the library for zk_pcs_verify_batch"""

    def __init__(self, ctx: "Ctx", powers_g2, g1_96=None, g2_stride: int = 192):
        self.ctx, self.h = ctx, 0
        pg2 = np.ascontiguousarray(powers_g2)
        n = pg2.nbytes // g2_stride
        g1 = None if g1_96 is None else np.ascontiguousarray(g1_96, dtype=np.uint64).reshape(12)
        h = ctypes.c_void_p()
        ctx._check(ctx.lib.zk_pcs_vk_create(ctx.h, _h(g1) if g1 is not None else None, _h(pg2), g2_stride, n, ctypes.byref(h)))
        self.h, self.n_g2 = h.value, n

    def free(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.zk_pcs_vk_free(self.ctx.h, self.h)
        self.h = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class WitnessPlan:
    """zk_witness_plan: the witness plan of one Plonk circuit (sources, levels, launch schedule and, built with qk and ts, the key table
    of its lookup), held by the library"""

    def __init__(self, ctx: "Ctx", sigma, N: int, out_sel=None, qk=None, ts=None, advice=None):
        self.ctx, self.h, self.N = ctx, 0, int(N)
        sg = np.ascontiguousarray(sigma, dtype=np.uint64).reshape(-1)
        if len(sg) != 3 * self.N:
            raise ValueError(f"sigma must hold {3 * self.N} slot numbers")
        if (qk is None) != (ts is None) or (ts is not None and len(ts) != 3):
            raise ValueError("a lookup plan needs qk and the three table columns")
        h = ctypes.c_void_p()
        if advice is not None:
            adv = np.ascontiguousarray(advice, dtype=np.uint32).reshape(-1)
            if len(adv) != self.N:
                raise ValueError(f"advice must hold {self.N} codes")
            rc = ctx.lib.zk_witness_plan_create_advice(ctx.h, _h(sg), _ptr(out_sel), _ptr(qk), ctx._ptr_array(ts) if ts is not None else None, _h(adv), self.N, ctypes.byref(h))
        elif qk is None:
            rc = ctx.lib.zk_witness_plan_create(ctx.h, _h(sg), _ptr(out_sel), self.N, ctypes.byref(h))
        else:
            rc = ctx.lib.zk_witness_plan_create_lookup(ctx.h, _h(sg), _ptr(out_sel), _ptr(qk), ctx._ptr_array(ts), self.N, ctypes.byref(h))
        if rc == ZK_ERR_INVALID:
            raise ValueError((ctx.lib.zk_last_error(ctx.h) or b"").decode())
        ctx._check(rc)
        self.h, self.wide, self.lookup = h.value, out_sel is not None, qk is not None

    def info(self) -> dict:
        """{"levels", "max_level_rows", "launches"} (zk_witness_plan_info)"""
        v = [ctypes.c_size_t(0) for _ in range(3)]
        self.ctx._check(self.ctx.lib.zk_witness_plan_info(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("levels", "max_level_rows", "launches"), (int(x.value) for x in v)))

    def free(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.zk_witness_plan_free(self.h)
        self.h = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def comm_init_all(ctxs) -> None:
    """zk_comm_init_all: one process holding a ctx per GPU (the reference's one-task-per-party model,
    mpc-net/src/multi.rs:330-352); ctxs[p] becomes party p.  Drive every party from its own thread afterwards."""
    lib = _lib.lib()
    arr = (ctypes.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    rc = lib.zk_comm_init_all(arr, len(ctxs))
    if rc != 0:
        raise ZkError(rc, (lib.zk_last_error(ctxs[0].h) or b"").decode() if ctxs else "zk_comm_init_all")


class MsmJob:
    """an asynchronous batch of MSMs in flight (zk_msm_g1_batch_async / zk_msm_wait)"""

    def __init__(self, ctx: "Ctx", srs_list, scalars_list, lens, offsets=None):
        self.ctx, self.count = ctx, len(lens)
        self.keep = (list(srs_list), list(scalars_list))  # inputs must outlive the job
        self.lens = [int(x) for x in lens]
        self.h = None
        self.res = None
        if self.count == 0:
            self.res = np.zeros((0, 18), dtype=np.uint64)
            return
        count = self.count
        h = (ctypes.c_void_p * count)(*[s.h for s in srs_list])
        sp = (ctypes.c_void_p * count)(*[_ptr(s) for s in scalars_list])
        nn = (ctypes.c_size_t * count)(*self.lens)
        off = (ctypes.c_size_t * count)(*[int(x) for x in (offsets or [0] * count)])
        job = ctypes.c_void_p()
        rc = ctx.lib.zk_msm_g1_batch_async(ctx.h, count, h, off, sp, nn, ctypes.byref(job))
        if rc == ZK_ERR_LENGTH:
            raise MsmLengthError(rc, (ctx.lib.zk_last_error(ctx.h) or b"").decode(), 0)
        ctx._check(rc)
        self.h = job.value

    def wait(self) -> np.ndarray:
        if self.res is None:
            out = np.zeros((self.count, 18), dtype=np.uint64)
            h, self.h = self.h, None
            self.ctx._check(self.ctx.lib.zk_msm_wait(self.ctx.h, h, _h(out)))
            self.res, self.keep = out, None
        return self.res

    def __del__(self):
        try:
            if self.h and getattr(self.ctx, "h", None):  # never waited for: drain and release it
                out = np.zeros((self.count, 18), dtype=np.uint64)
                self.ctx.lib.zk_msm_wait(self.ctx.h, self.h, _h(out))
                self.h = None
        except Exception:
            pass


class Ctx:
    def __init__(self, device: int = 0):
        self.lib = _lib.lib()
        h = ctypes.c_void_p()
        rc = self.lib.zk_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise ZkError(rc, "zk_ctx_create failed (no MI355X visible?) -- zkhip has no CPU fallback")
        self.h = h.value
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.zk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise ZkError(rc, (self.lib.zk_last_error(self.h) or b"").decode())

    def set_stream(self, hip_stream: int):
        self._check(self.lib.zk_ctx_set_stream(self.h, hip_stream))

    def sync(self):
        self._check(self.lib.zk_ctx_sync(self.h))

    # ---- memory ----
    def mem_info(self):
        """(free, total) bytes of this ctx's GPU"""
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._check(self.lib.zk_mem_info(self.h, ctypes.byref(f), ctypes.byref(t)))
        return f.value, t.value

    def arena_plan_export(self) -> np.ndarray:
        """the sizes this ctx's scratch arenas have grown to (zk_arena_plan_export): 48 u64 -- keep them beside the proving key"""
        plan = np.zeros(48, dtype=np.uint64)
        self._check(self.lib.zk_arena_plan_export(self.h, _h(plan)))
        return plan

    def arena_plan_import(self, plan):
        """grow the arenas to a plan exported after an earlier proof of the same shape: the first proof then allocates nothing"""
        plan = np.ascontiguousarray(plan, dtype=np.uint64).reshape(-1)
        assert plan.size == 48
        self._check(self.lib.zk_arena_plan_import(self.h, _h(plan)))

    def trim(self) -> int:
        """hand every parked zk_free block back to the driver; returns the bytes released"""
        f = ctypes.c_size_t(0)
        self._check(self.lib.zk_trim(self.h, ctypes.byref(f)))
        return f.value

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def temp(self, nbytes: int, key) -> DeviceBuffer:
        """a cached device buffer of at least nbytes for `key` (avoids hipMalloc/hipFree per call)"""
        cache = self.__dict__.setdefault("_temps", {})
        buf = cache.get(key)
        if buf is None or buf.nbytes < nbytes:
            buf = cache[key] = DeviceBuffer(self, max(nbytes, 1))
        return buf

    def fr_scale(self, b, alpha: np.ndarray, n: int, out=None):
        """out = alpha * b (element-wise, one public scalar)"""
        out = out or self.alloc(max(32 * n, 1))
        al = np.ascontiguousarray(alpha, dtype=np.uint64)
        zero = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.zk_fr_axpb(self.h, 0, _ptr(b), _h(al), _h(zero), _ptr(out), n))
        return out

    def copy_d2d(self, dst, src, nbytes: int):
        self._check(self.lib.zk_memcpy_d2d(self.h, _ptr(dst), _ptr(src), nbytes))

    def download_ptr(self, src, nbytes: int) -> np.ndarray:
        """nbytes from a device buffer / raw device address -> uint8 array"""
        out = np.empty(nbytes, dtype=np.uint8)
        if nbytes:
            self._check(self.lib.zk_memcpy_d2h(self.h, _h(out), _ptr(src), nbytes))
        return out

    def upload_ptr(self, dst, a: np.ndarray):
        a = np.ascontiguousarray(a)
        if a.nbytes:
            self._check(self.lib.zk_memcpy_h2d(self.h, _ptr(dst), _h(a), a.nbytes))

    def to_device(self, a: np.ndarray) -> DeviceBuffer:
        a = np.ascontiguousarray(a)
        return DeviceBuffer(self, max(a.nbytes, 1)).upload(a) if a.nbytes else DeviceBuffer(self, 1)

    # ---- element-wise ----
    def _binary(self, fn, a, b, n, out=None) -> DeviceBuffer:
        out = out or self.alloc(max(32 * n, 1))
        self._check(fn(self.h, _ptr(a), _ptr(b), _ptr(out), n))
        return out

    def fr_add(self, a, b, n, out=None):
        return self._binary(self.lib.zk_fr_add, a, b, n, out)

    def fr_sub(self, a, b, n, out=None):
        return self._binary(self.lib.zk_fr_sub, a, b, n, out)

    def fr_mul(self, a, b, n, out=None):
        return self._binary(self.lib.zk_fr_mul, a, b, n, out)

    def fr_apply_matrix(self, matrix: np.ndarray, d_in, in_vec_stride: int, in_comp_stride: int, k: int, out_vec_stride: int, out_row_stride: int, out=None):
        """out[j*osv + r*osr] = sum_c M[r][c] * in[j*isv + c*isc]; matrix [rows, cols, 4] Montgomery limbs"""
        m = np.ascontiguousarray(matrix, dtype=np.uint64)
        rows, cols = m.shape[0], m.shape[1]
        span = (k - 1) * out_vec_stride + (rows - 1) * out_row_stride + 1 if k and rows else 1
        out = out or self.alloc(32 * span)
        self._check(self.lib.zk_fr_apply_matrix(self.h, _h(m), rows, cols, _ptr(d_in), in_vec_stride, in_comp_stride, _ptr(out), out_vec_stride, out_row_stride, k))
        return out

    def fr_ntt_map(self, tables: dict, d_in, in_vec_stride: int, in_comp_stride: int, k: int, out_vec_stride: int, out_row_stride: int, out=None):
        """a PSS map by transforms (zk_fr_ntt_map); tables = PackedSharingParams.ntt_tables(kind)"""
        t = tables
        span = (k - 1) * out_vec_stride + (t["take"] - 1) * out_row_stride + 1 if k else 1
        out = out or self.alloc(32 * span)
        self._check(self.lib.zk_fr_ntt_map(self.h, t["A"], _h(t["winv"]), t["B"], _h(t["w"]), _h(t["scale"]), t["n_in"], t["take"], t["step"],
                                           _ptr(d_in), in_vec_stride, in_comp_stride, _ptr(out), out_vec_stride, out_row_stride, k))
        return out

    def fr_deinterleave(self, t, n):
        """(t[0::2], t[1::2]) for a table of 2n Fr -> two device buffers of n Fr"""
        even, odd = self.alloc(max(32 * n, 1)), self.alloc(max(32 * n, 1))
        self._check(self.lib.zk_fr_deinterleave(self.h, _ptr(t), _ptr(even), _ptr(odd), n))
        return even, odd

    def fr_batch_div(self, num, den, n, out=None):
        out = out or self.alloc(max(32 * n, 1))
        rc = self.lib.zk_fr_batch_div(self.h, _ptr(num), _ptr(den), _ptr(out), n)
        if rc == ZK_ERR_DIV_ZERO:
            raise ZeroDivisionError("zero denominator (the reference panics on inverse().unwrap())")
        self._check(rc)
        return out

    def fr_axpb(self, a, b, alpha: np.ndarray, beta: np.ndarray, n, out=None):
        out = out or self.alloc(max(32 * n, 1))
        al, be = np.ascontiguousarray(alpha, dtype=np.uint64), np.ascontiguousarray(beta, dtype=np.uint64)
        self._check(self.lib.zk_fr_axpb(self.h, _ptr(a), _ptr(b), _h(al), _h(be), _ptr(out), n))
        return out

    # ---- sumcheck family ----
    def sumcheck(self, tab, length: int, chal: np.ndarray):
        """-> (pairs [n,2,4], last [4])"""
        n = length.bit_length() - 1
        chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((n, 2, 4), dtype=np.uint64)
        last = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.zk_sumcheck(self.h, _ptr(tab), length, _h(chal), _h(out), _h(last)))
        return out, last

    def sumcheck_product(self, f, g, length: int, chal: np.ndarray):
        """-> (triples [n,3,4], last_f [4], last_g [4])"""
        n = length.bit_length() - 1
        chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((n, 3, 4), dtype=np.uint64)
        lf = np.zeros(4, dtype=np.uint64)
        lg = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.zk_sumcheck_product(self.h, _ptr(f), _ptr(g), length, _h(chal), _h(out), _h(lf), _h(lg)))
        return out, lf, lg

    def sumcheck_batch(self, reqs):
        """
        several INDEPENDENT calls of the family in one C-ABI call (zk_sumcheck_batch): one enqueue over several streams, one
        completion.  reqs: list of
            ("plain", tab, length, chal) | ("product", f, g, length, chal) | ("fold", tab, length, points[, out]) | ("open", tab, length, point[, q_out])
        -> list of what the single calls return: (pairs, last) | (triples, last_f, last_g) | folded buffer | (q buffer, value).
        """
        from ._lib import ScItem

        n = len(reqs)
        if n == 0:
            return []
        items = (ScItem * n)()
        keep, outs = [], []
        for i, r in enumerate(reqs):
            kind = r[0]
            it = items[i]
            if kind == "product":
                _, f, g, length, chal = r
                k = length.bit_length() - 1
                ch = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)[:k]
                tr, lf, lg = np.zeros((k, 3, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
                it.mode, it.d_f, it.d_g, it.len, it.h_chal, it.h_sums, it.h_last_f, it.h_last_g = 1, _ptr(f), _ptr(g), length, _h(ch), _h(tr), _h(lf), _h(lg)
                outs.append((tr, lf, lg))
            elif kind == "plain":
                _, f, length, chal = r
                k = length.bit_length() - 1
                ch = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)[:k]
                pr, last = np.zeros((k, 2, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
                it.mode, it.d_f, it.len, it.h_chal, it.h_sums, it.h_last_f = 0, _ptr(f), length, _h(ch), _h(pr), _h(last)
                outs.append((pr, last))
            elif kind == "fold":
                _, f, length, points = r[:4]
                k = length.bit_length() - 1
                ch = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
                out = (r[4] if len(r) > 4 else None) or self.alloc(32 * (length >> min(k, len(ch))))
                it.mode, it.d_f, it.len, it.h_chal, it.n_points, it.d_out = 2, _ptr(f), length, _h(ch), len(ch), _ptr(out)
                outs.append(out)
            elif kind == "open":
                _, f, length, point = r[:4]
                k = length.bit_length() - 1
                ch = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)[:k]
                q = (r[4] if len(r) > 4 else None) or self.alloc(max(32 * (length - 1), 1))
                val = np.zeros(4, dtype=np.uint64)
                it.mode, it.d_f, it.len, it.h_chal, it.h_last_f, it.d_out = 3, _ptr(f), length, _h(ch), _h(val), _ptr(q)
                outs.append((q, val))
            else:
                raise ValueError(kind)
            keep.append(ch)
        self._check(self.lib.zk_sumcheck_batch(self.h, n, items))
        return outs

    def fold(self, tab, length: int, points: np.ndarray, out=None):
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        n = length.bit_length() - 1
        rounds = min(n, len(points))
        out = out or self.alloc(32 * (length >> rounds))
        self._check(self.lib.zk_fold(self.h, _ptr(tab), length, _h(points), len(points), _ptr(out)))
        return out

    def eq_table(self, point: np.ndarray, out=None):
        """eq(point, x) over the cube, x_0 the top index bit -> device buffer of 2^n Fr (zk_eq_table)"""
        point = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        out = out or self.alloc(32 << len(point))
        self._check(self.lib.zk_eq_table(self.h, _h(point), len(point), _ptr(out)))
        return out

    # the six fused identities: ABI name -> (tables folded out into `last`, evaluations per round, a gamma is passed)
    _FUSED = {"gate": (7, 5, False), "wiring": (7, 4, True), "perm3": (11, 6, True), "gate_wide": (11, 8, False), "lookup": (6, 4, True), "lookup_sel": (7, 4, True)}

    def _fused(self, name: str, fs: bool, ptrs: tuple, length: int, gamma, drive):
        """What the twelve fused sumchecks share.  name: a key of _FUSED; ptrs: the pointer arguments of the C call, laid out by the caller
        (who has checked how many tables it was given); drive: the preset challenges (zk_sumcheck_<name>) or, with fs, the transcript they are drawn from
        (zk_sumcheck_<name>_fs).  -> (evals [n, evals, 4], last [tabs, 4]) and, with fs, chal [n, 4]"""
        tabs, evals, has_gamma = self._FUSED[name]
        n = max(length.bit_length() - 1, 0)
        out, last = np.zeros((n, evals, 4), dtype=np.uint64), np.zeros((tabs, 4), dtype=np.uint64)
        gamma = np.ascontiguousarray(gamma, dtype=np.uint64).reshape(4) if has_gamma else None  # a local: it must outlive the call
        args = (self.h, *ptrs, length) + ((_h(gamma),) if has_gamma else ())
        if fs:
            drawn = np.zeros((n, 4), dtype=np.uint64)
            self._check(getattr(self.lib, f"zk_sumcheck_{name}_fs")(*args, self._tr(drive), _h(out), _h(last), _h(drawn)))
            return out, last, drawn
        chal = np.ascontiguousarray(drive, dtype=np.uint64).reshape(-1, 4)
        if len(chal) < n:
            raise ValueError(f"{n} challenges needed, {len(chal)} given")
        self._check(getattr(self.lib, f"zk_sumcheck_{name}")(*args, _h(chal), _h(out), _h(last)))
        return out, last

    def _check_rows(self, rc: int) -> None:
        """_check for the calls that look at the caller's rows: their ZK_ERR_INVALID is a ValueError with the library's message"""
        if rc == ZK_ERR_INVALID:
            raise ValueError((self.lib.zk_last_error(self.h) or b"").decode())
        self._check(rc)

    def sumcheck_gate(self, eq, q1, q2, a, b, c, inp, length: int, chal: np.ndarray):
        """the gate identity eq [q1 (a + b) + q2 a b - c + in] as one degree-4 sumcheck -> (evals [n,5,4], last [7,4])"""
        return self._fused("gate", False, tuple(_ptr(t) for t in (eq, q1, q2, a, b, c, inp)), length, None, chal)

    def sumcheck_wiring(self, eq, tree, num, den, N: int, gamma: np.ndarray, chal: np.ndarray):
        """the wiring identity eq [v(1,x) - v(x,0) v(x,1) + gamma (den h - num)] on the product tree of h (2N Fr, read in place) as one
        degree-3 sumcheck -> (evals [mu,4,4], last [7,4]: eq, v1x, vx0, vx1, h, num, den)"""
        return self._fused("wiring", False, (_ptr(eq), _ptr(tree), _ptr(num), _ptr(den)), N, gamma, chal)

    @staticmethod
    def _ptr_array(bufs):
        arr = (ctypes.c_void_p * len(bufs))()
        for i, b in enumerate(bufs):
            arr[i] = _ptr(b)
        return arr

    def perm3_terms(self, ws, ssigmas, N: int, alpha: np.ndarray, beta: np.ndarray):
        """the derived tables of the three-column wiring identity in one pass (zk_perm3_terms; asynchronous): ws, ssigmas three device
        buffers of N Fr each -> (nums [3], dens [3], P = n_0 n_1 n_2, Q = d_0 d_1 d_2), device buffers of N Fr"""
        if len(ws) != 3 or len(ssigmas) != 3:
            raise ValueError("three wire columns and three permutation columns are needed")
        al, be = np.ascontiguousarray(alpha, dtype=np.uint64).reshape(4), np.ascontiguousarray(beta, dtype=np.uint64).reshape(4)
        nums, dens = [self.alloc(max(32 * N, 1)) for _ in range(3)], [self.alloc(max(32 * N, 1)) for _ in range(3)]
        P, Q = self.alloc(max(32 * N, 1)), self.alloc(max(32 * N, 1))
        self._check(self.lib.zk_perm3_terms(self.h, self._ptr_array(ws), self._ptr_array(ssigmas), N, _h(al), _h(be), self._ptr_array(nums), self._ptr_array(dens),
                                            _ptr(P), _ptr(Q)))
        return nums, dens, P, Q

    def sumcheck_perm3(self, eq, tree, nums, dens, N: int, gamma: np.ndarray, chal: np.ndarray):
        """the three-column wiring identity eq [v(1,x) - v(x,0) v(x,1) + gamma (h d_0 d_1 d_2 - n_0 n_1 n_2)] on the product tree of h (2N Fr,
        read in place) as one degree-5 sumcheck -> (evals [mu,6,4], last [11,4]: eq, v1x, vx0, vx1, h, n_0..2, d_0..2)"""
        if len(nums) != 3 or len(dens) != 3:
            raise ValueError("three numerator and three denominator tables are needed")
        return self._fused("perm3", False, (_ptr(eq), _ptr(tree), self._ptr_array(nums), self._ptr_array(dens)), N, gamma, chal)

    def sumcheck_gate_wide(self, tabs, length: int, chal: np.ndarray):
        """the wide gate identity eq [qL a + qR b + qM a b + qH a^5 - qO c + qC + in] as one degree-7 sumcheck; tabs: the eleven device
        buffers eq, qL, qR, qM, qO, qC, qH, a, b, c, in of `length` Fr -> (evals [n,8,4], last [11,4] in that order)"""
        if len(tabs) != 11:
            raise ValueError("eleven tables are needed: eq, qL, qR, qM, qO, qC, qH, a, b, c, in")
        return self._fused("gate_wide", False, (self._ptr_array(tabs),), length, None, chal)

    def lookup_multiplicities(self, f, t, idx, N: int, out=None):
        """m[y] = #{x : idx[x] = y} as N Fr for the lookup argument (zk_lookup_multiplicities; blocking): f, t device buffers of N Fr, idx one
        of N u32 with f[x] = t[idx[x]].  An index out of range or a row whose value is not the table's entry: ValueError -- as is every other ZK_ERR_INVALID of the call
        (N < 2, not a power of two or > 2^32, a null pointer), with the library's message."""
        out = out or self.alloc(max(32 * N, 1))
        rc = self.lib.zk_lookup_multiplicities(self.h, _ptr(f), _ptr(t), _ptr(idx), N, _ptr(out))
        self._check_rows(rc)
        return out

    def sumcheck_lookup(self, tabs, length: int, gamma: np.ndarray, chal: np.ndarray):
        """the lookup identity hf - ht + E [hf df - 1 + gamma (ht dt - m)] as one degree-3 sumcheck; tabs: the six device buffers
        E, df, dt, m, hf, ht of `length` Fr -> (evals [n,4,4], last [6,4] in that order)"""
        if len(tabs) != 6:
            raise ValueError("six tables are needed: E, df, dt, m, hf, ht")
        return self._fused("lookup", False, (self._ptr_array(tabs),), length, gamma, chal)

    def lookup3_multiplicities(self, ws, ts, qk, idx, N: int, out=None):
        """m[y] = #{x : qk(x) = 1, idx[x] = y} as N Fr for the lookup of a Plonk circuit (zk_lookup3_multiplicities; blocking): ws = (a, b, c),
        ts = (t0, t1, t2), qk device buffers of N Fr, idx one of N u32.  A selected row whose index is out of range or whose triple is not the
        table's entry, or a qk that is neither 0 nor 1: ValueError -- as is every other ZK_ERR_INVALID of the call, with the library's message."""
        if len(ws) != 3 or len(ts) != 3:
            raise ValueError("three wire columns and three table columns are needed")
        out = out or self.alloc(max(32 * N, 1))
        rc = self.lib.zk_lookup3_multiplicities(self.h, self._ptr_array(ws), self._ptr_array(ts), _ptr(qk), _ptr(idx), N, _ptr(out))
        self._check_rows(rc)
        return out

    def lookup_find(self, f, t, N: int, idx=None, m=None):
        """the row-to-table indices found on the device (zk_lookup_find; blocking): f, t device buffers of N Fr -> (idx, m), device buffers
        of N u32 (idx[x] = the smallest y with t[y] = f[x]) and of N Fr (the multiplicities of that idx).  A row whose value is no entry of the
        table: ValueError -- as is every other ZK_ERR_INVALID of the call (N < 2, not a power of two or > 2^31), with the library's message."""
        idx, m = idx or self.alloc(max(4 * N, 1)), m or self.alloc(max(32 * N, 1))
        rc = self.lib.zk_lookup_find(self.h, _ptr(f), _ptr(t), N, _ptr(idx), _ptr(m))
        self._check_rows(rc)
        return idx, m

    def lookup3_find(self, ws, ts, qk, N: int, idx=None, m=None):
        """the same for the lookup of a Plonk circuit (zk_lookup3_find; blocking): ws = (a, b, c), ts = (t0, t1, t2), qk device buffers of N Fr
        -> (idx, m): idx[x] = the smallest y with (t0, t1, t2)[y] = (a, b, c)[x] where qk(x) = 1, 0 where qk(x) = 0.  A selected row whose triple
        is no entry of the table, or a qk that is neither 0 nor 1: ValueError, with the library's message."""
        if len(ws) != 3 or len(ts) != 3:
            raise ValueError("three wire columns and three table columns are needed")
        idx, m = idx or self.alloc(max(4 * N, 1)), m or self.alloc(max(32 * N, 1))
        rc = self.lib.zk_lookup3_find(self.h, self._ptr_array(ws), self._ptr_array(ts), _ptr(qk), N, _ptr(idx), _ptr(m))
        self._check_rows(rc)
        return idx, m

    def witness_plan(self, sigma, N: int, out_sel=None) -> WitnessPlan:
        """the witness plan of a circuit (zk_witness_plan_create; host work, once per circuit): sigma 3N slot numbers, out_sel the wide gate's
        qO as a device buffer of N fully reduced Fr (None: every row computes).  A sigma that is not a permutation, a qO at or above r, or
        rows that depend on their own output: ValueError with the library's message."""
        return WitnessPlan(self, sigma, N, out_sel)

    def witness_plan_lookup(self, sigma, N: int, out_sel, qk, ts) -> WitnessPlan:
        """the witness plan of a circuit with its lookup (zk_witness_plan_create_lookup; blocking: the key table of (t0, t1) is built on
        the device): qk and ts = (t0, t1, t2) device buffers of N Fr.  Beyond witness_plan's refusals: a qk entry that is neither 0 nor 1,
        a table that is no function of (t0, t1) -- ValueError with the library's message."""
        return WitnessPlan(self, sigma, N, out_sel, qk, ts)

    def witness_plan_advice(self, sigma, N: int, out_sel, advice, qk=None, ts=None) -> WitnessPlan:
        """the witness plan of a circuit with its advice codes (zk_witness_plan_create_advice): advice N u32 on the host (0: none,
        plonk.ADV_INV0, plonk.adv_bits(shift, width)); qk and ts as witness_plan_lookup takes them, or both None.  Beyond the refusals of
        those two: unknown codes, advice rows that also compute by the gate or the table -- ValueError with the library's message.
        plonk_witness / plonk_witness_check take the plan as they take the others (with qk and ts when it has a lookup)."""
        return WitnessPlan(self, sigma, N, out_sel, qk, ts, advice)

    def plonk_witness(self, plan: WitnessPlan, sels, public_inputs: np.ndarray, free=None, out=None, qk=None, ts=None):
        """a, b, c generated on the device (zk_plonk_witness; blocking): sels the gate's selectors (2: basic, 6: wide) as device buffers,
        public_inputs [l, 4], free a device buffer of 3N Fr or None -> (a, b, c), device buffers of N Fr.  A bad gate row or copy:
        ValueError with the library's message.  With qk and ts = (t0, t1, t2), the ones a lookup plan was built from:
        zk_plonk_witness_lookup (a bad lookup is refused in the same way)."""
        N = plan.N
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        a, b, c = out or tuple(self.alloc(32 * N) for _ in range(3))
        if qk is None and ts is None:
            rc = self.lib.zk_plonk_witness(self.h, plan.h, int(len(sels) == 6), self._ptr_array(sels), _h(pi), len(pi), _ptr(free), _ptr(a), _ptr(b), _ptr(c))
        else:
            rc = self.lib.zk_plonk_witness_lookup(self.h, plan.h, int(len(sels) == 6), self._ptr_array(sels), _ptr(qk), self._ptr_array(ts), _h(pi), len(pi), _ptr(free),
                                                  _ptr(a), _ptr(b), _ptr(c))
        self._check_rows(rc)
        return a, b, c

    def plonk_witness_check(self, plan: WitnessPlan, sels, public_inputs: np.ndarray, a, b, c, qk=None, ts=None) -> dict:
        """zk_plonk_witness_check (blocking) -> {"bad_rows", "first_bad_row", "bad_copies", "first_bad_copy"} (the firsts None when there is none).
        With qk and ts = (t0, t1, t2) of a lookup plan: zk_plonk_witness_check_lookup, and the dict gains "bad_lookups", "first_bad_lookup"."""
        pi = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
        lookup = not (qk is None and ts is None)
        bad = np.zeros(6 if lookup else 4, dtype=np.uint64)
        if lookup:
            rc = self.lib.zk_plonk_witness_check_lookup(self.h, plan.h, int(len(sels) == 6), self._ptr_array(sels), _ptr(qk), self._ptr_array(ts), _h(pi), len(pi), _ptr(a),
                                                        _ptr(b), _ptr(c), _h(bad))
        else:
            rc = self.lib.zk_plonk_witness_check(self.h, plan.h, int(len(sels) == 6), self._ptr_array(sels), _h(pi), len(pi), _ptr(a), _ptr(b), _ptr(c), _h(bad))
        self._check_rows(rc)
        r, fr, k, fk = (int(x) for x in bad[:4])
        out = {"bad_rows": r, "first_bad_row": fr if r else None, "bad_copies": k, "first_bad_copy": fk if k else None}
        if lookup:
            out.update(bad_lookups=int(bad[4]), first_bad_lookup=int(bad[5]) if bad[4] else None)
        return out

    def lookup3_terms(self, ws, ts, N: int, zeta: np.ndarray, beta: np.ndarray):
        """df = beta + a + zeta b + zeta^2 c, dt = beta + t0 + zeta t1 + zeta^2 t2 in one pass (zk_lookup3_terms; asynchronous) -> (df, dt),
        device buffers of N Fr"""
        if len(ws) != 3 or len(ts) != 3:
            raise ValueError("three wire columns and three table columns are needed")
        ze, be = np.ascontiguousarray(zeta, dtype=np.uint64).reshape(4), np.ascontiguousarray(beta, dtype=np.uint64).reshape(4)
        df, dt = self.alloc(max(32 * N, 1)), self.alloc(max(32 * N, 1))
        self._check(self.lib.zk_lookup3_terms(self.h, self._ptr_array(ws), self._ptr_array(ts), N, _h(ze), _h(be), _ptr(df), _ptr(dt)))
        return df, dt

    def sumcheck_lookup_sel(self, tabs, length: int, gamma: np.ndarray, chal: np.ndarray):
        """the selector-gated lookup identity hf - ht + E [hf df - qk + gamma (ht dt - m)] as one degree-3 sumcheck; tabs: the seven device
        buffers E, df, dt, m, hf, ht, qk of `length` Fr -> (evals [n,4,4], last [7,4] in that order)"""
        if len(tabs) != 7:
            raise ValueError("seven tables are needed: E, df, dt, m, hf, ht, qk")
        return self._fused("lookup_sel", False, (self._ptr_array(tabs),), length, gamma, chal)

    def eq_table_acc(self, point: np.ndarray, weight: np.ndarray, acc):
        """acc[x] += weight * eq(point, x), acc a device buffer of 2^n Fr (zk_eq_table_acc; asynchronous) -> acc"""
        point = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        weight = np.ascontiguousarray(weight, dtype=np.uint64).reshape(4)
        self._check(self.lib.zk_eq_table_acc(self.h, _h(point), len(point), _h(weight), _ptr(acc)))
        return acc

    def fr_lincomb(self, tabs, coeffs: np.ndarray, length: int, out=None):
        """out[x] = sum_j coeffs[j] * tabs[j][x] over 1 .. 16 device buffers of `length` Fr (zk_fr_lincomb; asynchronous)"""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        if len(coeffs) != len(tabs):
            raise ValueError(f"{len(tabs)} tables, {len(coeffs)} coefficients")
        out = out or self.alloc(max(32 * length, 1))
        self._check(self.lib.zk_fr_lincomb(self.h, len(tabs), self._ptr_array(tabs), _h(coeffs), length, _ptr(out)))
        return out

    def sumcheck_multi(self, es, fs, length: int, chal: np.ndarray):
        """the rounds of sum_x sum_j es[j](x) fs[j](x) as one degree-2 sumcheck over 1 .. 16 pairs of device buffers of `length` Fr
        -> (triples [n,3,4], last_e [count,4], last_f [count,4])"""
        if len(es) != len(fs):
            raise ValueError(f"{len(es)} eq tables, {len(fs)} tables")
        n = max(length.bit_length() - 1, 0)
        chal = np.ascontiguousarray(chal, dtype=np.uint64).reshape(-1, 4)
        if len(chal) < n:
            raise ValueError(f"{n} challenges needed, {len(chal)} given")
        out = np.zeros((n, 3, 4), dtype=np.uint64)
        le, lf = np.zeros((len(es), 4), dtype=np.uint64), np.zeros((len(es), 4), dtype=np.uint64)
        self._check(self.lib.zk_sumcheck_multi(self.h, len(es), self._ptr_array(es), self._ptr_array(fs), length, _h(chal), _h(out), _h(le), _h(lf)))
        return out, le, lf

    # ---- the same sumchecks with their challenges drawn from a device transcript (zkhip.transcript.Transcript) ----
    @staticmethod
    def _tr(transcript) -> int:
        return getattr(transcript, "h", transcript) or 0

    def sumcheck_gate_fs(self, eq, q1, q2, a, b, c, inp, length: int, transcript):
        """sumcheck_gate with round i's challenge = hash of round i's evaluations -> (evals [n,5,4], last [7,4], chal [n,4])"""
        return self._fused("gate", True, tuple(_ptr(t) for t in (eq, q1, q2, a, b, c, inp)), length, None, transcript)

    def sumcheck_wiring_fs(self, eq, tree, num, den, N: int, gamma: np.ndarray, transcript):
        """sumcheck_wiring with derived challenges -> (evals [mu,4,4], last [7,4], chal [mu,4])"""
        return self._fused("wiring", True, (_ptr(eq), _ptr(tree), _ptr(num), _ptr(den)), N, gamma, transcript)

    def sumcheck_perm3_fs(self, eq, tree, nums, dens, N: int, gamma: np.ndarray, transcript):
        """sumcheck_perm3 with derived challenges -> (evals [mu,6,4], last [11,4], chal [mu,4])"""
        if len(nums) != 3 or len(dens) != 3:
            raise ValueError("three numerator and three denominator tables are needed")
        return self._fused("perm3", True, (_ptr(eq), _ptr(tree), self._ptr_array(nums), self._ptr_array(dens)), N, gamma, transcript)

    def sumcheck_gate_wide_fs(self, tabs, length: int, transcript):
        """sumcheck_gate_wide with derived challenges -> (evals [n,8,4], last [11,4], chal [n,4])"""
        if len(tabs) != 11:
            raise ValueError("eleven tables are needed: eq, qL, qR, qM, qO, qC, qH, a, b, c, in")
        return self._fused("gate_wide", True, (self._ptr_array(tabs),), length, None, transcript)

    def sumcheck_lookup_fs(self, tabs, length: int, gamma: np.ndarray, transcript):
        """sumcheck_lookup with derived challenges -> (evals [n,4,4], last [6,4], chal [n,4])"""
        if len(tabs) != 6:
            raise ValueError("six tables are needed: E, df, dt, m, hf, ht")
        return self._fused("lookup", True, (self._ptr_array(tabs),), length, gamma, transcript)

    def sumcheck_lookup_sel_fs(self, tabs, length: int, gamma: np.ndarray, transcript):
        """sumcheck_lookup_sel with derived challenges -> (evals [n,4,4], last [7,4], chal [n,4])"""
        if len(tabs) != 7:
            raise ValueError("seven tables are needed: E, df, dt, m, hf, ht, qk")
        return self._fused("lookup_sel", True, (self._ptr_array(tabs),), length, gamma, transcript)

    def sumcheck_multi_fs(self, es, fs, length: int, transcript):
        """sumcheck_multi with derived challenges -> (triples [n,3,4], last_e [count,4], last_f [count,4], chal [n,4])"""
        if len(es) != len(fs):
            raise ValueError(f"{len(es)} eq tables, {len(fs)} tables")
        n = max(length.bit_length() - 1, 0)
        out, chal = np.zeros((n, 3, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        le, lf = np.zeros((len(es), 4), dtype=np.uint64), np.zeros((len(es), 4), dtype=np.uint64)
        self._check(self.lib.zk_sumcheck_multi_fs(self.h, len(es), self._ptr_array(es), self._ptr_array(fs), length, self._tr(transcript), _h(out), _h(le), _h(lf),
                                                  _h(chal)))
        return out, le, lf, chal

    def open_rounds(self, tab, length: int, point: np.ndarray, q_out=None):
        """-> (q device buffer with length-1 Fr, value [4])"""
        point = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        q_out = q_out or self.alloc(max(32 * (length - 1), 1))
        val = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.zk_open_rounds(self.h, _ptr(tab), length, _h(point), _ptr(q_out), _h(val)))
        return q_out, val

    def product_tree(self, x, N: int, out=None):
        out = out or self.alloc(64 * N)
        self._check(self.lib.zk_product_tree(self.h, _ptr(x), N, _ptr(out)))
        return out

    # ---- MSM ----
    def srs_register(self, bases: np.ndarray, stride: int = 96) -> Srs:
        b = np.ascontiguousarray(bases)
        n = b.nbytes // stride
        h = ctypes.c_void_p()
        self._check(self.lib.zk_srs_register(self.h, _h(b), stride, n, ctypes.byref(h)))
        return Srs(self, h.value)

    def srs_wrap_device(self, d_bases, n: int) -> Srs:
        h = ctypes.c_void_p()
        self._check(self.lib.zk_srs_wrap_device(self.h, _ptr(d_bases), n, ctypes.byref(h)))
        return Srs(self, h.value)

    def srs_generate(self, k0: int, k1: int, n: int) -> Srs:
        from .field import int_to_limbs

        a, b = int_to_limbs(k0, 4), int_to_limbs(k1, 4)
        h = ctypes.c_void_p()
        self._check(self.lib.zk_srs_generate(self.h, _h(a), _h(b), n, ctypes.byref(h)))
        return Srs(self, h.value)

    def srs_powers(self, s: np.ndarray, g: np.ndarray = None):
        """PolynomialCommitmentCub::new (dpoly_comm.rs:37-67): s [n,4] Montgomery -> list of n+1 Srs levels"""
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
        n = len(s)
        handles = (ctypes.c_void_p * (n + 1))()
        gp = np.ascontiguousarray(g, dtype=np.uint64) if g is not None else None
        self._check(self.lib.zk_srs_powers(self.h, _h(gp) if gp is not None else 0, _h(s) if n else 0, n, handles))
        return [Srs(self, handles[k]) for k in range(n + 1)]

    def srs_to_packed(self, level: Srs, row_canon: np.ndarray, l: int) -> Srs:
        """to_packed (dpoly_comm.rs:164-194) for one party: row_canon [l,4] canonical pack coefficients"""
        row = np.ascontiguousarray(row_canon, dtype=np.uint64).reshape(-1, 4)
        assert len(row) >= min(l, len(level))
        h = ctypes.c_void_p()
        self._check(self.lib.zk_srs_to_packed(self.h, level.h, _h(row), l, ctypes.byref(h)))
        return Srs(self, h.value)

    def g1_apply_matrix(self, matrix_canon: np.ndarray, d_in, in_vec_stride: int, in_comp_stride: int, k: int, out_vec_stride: int, out_row_stride: int, out=None):
        """zk_fr_apply_matrix on affine G1 points (reference layout, 96 B): matrix [rows, cols, 4] CANONICAL scalars"""
        m = np.ascontiguousarray(matrix_canon, dtype=np.uint64)
        rows, cols = m.shape[0], m.shape[1]
        span = (k - 1) * out_vec_stride + (rows - 1) * out_row_stride + 1 if k and rows else 1
        out = out or self.alloc(96 * span)
        self._check(self.lib.zk_g1_apply_matrix(self.h, _h(m), rows, cols, _ptr(d_in), in_vec_stride, in_comp_stride, _ptr(out), out_vec_stride, out_row_stride, k))
        return out

    def msm_g1(self, srs: Srs, scalars, n: int, offset: int = 0) -> np.ndarray:
        """-> normalised Jacobian [18] uint64"""
        out = np.zeros(18, dtype=np.uint64)
        rc = self.lib.zk_msm_g1(self.h, srs.h, offset, _ptr(scalars), n, _h(out))
        if rc == ZK_ERR_LENGTH:
            raise MsmLengthError(rc, (self.lib.zk_last_error(self.h) or b"").decode(), min(n, max(len(srs) - offset, 0)))
        self._check(rc)
        if _TRACE_MSM:
            import sys

            print("zkhip-msm", [int(n)], [round(float(x), 3) for x in self.msm_last_timing()], file=sys.stderr)
        return out

    def msm_g1_batch(self, srs_list, scalars_list, lens, offsets=None) -> np.ndarray:
        """a batch of independent MSMs in one pipeline pass -> [count, 18]"""
        count = len(lens)
        out = np.zeros((count, 18), dtype=np.uint64)
        if count == 0:
            return out
        h = (ctypes.c_void_p * count)(*[s.h for s in srs_list])
        sp = (ctypes.c_void_p * count)(*[_ptr(s) for s in scalars_list])
        nn = (ctypes.c_size_t * count)(*[int(x) for x in lens])
        off = (ctypes.c_size_t * count)(*[int(x) for x in (offsets or [0] * count)])
        rc = self.lib.zk_msm_g1_batch(self.h, count, h, off, sp, nn, _h(out))
        if rc == ZK_ERR_LENGTH:
            raise MsmLengthError(rc, (self.lib.zk_last_error(self.h) or b"").decode(), 0)
        self._check(rc)
        if _TRACE_MSM:  # diagnostics: one line per batch (sizes + the library's phase timers)
            import sys

            print("zkhip-msm", [int(x) for x in lens], [round(float(x), 3) for x in self.msm_last_timing()], file=sys.stderr)
        return out

    def msm_g1_batch_async(self, srs_list, scalars_list, lens, offsets=None):
        """start a batch of MSMs on the ctx's job streams; -> job with .wait() -> [count, 18].  The scalar buffers must
        stay alive and unmodified until wait() (the job object keeps references to them)."""
        return MsmJob(self, srs_list, scalars_list, lens, offsets)

    # ---- G2 (same pipeline over Fq2) ----
    def srs_register_g2(self, bases: np.ndarray, stride: int = 192) -> Srs:
        """bases: affine G2 points x.c0|x.c1|y.c0|y.c1, [n, 24] uint64 Montgomery limbs (zeros = infinity)"""
        b = np.ascontiguousarray(bases)
        n = b.nbytes // stride
        h = ctypes.c_void_p()
        self._check(self.lib.zk_srs_register_g2(self.h, _h(b), stride, n, ctypes.byref(h)))
        s = Srs(self, h.value)
        s.g2 = True
        return s

    def msm_g2(self, srs: Srs, scalars, n: int, offset: int = 0) -> np.ndarray:
        """-> normalised Jacobian over Fq2, [36] uint64 (x.c0 x.c1 y.c0 y.c1 z.c0 z.c1)"""
        out = np.zeros(36, dtype=np.uint64)
        rc = self.lib.zk_msm_g2(self.h, srs.h, offset, _ptr(scalars), n, _h(out))
        if rc == ZK_ERR_LENGTH:
            raise MsmLengthError(rc, (self.lib.zk_last_error(self.h) or b"").decode(), min(n, max(len(srs) - offset, 0)))
        self._check(rc)
        return out

    def msm_g2_batch(self, srs_list, scalars_list, lens, offsets=None) -> np.ndarray:
        count = len(lens)
        out = np.zeros((count, 36), dtype=np.uint64)
        if count == 0:
            return out
        h = (ctypes.c_void_p * count)(*[s.h for s in srs_list])
        sp = (ctypes.c_void_p * count)(*[_ptr(s) for s in scalars_list])
        nn = (ctypes.c_size_t * count)(*[int(x) for x in lens])
        off = (ctypes.c_size_t * count)(*[int(x) for x in (offsets or [0] * count)])
        self._check(self.lib.zk_msm_g2_batch(self.h, count, h, off, sp, nn, _h(out)))
        return out

    def msm_g1_host(self, bases: np.ndarray, scalars: np.ndarray, stride: int = 96) -> np.ndarray:
        """drop-in for G::msm(&[Affine], &[Fr]) on host arrays"""
        b = np.ascontiguousarray(bases)
        s = np.ascontiguousarray(scalars, dtype=np.uint64)
        nb, ns = b.nbytes // stride, s.size // 4
        out = np.zeros(18, dtype=np.uint64)
        err = ctypes.c_size_t(0)
        rc = self.lib.zk_msm_g1_host(self.h, _h(b), stride, nb, _h(s), ns, _h(out), ctypes.byref(err))
        if rc == ZK_ERR_LENGTH:
            raise MsmLengthError(rc, (self.lib.zk_last_error(self.h) or b"").decode(), err.value)
        self._check(rc)
        return out

    def g1_lincomb(self, points: np.ndarray, scalars_canon: np.ndarray) -> np.ndarray:
        """sum_i k_i * P_i for a few points (host side, K9): points [n,18] Jacobian, scalars [n,4] canonical"""
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 18)
        sc = np.ascontiguousarray(scalars_canon, dtype=np.uint64).reshape(-1, 4)
        assert len(pts) == len(sc)
        out = np.zeros(18, dtype=np.uint64)
        self._check(self.lib.zk_g1_lincomb(self.h, _h(pts), _h(sc), len(pts), _h(out)))
        return out

    def g1_lincomb_batch(self, points: np.ndarray, scalars_canon: np.ndarray) -> np.ndarray:
        """points [count, n, 18], scalars [n, 4] shared by every row -> [count, 18]"""
        pts = np.ascontiguousarray(points, dtype=np.uint64)
        count, n = pts.shape[0], pts.shape[1]
        sc = np.ascontiguousarray(scalars_canon, dtype=np.uint64).reshape(-1, 4)
        assert len(sc) == n
        out = np.zeros((count, 18), dtype=np.uint64)
        if count:
            self._check(self.lib.zk_g1_lincomb_batch(self.h, _h(pts), _h(sc), n, count, _h(out)))
        return out

    # ---- the pairing and PolynomialCommitment::verify (dpoly_comm.rs:466-484) ----
    def pairing(self, g1_96: np.ndarray, g2, g2_stride: int = 192) -> np.ndarray:
        """e(P_i, Q_i): g1 [count, 12] affine, g2 [count, 24] affine (or raw records at g2_stride bytes) -> [count, 72] u64, ark's
        Fq12 layout (zkhip.pairing.fq12_from_ark); the value is zkhip.pairing.pairing(Q, P) ** ZK_PAIRING_EXP_MULTIPLE"""
        g1 = np.ascontiguousarray(g1_96, dtype=np.uint64).reshape(-1, 12)
        g2 = np.ascontiguousarray(g2)
        count = len(g1)
        assert g2.nbytes >= count * g2_stride or count == 0
        out = np.zeros((count, 72), dtype=np.uint64)
        self._check(self.lib.zk_pairing(self.h, count, _h(g1), _h(g2), g2_stride, _h(out)))
        return out

    def pairing_product_check(self, starts, g1_96: np.ndarray, g2, g2_stride: int = 192) -> np.ndarray:
        """ok[g] = prod_{starts[g] <= i < starts[g+1]} e(P_i, Q_i) == 1; starts: groups + 1 offsets -> [groups] bool"""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        groups = max(len(st) - 1, 0)
        g1 = np.ascontiguousarray(g1_96, dtype=np.uint64).reshape(-1, 12)
        g2 = np.ascontiguousarray(g2)
        ok = np.zeros(max(groups, 1), dtype=np.uint8)
        self._check(self.lib.zk_pairing_product_check(self.h, groups, _h(st), _h(g1), _h(g2), g2_stride, _h(ok)))
        return ok[:groups].astype(bool)

    def pcs_vk(self, powers_g2, g1_96=None, g2_stride: int = 192) -> "PcsVk":
        """the verifying key of PolynomialCommitment: g1 = powers_of_g[0][0] ([12] affine; None: the generator), powers_of_g2 [n, 24]"""
        return PcsVk(self, powers_g2, g1_96, g2_stride)

    def pcs_verify_batch(self, vk: "PcsVk", commitments, values, proofs, points) -> np.ndarray:
        """PolynomialCommitment::verify for count openings: commitments [count, 18] Jacobian, values [count, 4] Montgomery Fr,
        proofs [count, nvars, 18], points [count, nvars, 4] -> [count] bool"""
        cm = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 18)
        count = len(cm)
        vals = np.ascontiguousarray(values, dtype=np.uint64).reshape(count, 4)
        pf = np.ascontiguousarray(proofs, dtype=np.uint64)
        nvars = pf.shape[1] if pf.ndim == 3 else (pf.size // (18 * count) if count else 0)
        pf = pf.reshape(count, nvars, 18)
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(count, nvars, 4)
        ok = np.zeros(max(count, 1), dtype=np.uint8)
        self._check(self.lib.zk_pcs_verify_batch(self.h, vk.h, nvars, count, _h(cm), _h(vals), _h(pf), _h(pts), _h(ok)))
        return ok[:count].astype(bool)

    # ---- G1 points from outside: decompression and subgroup membership (csrc/zk_g1check.hip) ----
    def g1_decompress_check(self, data) -> Tuple[np.ndarray, np.ndarray]:
        """k compressed G1 points (bytes, or a uint8 array of k x 48) -> (points [k, 18] normalised Jacobian, status [k] uint8):
        0 ok, 1 bad encoding, 2 x not on the curve, 3 on the curve but not in G1 (include/zkhip.h; points of status 1 and 2 are zero)"""
        raw = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8).reshape(-1)
        if raw.size % 48:
            raise ValueError(f"{raw.size} bytes is not a whole number of 48-byte points")
        k = raw.size // 48
        out = np.zeros((k, 18), dtype=np.uint64)
        st = np.zeros(k, dtype=np.uint8)
        if k:
            self._check(self.lib.zk_g1_decompress_check(self.h, k, _h(raw), _h(out), _h(st)))
        return out, st

    def g1_check(self, points) -> np.ndarray:
        """points [k, 18] Jacobian in any representative -> status [k] uint8: 0 ok, 1 a coordinate >= q, 2 not on the curve, 3 not in G1"""
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 18)
        st = np.zeros(len(pts), dtype=np.uint8)
        if len(pts):
            self._check(self.lib.zk_g1_check(self.h, len(pts), _h(pts), _h(st)))
        return st

    # ---- G2 points from outside: decompression and subgroup membership (csrc/zk_g2check.hip) ----
    def g2_decompress_check(self, data) -> Tuple[np.ndarray, np.ndarray]:
        """k compressed G2 points (bytes, or a uint8 array of k x 96) -> (points [k, 24] affine Montgomery records, status [k] uint8):
        0 ok, 1 bad encoding, 2 x not on the twist, 3 on the twist but not in G2 (include/zkhip.h; points of status 1 and 2 and
        infinity are zero)"""
        raw = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8).reshape(-1)
        if raw.size % 96:
            raise ValueError(f"{raw.size} bytes is not a whole number of 96-byte points")
        k = raw.size // 96
        out = np.zeros((k, 24), dtype=np.uint64)
        st = np.zeros(k, dtype=np.uint8)
        if k:
            self._check(self.lib.zk_g2_decompress_check(self.h, k, _h(raw), _h(out), _h(st)))
        return out, st

    def g2_check(self, points, g2_stride: int = 192) -> np.ndarray:
        """points [k, 24] affine Montgomery records (or raw records at g2_stride bytes, as Ctx.pairing takes them) -> status [k] uint8:
        0 ok, 1 a coordinate >= q, 2 not on the twist, 3 not in G2"""
        pts = np.ascontiguousarray(points)
        if g2_stride < 192 or pts.nbytes % g2_stride:
            raise ValueError(f"{pts.nbytes} bytes is not a whole number of records of {g2_stride} bytes (>= 192)")
        k = pts.nbytes // g2_stride
        st = np.zeros(k, dtype=np.uint8)
        if k:
            self._check(self.lib.zk_g2_check(self.h, k, _h(pts), g2_stride, _h(st)))
        return st

    # ---- aggregated PCS verification: many openings, one pairing check (csrc/zk_g1seg.hip, csrc/zk_pairing.hip) ----
    def g1_lincomb_seg(self, starts, points, scalars_canon) -> np.ndarray:
        """out[s] = sum_{starts[s] <= t < starts[s+1]} k_t P_t on the device: starts [segments + 1] offsets from 0, points [terms, 18]
        Jacobian (any representative, Z = 0: infinity), scalars [terms, 4] canonical -> [segments, 18] normalised Jacobian.  A term that
        is not canonical or not on the curve raises ZkError(ZK_ERR_INVALID) naming the smallest such term"""
        st = np.ascontiguousarray(starts, dtype=np.uint64).reshape(-1)
        segments = max(len(st) - 1, 0)
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 18)
        sc = np.ascontiguousarray(scalars_canon, dtype=np.uint64).reshape(-1, 4)
        if segments and (len(pts) < int(st[-1]) or len(sc) < int(st[-1])):
            raise ValueError("fewer terms than the last offset")
        out = np.zeros((segments, 18), dtype=np.uint64)
        if segments:
            self._check(self.lib.zk_g1_lincomb_seg(self.h, segments, _h(st), _h(pts), _h(sc), _h(out)))
        return out

    @staticmethod
    def _agg_arrays(nvars, skip, cstart, cpoints, cscalars, values, proofs, points):
        nv = np.ascontiguousarray(nvars, dtype=np.uint64).reshape(-1)
        count = len(nv)
        sk = np.ascontiguousarray(skip, dtype=np.uint64).reshape(-1)
        cs = np.ascontiguousarray(cstart, dtype=np.uint64).reshape(-1)
        cp = np.ascontiguousarray(cpoints, dtype=np.uint64).reshape(-1, 18)
        ce = np.ascontiguousarray(cscalars, dtype=np.uint64).reshape(-1, 4)
        vals = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        pf = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 18)
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        rows = int(nv.sum()) if count else 0
        if len(sk) != count or len(cs) != count + 1 or len(vals) != count or len(pf) != rows or len(pts) != rows or len(cp) != len(ce) or len(cp) < int(cs[-1]):
            raise ValueError("pcs_verify_agg: the arrays disagree on the number of openings, terms or rows")
        return count, nv, sk, cs, cp, ce, vals, pf, pts

    @staticmethod
    def pcs_agg_weights(nvars, skip, cstart, cpoints, cscalars, values, proofs, points) -> np.ndarray:
        """the derived weights of pcs_verify_agg (zk_pcs_agg_weights: host only, needs no ctx and no GPU) -> [count, 2] u64"""
        count, nv, sk, cs, cp, ce, vals, pf, pts = Ctx._agg_arrays(nvars, skip, cstart, cpoints, cscalars, values, proofs, points)
        rho = np.zeros((count, 2), dtype=np.uint64)
        rc = _lib.lib().zk_pcs_agg_weights(count, _h(nv), _h(sk), _h(cs), _h(cp), _h(ce), _h(vals), _h(pf), _h(pts), _h(rho))
        if rc:
            raise ZkError(rc, "zk_pcs_agg_weights: the commitment offsets must start at 0 and not decrease")
        return rho

    def pcs_verify_agg(self, vk: "PcsVk", nvars, skip, cstart, cpoints, cscalars, values, proofs, points, rho=None) -> bool:
        """count openings of mixed variable counts in ONE pairing check (zk_pcs_verify_agg): nvars, skip [count]; opening k's commitment
        is sum_j e_j C_j over the terms cstart[k] .. cstart[k+1] of cpoints [*, 18] / cscalars [*, 4] (Montgomery); values [count, 4];
        proofs [rows, 18] and points [rows, 4]: the openings' rows one after another; rho [count, 2] u64 or None (derived)"""
        count, nv, sk, cs, cp, ce, vals, pf, pts = self._agg_arrays(nvars, skip, cstart, cpoints, cscalars, values, proofs, points)
        ok = np.zeros(1, dtype=np.uint8)
        r = None if rho is None else np.ascontiguousarray(rho, dtype=np.uint64).reshape(count, 2)
        self._check(self.lib.zk_pcs_verify_agg(self.h, vk.h, count, _h(nv), _h(sk), _h(cs), _h(cp), _h(ce), _h(vals), _h(pf), _h(pts),
                                               None if r is None else _h(r), _h(ok)))
        return bool(ok[0])

    # ---- a parameter set from a file: validation, halving and the consistency check on the device (csrc/zk_srsio.hip) ----
    def g1_decompress_check_device(self, d_in48, count: int, out=None, refuse_infinity: bool = False):
        """zk_g1_decompress_check on device memory: count compressed points at d_in48 -> (out: count x 96-byte affine records in the
        reference layout, as srs_wrap_device takes them; (bad, first, status): the number of points whose status is not 0, the smallest
        such index (None: none) and its status -- 4: a point at infinity, refused with refuse_infinity)"""
        out = out or self.alloc(max(96 * count, 16))
        res = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.zk_g1_decompress_check_device(self.h, count, _ptr(d_in48), _ptr(out), 1 if refuse_infinity else 0, _h(res)))
        bad = int(res[0])
        return out, (bad, int(res[1]) if bad else None, int(res[2]))

    def srs_halve(self, level: Srs) -> Srs:
        """out[j] = level[j] + level[j + m] for a level of 2m points; ZkError(ZK_ERR_INVALID) when a sum is the point at infinity"""
        h = ctypes.c_void_p()
        self._check(self.lib.zk_srs_halve(self.h, level.h, ctypes.byref(h)))
        return Srs(self, h.value)

    def fr_hash_expand(self, seed32: bytes, domain: int, n: int, out=None) -> DeviceBuffer:
        """out[j] = the low 128 bits of SHA-256(seed || u32le(domain) || u64le(j)) (the digest as a little-endian integer), Montgomery Fr"""
        seed32 = bytes(seed32)
        if len(seed32) != 32:
            raise ValueError(f"a seed of {len(seed32)} bytes, not 32")
        out = out or self.alloc(max(32 * n, 1))
        self._check(self.lib.zk_fr_hash_expand(self.h, seed32, domain, n, _ptr(out)))
        return out

    def srs_check(self, levels, powers_g2, seed32: bytes, g2_stride: int = 192) -> np.ndarray:
        """relation (B) of include/zkhip.h per level: levels [n + 1] Srs of 2^k points, powers_g2 [n + 1, 24] -> ok [n] bool; ok[k] says
        that level k + 1 matches the key powers_g2[n - k]"""
        n = len(levels) - 1
        seed32 = bytes(seed32)
        g2 = np.ascontiguousarray(powers_g2)
        if len(seed32) != 32 or g2.nbytes < (n + 1) * g2_stride:
            raise ValueError("srs_check: a 32-byte seed and n + 1 keys for n + 1 levels")
        h = (ctypes.c_void_p * (n + 1))(*[lv.h for lv in levels])
        ok = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.zk_srs_check(self.h, h, n, _h(g2), g2_stride, seed32, _h(ok)))
        return ok[:n].astype(bool)

    # ---- party exchanges through the C ABI (RCCL communicator inside the ctx) ----
    def comm_unique_id(self) -> bytes:
        buf = (ctypes.c_uint8 * 128)()
        rc = self.lib.zk_comm_unique_id(buf)
        if rc != 0:
            raise ZkError(rc, "zk_comm_unique_id failed (RCCL not loadable?)")
        return bytes(buf)

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == 128
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self.lib.zk_comm_init(self.h, rank, world, buf))

    def comm_destroy(self):
        self._check(self.lib.zk_comm_destroy(self.h))

    def comm_abort(self):
        """this party cannot go on: its peers' pending and later collectives end with ZK_ERR_COMM instead of waiting for it (zk_comm_abort)"""
        self._check(self.lib.zk_comm_abort(self.h))

    @property
    def comm_rank(self) -> int:
        return self.lib.zk_comm_rank(self.h)

    @property
    def comm_size(self) -> int:
        return self.lib.zk_comm_size(self.h)

    def allgather(self, d_send, nbytes: int, d_recv=None):
        d_recv = d_recv or self.alloc(max(nbytes * self.comm_size, 1))
        self._check(self.lib.zk_allgather(self.h, _ptr(d_send), nbytes, _ptr(d_recv)))
        return d_recv

    def alltoall(self, d_send, nbytes_per_peer: int, d_recv=None):
        d_recv = d_recv or self.alloc(max(nbytes_per_peer * self.comm_size, 1))
        self._check(self.lib.zk_alltoall(self.h, _ptr(d_send), nbytes_per_peer, _ptr(d_recv)))
        return d_recv

    def gather(self, d_send, nbytes: int, root: int, d_recv=None):
        if self.comm_rank == root:
            d_recv = d_recv or self.alloc(max(nbytes * self.comm_size, 1))
        self._check(self.lib.zk_gather(self.h, _ptr(d_send), nbytes, root, _ptr(d_recv)))
        return d_recv

    def scatter(self, d_send, nbytes: int, root: int, d_recv=None):
        d_recv = d_recv or self.alloc(max(nbytes, 1))
        self._check(self.lib.zk_scatter(self.h, _ptr(d_send), nbytes, root, _ptr(d_recv)))
        return d_recv

    def d_msm(self, srs_list, scalars_list, lens, coeffs_canon: np.ndarray, lam_mont=None, offsets=None) -> np.ndarray:
        """zk_d_msm: batch of local MSMs + all-gather + this party's row of the public map -> [count, 18]"""
        count = len(lens)
        out = np.zeros((count, 18), dtype=np.uint64)
        if count == 0:
            return out
        h = (ctypes.c_void_p * count)(*[s.h for s in srs_list])
        sp = (ctypes.c_void_p * count)(*[_ptr(s) for s in scalars_list])
        nn = (ctypes.c_size_t * count)(*[int(x) for x in lens])
        off = (ctypes.c_size_t * count)(*[int(x) for x in (offsets or [0] * count)])
        co = np.ascontiguousarray(coeffs_canon, dtype=np.uint64).reshape(-1, 4)
        assert len(co) == self.comm_size
        lam = np.ascontiguousarray(lam_mont, dtype=np.uint64) if lam_mont is not None else None
        rc = self.lib.zk_d_msm(self.h, count, h, off, sp, nn, _h(lam) if lam is not None else 0, _h(co), _h(out))
        if rc == ZK_ERR_LENGTH:
            raise MsmLengthError(rc, (self.lib.zk_last_error(self.h) or b"").decode(), 0)
        self._check(rc)
        return out

    def msm_set_window(self, c: int):
        self._check(self.lib.zk_msm_set_window(self.h, c))

    def sumcheck_last_timing(self) -> np.ndarray:
        """[first stage ms, all launches ms] of the last sumcheck-family call (recorded while dbg_tune("sc_ts", 3))"""
        t = np.zeros(2, dtype=np.float32)
        self._check(self.lib.zk_sumcheck_last_timing(self.h, _h(t)))
        return t

    def msm_last_timing(self) -> np.ndarray:
        t = np.zeros(6, dtype=np.float32)
        self._check(self.lib.zk_msm_last_timing(self.h, _h(t)))
        return t

    # ---- test hooks (include/zkhip_test.h: not part of the ABI; resolved on first use) ----
    def dbg_tune(self, key: str, value: int):
        """process-wide experiment / diagnostics knob (zk_dbg_tune; csrc/zk_ctx.hpp `struct Tuning`)"""
        rc = test_hooks().zk_dbg_tune(key.encode(), int(value))
        if rc != 0:
            raise ZkError(rc, f"zk_dbg_tune: unknown key {key!r}")

    def dbg_fq(self, op: str, a, b, n, out=None):
        h = test_hooks()
        fn = {"add": h.zk_dbg_fq_add, "sub": h.zk_dbg_fq_sub, "mul": h.zk_dbg_fq_mul, "mul2add": h.zk_dbg_fq_mul2add}[op]
        out = out or self.alloc(max(48 * n, 1))
        self._check(fn(self.h, _ptr(a), _ptr(b), _ptr(out), n))
        return out

    def dbg_g2_op(self, mode: int, p, q, n) -> np.ndarray:
        out = np.zeros((n, 36), dtype=np.uint64)
        self._check(test_hooks().zk_dbg_g2_op(self.h, mode, _ptr(p), _ptr(q), _h(out), n))
        return out

    def dbg_g1_op(self, mode: int, p, q, n) -> np.ndarray:
        out = np.zeros((n, 18), dtype=np.uint64)
        self._check(test_hooks().zk_dbg_g1_op(self.h, mode, _ptr(p), _ptr(q), _h(out), n))
        return out

    FQ30_MODES = ("csub_q", "csub_2q", "csub_4q", "csub_8q", "red4", "red8", "red16", "canon8", "sub2", "sub4", "sub6", "sub8", "sub12",
                  "add", "add2x", "mul", "sqr", "mul2add", "inv")
    FQ12_MODES = ("mul", "sqr", "cyc_sqr", "inv", "conj", "frob1", "frob2", "frob3", "mul_by_014", "exp_by_x", "final_exp", "f6_mul",
                  "f6_inv", "f2_mul", "f2_sqr", "f2_inv")

    def dbg_fq30(self, mode: str, x, kx, y, ky, n):
        """zk_dbg_fq30_op on device buffers (x, y: n x 48 bytes; kx, ky: n u32) -> (limbs [n, 13] u32, flags [n] u32)"""
        out, flags = self.alloc(max(64 * n, 1)), self.alloc(max(4 * n, 1))
        self._check(test_hooks().zk_dbg_fq30_op(self.h, self.FQ30_MODES.index(mode), _ptr(x), _ptr(kx), _ptr(y), _ptr(ky), _ptr(out),
                                                _ptr(flags), n))
        return out.download((n, 16), np.uint32)[:, :13], flags.download((n,), np.uint32)

    def dbg_fq12(self, mode: str, a, b, lift, n):
        """zk_dbg_fq12_op on device buffers (a, b: n x 576 bytes, ark layout; lift: n u32) -> (values [n, 72] u64, flags [n] u32)"""
        out, flags = self.alloc(max(576 * n, 1)), self.alloc(max(4 * n, 1))
        self._check(test_hooks().zk_dbg_fq12_op(self.h, self.FQ12_MODES.index(mode), _ptr(a), _ptr(b), _ptr(lift), _ptr(out), _ptr(flags), n))
        return out.download((n, 72)), flags.download((n,), np.uint32)

    XYZZ_MODES = ("madd", "madd_neg", "add", "dbl", "dbl_affine", "add_quad", "acc_quad")

    def dbg_xyzz(self, g2: bool, mode: str, a, lift_a, b, lift_b, rep, n):
        """zk_dbg_xyzz_op / zk_dbg_xyzz2_op (g2) on device buffers (a, b: n operands of 4 (8) integers below q, 48 bytes each, internal
        form; lift_a, lift_b, rep: n u32) -> raw limbs [n, 4 (8), 13] u32 in the order X, Y, ZZ, ZZZ (c0 then c1 for G2)"""
        nc = 8 if g2 else 4
        out = self.alloc(max(64 * nc * n, 1))
        fn = test_hooks().zk_dbg_xyzz2_op if g2 else test_hooks().zk_dbg_xyzz_op
        self._check(fn(self.h, self.XYZZ_MODES.index(mode), _ptr(a), _ptr(lift_a), _ptr(b), _ptr(lift_b), _ptr(rep), _ptr(out), n))
        return out.download((n, nc, 16), np.uint32)[:, :, :13]
