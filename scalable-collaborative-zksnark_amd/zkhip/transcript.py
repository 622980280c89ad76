"""
The Fiat-Shamir transcript of include/zkhip.h: a SHA-256 hash chain on a 32-byte state.

    init(label):   state = SHA256("zkhip-fs-v1" || label)
    absorb(data):  state = SHA256(state || 0x00 || data)   field elements and points as they sit in proof records (little-endian
                                                            u64 limbs, Montgomery form), integers as one little-endian u64
    challenge():   d = SHA256(state || 0x01), state = d;   the challenge is d as a little-endian integer with its top two bits
                                                            cleared (< 2^254 < r: no rejection loop)

`Transcript` keeps the state on the device (zk_transcript_*): the prover's sumchecks draw their challenges from it between kernels.
`HostTranscript` is the same chain on hashlib: the verifier's, which needs no device hashing.  One interface for both.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

from .field import fr_mont

DOMAIN = b"zkhip-fs-v1"


def _bytes(data) -> bytes:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    return np.ascontiguousarray(data, dtype="<u8").tobytes()


class HostTranscript:
    def __init__(self, label: bytes):
        self._state = hashlib.sha256(DOMAIN + bytes(label)).digest()

    def absorb(self, data):
        """bytes, or an array of u64 words (limbs of field elements / points) taken little-endian"""
        self._state = hashlib.sha256(self._state + b"\x00" + _bytes(data)).digest()
        return self

    def absorb_u64(self, value: int):
        return self.absorb(int(value).to_bytes(8, "little"))

    def challenge_int(self) -> int:
        self._state = hashlib.sha256(self._state + b"\x01").digest()
        return int.from_bytes(self._state, "little") & ((1 << 254) - 1)

    def challenges(self, count: int) -> np.ndarray:
        """-> [count, 4] Montgomery Fr"""
        return np.stack([fr_mont(self.challenge_int()) for _ in range(count)]) if count else np.zeros((0, 4), dtype=np.uint64)

    def challenge(self) -> np.ndarray:
        return self.challenges(1)[0]

    def state(self) -> bytes:
        return self._state


class Transcript:
    """the chain with its state in device memory (zk_transcript); freed before its Ctx"""

    def __init__(self, be, label: bytes):
        self.be, self.h = be, None
        label = bytes(label)
        h = ctypes.c_void_p()
        be._check(be.lib.zk_transcript_create(be.h, label, len(label), ctypes.byref(h)))
        self.h = h.value

    def free(self):
        if self.h and self.be.h:
            self.be.lib.zk_transcript_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def absorb(self, data):
        b = _bytes(data)
        self.be._check(self.be.lib.zk_transcript_absorb(self.be.h, self.h, b, len(b)))
        return self

    def absorb_u64(self, value: int):
        return self.absorb(int(value).to_bytes(8, "little"))

    def absorb_device(self, buf, nbytes: int):
        from .api import _ptr

        self.be._check(self.be.lib.zk_transcript_absorb_device(self.be.h, self.h, _ptr(buf), nbytes))
        return self

    def challenges(self, count: int) -> np.ndarray:
        out = np.zeros((count, 4), dtype=np.uint64)
        self.be._check(self.be.lib.zk_transcript_challenges(self.be.h, self.h, count, out.ctypes.data))
        return out

    def challenge(self) -> np.ndarray:
        return self.challenges(1)[0]

    def state(self) -> bytes:
        out = np.zeros(32, dtype=np.uint8)
        self.be._check(self.be.lib.zk_transcript_state(self.be.h, self.h, out.ctypes.data))
        return out.tobytes()
