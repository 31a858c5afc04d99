"""Blake2bWrite / Blake2bRead of halo2_proofs 0.2.0 (src/transcript.rs, as recalled; the reference reaches them from gen_proofs_and_verify,
src/test_utils.rs:21-68 of the reference) over the library's transcript handle (trh_tr_*, csrc/transcript.h): the hashing, the point
encoding and the reduction of a challenge run in libtrh.so on the host, no device is needed.

    w = Blake2bWrite(curve);  ... create_proof(..., w) ...;  proof = w.finalize()
    r = Blake2bRead(curve, proof);  ... verify_proof(..., r) ...;  r.finished()

Both have the duck type plonk.py documents: common_point(12-limb normalised Jacobian or 8-limb affine), common_scalar(4 Montgomery limbs),
squeeze_challenge_scalar() -> int; the writer write_point / write_scalar, the reader read_point() -> the 8-limb affine POD and
read_scalar() -> int.  The handle latches its first error; here it is raised as TranscriptError at the call that met it, and by
raise_if_failed() after an opening whose round loop called the handle from C (ipa.create_proof_native)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import api
from .poly import _MODULUS, _mont


class TranscriptError(api.TrhError):
    """the identity as a transcript point, bytes that are no point or no scalar, a proof that ends early"""


def _canon(limbs, m: int) -> int:
    v = 0
    for i in range(4):
        v |= int(limbs[i]) << (64 * i)
    return v * pow(1 << 256, -1, m) % m


class _Handle:
    def __init__(self, curve: str):
        self.curve = curve
        self._m = _MODULUS[api.SCALAR_FIELD[curve]]
        self._one = _mont(api.BASE_FIELD[curve], 1)  # Z = 1, for points that arrive affine
        self.handle = api._vp()
        self.squeezes = []

    def _check(self, rc: int):
        if rc != 0:
            raise TranscriptError(f"libtrh error {rc}: {api.lib().trh_last_error().decode()}")

    def _jacobian(self, limbs):
        p = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1)
        if p.size == 12:
            return p
        assert p.size == 8, "a point is 12 limbs (Jacobian) or 8 (affine)"
        return np.concatenate([p, self._one if p.any() else np.zeros(4, np.uint64)])

    def raise_if_failed(self):
        """the latched error of operations that could not report it: the C callbacks inside trh_ipa_create_proof"""
        self._check(api.lib().trh_tr_status(self.handle))

    def common_point(self, limbs):
        self._check(api.lib().trh_tr_common_point(self.handle, api._p(self._jacobian(limbs))))

    def common_scalar(self, limbs):
        self._check(api.lib().trh_tr_common_scalar(self.handle, api._p(np.ascontiguousarray(limbs, dtype=np.uint64).reshape(4))))

    def squeeze_challenge_scalar(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        self._check(api.lib().trh_tr_squeeze_challenge_scalar(self.handle, api._p(out)))
        self.squeezes.append(_canon(out, self._m))
        return self.squeezes[-1]

    def destroy(self):
        if self.handle:
            api.lib().trh_tr_destroy(self.handle)
            self.handle = api._vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Blake2bWrite(_Handle):
    def __init__(self, curve: str):
        super().__init__(curve)
        self._check(api.lib().trh_tr_create_writer(api.CURVE_ID[curve], ctypes.byref(self.handle)))

    def write_point(self, limbs):
        self._check(api.lib().trh_tr_write_point(self.handle, api._p(self._jacobian(limbs))))

    def write_scalar(self, limbs):
        self._check(api.lib().trh_tr_write_scalar(self.handle, api._p(np.ascontiguousarray(limbs, dtype=np.uint64).reshape(4))))

    def callbacks(self) -> api.Transcript:
        """the writer as trh_ipa_create_proof's transcript: ctx and three functions of the library; valid while this object lives"""
        tr = api.Transcript()
        self._check(api.lib().trh_tr_callbacks(self.handle, ctypes.byref(tr)))
        return tr

    def finalize(self) -> bytes:
        """Blake2bWrite::finalize: the proof so far"""
        n = ctypes.c_size_t(0)
        self._check(api.lib().trh_tr_bytes_len(self.handle, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(n.value, 1))
        self._check(api.lib().trh_tr_bytes(self.handle, buf, n.value))
        return buf.raw[:n.value]


class Blake2bRead(_Handle):
    def __init__(self, curve: str, proof: bytes):
        super().__init__(curve)
        proof = bytes(proof)
        self._check(api.lib().trh_tr_create_reader(api.CURVE_ID[curve], proof, len(proof), ctypes.byref(self.handle)))

    def read_point(self) -> np.ndarray:
        out = np.zeros(8, dtype=np.uint64)
        self._check(api.lib().trh_tr_read_point(self.handle, api._p(out)))
        return out

    def read_scalar(self) -> int:
        out = np.zeros(4, dtype=np.uint64)
        self._check(api.lib().trh_tr_read_scalar(self.handle, api._p(out)))
        return _canon(out, self._m)

    def remaining(self) -> int:
        n = ctypes.c_size_t(0)
        self._check(api.lib().trh_tr_remaining(self.handle, ctypes.byref(n)))
        return int(n.value)

    def finished(self) -> bool:
        """every byte of the proof has been read"""
        return self.remaining() == 0
