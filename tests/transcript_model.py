"""The proof transcript of halo2_proofs 0.2.0 (Blake2bWrite / Blake2bRead with Challenge255, src/transcript.rs as recalled) in Python: hashlib's
BLAKE2b with the personalisation "Halo2-Transcript", Python integers, and oracle/pasta.py for the fields and the curve equation.  It shares no
code with csrc/transcript.h; what it shares is the format:

    common_point   01 || x || y     32 bytes each, little endian, canonical; the identity is refused
    common_scalar  02 || s          32 bytes
    write_*        the same, and the proof grows by the 32-byte compressed point (x with the parity of y in bit 255) / by s
    squeeze        00, then the digest of a copy of the state as a little-endian integer modulo the scalar field's order
    read_point     32 bytes -> a point (x below the modulus, x^3 + 5 a square, not the identity), then common_point
    read_scalar    32 bytes -> a value below the modulus, then common_scalar

Writer / Reader speak limbs (the interface tiny_ram_halo2_amd.plonk documents, the one of plonk_model.Writer / Reader), ModelReader speaks
affine tuples and integers with plonk_model.ModelReader's interface and constructor, so that plonk_model.verify can read bytes: see verify()."""
import hashlib
from unittest import mock

import numpy as np

import pasta as o
import plonk_model as pm

PERSON = b"Halo2-Transcript"


class TranscriptError(Exception):
    """the model's refusal: the identity, bytes that are no point or no scalar, a proof that ends early"""


def compress(cv, pt) -> bytes:
    if pt is None:
        return bytes(32)
    return (pt[0] | (pt[1] & 1) << 255).to_bytes(32, "little")


def decompress(cv, data: bytes):
    """-> the affine tuple, None for the 32 zero bytes; TranscriptError for anything that is no encoding"""
    v = int.from_bytes(data, "little")
    if v == 0:
        return None
    sign, x = v >> 255, v & ((1 << 255) - 1)
    if x >= cv.base.m:
        raise TranscriptError("x is not below the modulus")
    y = cv.base.sqrt((x * x * x + cv.b) % cv.base.m)
    if y is None:
        raise TranscriptError("x^3 + 5 is not a square")
    if y & 1 != sign:
        y = cv.base.m - y
    return (x, y)


class _Sponge:
    def __init__(self, curve: str):
        self.curve, self.cv = curve, o.CURVES[curve]
        self.h = hashlib.blake2b(digest_size=64, person=PERSON)
        self.squeezes = []

    def absorb_point(self, pt):
        if pt is None:
            raise TranscriptError("cannot write points at infinity to the transcript")
        self.h.update(b"\x01" + pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little"))

    def absorb_scalar(self, v):
        self.h.update(b"\x02" + (v % self.cv.scalar.m).to_bytes(32, "little"))

    def squeeze_challenge_scalar(self):
        self.h.update(b"\x00")
        c = int.from_bytes(self.h.copy().digest(), "little") % self.cv.scalar.m
        self.squeezes.append(c)
        return c

    def _point_of(self, limbs):
        limbs = [int(v) for v in np.asarray(limbs).reshape(-1)]
        return self.cv.jacobian_limbs_to_affine(limbs) if len(limbs) == 12 else self.cv.affine_from_limbs(limbs)

    def _scalar_of(self, limbs):
        return self.cv.scalar.from_limbs([int(v) for v in np.asarray(limbs).reshape(-1)])


class Writer(_Sponge):
    """the prover's transcript over limbs; finalize() -> the proof"""

    def __init__(self, curve: str):
        super().__init__(curve)
        self.proof = bytearray()

    def common_point(self, limbs):
        self.absorb_point(self._point_of(limbs))

    def common_scalar(self, limbs):
        self.absorb_scalar(self._scalar_of(limbs))

    def write_point(self, limbs):
        pt = self._point_of(limbs)
        self.absorb_point(pt)
        self.proof += compress(self.cv, pt)

    def write_scalar(self, limbs):
        v = self._scalar_of(limbs)
        self.absorb_scalar(v)
        self.proof += v.to_bytes(32, "little")

    def finalize(self) -> bytes:
        return bytes(self.proof)


class _ByteReader(_Sponge):
    def __init__(self, curve: str, proof: bytes):
        super().__init__(curve)
        self.proof, self.at = bytes(proof), 0

    def _take(self) -> bytes:
        if len(self.proof) - self.at < 32:
            raise TranscriptError("fewer than 32 bytes of the proof are left")
        self.at += 32
        return self.proof[self.at - 32:self.at]

    def _read_point(self):
        pt = decompress(self.cv, self._take())
        self.absorb_point(pt)
        return pt

    def _read_scalar(self):
        v = int.from_bytes(self._take(), "little")
        if v >= self.cv.scalar.m:
            raise TranscriptError("the scalar is not below the modulus")
        self.absorb_scalar(v)
        return v

    def finished(self) -> bool:
        return self.at == len(self.proof)


class Reader(_ByteReader):
    """the device verifier's interface: limbs in, read_point() -> the 8-limb affine POD, read_scalar() -> int"""

    def common_point(self, limbs):
        self.absorb_point(self._point_of(limbs))

    def common_scalar(self, limbs):
        self.absorb_scalar(self._scalar_of(limbs))

    def read_point(self):
        return np.array(self.cv.affine_limbs(self._read_point()), dtype=np.uint64)

    def read_scalar(self):
        return self._read_scalar()


class ModelReader(_ByteReader):
    """plonk_model.ModelReader over bytes: affine tuples and integers throughout.  A proof that is no proof ends plonk_model.verify with
    TranscriptError."""

    def common_point(self, pt):
        self.absorb_point(pt)

    def common_scalar(self, v):
        self.absorb_scalar(v)

    def read_point(self):
        return self._read_point()

    def read_scalar(self):
        return self._read_scalar()


def verify(*args, **kwargs):
    """plonk_model.verify with the proof -- its `items` argument -- a byte string: the model's verifier builds its transcript by the name
    ModelReader(curve, items), which stands for the class above while it runs.  -> (accepted, squeezes, refused)"""
    with mock.patch.object(pm, "ModelReader", ModelReader):
        return pm.verify(*args, **kwargs)
