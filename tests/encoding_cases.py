"""Shared inputs and references of the square-root / point-encoding tests (tests/test_encoding_host.py, tests/test_gpu_encoding.py).
Every expected value comes from oracle/pasta.py integers; the encoder / decoder below restate the 32-byte format from its definition:
x canonical, little endian, bit 255 = parity of canonical y, identity = 32 zero bytes; a decoder rejects x >= m and x^3 + 5 non-square."""
import functools
import random

import numpy as np

import pasta as o

INVALID = "invalid"


def even_root(f, a):
    """the root csrc/fieldsqrt.h promises: the one whose canonical value is even (None: a is not a square)"""
    r = f.sqrt(a)
    if r is None:
        return None
    return r if r % 2 == 0 else f.m - r


@functools.lru_cache(maxsize=None)
def sqrt_records(field):
    """[(tag, a)] canonical: the fixed values, every order 2^j of the 2-part alone and under a random square, non-squares, random"""
    f = o.FIELDS[field]
    rng = random.Random(0x5A17 + len(field) + ord(field[1]))
    recs = [("0", 0), ("1", 1), ("4", 4), ("m-1", f.m - 1)]
    for j in range(33):
        recs.append((f"omega_{j}", f.omega(j)))
    r = rng.randrange(1, f.m)
    for j in range(32):
        recs.append((f"r^2*omega_{j}", r * r * f.omega(j) % f.m))
    recs.append(("generator", f.GENERATOR))
    recs.append(("5*r^2", 5 * r * r % f.m))
    for i in range(256):
        s = rng.randrange(f.m)
        recs.append((f"random-square-{i}", s * s % f.m))
    for i in range(256):
        recs.append((f"random-{i}", rng.randrange(f.m)))
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def sqrt_expected(field):
    """per record (root canonical or 0, flag)"""
    f = o.FIELDS[field]
    out = []
    for _, a in sqrt_records(field):
        r = even_root(f, a)
        out.append((0, 0) if r is None else (r, 1))
    return tuple(out)


def sqrt_input_limbs(field):
    f = o.FIELDS[field]
    return np.array([f.limbs(a) for _, a in sqrt_records(field)], np.uint64)


def sqrt_expected_limbs(field):
    f = o.FIELDS[field]
    exp = sqrt_expected(field)
    return np.array([f.limbs(r) for r, _ in exp], np.uint64), np.array([fl for _, fl in exp], np.uint8)


def check_sqrt(field, roots, flags):
    """roots: (n, 4) Montgomery limbs, flags: n bytes, for sqrt_records(field) in order.  Returns the list of failures: the flag, r^2 = a,
    the even-root convention -- and, together, limb-for-limb equality with the oracle's even root"""
    f = o.FIELDS[field]
    bad = []
    for (tag, a), (want, wflag), got_l, got_f in zip(sqrt_records(field), sqrt_expected(field), roots, flags):
        got = f.from_limbs(got_l)
        if int(got_f) != wflag:
            bad.append(f"{field} {tag}: is_square {int(got_f)}, expected {wflag}")
        elif wflag and got * got % f.m != a:
            bad.append(f"{field} {tag}: r^2 != a")
        elif wflag and got % 2:
            bad.append(f"{field} {tag}: the odd root")
        elif [int(v) for v in got_l] != f.limbs(want):
            bad.append(f"{field} {tag}: {got:#x}, expected {want:#x}")
    return bad


# ---- the 32-byte encoding -------------------------------------------------------------------------------------------------------------
def encode(curve, pt) -> bytes:
    if pt is None:
        return bytes(32)
    x, y = pt
    return (x | ((y & 1) << 255)).to_bytes(32, "little")


def decode(curve, b: bytes):
    """-> affine point, None (identity) or INVALID"""
    cv = o.CURVES[curve]
    v = int.from_bytes(b, "little")
    if v == 0:
        return None
    s, x = v >> 255, v & ((1 << 255) - 1)
    if x >= cv.base.m:
        return INVALID
    pt = cv.lift_x(x)
    if pt is None:
        return INVALID
    y = pt[1]
    if y & 1 != s:
        y = cv.base.m - y
    return (x, y)


def enc_int(x, sign=0) -> bytes:
    return (x | (sign << 255)).to_bytes(32, "little")


def special_encodings(curve):
    """[(tag, bytes)], each with its answer from decode(): the rejections the format defines and the identity"""
    m = o.CURVES[curve].base.m
    return [("identity", bytes(32)), ("sign-bit-only", enc_int(0, 1)), ("x=m", enc_int(m)), ("x=m,sign", enc_int(m, 1)), ("x=m+1", enc_int(m + 1)),
            ("x=2^255-1", enc_int((1 << 255) - 1)), ("x=2^255-1,sign", enc_int((1 << 255) - 1, 1)), ("x=2", enc_int(2)), ("x=2,sign", enc_int(2, 1))]


def pod(curve, pt):
    """the library's 64-byte affine POD as 8 u64 (identity and INVALID: all zero)"""
    return [0] * 8 if pt is None or pt == INVALID else o.CURVES[curve].affine_limbs(pt)


def encode_pods(curve, xy) -> bytes:
    """(n, 8) affine PODs (Montgomery limbs) -> n * 32 bytes, through the Python encoder"""
    cv = o.CURVES[curve]
    return b"".join(encode(curve, cv.affine_from_limbs(row)) for row in np.asarray(xy, np.uint64).reshape(-1, 8))
