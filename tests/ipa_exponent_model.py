"""The IPA opening in the exponent: halo2's poly::commitment::prover::create_proof (the description at the top of csrc/ipa.hip) over
generators that are KNOWN multiples of the curve generator G -- g_i = a_i G (a_i = 0: the identity, an all-zero record), W = omega G,
U = upsilon G.  Every point of the opening is then an integer mod the group order q, times G:

    S   = (<s', a> + s_blind omega) G                              s' = s - s(x3)
    L_j = (<p'[half..], a'[..half]> + rand_l omega + z value_l upsilon) G      value_l = <p'[half..], b[..half]>
    R_j = (<p'[..half], a'[half..]> + rand_r omega + z value_r upsilon) G      value_r = <p'[..half], b[half..]>
    a'[i] += u_j a'[i + half]      p'[i] += u_j^-1 p'[i + half]      b[i] += u_j b[i + half]
    c = p'[0] after the last fold,  f = s_blind xi + p_blind + sum_j (rand_l u_j^-1 + rand_r u_j)

Python integers only; nothing of the code under test enters it, and no group arithmetic either: the caller turns a log into a point (one
scalar multiplication of an oracle) where the transcript needs its bytes.  tests/test_ipa_exponent_model.py pins it to
oracle/pasta.py::ipa_create_proof; tests/test_gpu_ipa_collisions.py compares the device's transcript with it, and
tests/ipa_collision_cases.py takes the scalar rows of the first MSMs from it.

`transcript` has write_point(log), write_scalar(int) and squeeze_challenge_scalar() -> int; `rng()` -> int, two draws per round
(rand_l, then rand_r), as oracle/pasta.py::ipa_create_proof takes them."""
import numpy as np

from common import HashTranscript


class Opening:
    """what create_proof returns: the logs of S, L_j, R_j, the scalars c and f, the challenges, and the scalar rows of the MSMs that run
    over the ORIGINAL generators g || w || u (the commitment to s' and round 0), index for index"""

    def __init__(self):
        self.S, self.L, self.R, self.c, self.f = 0, [], [], 0, 0
        self.xi = self.z = 0
        self.u = []
        self.row_s = self.row_l0 = self.row_r0 = None

    def items(self):
        """the transcript in order: ("S" | "L_j" | "R_j", log) ..., ("c", int), ("f", int)"""
        out = [("S", self.S)]
        for j, (l, r) in enumerate(zip(self.L, self.R)):
            out += [(f"L_{j}", l), (f"R_{j}", r)]
        return out + [("c", self.c), ("f", self.f)]


def eval_poly(poly, x, q):
    acc = 0
    for cf in reversed(poly):
        acc = (acc * x + cf) % q
    return acc


def dot(x, y, q):
    return sum(v * w for v, w in zip(x, y)) % q


def create_proof(q, k, a, omega, upsilon, rng, transcript, p_poly, p_blind, x3, s_poly, s_blind, rounds=None):
    """rounds: stop behind that many rounds (the cases only need the rows of S, L_0 and R_0); c and f are then not written"""
    n = 1 << k
    assert len(a) == n and len(p_poly) == n and len(s_poly) == n
    out = Opening()
    a = [v % q for v in a]
    s_prime = [v % q for v in s_poly]
    s_prime[0] = (s_prime[0] - eval_poly(s_prime, x3, q)) % q
    out.row_s = s_prime + [s_blind % q, 0]
    out.S = (dot(s_prime, a, q) + s_blind * omega) % q
    transcript.write_point(out.S)
    xi = out.xi = transcript.squeeze_challenge_scalar()
    z = out.z = transcript.squeeze_challenge_scalar()
    p_prime = [(s * xi + p) % q for s, p in zip(s_prime, p_poly)]
    p_prime[0] = (p_prime[0] - eval_poly(p_prime, x3, q)) % q
    f = (s_blind * xi + p_blind) % q
    b, cur = [], 1
    for _ in range(n):
        b.append(cur)
        cur = cur * x3 % q
    for j in range(k if rounds is None else rounds):
        half = 1 << (k - j - 1)
        value_l, value_r = dot(p_prime[half:], b[:half], q), dot(p_prime[:half], b[half:], q)
        rand_l, rand_r = rng() % q, rng() % q
        if j == 0:
            out.row_l0 = p_prime[half:] + [0] * half + [rand_l, z * value_l % q]
            out.row_r0 = [0] * half + p_prime[:half] + [rand_r, z * value_r % q]
        l_j = (dot(p_prime[half:], a[:half], q) + rand_l * omega + z * value_l % q * upsilon) % q
        r_j = (dot(p_prime[:half], a[half:], q) + rand_r * omega + z * value_r % q * upsilon) % q
        out.L.append(l_j)
        out.R.append(r_j)
        transcript.write_point(l_j)
        transcript.write_point(r_j)
        u_j = transcript.squeeze_challenge_scalar()
        assert u_j % q, "a zero challenge: the Rust prover panics here"
        u_inv = pow(u_j, -1, q)
        out.u.append(u_j)
        p_prime = [(p_prime[i] + p_prime[i + half] * u_inv) % q for i in range(half)]
        b = [(b[i] + b[i + half] * u_j) % q for i in range(half)]
        a = [(a[i] + a[i + half] * u_j) % q for i in range(half)]
        f = (f + rand_l * u_inv + rand_r * u_j) % q
    if rounds is not None and rounds < k:
        return out
    out.c, out.f = p_prime[0], f
    transcript.write_scalar(out.c)
    transcript.write_scalar(out.f)
    return out


class LogTranscript(HashTranscript):
    """the hash transcript of tests/common.py, fed with logs: a point is absorbed as the 64 bytes of point_of(log) -- (8,) uint64 affine
    limbs, all zero for the identity -- so that its challenges are those of a DeviceTranscript that saw the same points"""

    def __init__(self, field, point_of):
        super().__init__(field.m)
        self.field, self.point_of = field, point_of
        self.challenges = []

    def write_point(self, log):
        self._absorb(b"P", np.ascontiguousarray(self.point_of(log % self.m), dtype=np.uint64).reshape(8).tobytes())

    def write_scalar(self, v):
        self._absorb(b"S", np.array(self.field.limbs(v % self.m), dtype=np.uint64).tobytes())

    def squeeze_challenge_scalar(self):
        c = super().squeeze_challenge_scalar()
        self.challenges.append(c)
        return c
