"""Host-side mirror of `halo2_proofs::poly::commitment::prover::create_proof` (the IPA opening that
`poly::multiopen::create_proof` ends with; reference call site /root/reference/src/test_utils.rs:41-49,
SURVEY.md section 8 row a7).  Vectors p', b and the generators G' stay in device memory for the k
rounds; per round only the two points L_j, R_j and the challenge cross the host boundary.

The transcript (BLAKE2b, on the Rust host) and the prover's randomness are injected:
    transcript.write_point(jacobian12), .write_scalar(limbs4), .squeeze_challenge_scalar() -> int (canonical)
    rng() -> int (canonical scalar)
so the flow can be replayed bit-for-bit against the oracle restatement.

The verifier's side (`poly::commitment::{MSM, Guard}`, verify_proof's arithmetic, BatchVerifier::finalize's fold) follows
create_proof below: MSM, verify_proof, batch_verify.
"""
from __future__ import annotations

import numpy as np

from . import api
from .poly import _MODULUS, _mont, _stream
from .transcript import Blake2bWrite


def _canon(field: str, limbs) -> int:
    m = _MODULUS[field]
    v = 0
    for i, w in enumerate(np.asarray(limbs, dtype=np.uint64).reshape(4)):
        v |= int(w) << (64 * i)
    return v * pow(1 << 256, -1, m) % m


class RngScalarFn:
    """An api.Rng as the `trh_rng_scalar_fn` callback of trh_ipa_create_proof: every call is one trh_rng_next_scalar in the scalar field
    of `curve`, written straight into the library's buffer.  The callback runs with the context locked; trh_rng_next_scalar is host-only
    and takes nothing but the handle's own lock, so that is allowed (include/trh.h).  A C callback cannot fail: a refused draw (the end of
    the stream) leaves the scalar zero and is kept in `error`, which create_proof_native raises after the call."""

    def __init__(self, rng: api.Rng, curve: str):
        self.rng, self.error = rng, None
        lib, fid = api.lib(), api.FIELD_ID[api.SCALAR_FIELD[curve]]

        def draw(ctx, out):
            if lib.trh_rng_next_scalar(rng.handle, fid, out) != 0:
                self.error = self.error or lib.trh_last_error().decode()
                for i in range(4):
                    out[i] = 0

        self.fn = api.RNG_FN(draw)


def create_proof_native(params, rng, transcript, p_poly, p_blind: int, x3: int, s_poly, s_blind: int):
    """The same opening through the single C entry point `trh_ipa_create_proof` (csrc/ipa.hip): the round loop
    and all host-side scalar arithmetic run in C++, the transcript and randomness are callbacks.  rng: a callable returning canonical ints, or
    an RngScalarFn (the library's own stream); s_poly: host limbs (uploaded here) or a device tensor (one filled by api.Rng.fill, say).
    transcript: a transcript.Blake2bWrite hands the library its own three functions, so the round loop never enters the interpreter (its
    latched error, if any, is raised when the call has returned); any other writer is called through three closures."""
    import ctypes

    import torch

    curve, k, n = params.curve, params.k, params.n
    sf = api.SCALAR_FIELD[curve]

    def limbs_of(ptr, count):
        return np.array([ptr[i] for i in range(count)], dtype=np.uint64)

    def put(ptr, limbs):
        for i in range(4):
            ptr[i] = int(limbs[i])

    native = isinstance(transcript, Blake2bWrite)
    if native:
        tr = transcript.callbacks()
    else:
        wp = api.WRITE_POINT_FN(lambda ctx, p: transcript.write_point(limbs_of(p, 12)))
        ws = api.WRITE_SCALAR_FN(lambda ctx, p: transcript.write_scalar(limbs_of(p, 4)))
        sq = api.SQUEEZE_FN(lambda ctx, out: put(out, _mont(sf, transcript.squeeze_challenge_scalar())))
        tr = api.Transcript(None, wp, ws, sq)
    rn = rng.fn if isinstance(rng, RngScalarFn) else api.RNG_FN(lambda ctx, out: put(out, _mont(sf, rng())))
    # (np.require copies only when s_poly is not already contiguous and writable: an unconditional .copy() of the 8 MiB was 1 ms of every k = 18 opening)
    s_dev = s_poly if isinstance(s_poly, torch.Tensor) else torch.from_numpy(np.require(s_poly, dtype=np.uint64, requirements=["C", "W"]).view(np.int64)).to(p_poly.device)
    out_c, out_f = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    u = np.ascontiguousarray(params.u, dtype=np.uint64).reshape(8)
    bases = params.ipa_bases() if hasattr(params, "ipa_bases") else params._g
    api._check(api.lib().trh_ipa_create_proof(bases.handle, api._p(u), k, api._devptr(p_poly), api._p(_mont(sf, p_blind)), api._p(_mont(sf, x3)),
                                              api._devptr(s_dev), api._p(_mont(sf, s_blind)), ctypes.byref(tr), rn, None, _stream(p_poly),
                                              api._p(out_c), api._p(out_f)))
    if isinstance(rng, RngScalarFn) and rng.error:
        raise api.TrhError(rng.error)
    if native:
        transcript.raise_if_failed()
    return _canon(sf, out_c), _canon(sf, out_f)


def create_proof(params, rng, transcript, p_poly, p_blind: int, x3: int, s_poly=None, s_blind: int | None = None):
    """p_poly: device tensor (n, 4) of coefficients (Montgomery limbs); p_blind, x3 canonical ints.
    s_poly (host numpy (n, 4), random with s(x3) = 0 enforced here) and s_blind default to rng draws."""
    import torch

    curve, k, n = params.curve, params.k, params.n
    sf = api.SCALAR_FIELD[curve]
    m = _MODULUS[sf]
    dev = p_poly.device
    st = _stream(p_poly)

    def dev_of(host_limbs):
        return torch.from_numpy(np.ascontiguousarray(host_limbs, dtype=np.uint64).view(np.int64).copy()).to(dev)

    # b = (1, x3, x3^2, ...)
    b = torch.empty((n, 4), dtype=torch.int64, device=dev)
    api.powers_dev(sf, b, n, _mont(sf, x3), stream=st)

    # s(X): random with a root at x3
    if s_poly is None:
        s_poly = np.stack([_mont(sf, rng()) for _ in range(n)])
    s_dev = dev_of(s_poly)
    s_at_x3 = _canon(sf, api.inner_product_dev(sf, s_dev, b, n, stream=st))
    c0 = (_canon(sf, s_poly[0]) - s_at_x3) % m
    s_dev[0] = dev_of(_mont(sf, c0))
    if s_blind is None:
        s_blind = rng()
    s_commitment = params.commit(s_dev, _mont(sf, s_blind))
    transcript.write_point(s_commitment)
    xi = transcript.squeeze_challenge_scalar()
    z = transcript.squeeze_challenge_scalar()

    # p'(X) = p(X) + xi s(X) - v,  v = p'(x3) before the subtraction
    p_prime = p_poly.clone()
    api.axpy_dev(sf, p_prime, s_dev, n, _mont(sf, xi), stream=st)
    v = _canon(sf, api.inner_product_dev(sf, p_prime, b, n, stream=st))
    p0 = (_canon(sf, p_prime[0].cpu().numpy().view(np.uint64)) - v) % m
    p_prime[0] = dev_of(_mont(sf, p0))
    f = (s_blind * xi + p_blind) % m

    # G' starts as a private copy of params.g (n points); u and w are the last two bases of the 2-term MSMs
    g_prime = torch.empty((n, 8), dtype=torch.int64, device=dev)
    g_host = params._g.download(0, n)
    g_prime.copy_(dev_of(g_host))
    uw = api.Bases.from_host(curve, np.concatenate([np.asarray(params.u, dtype=np.uint64).reshape(1, 8), params.w]))
    gp = api.Bases.wrap_device(curve, g_prime, n)

    for j in range(k):
        half = 1 << (k - j - 1)
        l_j = gp.msm_dev(p_prime[half:2 * half], half, offset=0, stream=st)          # <p'[half..], G'[..half]>
        r_j = gp.msm_dev(p_prime[:half], half, offset=half, stream=st)               # <p'[..half], G'[half..]>
        value_l = _canon(sf, api.inner_product_dev(sf, p_prime[half:2 * half], b[:half], half, stream=st))
        value_r = _canon(sf, api.inner_product_dev(sf, p_prime[:half], b[half:2 * half], half, stream=st))
        l_rand, r_rand = rng(), rng()
        l_j = api.point_sum(curve, np.stack([l_j, uw.msm(np.stack([_mont(sf, value_l * z % m), _mont(sf, l_rand)]))]))
        r_j = api.point_sum(curve, np.stack([r_j, uw.msm(np.stack([_mont(sf, value_r * z % m), _mont(sf, r_rand)]))]))
        transcript.write_point(l_j)
        transcript.write_point(r_j)
        u_j = transcript.squeeze_challenge_scalar()
        u_inv = pow(u_j, -1, m)
        # collapse p', b and the generators
        api.axpy_dev(sf, p_prime[:half], p_prime[half:2 * half], half, _mont(sf, u_inv), stream=st)
        api.axpy_dev(sf, b[:half], b[half:2 * half], half, _mont(sf, u_j), stream=st)
        api.bases_fold_dev(curve, g_prime[:half], g_prime[half:2 * half], half, _mont(sf, u_j), stream=st)
        f = (f + l_rand * u_inv + r_rand * u_j) % m

    c = _canon(sf, p_prime[0].cpu().numpy().view(np.uint64))
    transcript.write_scalar(_mont(sf, c))
    transcript.write_scalar(_mont(sf, f))
    return c, f


# ---------------------------------------------------------------------------------------
# The verifier's arithmetic: halo2_proofs 0.2.0 poly/commitment/{msm.rs, verifier.rs} (reference call site
# /root/reference/src/test_utils.rs:52-68).  Transcript reading and challenge squeezing stay with the caller: the functions below
# take the already-parsed proof.  Scalars are canonical ints, points 8-limb affine PODs (all-zero = identity).
# ---------------------------------------------------------------------------------------
class MSM:
    """poly::commitment::msm::MSM over the opening's resident base set (params.ipa_bases(): g || w, or g || w || u with its
    fixed-base tables -- no second copy of g goes to the device).  The g scalars stay in device memory (csrc/ipaverify.hip)."""

    def __init__(self, params, stream=None):
        import ctypes
        self.params, self.curve, self.k, self.n = params, params.curve, params.k, params.n
        self.sf = api.SCALAR_FIELD[self.curve]
        self.stream = stream
        self.handle = api._vp()
        u = np.ascontiguousarray(params.u, dtype=np.uint64).reshape(8)
        api._check(api.lib().trh_ipa_msm_create(params.ipa_bases().handle, params.k, api._p(u), ctypes.byref(self.handle)))

    def _m(self, v):
        return _mont(self.sf, v)

    def append_term(self, scalar: int, point_xy):
        api._check(api.lib().trh_ipa_msm_append_term(self.handle, api._p(self._m(scalar)), api._p(api._c(point_xy).reshape(8))))

    def add_constant_term(self, c: int):
        api._check(api.lib().trh_ipa_msm_add_constant_term(self.handle, api._p(self._m(c))))

    def add_to_w_scalar(self, s: int):
        api._check(api.lib().trh_ipa_msm_add_to_w_scalar(self.handle, api._p(self._m(s))))

    def add_to_u_scalar(self, s: int):
        api._check(api.lib().trh_ipa_msm_add_to_u_scalar(self.handle, api._p(self._m(s))))

    def add_to_g_scalars_dev(self, scalars_dev):
        """scalars_dev: 2^k Montgomery scalars in device memory (torch tensor, DeviceBuffer or pointer)"""
        api._check(api.lib().trh_ipa_msm_add_to_g_scalars_dev(self.handle, api._devptr(scalars_dev), self.stream))

    def use_challenges(self, challenges, neg_cs, weights=None, alpha=None):
        """g <- alpha g + sum_p weights[p] neg_cs[p] s(challenges[p]) in one pass (Guard::use_challenges for one guard and no
        weights / alpha; challenges[p]: the k round challenges of guard p)"""
        u = np.stack([self._m(v) for row in challenges for v in row])
        nc = np.stack([self._m(v) for v in neg_cs])
        assert u.shape[0] == len(neg_cs) * self.k
        wt = None if weights is None else np.stack([self._m(v) for v in weights])
        al = None if alpha is None else self._m(alpha)
        api._check(api.lib().trh_ipa_msm_use_challenges(self.handle, len(neg_cs), api._p(u), api._p(nc), None if wt is None else api._p(wt),
                                                        None if al is None else api._p(al), self.stream))

    def scale(self, factor: int):
        api._check(api.lib().trh_ipa_msm_scale(self.handle, api._p(self._m(factor)), self.stream))

    def add_msm(self, other: "MSM"):
        api._check(api.lib().trh_ipa_msm_add_msm(self.handle, other.handle, self.stream))

    def eval(self):
        """MSM::eval -> (is_identity, the point as normalised Jacobian (12,) limbs)"""
        import ctypes
        flag = ctypes.c_int(0)
        out = np.zeros(12, dtype=np.uint64)
        api._check(api.lib().trh_ipa_msm_eval(self.handle, self.stream, ctypes.byref(flag), api._p(out)))
        return bool(flag.value), out

    def g_scalars(self):
        """the 2^k g scalars (Montgomery limbs, (n, 4)) or None while the accumulator has no g part"""
        ptr = api.lib().trh_ipa_msm_g_scalars_dev(self.handle)
        if not ptr:
            return None
        api._check(api.lib().trh_stream_synchronize(self.stream))
        out = np.empty((self.n, 4), dtype=np.uint64)
        api._check(api.lib().trh_memcpy_d2h(out.ctypes.data_as(api._vp), api._vp(ptr), out.nbytes))
        return out

    def destroy(self):
        if self.handle:
            api.lib().trh_ipa_msm_destroy(self.handle)
            self.handle = api._vp()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def compute_b(sf: str, x: int, u) -> int:
    """poly/commitment/verifier.rs compute_b: prod_j (1 + u_{k-1-j} x^(2^j)), O(k) on the host"""
    m = _MODULUS[sf]
    tmp, cur = 1, x % m
    for u_j in reversed(u):
        tmp = tmp * (1 + u_j * cur) % m
        cur = cur * cur % m
    return tmp


class Guard:
    """poly::commitment::verifier::Guard: the MSM's host-side terms with neg_c and the challenges; use_challenges() makes the MSM"""

    def __init__(self, params, terms, constant: int, w_scalar: int, u_scalar: int, neg_c: int, u):
        self.params, self.terms, self.constant = params, terms, constant
        self.w_scalar, self.u_scalar, self.neg_c, self.u = w_scalar, u_scalar, neg_c, list(u)

    def _fill(self, msm: MSM, weight: int = 1):
        m = _MODULUS[msm.sf]
        for s, pt in self.terms:
            msm.append_term(s * weight % m, pt)
        msm.add_to_w_scalar(self.w_scalar * weight % m)
        msm.add_to_u_scalar(self.u_scalar * weight % m)

    def use_challenges(self, stream=None) -> MSM:
        msm = MSM(self.params, stream)
        self._fill(msm)
        msm.add_constant_term(self.constant)
        msm.use_challenges([self.u], [self.neg_c])
        return msm


def verify_proof(params, p_terms, v: int, x3: int, s_commitment, xi: int, z: int, rounds, c: int, f: int) -> Guard:
    """the arithmetic of poly/commitment/verifier.rs verify_proof on the parsed proof: p_terms = [(scalar, point)] of P (the multiopen
    verifier's commitments; [(1, P)] for one), v = P(x3), S, xi, z, rounds = [(L_j, R_j, u_j)], c, f.  Returns the guard."""
    m = _MODULUS[api.SCALAR_FIELD[params.curve]]
    terms = [(s % m, pt) for s, pt in p_terms] + [(xi % m, s_commitment)]
    for l_j, r_j, u_j in rounds:
        terms += [(pow(u_j, -1, m), l_j), (u_j % m, r_j)]
    u = [u_j for _, _, u_j in rounds]
    neg_c = -c % m
    b = compute_b(api.SCALAR_FIELD[params.curve], x3, u)
    return Guard(params, terms, -v % m, -f % m, neg_c * b % m * z % m, neg_c, u)


def batch_msm(params, guards, weights, stream=None) -> MSM:
    """sum_p weights[p] guards[p].use_challenges() as ONE accumulator: the guards' g parts in one pass over the 2^k vector.
    BatchVerifier::finalize folds acc = r_p acc + msm_p, i.e. weights[p] = prod_{q > p} r_q."""
    m = _MODULUS[api.SCALAR_FIELD[params.curve]]
    acc = MSM(params, stream)
    const = 0
    for g, w in zip(guards, weights):
        g._fill(acc, w)
        const = (const + g.constant * w) % m
    acc.add_constant_term(const)
    acc.use_challenges([g.u for g in guards], [g.neg_c for g in guards], weights=list(weights))
    return acc


def batch_verify(params, guards, weights, stream=None) -> bool:
    """the arithmetic of BatchVerifier::finalize: the weighted sum of the guards' MSMs is the identity"""
    acc = batch_msm(params, guards, weights, stream)
    ok, _ = acc.eval()
    acc.destroy()
    return ok
