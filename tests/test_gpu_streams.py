"""GPU tests (-m gpu) of the layer between the kernels and the real hosts: every `*_dev` entry of include/trh.h takes a `void* stream`, the
production hosts (the Rust shim, examples/replay.cpp, replay.py --overlap) pass a NON-BLOCKING stream there, and the rest of this suite
passes the null stream almost everywhere.  Two properties are pinned here.

A. Stream fidelity (test_entry_rides_the_callers_stream, one row of ROWS per stream-taking entry): every launch, hipMemcpyAsync and
   hipMemsetAsync inside an entry rides the caller's stream.  A site that lands on the null stream is right in every null-stream test.
B. Ordering through the context (test_b*): Enter::begin / ~Enter (csrc/capi.hip, order_ev / last_stream in csrc/ctx.h) make a call on
   another stream than the context's previous one wait for it; the stream-less entries (trh_memcpy_d2h / _h2d, trh_free, trh_expr_set_const)
   and the shared scratch rest on that one hipStreamWaitEvent.

The method, the same in every case: a delay window on a non-blocking side stream S (torch.cuda.Stream()).
  1. warm up: the entry once on the null stream with the real input (tables, scratch sizes, function attributes: nothing of that may
     synchronise later); its result is kept;
  2. prefill the entry's input with VALID BUT DIFFERENT data (zeros for field vectors, the all-zero identity for points, a second valid
     vector for lookups) and zero its outputs; synchronise the device;
  3. on S: a delay kernel (torch.cuda._sleep), a torch event E behind it, the copies of the real input over the prefill from device
     staging tensors, and a zeroing of the separate output buffers (so that a misplaced LAST kernel is overwritten as well);
  4. the entry with stream = S.cuda_stream, no host synchronisation before it;
  5. the window check: `not E.query()` on the line after the call (entries that do not synchronise) or the line before it (entries that
     synchronise the stream: they return a value to the host, or stage a caller's host array -- the row says which).  The delay was still
     running, so whatever the entry put on another stream ran against the prefill.  A closed window fails the test, it never skips;
  6. outputs are copied on S, S is synchronised, and everything is compared bit for bit: with the oracle (oracle/cpu_ref, oracle/pasta)
     where it has the operation, with the warm-up result of step 1 for the composite entries, which named existing tests pin to the
     oracle (the row names the test): ordering is under test here, not arithmetic.
What a row of a synchronising entry covers.  Behind the entry's FIRST hipStreamSynchronize the delay is over and S has written the real
input, so a launch misplaced after that point reads right data and the row stays green.  Covered in full (the only synchronisation is the
read-back at the end): inner_product, eval_batch, msm-4098, msm-2^14, msm_batch-2, msm_halves, perm_check, decompress-first_bad,
ipa_collapse, ipa_msm-eval.  Covered up to a synchronisation in the middle: msm-2^14-tabled (to the sampler's vote), msm_batch-9 (to the
chunk's first read-back), ipa_create_proof (to the finish of round 0's MSM), lookup (to the read-back of the tie and miss flags), expr
(the first evaluation; the second is there for trh_expr_set_const).  Covered for the staging copy ALONE, because the entry drains the
stream before its compute kernel: scale, scale_periodic, scale_rows, product_terms, lincomb, commit_batch, point_fft -- their rows say
so.  For these the claim of A is pinned for the copy only: about the stream of their kernels this module says nothing.

The negative controls (test_control_*) repeat 2 - 3 and call trh_ntt_dev / trh_msm_dev with stream = None on purpose: the answer is the
oracle's answer FOR THE PREFILL while the window is still open, so the null stream really does not wait for S on this machine and a
positive case cannot pass by accident.

Entries that stage a small constant through the context's pinned ring (trh_field_axpy_dev, trh_field_powers_dev, trh_bases_fold_dev) drain the
device on every 64th such call of a context (csrc/ipa.hip stage_constant, the ring's wrap-around).  A row marked `ring` whose window is
found closed after the call is therefore run once more -- two consecutive calls cannot both wrap -- and the second window must be open;
the result of the first attempt is compared all the same.  This is a finding about the library rather than a property of the test: three
entries documented as asynchronous drain the whole device now and then, the ring's position is visible through no stat, and an entry that
synchronised now and then for ANOTHER reason would pass these three rows too.

Which side streams.  Streams that nothing orders can still share ONE hardware queue: the runtime spreads its streams over
GPU_MAX_HW_QUEUES of them (four by default) and torch's pool alone has 32.  On a stream that shares the null stream's queue a misplaced
kernel queues behind the delay and the fill all the same, every case is blind and the controls fail (seen on the MI355X: about one pool
stream in four).  _window() therefore probes torch's pool for three streams A, B, C that overlap with the null stream and with each other
(_overlap: work on one completes while the other is held by a short delay), and every case uses those.  The limit of that: the null
stream and A, B, C take four distinct hardware queues, which is all the runtime's default has, so a runtime that hands out queues
otherwise (or fewer of them) fails _window()'s assertion -- loudly, never as a skip -- and a launch misplaced on a stream INSIDE the
library (the context's own stream, the staging streams) that happens to share A's queue would still queue behind the delay and stay
invisible; only launches that land on the null stream, or on a queue other than S's, are caught.

The delay is measured, not guessed: _window() times torch.cuda._sleep with events and sizes the spin to DELAY_MS of device time.
Measured on an MI355X at the parent commit: the longest host-side enqueue sequence of any case (fill, call, read-back enqueue;
perf_counter) is 0.181 ms (ntt-12-b1; 0.156 ms, ipa_msm-use_challenges-vesta, in a second run; most rows take 0.05 - 0.11 ms); the delay
is 20 ms of device time; the ratio is 110.  Fifty times the sequence would be 9 ms: the rest is room for a host that stalls for a few
milliseconds between the fill and the check, at 1.6 s of spinning for the whole module (it runs in about 6 s).  The module prints the
figures of its own run when it ends (pytest -s).
"""
import ctypes
import functools
import os
import random
import re
import time
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# milliseconds of device time every case spins for, and what it was sized against (see the docstring)
DELAY_MS = 20.0

EINVAL = -1
TIMES = {}            # row -> host seconds from the first enqueue on S to the end of the host-side sequence
_FAULT = []           # a HIP error seen by an earlier case: nothing more is started on the device


# ---------------------------------------------------------------------------------------------------------------------------------------------
# helpers (everything that needs torch / the library is imported inside, so that the completeness test runs without a device)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _mods():
    import torch

    import cpu_ref
    import pasta as o
    from tiny_ram_halo2_amd import api, synth
    return SimpleNamespace(torch=torch, cpu_ref=cpu_ref, o=o, api=api, synth=synth, lib=api.lib())


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64).copy() if a.dtype == np.uint64 else a.copy()).cuda()


def host(t):
    c = t.cpu().numpy()
    return c.view(np.uint64) if c.dtype == np.int64 else c


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def limbs(field, v):
    import pasta as o
    f = o.FIELDS[field]
    return np.array(f.limbs(v % f.m), np.uint64)


def rows_of(field, vals):
    import pasta as o
    f = o.FIELDS[field]
    return np.array([f.limbs(v % f.m) for v in vals], np.uint64).reshape(-1, 4)


def ints_of(field, a):
    import pasta as o
    f = o.FIELDS[field]
    return [f.from_limbs(r) for r in np.asarray(a, np.uint64).reshape(-1, 4)]


def stored_rows(vals):
    import pasta as o
    return np.array([o.int_to_limbs(v) for v in vals], np.uint64).reshape(-1, 4)


def ck(rc):
    from tiny_ram_halo2_amd import api
    api._check(rc)
    return []


class Run:
    """One case, built on the device: its buffers, its call and what the result is compared with."""

    def __init__(self):
        self.inputs, self.outputs, self.keep = [], [], []
        self.want = None                      # the oracle's answer (host results of the call, then the outputs); None: the warm-up result
        self.prepare = lambda: None           # before each of the two runs, on the null stream: handles back to their starting state
        self.call = None                      # call(stream, window) -> list of host arrays; `window` is the check, for calls that place it themselves
        self.late = lambda: []                # host arrays read after S has been synchronised (state kept inside a handle)
        self.view = lambda arrs: arrs         # what of the results is compared (the affine part of a normalised Jacobian point, say)

    def inp(self, real, prefill=None):
        real_d = dev(real)
        pre_d = real_d.new_zeros(real_d.shape) if prefill is None else dev(prefill)
        buf = real_d.clone()
        self.inputs.append((buf, real_d, pre_d))
        return buf

    def out(self, shape, dtype=None):
        import torch
        t = torch.zeros(shape, dtype=dtype or torch.int64, device="cuda")
        self.outputs.append(t)
        return t

    def inout(self, real, prefill=None):
        buf = self.inp(real, prefill)
        self.outputs.append(buf)
        return buf

    def separate_outputs(self):
        ins = {b.data_ptr() for b, _, _ in self.inputs}
        return [t for t in self.outputs if t.data_ptr() not in ins]


def _overlap(x, y, ticks):
    """whether work on stream x runs while stream y is held by a delay.  Two streams that nothing orders can still be served by ONE hardware
    queue (the runtime spreads its streams over GPU_MAX_HW_QUEUES of them, four by default), and then they run in the order of submission"""
    import torch
    held, ran = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(y):
        torch.cuda._sleep(ticks)
        held.record(y)
    with torch.cuda.stream(x):
        probe = torch.zeros(16, dtype=torch.int64, device="cuda")
        probe.add_(1)
        ran.record(x)
    ran.synchronize()
    free = not held.query()
    y.synchronize()
    return free


@functools.lru_cache(maxsize=None)
def _window():
    """the spin that lasts DELAY_MS on this device (torch.cuda._sleep counts ticks of a clock whose rate is not ours to know), and three
    non-blocking streams A, B, C that overlap with the null stream and with each other: without that a kernel misplaced on the null stream
    would queue behind the delay all the same, and every case would be blind"""
    import torch
    from tiny_ram_halo2_amd import api
    api.init(0)
    ticks = 2_000_000
    torch.cuda._sleep(ticks)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(ticks)
    e1.record()
    e1.synchronize()
    per_ms = ticks / e0.elapsed_time(e1)
    null, chosen, seen = torch.cuda.default_stream(), [], set()
    for _ in range(64):
        c = torch.cuda.Stream()  # torch hands out the streams of its pool in turn
        if c.cuda_stream in seen:
            break
        seen.add(c.cuda_stream)
        with torch.cuda.stream(c):  # first use of the stream, and of the kernels the cases enqueue on it
            torch.zeros(16, dtype=torch.uint8, device="cuda").clone().zero_()
        c.synchronize()
        if all(_overlap(c, other, int(3 * per_ms)) and _overlap(other, c, int(3 * per_ms)) for other in [null] + chosen):
            chosen.append(c)
        if len(chosen) == 3:
            break
    assert len(chosen) == 3, (f"of {len(seen)} torch streams only {len(chosen)} overlap with the null stream and with each other: the cases need three "
                              "(four hardware queues, the runtime's default)")
    return SimpleNamespace(ticks=int(DELAY_MS * per_ms), per_ms=per_ms, A=chosen[0], B=chosen[1], C=chosen[2])


def on_the_device(test):
    """every GPU case of this module: nothing is started on the device once a case has met a HIP error (a fault makes every later call fail,
    and programs that went on after one have cost whole machines), and a HIP error met here is remembered for the cases that follow"""
    @functools.wraps(test)
    def guarded(*args, **kwargs):
        if _FAULT:
            pytest.fail("an earlier case of this module met a HIP error (%s): nothing more is started on the device" % _FAULT[0])
        try:
            return test(*args, **kwargs)
        except Exception as exc:
            text = str(exc)
            if "libtrh error -3" in text or "HIP error" in text or "hipError" in text or "illegal memory access" in text:
                _FAULT.append(text[:200])
            raise
    return pytest.mark.gpu(guarded)


def delayed_fill(S, run, extra=()):
    """step 3: on S the delay, the event behind it, the real inputs over the prefill, zeros over the separate outputs"""
    import torch
    E = torch.cuda.Event()
    with torch.cuda.stream(S):
        torch.cuda._sleep(_window().ticks)
        E.record(S)
        for buf, real, _ in run.inputs:
            buf.copy_(real, non_blocking=True)
        for t in list(run.separate_outputs()) + list(extra):
            t.zero_()
    return E


def prefill(run):
    import torch
    for buf, _, pre in run.inputs:
        buf.copy_(pre)
    for t in run.separate_outputs():
        t.zero_()
    run.prepare()
    torch.cuda.synchronize()


def equal_lists(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, i, g.shape, w.shape)
        if not (g == w).all():
            flat = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1)) if g.ndim > 1 else np.flatnonzero(g != w)
            raise AssertionError(f"{what}: result {i} differs in {flat.size} of {g.shape[0] if g.ndim else 1} rows, first at {int(flat[0])}"
                                 + ("; it is all zero (the prefill's answer, or a poisoned output)" if not g.any() else ""))


def drive(name, run, sync, ring=False):
    """steps 1 - 6 of the module docstring for one Run"""
    import torch
    S = _window().A
    # 1. warm up on the null stream with the real input
    for buf, real, _ in run.inputs:
        buf.copy_(real)
    for t in run.separate_outputs():
        t.zero_()
    run.prepare()
    torch.cuda.synchronize()
    res = run.call(None, lambda: True)
    torch.cuda.synchronize()
    warm = run.view(list(res) + [host(t) for t in run.outputs] + list(run.late()))
    want = warm if run.want is None else [np.asarray(w) for w in run.want]
    if run.want is not None:
        equal_lists(warm, want, f"{name}: the warm-up call on the null stream against the oracle (arithmetic, not ordering)")
    for attempt in range(2 if ring else 1):
        # 2. prefill, 3. delay + event + fill on S
        prefill(run)
        checked, stamps = [], []

        def window():
            checked.append(not E.query())
            stamps.append(time.perf_counter())
            return checked[-1]

        t0 = time.perf_counter()
        E = delayed_fill(S, run)
        try:
            # 4. the call, 5. the window check before or after it
            if sync:
                open_ = window()
                t1 = time.perf_counter()
                assert open_, f"{name}: the delay of {DELAY_MS} ms had ended before the call was made ({(t1 - t0) * 1e3:.2f} ms of host time)"
                res = run.call(S.cuda_stream, window)
            else:
                res = run.call(S.cuda_stream, window)
                mid = bool(checked)                  # the call placed the check itself, before its synchronising half
                open_ = checked[-1] if mid else window()
            with torch.cuda.stream(S):
                outs = [t.clone() for t in run.outputs]
            if not sync:
                t1 = stamps[0] if mid else time.perf_counter()
        finally:
            S.synchronize()
        TIMES[name] = max(TIMES.get(name, 0.0), t1 - t0)
        # 6. bit for bit (a ring row's first attempt as well, whatever its window was)
        got = run.view(list(res) + [host(t) for t in outs] + list(run.late()))
        equal_lists(got, want, f"{name} on a non-blocking stream behind a delay")
        if open_ or not ring or attempt == 1:
            break
    assert open_, (f"{name}: the window was closed when the call returned ({(t1 - t0) * 1e3:.2f} ms of host time, delay {DELAY_MS} ms): the entry "
                   "synchronised, or the host was slower than the delay")
    assert all(checked), name


# ---------------------------------------------------------------------------------------------------------------------------------------------
# A. the rows.  Builders run on the device; each returns a Run.
# ---------------------------------------------------------------------------------------------------------------------------------------------
FID = {"fp": 0, "fq": 1}
CID = {"pallas": 0, "vesta": 1}
SCALAR = {"pallas": "fq", "vesta": "fp"}
BASE = {"pallas": "fp", "vesta": "fq"}


def elems(seed, n):
    from tiny_ram_halo2_amd import synth
    return synth.field_elements(0x57E4 + seed, n)


@functools.lru_cache(maxsize=None)
def gen_bases(curve, n, seed=31):
    """n structured bases from the C++ oracle (host array; never written to)"""
    import cpu_ref
    a = cpu_ref.gen_bases(curve, seed, 7, n, threads=4)
    a.setflags(write=False)
    return a


def jacobian(curve, xy):
    xy = np.asarray(xy, np.uint64).reshape(-1, 8)
    return np.concatenate([xy, np.tile(limbs(BASE[curve], 1), (xy.shape[0], 1))], axis=1)


def b_field_op(field):
    m, n, r = _mods(), 1000, Run()
    a_h, b_h = elems(1, n), elems(2, n)
    a, b, out = r.inp(a_h), r.inp(b_h), r.out((n, 4))
    r.call = lambda s, w: ck(m.lib.trh_field_op_dev(FID[field], m.api.FIELD_OPS["mul"], P(a), P(b), P(out), n, s))
    r.want = [m.cpu_ref.field_op(field, "mul", a_h, b_h)]
    return r


def b_point_op(curve):
    m, n, r = _mods(), 100, Run()
    p_h, q_h = jacobian(curve, gen_bases(curve, 2 * n)[:n]), jacobian(curve, gen_bases(curve, 2 * n)[n:])
    p, q, out = r.inp(p_h), r.inp(q_h), r.out((n, 12))
    r.call = lambda s, w: ck(m.lib.trh_point_op_dev(CID[curve], m.api.POINT_OPS["add"], P(p), P(q), P(out), n, s))
    r.view = lambda arrs: [a[:, :8] for a in arrs]
    r.want = [np.stack([m.cpu_ref.to_affine(curve, m.cpu_ref.point_op(curve, "add", p_h[i], q_h[i])) for i in range(n)])]
    return r


def b_scale(kind, field):
    m, r = _mods(), Run()
    rows, row_len, active = (3, 64, 50) if kind == "rows" else (1, 1000, 1000)
    fac = rows_of(field, [0xC0FFEE] if kind == "scale" else [1, 0xC0FFEE, 0xBEEF11])
    a_h = elems(3, rows * row_len)
    a = r.inout(a_h)
    if kind == "scale":
        r.call = lambda s, w: ck(m.lib.trh_field_scale_dev(FID[field], P(a), rows * row_len, m.api._p(fac), s))
    elif kind == "periodic":
        r.call = lambda s, w: ck(m.lib.trh_field_scale_periodic_dev(FID[field], P(a), rows * row_len, m.api._p(fac), 3, s))
    else:
        r.call = lambda s, w: ck(m.lib.trh_field_scale_rows_dev(FID[field], P(a), rows, row_len, active, m.api._p(fac), 3, s))
    full = np.tile(fac, (row_len, 1))[:active]
    want = a_h.reshape(rows, row_len, 4).copy()
    for i in range(rows):
        want[i, :active] = m.cpu_ref.field_op(field, "mul", want[i, :active], full)
    r.want = [want.reshape(-1, 4)]
    return r


def b_ntt(field, log_n, batch):
    m, r = _mods(), Run()
    n = 1 << log_n
    a_h = elems(4 + log_n, batch * n).reshape(batch, n, 4)
    omega = limbs(field, m.o.FIELDS[field].omega(log_n))
    a = r.inout(a_h)
    r.call = lambda s, w: ck(m.lib.trh_ntt_dev(FID[field], P(a), log_n, m.api._p(omega), batch, s))
    r.want = [np.stack([m.cpu_ref.best_fft(field, a_h[i], omega, log_n, threads=4) for i in range(batch)])]
    return r


def b_domain(op, field, k):
    """EvaluationDomain::new(j = 3, k): quotient degree 2, extended_k = k + 1, two coset blocks; batch 2.  k = 8 runs the unfused passes,
    k = 11 the fused ones (ntt_can_fuse)"""
    from tiny_ram_halo2_amd import poly
    m, r, batch = _mods(), Run(), 2
    d = poly.EvaluationDomain(field, 3, k)
    h, n, en, nb = d.handle(), 1 << k, d.extended_len(), d.quotient_poly_degree
    r.keep.append(d)
    lib = m.lib
    if op == "lagrange_to_coeff":
        a = r.inout(elems(20, batch * n).reshape(batch, n, 4))
        r.call = lambda s, w: ck(lib.trh_domain_lagrange_to_coeff(h, P(a), batch, s))
    elif op == "coeff_to_extended":
        a, e = r.inp(elems(21, batch * n).reshape(batch, n, 4)), r.out((batch, en, 4))
        r.call = lambda s, w: ck(lib.trh_domain_coeff_to_extended(h, P(a), P(e), batch, s))
    elif op == "extended_to_coeff":
        a = r.inout(elems(22, batch * en).reshape(batch, en, 4))
        r.call = lambda s, w: ck(lib.trh_domain_extended_to_coeff(h, P(a), batch, s))
    elif op == "divide_by_vanishing_poly":
        a = r.inout(elems(23, batch * en).reshape(batch, en, 4))
        r.call = lambda s, w: ck(lib.trh_domain_divide_by_vanishing_poly(h, P(a), batch, s))
    elif op == "coeff_to_extended_blocks":
        assert nb == int(lib.trh_domain_quotient_blocks(h)) == 2
        a, e = r.inp(elems(24, batch * n).reshape(batch, n, 4)), r.out((batch, nb, n, 4))
        r.call = lambda s, w: ck(lib.trh_domain_coeff_to_extended_blocks(h, P(a), P(e), batch, nb, s))
    else:
        a, q = r.inp(elems(25, nb * n).reshape(nb, n, 4)), r.out((nb * n, 4))  # the numerator is overwritten: scratch afterwards
        r.call = lambda s, w: ck(lib.trh_domain_blocks_to_quotient(h, P(a), P(q), 1, s))
    return r


def b_inner_product(field):
    m, n, r = _mods(), 70000, Run()
    a_h, b_h = elems(30, n), elems(31, n)
    a, b = r.inp(a_h), r.inp(b_h)
    out = np.zeros(4, np.uint64)

    def call(s, w):
        ck(m.lib.trh_field_inner_product_dev(FID[field], P(a), P(b), n, s, m.api._p(out)))
        return [out.copy()]
    r.call = call
    from common import stored_ints
    r.want = [stored_rows([sum(stored_ints(m.cpu_ref.field_op(field, "mul", a_h, b_h))) % m.o.FIELDS[field].m])[0]]  # the stored form is linear
    return r


def b_eval_batch(field):
    m, n, batch, r = _mods(), 4097, 3, Run()
    a_h, x = elems(32, batch * n).reshape(batch, n, 4), limbs(field, 0x1234567890ABCDEF0123)
    a = r.inp(a_h)
    r.call = lambda s, w: [m.api.poly_eval_batch_dev(field, a, n, batch, x, stream=s)]
    r.want = [np.stack([m.cpu_ref.eval_polynomial(field, a_h[i], x) for i in range(batch)])]
    return r


def b_axpy(field):
    m, n, r = _mods(), 1000, Run()
    y_h, x_h, c = elems(33, n), elems(34, n), limbs(field, 0xC0FFEE77)
    y, x = r.inout(y_h), r.inp(x_h)
    r.call = lambda s, w: ck(m.lib.trh_field_axpy_dev(FID[field], P(y), P(x), n, m.api._p(c), s))
    r.want = [m.cpu_ref.field_op(field, "add", y_h, m.cpu_ref.field_op(field, "mul", x_h, np.tile(c, (n, 1))))]
    return r


def b_powers(field):
    """no device input: the window shows in the output alone -- S zeroes it behind the delay, the entry's kernel has to come after that"""
    m, n, r = _mods(), 1000, Run()
    f, x = m.o.FIELDS[field], 0x123456789ABCDEF
    out = r.out((n, 4))
    xl = limbs(field, x)
    r.call = lambda s, w: ck(m.lib.trh_field_powers_dev(FID[field], P(out), n, m.api._p(xl), s))
    r.want = [rows_of(field, [pow(x, i, f.m) for i in range(n)])]
    return r


def b_batch_invert(field, mul):
    m, n, r = _mods(), 16385, Run()
    a_h, num_h = elems(35, n), elems(36, n)
    a = r.inout(a_h)
    inv = m.cpu_ref.field_op(field, "inv", a_h)
    if mul:
        num = r.inp(num_h)
        r.call = lambda s, w: ck(m.lib.trh_field_batch_invert_mul_dev(FID[field], P(a), P(num), n, s))
        r.want = [m.cpu_ref.field_op(field, "mul", num_h, inv)]
    else:
        r.call = lambda s, w: ck(m.lib.trh_field_batch_invert_dev(FID[field], P(a), n, s))
        r.want = [inv]
    return r


def b_product_terms(field):
    m, n, r = _mods(), 1000, Run()
    cols_h = [elems(40 + i, n) for i in range(4)]
    cols = [r.inp(c) for c in cols_h]
    out = r.out((2, n, 4))
    c1, g1, g2 = limbs(field, 0xBE7A), limbs(field, 0x6A44A), limbs(field, 77)
    rows = [[(cols[0], cols[1], c1, g1), (cols[2], None, None, g2)], [(cols[3], cols[0], c1, g2)]]
    r.call = lambda s, w: m.api.product_terms_dev(field, rows, n, out, stream=s) or []
    fo = m.cpu_ref.field_op

    def term(x, y, c, g):
        t = x if y is None else fo(field, "add", x, fo(field, "mul", y, np.tile(c, (n, 1))))
        return fo(field, "add", t, np.tile(g, (n, 1)))
    r.want = [np.stack([fo(field, "mul", term(cols_h[0], cols_h[1], c1, g1), term(cols_h[2], None, None, g2)), term(cols_h[3], cols_h[0], c1, g2)])]
    return r


def b_scan(kind, field):
    from common import stored_ints
    m, n, r = _mods(), 4097, Run()
    rows = 2 if kind == "product_rows" else 1
    a_h = elems(45, rows * n).reshape(rows, n, 4)
    a, out = r.inp(a_h), r.out((rows, n, 4))
    if kind == "product":
        r.call = lambda s, w: ck(m.lib.trh_field_prefix_product_dev(FID[field], P(a), P(out), n, s))
    elif kind == "product_rows":
        r.call = lambda s, w: ck(m.lib.trh_field_prefix_product_rows_dev(FID[field], P(a), P(out), n, rows, s))
    else:
        r.call = lambda s, w: ck(m.lib.trh_field_prefix_sum_dev(FID[field], P(a), P(out), n, s))
    if kind == "sum":  # the stored form is linear: running sums of the stored words mod m
        mod, acc, vals = m.o.FIELDS[field].m, 0, []
        for v in stored_ints(a_h[0]):
            vals.append(acc)
            acc = (acc + v) % mod
        r.want = [stored_rows(vals).reshape(1, n, 4)]
    else:
        r.want = [np.stack([m.cpu_ref.prefix_product(field, a_h[i]) for i in range(rows)])]
    return r


def b_lincomb(field):
    m, n, batch, r = _mods(), 1000, 3, Run()
    a_h, co = elems(46, batch * n).reshape(batch, n, 4), rows_of(field, [0xA1, 0xB2B2B2B2B2, 0xC3C3C3C3C3C3C3C3C3])
    a, out = r.inp(a_h), r.out((n, 4))
    r.call = lambda s, w: ck(m.lib.trh_poly_lincomb_dev(FID[field], P(a), n, batch, m.api._p(co), P(out), s))
    want = np.zeros((n, 4), np.uint64)
    for i in range(batch):
        want = m.cpu_ref.field_op(field, "add", want, m.cpu_ref.field_op(field, "mul", a_h[i], np.tile(co[i], (n, 1))))
    r.want = [want]
    return r


def b_kate(field):
    m, n, r = _mods(), 4097, Run()
    f, z = m.o.FIELDS[field], 0x5EED5EED5EED5EED
    a_h = elems(47, n)
    a, q = r.inp(a_h), r.out((n - 1, 4))
    pz, pzinv = dev(rows_of(field, [pow(z, i, f.m) for i in range(n)])), dev(rows_of(field, [pow(z, -i, f.m) for i in range(n)]))
    scratch = dev(np.zeros((2 * n, 4), np.uint64))
    r.keep += [pz, pzinv, scratch]
    r.call = lambda s, w: ck(m.lib.trh_poly_kate_division_dev(FID[field], P(a), n, P(pz), P(pzinv), P(scratch), P(q), s))
    r.want = [rows_of(field, m.o.kate_division(f, ints_of(field, a_h), z))]
    return r


def b_lookup(batch, field):
    """4097 usable rows (three tiles of the sort, two blocks of its scans).  The prefill is a second valid input column: every value of it
    occurs in the table, so a misplaced kernel sorts other data and cannot fail the lookup"""
    m, n, r = _mods(), 4097, Run()
    f, rng = m.o.FIELDS[field], random.Random(0x100C + batch)
    nl = max(batch, 1)
    tables, ins, pres = [], [], []
    for _ in range(nl):
        distinct = [rng.randrange(f.m) for _ in range(n // 3)]
        table = [distinct[i % len(distinct)] for i in range(n)]
        rng.shuffle(table)
        tables.append(rows_of(field, table))
        ins.append(rows_of(field, rng.choices(distinct, k=n)))
        pres.append(rows_of(field, rng.choices(distinct[: len(distinct) // 2], k=n)))
    t = dev(np.stack(tables))
    a = r.inp(np.stack(ins), np.stack(pres))
    oa, os_ = r.out((nl, n, 4)), r.out((nl, n, 4))
    r.keep.append(t)
    if batch == 0:
        r.call = lambda s, w: ck(m.lib.trh_lookup_permute_dev(FID[field], P(a), P(t), n, P(oa), P(os_), s))
    else:
        r.call = lambda s, w: ck(m.lib.trh_lookup_permute_batch_dev(FID[field], P(a), P(t), n, n, nl, P(oa), P(os_), s))
    return r


def b_expr(blocks, field):
    """a gate whose evaluation keeps one stack entry in LDS (below the two register ones); constant 0 is the folding challenge, replaced
    through trh_expr_set_const BETWEEN two evaluations on S: that entry takes no stream and enters the context on the null stream"""
    from tiny_ram_halo2_amd import expr
    m, r = _mods(), Run()
    f = m.o.FIELDS[field]
    A = lambda i, rot=0: expr.Advice(i, rot)  # noqa: E731
    g = (A(0) + 1) * (A(1, 1) + 2) - A(2, -1)
    prog = expr.compile_gates(field, [g, -g * 3 + A(3)], 7)
    ev = expr.GateEvaluator(prog)
    assert expr._need(g) == 3 and ev.lds_slots() == 1
    log_n, nb = 5, 2
    rows = (nb << log_n) if blocks else (1 << log_n)
    cols = {key: r.inp(elems(50 + i, rows)) for i, key in enumerate(prog.columns)}
    out1, out2 = r.out((rows, 4)), r.out((rows, 4))
    y1, y2 = 7, (0x1234567 * 0x89ABCDEF) % f.m
    r.keep.append(ev)
    r.prepare = lambda: ev.set_challenge(y1)

    def call(s, w):
        for y, o_ in ((y1, out1), (y2, out2)):
            ev.set_challenge(y)
            if blocks:
                ev.eval_blocks(cols, log_n, nb, out=o_, stream=s)
            else:
                ev.eval(cols, log_n, 1, out=o_, stream=s)
        return []
    r.call = call
    return r


def b_point_fft(curve):
    m, k, r = _mods(), 6, Run()
    g_h = gen_bases(curve, 1 << k, seed=97)
    omega = limbs(SCALAR[curve], m.o.FIELDS[SCALAR[curve]].omega(k))
    g = r.inout(g_h)
    r.call = lambda s, w: ck(m.lib.trh_point_fft_dev(CID[curve], P(g), k, m.api._p(omega), None, s))
    r.want = [m.cpu_ref.best_fft_points(curve, g_h, omega, k)]
    return r


def b_bases_fold(curve):
    m, half, r = _mods(), 130, Run()
    g_h = gen_bases(curve, 2 * half, seed=17)
    u = limbs(SCALAR[curve], 0x1D0F5A7E9B3C2468ACE13579BDF02468ACE13579BDF0246)
    lo, hi = r.inout(g_h[:half]), r.inp(g_h[half:])
    r.call = lambda s, w: ck(m.lib.trh_bases_fold_dev(CID[curve], P(lo), P(hi), half, m.api._p(u), s))
    scaled = m.cpu_ref.scale_points_each(curve, g_h[half:], np.tile(u, (half, 1)), threads=4)
    lo_j = jacobian(curve, g_h[:half])
    r.want = [np.stack([m.cpu_ref.to_affine(curve, m.cpu_ref.point_op(curve, "madd", lo_j[i], scaled[i])) for i in range(half)])]
    return r


def b_sqrt(field):
    import encoding_cases as ec
    import torch
    m, r = _mods(), Run()
    a_h = ec.sqrt_input_limbs(field)
    n = a_h.shape[0]
    a, out, flags = r.inp(a_h), r.out((n, 4)), r.out((n,), torch.uint8)
    r.call = lambda s, w: ck(m.lib.trh_field_sqrt_dev(FID[field], P(a), P(out), P(flags), n, s))
    r.want = list(ec.sqrt_expected_limbs(field))
    return r


def b_compress(curve):
    import encoding_cases as ec
    import torch
    m, n, r = _mods(), 65, Run()
    xy_h = gen_bases(curve, n, seed=55).copy()
    xy_h[7] = 0  # an identity among them
    xy, by = r.inp(xy_h), r.out((n * 32,), torch.uint8)
    r.call = lambda s, w: ck(m.lib.trh_points_compress_dev(CID[curve], P(xy), P(by), n, s))
    r.want = [np.frombuffer(ec.encode_pods(curve, xy_h), np.uint8)]
    return r


def b_decompress(curve, first_bad):
    """without first_bad the entry does not synchronise; with it the smallest invalid index comes back through a copy on the stream"""
    import encoding_cases as ec
    import torch
    m, n, r = _mods(), 65, Run()
    xy_h = gen_bases(curve, n, seed=56).copy()
    xy_h[9] = 0
    enc = bytearray(ec.encode_pods(curve, xy_h))
    want_xy, want_ok, bad = xy_h.copy(), np.ones(n, np.uint8), n
    if first_bad:  # one invalid encoding: x = the modulus
        enc[32 * 40:32 * 41] = ec.enc_int(m.o.CURVES[curve].base.m)
        want_xy[40], want_ok[40], bad = 0, 0, 40
    by = r.inp(np.frombuffer(bytes(enc), np.uint8))
    xy, ok = r.out((n, 8)), r.out((n,), torch.uint8)
    fb = ctypes.c_uint64(0)

    def call(s, w):
        ck(m.lib.trh_points_decompress_dev(CID[curve], P(by), P(xy), P(ok), n, s, ctypes.byref(fb) if first_bad else None))
        return [np.array([fb.value if first_bad else n], np.uint64)]
    r.call = call
    r.want = [np.array([bad], np.uint64), want_xy, want_ok]
    return r


def b_rng(rows_form, field):
    m, r = _mods(), Run()
    rng = m.api.Rng(bytes(range(32)), 3)
    r.keep.append(rng)
    r.prepare = lambda: rng.seek(5)
    if rows_form:
        rows, row_len, first, count = 3, 100, 90, 7
        cols = r.inout(elems(60, rows * row_len).reshape(rows, row_len, 4))
        r.call = lambda s, w: ck(m.lib.trh_rng_fill_rows_dev(rng.handle, FID[field], P(cols), rows, row_len, first, count, s))
    else:
        n = 1000
        out = r.out((n, 4))
        r.call = lambda s, w: ck(m.lib.trh_rng_fill_dev(rng.handle, FID[field], P(out), n, s))
    return r


def b_perm(check, field):
    """sigma: the mapping's device copy is made by the warm-up call (the first device call after a copy synchronises once), the call under
    test is asynchronous and writes an output only.  check: the real columns break the copy constraints, the all-zero prefill satisfies them"""
    from tiny_ram_halo2_amd import permutation
    m, k, ncol, r = _mods(), 8, 3, Run()
    n = 1 << k
    asm = permutation.Assembly(field, k, ncol)
    rnd = random.Random(0x9E47)
    asm.copy_many([(rnd.randrange(ncol), rnd.randrange(n), rnd.randrange(ncol), rnd.randrange(n)) for _ in range(200)])
    r.keep.append(asm)
    if not check:
        out = r.out((ncol, n, 4))
        r.call = lambda s, w: ck(m.lib.trh_perm_sigma_dev(asm.handle, FID[field], 0, ncol, P(out), s))
        return r
    cols = [r.inp(elems(61 + j, n)) for j in range(ncol)]
    ptrs = (ctypes.c_void_p * ncol)(*[t.data_ptr() for t in cols])
    n_bad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(s, w):
        ck(m.lib.trh_perm_check_dev(asm.handle, FID[field], ptrs, ctypes.byref(n_bad), ctypes.byref(first), s))
        assert n_bad.value > 0  # the prefill's answer is 0
        return [np.array([n_bad.value, first.value], np.uint64)]
    r.call = call
    return r


def b_h2c(kind, curve):
    m, n, r = _mods(), 300, Run()
    prefix = m.api._prefix(m.api.HALO2_PARAMS_PREFIX)
    if kind == "field":
        u = r.out((n, 8))
        r.call = lambda s, w: ck(m.lib.trh_hash_to_field_indexed_dev(CID[curve], prefix, 0, 0, n, P(u), s))
    elif kind == "curve":
        xy = r.out((n, 8))
        r.call = lambda s, w: ck(m.lib.trh_hash_to_curve_indexed_dev(CID[curve], prefix, 0, 0, n, P(xy), s))
    else:  # the map alone: u = 0 (the prefill) is a valid input and maps to another point
        u, xy = r.inp(elems(64, 2 * n).reshape(n, 8)), r.out((n, 8))
        r.call = lambda s, w: ck(m.lib.trh_map_to_curve_dev(CID[curve], P(u), n, 2, P(xy), s))
    return r


_SETS = {}


def resident(curve, n, tabled=False):
    """a device-generated base set and its host copy; kept for the module (the tables of a tabled set are built once)"""
    m = _mods()
    key = (curve, n, tabled)
    if key not in _SETS:
        b = m.api.Bases.generate(curve, m.synth.BASE_S0, m.synth.BASE_D, n)
        if tabled:
            assert b.precompute(0) > 0
        _SETS[key] = (b, b.download())
    return _SETS[key]


def msm_want(curve, sc, bases_h):
    import cpu_ref
    return cpu_ref.to_affine(curve, cpu_ref.best_multiexp(curve, sc, bases_h, threads=8))


def b_msm(curve, n, tabled):
    m, r = _mods(), Run()
    b, bases_h = resident(curve, n, tabled)
    sc_h = elems(70 + (n & 0xff), n)
    sc = r.inp(sc_h)
    small = n <= 8448 and not tabled  # msm_small_kernel's range: the row is there for that path, so it is seen to be taken

    def call(s, w):
        before = m.api.stat("msm_small_launches")
        out = [b.msm_dev(sc, n, stream=s)]
        assert m.api.stat("msm_small_launches") - before == (1 if small else 0)
        return out
    r.call = call
    r.view = lambda arrs: [a[..., :8] for a in arrs]
    r.want = [msm_want(curve, sc_h, bases_h)]
    return r


def b_msm_batch(curve, batch):
    m, n, r = _mods(), 4097, Run()
    b, bases_h = resident(curve, n)
    sc_h = elems(72 + batch, batch * n).reshape(batch, n, 4)
    sc = r.inp(sc_h)
    r.call = lambda s, w: [b.msm_batch_dev(sc, n, batch, stream=s)]
    r.view = lambda arrs: [a[..., :8] for a in arrs]
    r.want = [np.stack([msm_want(curve, sc_h[i], bases_h) for i in range(batch)])]
    return r


def b_commit_batch(curve):
    m, n, batch, r = _mods(), 1024, 3, Run()
    b, bases_h = resident(curve, n + 1)
    sc_h, blinds = elems(75, batch * n).reshape(batch, n, 4), elems(76, batch)
    sc = r.inp(sc_h)
    r.call = lambda s, w: [b.commit_batch_dev(sc, n, batch, blinds, stream=s)]
    r.view = lambda arrs: [a[..., :8] for a in arrs]
    r.want = [np.stack([msm_want(curve, np.concatenate([sc_h[i], blinds[i:i + 1]]), bases_h) for i in range(batch)])]
    return r


def b_msm_halves(curve):
    """trh_msm_dev_enqueue returns at once over a set without tables: the window check stands between the halves; finish synchronises"""
    m, n, r = _mods(), 1 << 14, Run()
    b, bases_h = resident(curve, n)
    sc_h = elems(77, n)
    sc = r.inp(sc_h)

    def call(s, w):
        b.msm_dev_enqueue(sc, n, stream=s)
        open_ = w()
        out = [b.msm_dev_finish(stream=s)]  # whatever the check says: no MSM is left pending on the context
        assert open_, "the window was closed when trh_msm_dev_enqueue returned"
        return out
    r.call = call
    r.view = lambda arrs: [a[..., :8] for a in arrs]
    r.want = [msm_want(curve, sc_h, bases_h)]
    return r


@functools.lru_cache(maxsize=None)
def ipa_params(curve, k, tables):
    import cpu_ref
    from tiny_ram_halo2_amd import poly
    seed = 0x57A0 + 16 * k + (curve == "vesta")
    g, w, u = cpu_ref.gen_bases_hashed(curve, seed, 1 << k), cpu_ref.gen_bases_hashed(curve, seed ^ 0x5151, 1), cpu_ref.gen_bases_hashed(curve, seed ^ 0x6262, 1)
    return poly.Params(curve, k, g, g, w, u=u, precompute=tables)


def b_ipa_proof(curve, tables):
    """the whole opening at k = 10 (callbacks on the host every round: the entry synchronises); compared: c, f and every byte written to the transcript"""
    from common import DeviceTranscript
    m, k, r = _mods(), 10, Run()
    n, sf = 1 << k, SCALAR[curve]
    fs = m.o.FIELDS[sf]
    params = ipa_params(curve, k, tables)
    bases = params.ipa_bases()
    assert len(bases) == n + (2 if tables else 1)
    p, sp = r.inp(elems(80, n)), r.inp(elems(81, n))
    rnd = random.Random(0x1FA)
    p_blind, s_blind, x3 = (limbs(sf, rnd.randrange(fs.m)) for _ in range(3))
    draws = [limbs(sf, rnd.randrange(fs.m)) for _ in range(2 * k)]
    u_xy = np.ascontiguousarray(params.u, np.uint64).reshape(8)

    def call(s, w):
        tr, it = DeviceTranscript(fs.m), iter(draws)

        def put(ptr, v):
            for i in range(4):
                ptr[i] = int(v[i])
        wp = m.api.WRITE_POINT_FN(lambda c, q: tr.write_point(np.array([q[i] for i in range(12)], np.uint64)))
        ws = m.api.WRITE_SCALAR_FN(lambda c, q: tr.write_scalar(np.array([q[i] for i in range(4)], np.uint64)))
        sq = m.api.SQUEEZE_FN(lambda c, out: put(out, limbs(sf, tr.squeeze_challenge_scalar())))
        rn = m.api.RNG_FN(lambda c, out: put(out, next(it)))
        t = m.api.Transcript(None, wp, ws, sq)
        oc, of = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        ck(m.lib.trh_ipa_create_proof(bases.handle, m.api._p(u_xy), k, P(p), m.api._p(p_blind), m.api._p(x3), P(sp), m.api._p(s_blind), ctypes.byref(t),
                                      rn, None, s, m.api._p(oc), m.api._p(of)))
        assert len(tr.log) == 1 + 2 * k + 2
        return [oc, of, np.frombuffer(b"".join(tag + data for tag, data in tr.log), np.uint8)]
    r.call = call
    return r


def b_collapse(curve):
    """(k, r, c) = (10, 2, 10) over 2^10 + 2 rows: the entry's smallest shape.  Its inputs are the table of the set and two host challenges, so
    the window shows in the outputs alone (zeroed on S behind the delay)"""
    import cpu_ref
    import torch
    m, k, rr, r = _mods(), 10, 2, Run()
    key = ("collapse", curve)
    if key not in _SETS:
        b = m.api.Bases.from_host(curve, cpu_ref.gen_bases_hashed(curve, 0xC011, (1 << k) + 2))
        assert b.precompute(10) == 10
        _SETS[key] = (b, None)
    b = _SETS[key][0]
    u = rows_of(SCALAR[curve], [0x1234567890ABCDEF1234567, 0xFEDCBA9876543210FED])
    mm = 1 << (k - rr)
    xy, rec = r.out((mm, 8)), r.out((mm, 32), torch.int32)
    r.call = lambda s, w: ck(m.lib.trh_ipa_collapse_generators_dev(b.handle, k, rr, m.api._p(u), P(xy), P(rec), s))
    return r


def b_ipa_msm(op, curve):
    """the verifier's accumulator at k = 6.  The g scalars live inside the handle, so every row builds them ON S, behind the delay, by steps
    that do not commute with the entry under test, and a kernel of the entry that left S -- it would run at once, before those steps --
    changes the compared words:
      prepare (null stream)   g = c0 e_0 (not in the -fresh row, whose first addition is a copy); in the add_msm row the source's g = 0
      on S                    g += v (trh_ipa_msm_add_to_g_scalars_dev, v = the device vector S fills behind the delay), then g *= f0
      the entry, on S         add_constant_term: f0 (c0 e_0 + v) + c1 e_0   -- on the null stream (c0 + c1) f0 e_0 + f0 v
                              use_challenges, alpha != 1, a weight: alpha f0 (c0 e_0 + v) + w nc s(u) -- misplaced, alpha and f0 reach other terms
                              scale: f f0 (c0 e_0 + v) -- misplaced, f misses v
                              add_msm: c0 e_0 + f0 v, the source built on S -- misplaced, it adds the source's zeros
                              eval: the MSM over f0 (c0 e_0 + v) || w || u -- misplaced, over c0 e_0
    add_constant_term takes no stream: it has to follow on S, the stream of the accumulator's previous call.  The two add_to_g rows are the
    first step alone: misplaced, it reads the prefill of v.  Before either run a decoy accumulator takes other challenges through
    use_challenges and is destroyed, so that the blocks the pool hands to the accumulator under test hold another table and other
    parameters than the right ones: a tables kernel that ran before its parameters had arrived on S shows.
    The g scalars are compared with integers computed here (compute_s restated: s_i = the product of u_j over the set bits k - 1 - j of i);
    the point of eval with the warm-up result."""
    from tiny_ram_halo2_amd import ipa
    m, k, r = _mods(), 6, Run()
    n, sf = 1 << k, SCALAR[curve]
    mod = m.o.FIELDS[sf].m
    params = ipa_params(curve, k, False)
    v_h = elems(90, n)
    scal = r.inp(v_h)
    st = SimpleNamespace(dst=None, src=None)
    u, nc, wt, alpha = [0x1111 * (j + 3) for j in range(k)], 0xABCDEF, 0x77777, 0x5A5A5A5A5
    u_decoy = [0x2222 * (j + 5) + 1 for j in range(k)]
    f0, fac, c0, c1 = 0x9E3779B9, 0x13579BDF, 0x2468, 0x13572468
    fresh = op == "add_to_g_fresh"

    def prepare():
        for a in (st.dst, st.src):
            if a is not None:
                a.destroy()
        decoy = ipa.MSM(params)
        decoy.use_challenges([u_decoy], [nc + 1], weights=[wt + 1], alpha=alpha + 1)
        m.torch.cuda.synchronize()
        decoy.destroy()
        st.dst, st.src = ipa.MSM(params), ipa.MSM(params)
        if not fresh:
            st.dst.add_constant_term(c0)   # the g part exists: additions run the kernel, not the first copy
        st.src.add_constant_term(0)        # the source's g exists and is zero
        st.dst.add_to_w_scalar(5)
        st.dst.append_term(9, gen_bases(curve, 4)[1])
    r.prepare = prepare

    def call(s, w):
        d = st.dst
        d.stream = st.src.stream = s
        if op == "add_msm":
            st.src.add_to_g_scalars_dev(scal)
            st.src.scale(f0)
            d.add_msm(st.src)
            return []
        d.add_to_g_scalars_dev(scal)
        if op in ("add_to_g", "add_to_g_fresh"):
            return []
        d.scale(f0)
        if op == "use_challenges":
            d.use_challenges([u], [nc], weights=[wt], alpha=alpha)
        elif op == "scale":
            d.scale(fac)
        elif op == "add_constant_term":
            d.add_constant_term(c1)
        else:
            assert w(), "the window was closed before trh_ipa_msm_eval"
            ident, pt = d.eval()
            assert not ident
            return [pt]
        return []
    r.call = call
    r.late = lambda: [st.dst.g_scalars()]
    if op != "eval":
        v = ints_of(sf, v_h)
        e0 = [1] + [0] * (n - 1)
        built = [(f0 * ((0 if fresh else c0) * e + x)) % mod for e, x in zip(e0, v)]   # after the two steps on S
        if op == "add_to_g":
            g = [(c0 * e + x) % mod for e, x in zip(e0, v)]
        elif fresh:
            g = v
        elif op == "use_challenges":
            s_vec = []
            for i in range(n):
                p = 1
                for j_ in range(k):
                    if (i >> (k - 1 - j_)) & 1:
                        p = p * u[j_] % mod
                s_vec.append(p)
            g = [(alpha * b_ + wt * nc * t) % mod for b_, t in zip(built, s_vec)]
        elif op == "scale":
            g = [fac * b_ % mod for b_ in built]
        elif op == "add_constant_term":
            g = [(b_ + c1 * e) % mod for b_, e in zip(built, e0)]
        else:
            g = [(c0 * e + f0 * x) % mod for e, x in zip(e0, v)]
        r.want = [rows_of(sf, g)]
    return r


class Row:
    def __init__(self, name, entries, build, sync=False, ring=False, ref="oracle"):
        self.name, self.entries, self.build, self.sync, self.ring, self.ref = name, entries, build, sync, ring, ref


def row(name, entries, build, *args, sync=False, ring=False, ref="oracle"):
    return Row(name, (entries,) if isinstance(entries, str) else tuple(entries), functools.partial(build, *args), sync, ring, ref)


_DOMAIN_REF = ("warm-up; pinned by test_gpu_poly.py::test_domain_vs_oracle[8-3-*], ::test_domain_fused_passes_vs_unfused_primitives[11-3-*], "
               "::test_extended_domain_as_coset_blocks")
_VERIFY_REF = "warm-up; pinned by test_gpu_ipa_verify.py::test_accumulator_algebra_matches_explicit_msm[*-6-*], ::test_use_challenges_is_compute_s"

# One row per stream-taking entry of include/trh.h (some entries have several).  sync: the entry synchronises the stream, and why; the window
# check then stands before the call.  ref: "oracle", or the warm-up result and the existing test that pins the entry to the oracle.
# Fields / curves: the entries differ by a template argument only (with_field / with_curve, csrc/dispatch.h), so one of each runs; the rows
# alternate between the two so that both instantiations are loaded behind a delay somewhere.
ROWS = [
    row("field_op-fp", "trh_field_op_dev", b_field_op, "fp"),                                  # raw ctypes: the Python wrapper takes no stream
    row("point_op-vesta", "trh_point_op_dev", b_point_op, "vesta"),                            # raw ctypes
    row("scale-fq", "trh_field_scale_dev", b_scale, "scale", "fq", sync="the caller's factor is staged, hipStreamSynchronize BEFORE the compute kernel: only the staging copy is inside the window"),
    row("scale_periodic-fp", "trh_field_scale_periodic_dev", b_scale, "periodic", "fp", sync="the caller's factors are staged BEFORE the compute kernel: only the staging copy is inside the window"),
    row("scale_rows-fq", "trh_field_scale_rows_dev", b_scale, "rows", "fq", sync="the caller's factors are staged BEFORE the compute kernel: only the staging copy is inside the window"),
    row("ntt-8-b1", "trh_ntt_dev", b_ntt, "fp", 8, 1),                                         # one pass
    row("ntt-12-b1", "trh_ntt_dev", b_ntt, "fq", 12, 1),                                       # two lazy passes, the inter-pass table
    row("ntt-8-b9", "trh_ntt_dev", b_ntt, "fq", 8, 9),                                         # the batch-major grid
    row("ntt-12-b9", "trh_ntt_dev", b_ntt, "fp", 12, 9),
] + [
    row(f"domain-{op}-k{k}", "trh_domain_" + op, b_domain, op, field, k, ref=_DOMAIN_REF)
    for k, field in ((8, "fp"), (11, "fq"))
    for op in ("lagrange_to_coeff", "coeff_to_extended", "extended_to_coeff", "divide_by_vanishing_poly", "coeff_to_extended_blocks", "blocks_to_quotient")
] + [
    row("inner_product-fp", "trh_field_inner_product_dev", b_inner_product, "fp", sync="returns the sum to the host"),      # 70 000: more than one partial
    row("eval_batch-fq", "trh_poly_eval_batch_dev", b_eval_batch, "fq", sync="returns the values to the host"),
    row("axpy-fp", "trh_field_axpy_dev", b_axpy, "fp", ring=True),
    row("powers-fq", "trh_field_powers_dev", b_powers, "fq", ring=True),
    row("batch_invert-fp", "trh_field_batch_invert_dev", b_batch_invert, "fp", False),           # 16 385: two workgroups
    row("batch_invert_mul-fq", "trh_field_batch_invert_mul_dev", b_batch_invert, "fq", True),
    row("product_terms-fp", "trh_product_terms_dev", b_product_terms, "fp", sync="the caller's descriptors are staged BEFORE the compute kernel: only the staging copy is inside the window"),
    row("prefix_product-fq", "trh_field_prefix_product_dev", b_scan, "product", "fq"),           # 4097: two scan blocks
    row("prefix_product_rows-fp", "trh_field_prefix_product_rows_dev", b_scan, "product_rows", "fp"),
    row("prefix_sum-fq", "trh_field_prefix_sum_dev", b_scan, "sum", "fq"),
    row("lincomb-fp", "trh_poly_lincomb_dev", b_lincomb, "fp", sync="the caller's coefficients are staged BEFORE the compute kernel: only the staging copy is inside the window"),
    row("kate_division-fq", "trh_poly_kate_division_dev", b_kate, "fq"),
    row("lookup-fp", "trh_lookup_permute_dev", b_lookup, 0, "fp", sync="documented: reads the miss flag back",
        ref="warm-up; pinned by test_gpu_lookup_sizes.py::test_small_cases_match_oracle[sizes-fp-4097-wide]"),
    row("lookup_batch-fq", "trh_lookup_permute_batch_dev", b_lookup, 3, "fq", sync="documented: one host synchronisation per batch",
        ref="warm-up; pinned by test_gpu_lookup_sizes.py::test_small_cases_match_oracle[sizes-fq-4097-wide], ::test_chunks_match_oracle"),
    row("expr_eval-fp", "trh_expr_eval_dev", b_expr, False, "fp", sync="documented: synchronises the stream",
        ref="warm-up; pinned by test_gpu_expr.py::test_deep_expression_spills_to_lds, ::test_synthetic_gates_vs_oracle"),
    row("expr_eval_blocks-fq", "trh_expr_eval_blocks_dev", b_expr, True, "fq", sync="documented: synchronises the stream",
        ref="warm-up; pinned by test_gpu_poly.py::test_extended_domain_as_coset_blocks (the block layout), test_gpu_expr.py::test_synthetic_gates_vs_oracle"),
    row("point_fft-pallas", "trh_point_fft_dev", b_point_fft, "pallas", sync="the twiddle scalars are staged from a stack buffer BEFORE the compute kernel: only the staging copy is inside the window"),
    row("bases_fold-vesta", "trh_bases_fold_dev", b_bases_fold, "vesta", ring=True),
    row("sqrt-fp", "trh_field_sqrt_dev", b_sqrt, "fp"),
    row("compress-pallas", "trh_points_compress_dev", b_compress, "pallas"),
    row("decompress-vesta", "trh_points_decompress_dev", b_decompress, "vesta", False),
    row("decompress-first_bad-pallas", "trh_points_decompress_dev", b_decompress, "pallas", True, sync="documented: reads first_bad back"),
    row("rng_fill-fp", "trh_rng_fill_dev", b_rng, False, "fp", ref="warm-up; pinned by test_gpu_rng.py::test_fill_matches_the_model[*-1000]"),
    row("rng_fill_rows-fq", "trh_rng_fill_rows_dev", b_rng, True, "fq", ref="warm-up; pinned by test_gpu_rng.py::test_fill_rows_writes_the_blinding_cells_only"),
    row("perm_sigma-fp", "trh_perm_sigma_dev", b_perm, False, "fp", ref="warm-up; pinned by test_gpu_permkeygen.py::test_sigma_columns_against_big_integers"),
    row("perm_check-fq", "trh_perm_check_dev", b_perm, True, "fq", sync="documented: returns the counts to the host",
        ref="warm-up; pinned by test_gpu_permkeygen.py::test_check_against_numpy, ::test_grand_product_closes_and_check_agrees"),
    row("hash_to_field-pallas", "trh_hash_to_field_indexed_dev", b_h2c, "field", "pallas", ref="warm-up; pinned by test_gpu_hashtocurve.py::test_hash_to_field_index_ranges[*-0-300]"),
    row("map_to_curve-vesta", "trh_map_to_curve_dev", b_h2c, "map", "vesta", ref="warm-up; pinned by test_gpu_hashtocurve.py::test_map_two_elements_per_point"),
    row("hash_to_curve-vesta", "trh_hash_to_curve_indexed_dev", b_h2c, "curve", "vesta", ref="warm-up; pinned by test_gpu_hashtocurve.py::test_fused_entry_index_ranges[*-0-300]"),
    row("msm-4098-pallas", "trh_msm_dev", b_msm, "pallas", 4098, False, sync="documented: returns the point to the host"),          # msm_small_kernel
    row("msm-2^14-vesta", "trh_msm_dev", b_msm, "vesta", 1 << 14, False, sync="documented: returns the point to the host"),          # the pipeline
    row("msm-2^14-tabled-pallas", "trh_msm_dev", b_msm, "pallas", 1 << 14, True, sync="documented: the sampler synchronises, then the point"),
    row("msm_batch-2-vesta", "trh_msm_batch_dev", b_msm_batch, "vesta", 2, sync="documented: returns the points to the host"),
    row("msm_batch-9-pallas", "trh_msm_batch_dev", b_msm_batch, "pallas", 9, sync="documented: chunks of >= 8 synchronise"),
    row("commit_batch-vesta", "trh_commit_batch_dev", b_commit_batch, "vesta", sync="the caller's blinds are staged BEFORE the compute kernel: only the staging copy is inside the window; returns the points"),
    row("msm_halves-pallas", ("trh_msm_dev_enqueue", "trh_msm_dev_finish"), b_msm_halves, "pallas", sync="mid"),
    row("ipa_create_proof-vesta", "trh_ipa_create_proof", b_ipa_proof, "vesta", False, sync="callbacks on the host every round",
        ref="warm-up; pinned by test_gpu_ipa.py::test_ipa_create_proof_vs_oracle, test_gpu_ipa_verify.py::test_proofs_accepted_on_both_base_set_forms[vesta-10]"),
    row("ipa_create_proof-tables-pallas", "trh_ipa_create_proof", b_ipa_proof, "pallas", True, sync="callbacks on the host every round",
        ref="warm-up; pinned by test_gpu_ipa_verify.py::test_proofs_accepted_on_both_base_set_forms[pallas-10], test_gpu_ipa.py::test_ipa_base_set_forms_agree"),
    row("ipa_collapse-pallas", "trh_ipa_collapse_generators_dev", b_collapse, "pallas", sync="documented: returns with the stream synchronised",
        ref="warm-up; pinned by test_gpu_ipa_collapse.py::test_collapse_matches_integer_reference[10-2-10-2-pallas]"),
    row("ipa_msm-add_to_g-pallas", "trh_ipa_msm_add_to_g_scalars_dev", b_ipa_msm, "add_to_g", "pallas"),
    row("ipa_msm-add_to_g-fresh-vesta", "trh_ipa_msm_add_to_g_scalars_dev", b_ipa_msm, "add_to_g_fresh", "vesta"),
    row("ipa_msm-use_challenges-vesta", "trh_ipa_msm_use_challenges", b_ipa_msm, "use_challenges", "vesta"),
    row("ipa_msm-scale-pallas", "trh_ipa_msm_scale", b_ipa_msm, "scale", "pallas"),
    row("ipa_msm-add_msm-vesta", "trh_ipa_msm_add_msm", b_ipa_msm, "add_msm", "vesta"),
    row("ipa_msm-add_constant_term-pallas", "trh_ipa_msm_add_constant_term", b_ipa_msm, "add_constant_term", "pallas"),
    row("ipa_msm-eval-vesta", "trh_ipa_msm_eval", b_ipa_msm, "eval", "vesta", sync="mid", ref=_VERIFY_REF),
]

# declarations with a `stream` parameter that have no row above, and where they are tested instead
ELSEWHERE = {
    "trh_stream_synchronize": "B: test_b4_stream_synchronize_on_another_stream_waits_for_the_first",
    "trh_event_record": "B: test_b5_events_ride_the_stream",
}
# entries without a stream parameter that take the stream of an earlier call, and so have a row all the same
STREAMLESS_ROWS = {"trh_ipa_msm_add_constant_term"}


def test_the_table_is_complete():
    """no device needed: every declaration of include/trh.h with a `void* stream` parameter has a row, or stands in ELSEWHERE with its reason"""
    header = open(os.path.join(ROOT, "include", "trh.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = {name for name, args in re.findall(r"\b(trh_\w+)\s*\(([^;{}]*?)\)\s*;", header) if re.search(r"\bvoid\s*\*\s*stream\b", args)}
    assert len(declared) >= 54, sorted(declared)
    covered = {e for r in ROWS for e in r.entries}
    assert not (covered & set(ELSEWHERE)), sorted(covered & set(ELSEWHERE))
    assert declared == (covered - STREAMLESS_ROWS) | set(ELSEWHERE), sorted(declared ^ ((covered - STREAMLESS_ROWS) | set(ELSEWHERE)))
    assert STREAMLESS_ROWS <= covered and not (STREAMLESS_ROWS & declared)
    assert len({r.name for r in ROWS}) == len(ROWS)
    for r in ROWS:
        assert r.ref == "oracle" or ("pinned by test_" in r.ref and "::test_" in r.ref), r.name
        assert not (r.sync and r.ring), r.name


@pytest.fixture(scope="module")
def device():
    from tiny_ram_halo2_amd import api
    api.init(0)
    w = _window()
    yield w
    if TIMES:
        name = max(TIMES, key=TIMES.get)
        longest = TIMES[name] * 1e3
        print(f"\n[test_gpu_streams] delay {DELAY_MS:.1f} ms ({w.ticks} ticks, {w.per_ms:.0f} ticks/ms); longest host-side enqueue sequence "
              f"{longest:.3f} ms ({name}); ratio {DELAY_MS / longest:.0f}")
        for k_, v in sorted(TIMES.items(), key=lambda kv: -kv[1])[:8]:
            print(f"[test_gpu_streams]   {v * 1e3:8.3f} ms  {k_}")


@pytest.mark.parametrize("r", ROWS, ids=[r.name for r in ROWS])
@on_the_device
def test_entry_rides_the_callers_stream(r, device):
    drive(r.name, r.build(), sync=bool(r.sync) and r.sync != "mid", ring=r.ring)


# ---- negative controls: the window exists on this machine ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefill_kind", ["zeros", "delta"])
@on_the_device
def test_control_ntt_on_the_null_stream_sees_the_prefill(prefill_kind, device):
    """steps 2 - 3, then trh_ntt_dev with stream = None ON PURPOSE: the null stream does not wait for S, so the transform runs on the prefill
    while the delay spins.  Its result, copied on the null stream with the window still open, is the oracle's transform OF THE PREFILL: all
    zeros for the zero vector -- and, so that the kernel is seen to have run at all, all ones for (1, 0, 0, ...)"""
    import torch
    m, field, log_n = _mods(), "fp", 12
    n = 1 << log_n
    real = elems(4 + log_n, n)
    pre = np.zeros((n, 4), np.uint64)
    if prefill_kind == "delta":
        pre[0] = limbs(field, 1)
    omega = limbs(field, m.o.FIELDS[field].omega(log_n))
    r = Run()
    a = r.inout(real, pre)
    ck(m.lib.trh_ntt_dev(FID[field], P(a), log_n, m.api._p(omega), 1, None))  # warm: tables
    prefill(r)
    S = device.A
    E = delayed_fill(S, r)
    try:
        ck(m.lib.trh_ntt_dev(FID[field], P(a), log_n, m.api._p(omega), 1, None))
        snap = a.clone()                             # on the null stream, behind the transform
        torch.cuda.default_stream().synchronize()
        open_ = not E.query()
    finally:
        S.synchronize()
    assert open_, "the null stream waited for the side stream (or the host was slower than the delay): no window on this machine"
    want = m.cpu_ref.best_fft(field, pre, omega, log_n, threads=4)
    assert (want == (limbs(field, 1) if prefill_kind == "delta" else 0)).all()
    assert (host(snap) == want).all()
    assert (host(a) == real).all()                   # and S then wrote the real input over it, untransformed


@on_the_device
def test_control_msm_on_the_null_stream_sees_the_prefill(device):
    """the same for the curve family: trh_msm_dev with stream = None over scalars that S will fill behind its delay returns the identity"""
    import torch
    m, curve, n = _mods(), "vesta", 1 << 14
    b, _ = resident(curve, n)
    r = Run()
    sc = r.inp(elems(70, n))
    assert b.msm_dev(sc, n)[:8].any()                # warm, and the real scalars do not sum to the identity
    prefill(r)
    S = device.A
    E = delayed_fill(S, r)
    try:
        got = b.msm_dev(sc, n, stream=None)
        open_ = not E.query()
    finally:
        S.synchronize()
    assert open_, "the null stream waited for the side stream (or the host was slower than the delay): no window on this machine"
    assert not got.any(), "the MSM of the all-zero prefill is the identity"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# B. ordering through the context
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _ntt_case(field="fp", log_n=10):
    m = _mods()
    n = 1 << log_n
    real = elems(100 + log_n, n)
    omega = limbs(field, m.o.FIELDS[field].omega(log_n))
    r = Run()
    a = r.inout(real)
    ntt = lambda s: ck(m.lib.trh_ntt_dev(FID[field], P(a), log_n, m.api._p(omega), 1, s))  # noqa: E731
    ntt(None)  # warm: tables
    want = m.cpu_ref.best_fft(field, real, omega, log_n, threads=4)
    return m, r, a, n, ntt, real, want


@on_the_device
def test_b1_memcpy_d2h_waits_for_the_stream_of_the_previous_call(device):
    """trh_ntt_dev on A behind the delay returns at once; trh_memcpy_d2h (TRH_ENTER(0): a wait enqueued on the null stream, then a
    synchronous hipMemcpy) must deliver the transform"""
    import torch
    m, r, a, n, ntt, real, want = _ntt_case()
    prefill(r)
    A = device.A
    E = delayed_fill(A, r)
    try:
        ntt(A.cuda_stream)
        open_ = not E.query()
        got = np.empty((n, 4), np.uint64)
        ck(m.lib.trh_memcpy_d2h(got.ctypes.data_as(ctypes.c_void_p), P(a), got.nbytes))
    finally:
        A.synchronize()
    assert open_, "the window was closed when trh_ntt_dev returned"
    assert (got == want).all(), "trh_memcpy_d2h did not wait for the transform on the other stream" + ("; it read the prefill" if not got.any() else "")


@on_the_device
def test_b1_memcpy_h2d_waits_for_the_reader_of_the_old_input(device):
    """an asynchronous call on A still reads `a` (A is held by the delay) when trh_memcpy_h2d uploads a new input into it: the call's
    result is that of the OLD input, and `a` holds the new one afterwards"""
    import torch
    m, field, n = _mods(), "fq", 4096
    old, new, b_h = elems(110, n), elems(111, n), elems(112, n)
    a, b, out = dev(old), dev(b_h), dev(np.zeros((n, 4), np.uint64))
    op = lambda s: ck(m.lib.trh_field_op_dev(FID[field], m.api.FIELD_OPS["mul"], P(a), P(b), P(out), n, s))  # noqa: E731
    op(None)
    out.zero_()
    torch.cuda.synchronize()
    A = device.A
    E = torch.cuda.Event()
    with torch.cuda.stream(A):
        torch.cuda._sleep(device.ticks)
        E.record(A)
    try:
        op(A.cuda_stream)
        open_ = not E.query()
        ck(m.lib.trh_memcpy_h2d(P(a), new.ctypes.data_as(ctypes.c_void_p), new.nbytes))
    finally:
        A.synchronize()
    torch.cuda.synchronize()
    assert open_, "the window was closed when trh_field_op_dev returned"
    assert (host(out) == m.cpu_ref.field_op(field, "mul", old, b_h)).all(), "the upload overtook the kernel that was still to read the old input"
    assert (host(a) == new).all()


@on_the_device
def test_b1_free_waits_for_the_kernel_that_writes_the_block(device):
    """trh_free of a trh_malloc block that a kernel held on A is still to write: the block, taken again from the pool, holds the result"""
    import torch
    m, field, n = _mods(), "fp", 4096
    if not m.api.get_option("pool_mb"):
        pytest.fail("the pool is switched off (pool_mb = 0): this case needs trh_free to keep the block")
    x_h, y_h = elems(113, n), elems(114, n)
    x, y = dev(x_h), dev(y_h)
    blk = ctypes.c_void_p()
    ck(m.lib.trh_malloc(ctypes.byref(blk), n * 32))
    zeros = np.zeros((n, 4), np.uint64)
    ck(m.lib.trh_memcpy_h2d(blk, zeros.ctypes.data_as(ctypes.c_void_p), zeros.nbytes))
    op = lambda s: ck(m.lib.trh_field_op_dev(FID[field], m.api.FIELD_OPS["mul"], P(x), P(y), blk, n, s))  # noqa: E731
    torch.cuda.synchronize()
    A = device.A
    E = torch.cuda.Event()
    with torch.cuda.stream(A):
        torch.cuda._sleep(device.ticks)
        E.record(A)
    taken, got = [], np.empty((n, 4), np.uint64)
    try:
        op(A.cuda_stream)
        open_ = not E.query()
        ck(m.lib.trh_free(blk))
        while len(taken) < 64 and blk.value not in taken:  # the pool may hold other idle blocks of this size: take until ours comes back
            again = ctypes.c_void_p()
            ck(m.lib.trh_malloc(ctypes.byref(again), n * 32))
            taken.append(again.value)
        ck(m.lib.trh_memcpy_d2h(got.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(taken[-1]), got.nbytes))
    finally:
        A.synchronize()
        for ptr in taken:
            m.lib.trh_free(ctypes.c_void_p(ptr))
    assert open_, "the window was closed when trh_field_op_dev returned"
    assert taken[-1] == blk.value, "the pool did not hand the freed block out again"
    assert (got == m.cpu_ref.field_op(field, "mul", x_h, y_h)).all(), "the block came back from trh_free before the kernel had written it"


@on_the_device
def test_b2_a_call_on_another_stream_waits_for_its_predecessor(device):
    """a data dependence carried by the context alone: trh_ntt_dev on A behind the delay, then trh_field_inner_product_dev of that buffer on B.
    Nothing else orders B behind A: a plain torch copy on B, made between the two calls, reads the prefill while the window is open"""
    import torch
    from common import stored_ints
    m, r, a, n, ntt, real, want = _ntt_case("fq", 10)
    field = "fq"
    w_h = elems(120, n)
    w = dev(w_h)
    m.api.inner_product_dev(field, a, w, n)  # warm: scratch
    prefill(r)
    A, B = device.A, device.B
    E = delayed_fill(A, r)
    try:
        ntt(A.cuda_stream)
        open_ = not E.query()
        with torch.cuda.stream(B):                   # the control: B bypassing the library
            snap = a.clone()
        B.synchronize()
        still_open = not E.query()
        got = m.api.inner_product_dev(field, a, w, n, stream=B.cuda_stream)
    finally:
        A.synchronize()
        B.synchronize()
    assert open_ and still_open, "the window was closed: " + ("trh_ntt_dev synchronised" if not open_ else "the copy on B waited for A")
    assert not host(snap).any(), "the torch copy on B should have read the prefill: B is ordered behind A by something else than the library"
    ip = sum(stored_ints(m.cpu_ref.field_op(field, "mul", want, w_h))) % m.o.FIELDS[field].m
    assert (got == stored_rows([ip])[0]).all(), "the inner product on B did not wait for the transform on A"


@on_the_device
def test_b2_chain_over_three_streams(device):
    """A -> B -> C -> A, a different entry at each step, each consuming its predecessor's output: the transform on A behind the delay, the
    batch inversion of it on B, the prefix product of that on C, and on A again the element-wise product of the inverses and the scan"""
    import torch
    m, r, a, n, ntt, real, want = _ntt_case("fp", 10)
    field = "fp"
    z, out = dev(np.zeros((n, 4), np.uint64)), dev(np.zeros((n, 4), np.uint64))
    lib = m.lib
    inv = lambda s: ck(lib.trh_field_batch_invert_dev(FID[field], P(a), n, s))               # noqa: E731
    scan = lambda s: ck(lib.trh_field_prefix_product_dev(FID[field], P(a), P(z), n, s))      # noqa: E731
    mul = lambda s: ck(lib.trh_field_op_dev(FID[field], m.api.FIELD_OPS["mul"], P(a), P(z), P(out), n, s))  # noqa: E731
    for fn in (inv, scan, mul):
        fn(None)  # warm: scratch
    prefill(r)
    z.zero_()
    out.zero_()
    torch.cuda.synchronize()
    A, B, C = device.A, device.B, device.C
    E = delayed_fill(A, r)
    try:
        ntt(A.cuda_stream)
        inv(B.cuda_stream)
        scan(C.cuda_stream)
        mul(A.cuda_stream)
        open_ = not E.query()
        with torch.cuda.stream(A):
            got = out.clone()
    finally:
        for s in (A, B, C):
            s.synchronize()
    assert open_, "the window was closed after four asynchronous calls"
    inv_h = m.cpu_ref.field_op(field, "inv", want)
    assert (host(got) == m.cpu_ref.field_op(field, "mul", inv_h, m.cpu_ref.prefix_product(field, inv_h))).all()


@on_the_device
def test_b3_two_streams_share_the_scan_scratch(device):
    """trh_field_prefix_product_dev over 2^20 elements on A, no delay, and straight after it trh_poly_eval_batch_dev on B: both use Ctx::scan.
    NOT DECISIVE: it needs the two to overlap for real, which no test can force -- a pass says little, a failure says the scratch was shared
    unordered.  The b1 / b2 cases are the ones that pin the wait."""
    import torch
    m, field, n, ne, batch = _mods(), "fq", 1 << 20, 4097, 3
    a_h, p_h, x = elems(130, n), elems(131, batch * ne).reshape(batch, ne, 4), limbs("fq", 0xABCDEF0123)
    a, p, out = dev(a_h), dev(p_h), dev(np.zeros((n, 4), np.uint64))
    m.api.prefix_product_dev(field, a, out, n)
    m.api.poly_eval_batch_dev(field, p, ne, batch, x)
    out.zero_()
    torch.cuda.synchronize()
    A, B = device.A, device.B
    try:
        m.api.prefix_product_dev(field, a, out, n, stream=A.cuda_stream)
        got = m.api.poly_eval_batch_dev(field, p, ne, batch, x, stream=B.cuda_stream)
    finally:
        A.synchronize()
        B.synchronize()
    torch.cuda.synchronize()
    z = host(out)
    assert (z[0] == limbs(field, 1)).all() and (m.cpu_ref.field_op(field, "mul", z[:-1], a_h[:-1]) == z[1:]).all()  # the scan, by induction
    assert (got == np.stack([m.cpu_ref.eval_polynomial(field, p_h[i], x) for i in range(batch)])).all()


@on_the_device
def test_b4_an_msm_in_flight_and_a_transform_on_another_stream(device):
    """trh_msm_dev_enqueue on A behind the delay, trh_ntt_dev on B, a finish that names B (refused: msm_finish's stream check, the MSM stays
    pending), then trh_msm_dev_finish on A: both results against the oracle"""
    import torch
    m, curve, n = _mods(), "pallas", 1 << 14
    b, bases_h = resident(curve, n)
    mr = Run()
    sc_h = elems(77, n)
    sc = mr.inp(sc_h)
    assert b.msm_dev(sc, n).any()  # warm
    _, nr, a, nn, ntt, real, want = _ntt_case("fq", 10)
    a.copy_(nr.inputs[0][1])  # the warm-up transformed it in place
    prefill(mr)
    A, B = device.A, device.B
    E = delayed_fill(A, mr)
    out = np.zeros(12, np.uint64)
    try:
        b.msm_dev_enqueue(sc, n, stream=A.cuda_stream)
        ntt(B.cuda_stream)
        open_ = not E.query()
        rc = m.lib.trh_msm_dev_finish(b.handle, B.cuda_stream, m.api._p(out))
        err = m.lib.trh_last_error().decode()
        got = b.msm_dev_finish(stream=A.cuda_stream)
        with torch.cuda.stream(B):
            t = a.clone()
    finally:
        A.synchronize()
        B.synchronize()
    assert open_, "the window was closed after the enqueue and the transform"
    assert rc == EINVAL and "stream" in err, (rc, err)
    assert (got[:8] == msm_want(curve, sc_h, bases_h)).all()
    assert (host(t) == want).all()


@on_the_device
def test_b4_stream_synchronize_on_another_stream_waits_for_the_first(device):
    """trh_stream_synchronize(B) straight after an asynchronous call on A returns only when A's work is done: the output is then read by a
    torch copy on B, which waits for nothing but B"""
    import torch
    m, r, a, n, ntt, real, want = _ntt_case("fp", 10)
    prefill(r)
    A, B = device.A, device.B
    E = delayed_fill(A, r)
    try:
        ntt(A.cuda_stream)
        open_ = not E.query()
        ck(m.lib.trh_stream_synchronize(B.cuda_stream))
        done = E.query()
        with torch.cuda.stream(B):
            t = a.clone()
        B.synchronize()
        got = host(t)
    finally:
        A.synchronize()
    assert open_, "the window was closed when trh_ntt_dev returned"
    assert done, "trh_stream_synchronize(B) returned while A was still held by the delay"
    assert (got == want).all()


@on_the_device
def test_b5_events_ride_the_stream(device):
    """trh_event_record on S before the delay and after a call behind it: the elapsed device time is at least the delay, so both events rode S
    (on the null stream they would be a few microseconds apart); the delay itself is measured by torch events that stand between them on S"""
    import torch
    m, r, a, n, ntt, real, want = _ntt_case("fq", 10)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    ck(m.lib.trh_event_create(ctypes.byref(e0)))
    ck(m.lib.trh_event_create(ctypes.byref(e1)))
    prefill(r)
    S = device.A
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)  # torch's own, around the delay alone: the measured delay
    try:
        ck(m.lib.trh_event_record(e0, S.cuda_stream))
        t0.record(S)
        E = delayed_fill(S, r)
        t1.record(S)
        ntt(S.cuda_stream)
        ck(m.lib.trh_event_record(e1, S.cuda_stream))
        open_ = not E.query()
        ms = ctypes.c_float(0)
        ck(m.lib.trh_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
    finally:
        S.synchronize()
        m.lib.trh_event_destroy(e0)
        m.lib.trh_event_destroy(e1)
    delay = t0.elapsed_time(t1)
    assert open_, "the window was closed after the second record"
    assert delay >= 0.5 * DELAY_MS, f"the delay lasted {delay:.2f} ms, it is sized for {DELAY_MS} ms"
    assert ms.value >= delay, f"{ms.value:.2f} ms between the library's events, {delay:.2f} ms of delay between them on the same stream"
    assert (host(a) == want).all()
