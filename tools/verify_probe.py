"""Device time of the IPA verifier's accumulator (csrc/ipaverify.hip) at k = 18 on Vesta:
  * use_challenges with P = 1, 8 and 32 guards (one pass over the 2^k g scalars);
  * eval over the g || w set (Params without tables) and over the tabled g || w || u set;
  * the whole batch check of 8 proofs (verify_proof's arithmetic per proof on the host, one accumulator, eval).
Next to them, the same accumulator computed by the test restatement (tests/common.py's compute_s construction and cpu_ref.best_multiexp
on 16 threads): a CPU stand-in for halo2's Rust loop, NOT a measurement of it.
    python tools/verify_probe.py [out_file]"""
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401  (torch first: one HIP runtime in the process)

import cpu_ref  # noqa: E402
import pasta as o  # noqa: E402
from tiny_ram_halo2_amd import api, ipa, poly, synth  # noqa: E402
from test_gpu_ipa_verify import RecordingTranscript, to_dev  # noqa: E402

K, CURVE, SFIELD, REPS = 18, "vesta", "fp", 10


class Events:
    def __init__(self):
        self.a, self.b = api._vp(), api._vp()
        api._check(api.lib().trh_event_create(self.a))
        api._check(api.lib().trh_event_create(self.b))

    def time(self, fn, reps=REPS, warm=2):
        for _ in range(warm):
            fn()
        ms = []
        for _ in range(reps):
            api._check(api.lib().trh_event_record(self.a, None))
            fn()
            api._check(api.lib().trh_event_record(self.b, None))
            v = api.ctypes.c_float(0)
            api._check(api.lib().trh_event_elapsed_ms(self.a, self.b, api.ctypes.byref(v)))
            ms.append(v.value)
        return min(ms), sorted(ms)[len(ms) // 2]


def main():
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    api.init(0)
    fs = o.CURVES[CURVE].scalar
    m, n = fs.m, 1 << K
    g_l = cpu_ref.gen_bases_hashed(CURVE, 0x7E18, n)
    w_l, u_l = cpu_ref.gen_bases_hashed(CURVE, 0x7E18 ^ 0x5151, 1), cpu_ref.gen_bases_hashed(CURVE, 0x7E18 ^ 0x6262, 1)
    tabled = poly.Params(CURVE, K, g_l, g_l, w_l, u=u_l, precompute=True)
    plain = poly.Params(CURVE, K, g_l, g_l, w_l, u=u_l, precompute=False)
    say(f"verify_probe: k = {K}, {CURVE}, {api.lib().trh_version().decode()}")
    say(f"  base sets: g || w = {len(plain.ipa_bases())} points; g || w || u = {len(tabled.ipa_bases())} points, table window "
        f"{int(api.lib().trh_bases_precomputed_window_bits(tabled.ipa_bases().handle))} bits")
    ev = Events()
    rnd = random.Random(0x9E)

    for count in (1, 8, 32):
        us = [[rnd.randrange(1, m) for _ in range(K)] for _ in range(count)]
        ncs = [rnd.randrange(m) for _ in range(count)]
        ws = None if count == 1 else [rnd.randrange(m) for _ in range(count)]
        acc = ipa.MSM(tabled)
        acc.use_challenges(us, ncs, weights=ws)       # the g part exists from here on: the timed calls read and write it
        lo, med = ev.time(lambda: acc.use_challenges(us, ncs, weights=ws))
        say(f"  use_challenges P = {count:2d}: {lo:.3f} ms min, {med:.3f} ms median (device events; {REPS} calls)")
        acc.destroy()

    u1, nc1 = [rnd.randrange(1, m) for _ in range(K)], rnd.randrange(m)
    pts = cpu_ref.gen_bases_hashed(CURVE, 0xE7A1, 2 * K + 1)
    terms = [(rnd.randrange(m), pts[i]) for i in range(2 * K + 1)]
    w_s, u_s = rnd.randrange(m), rnd.randrange(m)
    points = {}
    for name, params in (("g || w", plain), ("g || w || u (tables)", tabled)):
        acc = ipa.MSM(params)
        for s, p in terms:
            acc.append_term(s, p)
        acc.add_to_w_scalar(w_s); acc.add_to_u_scalar(u_s)
        acc.use_challenges([u1], [nc1])
        lo, med = ev.time(lambda: acc.eval(), reps=5)
        t0 = time.perf_counter(); _, pt = acc.eval(); wall = (time.perf_counter() - t0) * 1e3
        points[name] = pt
        say(f"  eval over {name}: {lo:.3f} ms min, {med:.3f} ms median (device events around the call), {wall:.3f} ms wall; "
            f"2^k + {len(params.ipa_bases()) - n} pairs in the full-range MSM + {2 * K + 1 + (1 if params is plain else 0)} small")
        acc.destroy()
    say(f"  the two forms give the same point: {bool((points['g || w'] == points['g || w || u (tables)']).all())}")

    # the whole batch check of 8 proofs (openings by trh_ipa_create_proof)
    proofs = []
    for p in range(8):
        r = random.Random(0xBA70 + p)
        p_l, s_l = synth.field_elements(0x5100 + 2 * p, n), synth.field_elements(0x5101 + 2 * p, n)
        p_blind, s_blind, x3 = r.randrange(m), r.randrange(m), r.randrange(m)
        draws = iter([r.randrange(m) for _ in range(2 * K)])
        com = cpu_ref.to_affine(CURVE, tabled.commit(p_l, np.array(fs.limbs(p_blind), np.uint64)))
        tr = RecordingTranscript(m)
        c, f = ipa.create_proof_native(tabled, lambda: next(draws), tr, to_dev(p_l), p_blind, x3, s_l, s_blind)
        v = fs.from_limbs(cpu_ref.eval_polynomial(SFIELD, p_l, np.array(fs.limbs(x3), np.uint64)))
        rounds = [(tr.points[1 + 2 * j], tr.points[2 + 2 * j], tr.challenges[2 + j]) for j in range(K)]
        proofs.append((com, v, x3, tr.points[0], tr.challenges[0], tr.challenges[1], rounds, c, f))
    rs = [rnd.randrange(1, m) for _ in range(8)]
    weights = [1] * 8
    for p in range(8):
        for q in range(p + 1, 8):
            weights[p] = weights[p] * rs[q] % m

    def batch():
        guards = [ipa.verify_proof(tabled, [(1, P)], v, x3, S, xi, z, rounds, c, f) for P, v, x3, S, xi, z, rounds, c, f in proofs]
        return ipa.batch_verify(tabled, guards, weights)

    ok = batch()
    lo, med = ev.time(batch, reps=5, warm=1)
    t0 = time.perf_counter(); batch(); wall = (time.perf_counter() - t0) * 1e3
    say(f"  batch check of 8 proofs: accepted = {ok}; {lo:.3f} ms min, {med:.3f} ms median (device events around the whole check), "
        f"{wall:.3f} ms wall incl. the Python host side")

    # CPU stand-in for the same P = 1 accumulator and its eval (the test restatement; not halo2's Rust loop)
    from test_gpu_ipa_verify import s_times
    t0 = time.perf_counter()
    g = s_times(CURVE, K, u1, nc1)
    t_s = (time.perf_counter() - t0) * 1e3
    lim = lambda val: np.array(fs.limbs(val % m), np.uint64)  # noqa: E731
    sc = np.concatenate([g, np.stack([lim(s) for s, _ in terms])])
    bs = np.concatenate([g_l, np.stack([p for _, p in terms])])
    t0 = time.perf_counter()
    cpu_ref.best_multiexp(CURVE, sc, bs, threads=16)
    t_e = (time.perf_counter() - t0) * 1e3
    say(f"  CPU stand-in (test restatement, cpu_ref; NOT a measurement of halo2's Rust loop): compute_s x neg_c {t_s:.1f} ms "
        f"(numpy + cpu_ref.field_op, one thread), eval's 2^k + {2 * K + 1} MSM {t_e:.1f} ms (cpu_ref.best_multiexp, 16 threads)")

    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()
