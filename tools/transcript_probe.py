"""What the transcript's host turn costs: tools/transcript_probe.py [k] [reps]
1. The IPA opening alone at size k (tools/ipa_probe.py's shape) with a transcript.Blake2bWrite -- the library's own functions inside
   trh_ipa_create_proof -- against tests/transcript_model.py's writer, the same format through three Python closures (the path of every
   other transcript object).  The two alternate, after one untimed opening each; every opening ends in a device synchronise.  Prints the
   per-opening times, the medians, and checks that both wrote the same bytes.
2. The host time of a reader's read_point (one field square root each), over points of the curve: what verify_proof_bytes spends decoding."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import transcript_model as tm
from tiny_ram_halo2_amd import api, ipa, poly, synth, transcript

k = int(sys.argv[1]) if len(sys.argv) > 1 else 18
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n = 1 << k
curve = "vesta"
api.init(0)
g = api.Bases.generate(curve, synth.BASE_S0, synth.BASE_D, n + 1)
params = poly.Params.__new__(poly.Params)
params.curve, params.k, params.n = curve, k, n
params._g = g
params.w = g.download(n, 1)
params.u = api.Bases.generate(curve, 4242, 1, 1).download()
g.precompute(0)  # Params use tables: ipa_bases() then builds g || w || u with its own table
p_dev = torch.from_numpy(synth.field_elements(0x1FA, n).view(np.int64)).cuda()
s_dev = torch.from_numpy(synth.field_elements(0x5A, n).view(np.int64)).cuda()


def opening(writer):
    draws = iter(range(7, 10 ** 9, 13))
    s_poly = s_dev.clone()  # the opening adjusts its constant term
    torch.cuda.synchronize()
    t = time.perf_counter()
    ipa.create_proof_native(params, lambda: next(draws), writer, p_dev, 0x1234, 0x77777, s_poly, 0x99)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, writer.finalize()


kinds = {"native": lambda: transcript.Blake2bWrite(curve), "closures": lambda: tm.Writer(curve)}
proofs = {name: opening(make())[1] for name, make in kinds.items()}  # warm-up
assert proofs["native"] == proofs["closures"] and len(proofs["native"]) == 32 * (2 * k + 3), "the two transcripts wrote different bytes"
times = {name: [] for name in kinds}
for _ in range(reps):
    for name, make in kinds.items():
        ms, proof = opening(make())
        assert proof == proofs[name]
        times[name].append(ms)
for name, ts in times.items():
    print(f"ipa k={k} {name:8s}: median {statistics.median(ts):.2f} ms, min {min(ts):.2f}, max {max(ts):.2f}  ({' '.join(f'{t:.2f}' for t in ts)})")
print(f"ipa k={k}: closures - native = {statistics.median(times['closures']) - statistics.median(times['native']):.2f} ms (medians of {reps})")

# 2. decoding
count = 256
pts = g.download(0, count)
w = transcript.Blake2bWrite(curve)
for row in pts:
    w.write_point(row)
data = w.finalize()
best = None
for _ in range(5):
    r = transcript.Blake2bRead(curve, data)
    t = time.perf_counter()
    for _ in range(count):
        r.read_point()
    dt = (time.perf_counter() - t) / count * 1e6
    best = dt if best is None else min(best, dt)
    assert r.finished()
lib, out = api.lib(), np.zeros(8, dtype=np.uint64)
out_p, raw = api._p(out), None
for _ in range(5):
    r = transcript.Blake2bRead(curve, data)
    t = time.perf_counter()
    for _ in range(count):
        lib.trh_tr_read_point(r.handle, out_p)
    dt = (time.perf_counter() - t) / count * 1e6
    raw = dt if raw is None else min(raw, dt)
print(f"read_point: {best:.1f} us per point through transcript.Blake2bRead, {raw:.1f} us through ctypes alone (best of 5 x {count})")
