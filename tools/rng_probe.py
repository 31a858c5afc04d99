"""Device time of the random-scalar fills (trh_rng_fill_dev, trh_rng_fill_rows_dev) beside the upload they replace: tools/rng_probe.py [out file]
Per field: fill of 2^18 and 2^24 elements, fill_rows of 400 x 6 blinding cells at row_len 2^18 -- trh_event_* around each call, median of REPS
after WARM warm-up calls -- and trh_memcpy_h2d of the same number of bytes from a pageable host array (host clock around the synchronous copy)."""
import ctypes, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from tiny_ram_halo2_amd import api
WARM, REPS = 3, 15
api.init(0)
lib = api.lib()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def event():
    e = api._vp()
    api._check(lib.trh_event_create(ctypes.byref(e)))
    return e


def device_ms(call):
    e0, e1 = event(), event()
    out = []
    for i in range(WARM + REPS):
        api._check(lib.trh_event_record(e0, None))
        call()
        api._check(lib.trh_event_record(e1, None))
        ms = ctypes.c_float(0)
        api._check(lib.trh_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        if i >= WARM:
            out.append(ms.value)
    lib.trh_event_destroy(e0); lib.trh_event_destroy(e1)
    return statistics.median(out), min(out), max(out)


def h2d_ms(dev, nbytes):
    src = np.random.default_rng(1).integers(0, 1 << 63, size=max(nbytes // 8, 1), dtype=np.uint64)
    out = []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api._check(lib.trh_memcpy_h2d(api._devptr(dev), src.ctypes.data_as(api._vp), nbytes))
        out.append((time.perf_counter() - t0) * 1e3)
    out = out[WARM:]
    return statistics.median(out), min(out), max(out)


say(f"rng_probe: {torch.cuda.get_device_name(0)}, median (min .. max) of {REPS} after {WARM} warm-up calls, ms")
rng = api.Rng(bytes(range(32)), 1)
rows, row_len, first, count = 400, 1 << 18, (1 << 18) - 6, 6
big = torch.empty((rows * row_len, 4), dtype=torch.int64, device="cuda")
for log_n in (18, 24):
    n = 1 << log_n
    for field in ("fp", "fq"):
        med, lo, hi = device_ms(lambda: rng.fill(field, big, n))
        say(f"fill      {field} n=2^{log_n:<2}            {med:9.4f} ({lo:.4f} .. {hi:.4f})   {n * 32 / med / 1e6:8.1f} GB/s stored   {med * 1e6 / n:7.4f} ns/element")
    med, lo, hi = h2d_ms(big, n * 32)
    say(f"memcpy_h2d   {n * 32:>10} B         {med:9.4f} ({lo:.4f} .. {hi:.4f})   {n * 32 / med / 1e6:8.1f} GB/s (pageable source, host clock)")
for field in ("fp", "fq"):
    med, lo, hi = device_ms(lambda: rng.fill_rows(field, big, rows, row_len, first, count))
    say(f"fill_rows {field} {rows} x {count} @ 2^18      {med:9.4f} ({lo:.4f} .. {hi:.4f})")
med, lo, hi = h2d_ms(big, rows * count * 32)
say(f"memcpy_h2d   {rows * count * 32:>10} B         {med:9.4f} ({lo:.4f} .. {hi:.4f})   (one contiguous copy; the blinding rows are {rows} separate 192-byte ranges)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
