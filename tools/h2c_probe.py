"""Device time of Params::new's generators (trh_hash_to_curve_indexed_dev, and its two kernels on their own): tools/h2c_probe.py [out file]
Per curve and n = 2^18, 2^20: trh_event_* around each call, median of REPS after WARM warm-up calls.  Under tools/prof_cmd.sh the kernel
trace splits the fused entry between h2c_hash_kernel and h2c_map_kernel."""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from tiny_ram_halo2_amd import api
WARM, REPS = 3, 9
PREFIX = api.HALO2_PARAMS_PREFIX
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


say(f"h2c_probe: {torch.cuda.get_device_name(0)}, median (min .. max) of {REPS} after {WARM} warm-up calls, ms")
xy = torch.empty((1 << 20, 8), dtype=torch.int64, device="cuda")
u = torch.empty((1 << 20, 8), dtype=torch.int64, device="cuda")
for log_n in (18, 20):
    n = 1 << log_n
    for curve in ("pallas", "vesta"):
        for name, call in (("hash_to_curve ", lambda: api.hash_to_curve_indexed_dev(curve, PREFIX, 0, 0, n, xy)),
                           ("hash_to_field ", lambda: api.hash_to_field_indexed_dev(curve, PREFIX, 0, 0, n, u)),
                           ("map_to_curve x2", lambda: api.map_to_curve_dev(curve, u, n, 2, xy))):
            med, lo, hi = device_ms(call)
            say(f"{name} {curve:6s} n=2^{log_n}   {med:9.4f} ({lo:.4f} .. {hi:.4f})   {med * 1e6 / n:8.2f} ns/point")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
