"""What the packed witness intake costs at the reference's shape: tools/witness_probe.py [k] [reps]
The columns are replay.column_classes(32)'s instance and advice columns -- 220 flags, 114 words, 23 even-bits halves -- at 2^k rows (default
k = 18) with the first n / 4 live.  The halves come out of the split in pairs, so the destination has one spare column: 358.  Medians of
`reps` (default 9), the two sides of every comparison alternating, after one untimed run each.
1. The expansion from RESIDENT bitmaps and words (three launches: bits, u32 words, the split of 12 words) against a plain device fill of
   the same destination (tensor.zero_()), timed with device events.
2. Intake from PAGEABLE host memory: bitmaps and words through trh_columns_from_ints_host plus the split on the device, against the full
   32-byte columns through trh_memcpy_h2d -- from one buffer again and again, which the runtime page-locks at first sight, and from a
   fresh copy every time; wall time to a device synchronise, and the bytes each moved (trh_io_stats for the packed route).
3. One instance column of n / 4 values through plonk._instance_columns: a Python list (multiopen._limbs_many) against a numpy array."""
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import torch

from tiny_ram_halo2_amd import api, plonk, replay, witness

k = int(sys.argv[1]) if len(sys.argv) > 1 else 18
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
field, n = "fp", 1 << k
live = n // 4
classes = [c for c in replay.column_classes(32) if c[1] in ("flag", "word", "even")]
n_flag, n_word, n_even = (sum(c[0] for c in classes if c[1] == kind) for kind in ("flag", "word", "even"))
n_split = (n_even + 1) // 2
total = n_flag + n_word + 2 * n_split
print(f"k = {k}: {n_flag} flag, {n_word} word and {n_even} even-bits columns of {n} rows, {live} live; destination {total} columns = {total * n * 32 / 1e9:.2f} GB")

api.init(0)
rng = np.random.default_rng(0x517)
flags = rng.integers(0, 2, size=(n_flag, live)).astype(bool)
words = rng.integers(0, 1 << 32, size=(n_word, live), dtype=np.uint32)
bitmaps = witness.pack_bits(flags)
d_bitmaps = torch.from_numpy(bitmaps.view(np.int32)).cuda()
d_words, _ = witness.to_device_words(words)
dst = torch.empty((total, n, 4), dtype=torch.int64, device="cuda")
lo, mid = n_flag, n_flag + n_word


def split():
    witness.even_odd(field, d_words[:n_split], n, out_even=dst[mid:mid + n_split], out_odd=dst[mid + n_split:], kind="u32")


def expand_resident():
    witness.columns_from_ints(field, d_bitmaps, n, out=dst[:lo], kind="bits", live=live)
    witness.columns_from_ints(field, d_words, n, out=dst[lo:mid], kind="u32")
    split()


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(sides, timer, prepare=None):
    """prepare: {name: function} run before every timed call of that side, outside the timed window"""
    prepare = prepare or {}
    for name, fn in sides.items():
        prepare.get(name, lambda: None)()
        timer(fn)
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            prepare.get(name, lambda: None)()
            times[name].append(timer(fn))
    for name, ts in times.items():
        print(f"   {name:28s}: median {statistics.median(ts):9.3f} ms, min {min(ts):9.3f}, max {max(ts):9.3f}")
    return {name: statistics.median(ts) for name, ts in times.items()}


print("1. resident sources -> columns, against a device fill of the same destination (device events)")
m = alternate({"expand (3 launches)": expand_resident, "tensor.zero_()": dst.zero_}, device_ms)
print(f"   expand / fill = {m['expand (3 launches)'] / m['tensor.zero_()']:.2f};  expand writes {total * n * 32 / m['expand (3 launches)'] / 1e6:.0f} GB/s, "
      f"the fill {total * n * 32 / m['tensor.zero_()'] / 1e6:.0f} GB/s")

expand_resident()
torch.cuda.synchronize()
full = dst[:mid + n_even].cpu().numpy()   # the full-width columns in pageable host memory: what the ABI took before
full_dev = dst[:mid + n_even]
lib = api.lib()


def packed_route():
    witness.columns_from_ints(field, bitmaps, n, out=dst[:lo], kind="bits", live=live)
    witness.columns_from_ints(field, words, n, out=dst[lo:mid])
    split()


def full_route():
    api._check(lib.trh_memcpy_h2d(full_dev.data_ptr(), full.ctypes.data, full.nbytes))


fresh = [None]


def make_fresh():
    fresh[0] = None
    fresh[0] = full.copy()   # pages the runtime has not seen: a witness is new memory for every proof


def full_route_fresh():
    api._check(lib.trh_memcpy_h2d(full_dev.data_ptr(), fresh[0].ctypes.data, fresh[0].nbytes))


print("2. pageable host memory -> columns on the device (wall time to a synchronise)")
api.io_stats(reset=True)
packed_route()
torch.cuda.synchronize()
packed_bytes = api.io_stats()["h2d_bytes"]
m = alternate({"packed (bitmaps + u32 words)": packed_route, "full width, same buffer": full_route, "full width, fresh buffer": full_route_fresh}, wall_ms,
              prepare={"full width, fresh buffer": make_fresh})
print(f"   bytes over the link: packed {packed_bytes / 1e6:.2f} MB (trh_io_stats), full width {full.nbytes / 1e6:.2f} MB (trh_memcpy_h2d): 1 : {full.nbytes / packed_bytes:.1f}")
print(f"   time full / packed = {m['full width, same buffer'] / m['packed (bitmaps + u32 words)']:.1f} (a buffer the runtime has page-locked at first sight), "
      f"{m['full width, fresh buffer'] / m['packed (bitmaps + u32 words)']:.1f} (a fresh buffer)")

print(f"3. one instance column of {live} values through plonk._instance_columns")
cs = types.SimpleNamespace(field=field, num_instance=1, usable_rows=lambda rows: rows - 6)
values = rng.integers(0, 1 << 32, size=live, dtype=np.uint64)
as_list = [int(v) for v in values]
dev = torch.device("cuda", 0)
a, b = plonk._instance_columns(cs, n, [as_list], dev), plonk._instance_columns(cs, n, [values], dev)
torch.cuda.synchronize()
assert torch.equal(a, b)
m = alternate({"list of ints (_limbs_many)": lambda: plonk._instance_columns(cs, n, [as_list], dev),
               "numpy uint64 array": lambda: plonk._instance_columns(cs, n, [values], dev)}, wall_ms)
print(f"   list / array = {m['list of ints (_limbs_many)'] / m['numpy uint64 array']:.1f}")
