"""What the Exe chips cost on the device: tools/exechips_probe.py [reps]  (writes profiles/exechips_probe.txt when its output is redirected there)
One shape: k = 18, reg_count = 8, word_bits = 32, m = 2^18 - 1 steps drawn independently (every opcode, both operand kinds), 60 columns of
2^18 rows = 503 MB.  Device events, medians of `reps` (default 9) after one untimed run each, alternating:
  entry             trh_exe_chips_dev on resident step arrays: the validation kernel, the host's read of its verdict (the entry's one
                    synchronisation lies inside the window), the row kernel and the inversion kernel over the a_flag column
  entry, no flag2   the same call with a chips table that has lost its flag2 bits: the inversion kernel finds no row to load, so this is
                    validation, verdict and the row kernel
  entry, refused    the same call with a last step that does not answer: validation and the verdict's read alone, nothing written
  fill              tensor.zero_() of the same destination
Then tools/exechips_inv_probe (built by `make tools/exechips_inv_probe`), a program of its own: the inversion kernel alone at strips of 1,
4 and 8 rows per lane next to a fill of its column, at k = 18, 20 and 22."""
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import torch

from tiny_ram_halo2_amd import api, exetable, witness

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
field, W, R, k = "fp", 32, 8, 18
n = 1 << k
m = n - 1
ncols = len(exetable.chip_columns(R))


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def alternate(sides):
    for fn in sides.values():
        device_ms(fn)
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            times[name].append(device_ms(fn))
    for name, ts in times.items():
        print(f"   {name:44s}: median {statistics.median(ts):9.3f} ms, min {min(ts):9.3f}, max {max(ts):9.3f}")
    return {name: statistics.median(ts) for name, ts in times.items()}


api.init(0)
rng = np.random.default_rng(k)
codes = np.array(sorted(exetable.OPCODES.values()), dtype=np.uint32)
op = codes[rng.integers(0, len(codes), size=m)]
op[-1] = exetable.ANSWER
a_is_reg = rng.integers(0, 2, size=m).astype(bool)
ri, rj = rng.integers(0, R, size=m, dtype=np.uint32), rng.integers(0, R, size=m, dtype=np.uint32)
word = lambda *shape: rng.integers(0, 1 << 32, size=shape, dtype=np.uint32)  # noqa: E731
a = np.where(a_is_reg, rng.integers(0, R, size=m, dtype=np.uint32), np.where(rng.integers(0, 4, size=m) == 0, rng.integers(1, 40, size=m, dtype=np.uint32), word(m)))  # shift amounts among the immediates
inst = op | ri << 8 | rj << 12 | a_is_reg.astype(np.uint32) << 16
flags = rng.integers(0, 2, size=m).astype(bool)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.int32)).cuda()  # noqa: E731
pc, inst_d, a_d, regs, bits, value = dev(word(m)), dev(inst), dev(a), dev(word(m, R)), dev(witness.pack_bits(flags)), dev(word(m))
bad = inst.copy()
bad[-1] = exetable.OPCODES["jmp"]
inst_bad = dev(bad)
out = torch.empty((ncols, n, 4), dtype=torch.int64, device="cuda")
no_flag2 = {name: bits_ & ~exetable.FLAG2 for name, bits_ in exetable.DEFAULT_CHIPS.items()}


def entry():
    exetable.build_chips(field, W, R, pc, inst_d, a_d, regs, bits, value, out=out, m=m)


def rows_only():
    exetable.build_chips(field, W, R, pc, inst_d, a_d, regs, bits, value, out=out, m=m, chips=no_flag2)


def refused():
    try:
        exetable.build_chips(field, W, R, pc, inst_bad, a_d, regs, bits, value, out=out, m=m)
    except api.TrhError:
        return
    raise AssertionError("a trace that does not answer was accepted")


rows_only()
assert api.stat("exechips_flag2_rows") == 0
entry()
flag2_rows = api.stat("exechips_flag2_rows")
with_flag2 = {exetable.OPCODES[name] for name, bits_ in exetable.DEFAULT_CHIPS.items() if bits_ & exetable.FLAG2}
assert flag2_rows == int(np.isin(op, list(with_flag2)).sum())
in_entry = 4 * 4 + 4 * R + 1 / 8
print(f"k = {k}: m = {m} steps, reg_count = {R}, word_bits = {W} -> {ncols} columns of {n} rows = {ncols * n * 32 / 1e6:.0f} MB; {flag2_rows} rows carry flag2 "
      f"({100 * flag2_rows / m:.0f} %); strip of the inversion kernel: {exetable.INVERSE_STRIP} rows per lane")
print(f"   bytes per row: the entry reads {in_entry:.3f} (pc, inst, a, value, {R} registers, one flag bit) and writes {ncols * 32}; the inversion reads and writes 32 more on a flag2 row")
med = alternate({"entry (validate, verdict, rows, inverse)": entry, "entry, no flag2 (validate, verdict, rows)": rows_only, "entry, refused (validate, verdict)": refused,
                 "tensor.zero_() of the destination": out.zero_})
e, r0, r, f = (med[key] for key in med)
gb = ncols * n * 32 / 1e6
print(f"   entry / fill = {e / f:.2f}; (entry - refused) / fill = {(e - r) / f:.2f}; rows alone: (no flag2 - refused) / fill = {(r0 - r) / f:.2f}; "
      f"the inversion inside the entry: entry - no flag2 = {e - r0:.3f} ms")
print(f"   the entry writes {gb / e:.0f} GB/s end to end, {gb / (e - r):.0f} GB/s behind its verdict; the row kernel {gb / (r0 - r):.0f} GB/s; the fill {gb / f:.0f} GB/s")
del out, pc, inst_d, a_d, regs, bits, value
torch.cuda.empty_cache()
sys.stdout.flush()
probe = os.path.join(ROOT, "tools", "exechips_inv_probe")
if os.path.exists(probe):
    for log_rows in (k, 20, 22):  # the strips part ways once the grid exceeds one wave per SIMD
        subprocess.run([probe, str(log_rows), str(reps)], check=True, timeout=300)
else:
    print("   tools/exechips_inv_probe is not built (make tools/exechips_inv_probe): the strips were not measured")
