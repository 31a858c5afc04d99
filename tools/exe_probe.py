"""What the Exe table costs on the device: tools/exe_probe.py [reps]  (writes profiles/exe_probe.txt when its output is redirected there)
One shape: k = 18, reg_count = 8, word_bits = 32, m = 2^18 - 1 steps drawn independently (every opcode, both operand kinds), 100 columns of
2^18 rows = 839 MB.  Device events, medians of `reps` (default 9) after one untimed run each, alternating:
  entry             trh_exe_table_dev on resident step arrays: the validation kernel, the host's read of its verdict (the entry's one
                    synchronisation lies inside the window) and the row kernel
  entry, refused    the same call with a last step that does not answer: validation and the verdict's read alone, nothing written -- what
                    the entry spends before its row kernel starts
  fill              tensor.zero_() of the same destination
  expand            witness.columns_from_ints of the same 100 columns from resident, already-computed words and bitmaps (84 bit columns,
                    12 u32 columns, the four temporary variables as i64): three launches.  The words are taken back from the entry's own
                    output first, and the expansion's columns are compared with the entry's word for word before anything is timed.  The
                    shr steps shift by an immediate in 1 .. 31: by 0 or by 32 the cell 2^s RJ - 2^32 (RJ >> s) leaves the range of an i64
                    column -- the entry writes such cells, the expansion cannot hold them."""
import ctypes
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import pasta
import torch

from tiny_ram_halo2_amd import api, exetable, witness

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
field, W, R, k = "fp", 32, 8, 18
n = 1 << k
m = n - 1
names = exetable.columns(R)
ncols = len(names)


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
shr = op == exetable.OPCODES["shr"]
a_is_reg &= ~shr
a = np.where(shr, rng.integers(1, 32, size=m, dtype=np.uint32), a)
inst = op | ri << 8 | rj << 12 | a_is_reg.astype(np.uint32) << 16
flags = rng.integers(0, 2, size=m).astype(bool)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).reshape(-1).view(np.int32)).cuda()  # noqa: E731
pc, inst_d, a_d, regs, bits, value = dev(word(m)), dev(inst), dev(a), dev(word(m, R)), dev(witness.pack_bits(flags)), dev(word(m))
bad = inst.copy()
bad[-1] = exetable.OPCODES["jmp"]
inst_bad = dev(bad)
out = torch.empty((ncols, n, 4), dtype=torch.int64, device="cuda")


def entry():
    exetable.build(field, W, R, pc, inst_d, a_d, regs, bits, value, out=out, m=m)


def refused():
    try:
        exetable.build(field, W, R, pc, inst_bad, a_d, regs, bits, value, out=out, m=m)
    except api.TrhError:
        return
    raise AssertionError("a trace that does not answer was accepted")


# the words of the same columns, from the entry's own output: canonical limbs, the low one is the value; a negative value is m - |v|
entry()
plain = torch.empty_like(out)
api._check(api.lib().trh_field_op_dev(api.FIELD_ID[field], api.FIELD_OPS["from_mont"], ctypes.c_void_p(out.data_ptr()), None, ctypes.c_void_p(plain.data_ptr()), ncols * n, None))
torch.cuda.synchronize()
bit_cols = [i for i, name in enumerate(names) if name in ("s_trace", "flag") or name[:3] in ("sa_", "sb_", "sc_", "sd_")]
tv_cols = [names.index(f"tv_{v}") for v in "abcd"]
u32_cols = [i for i in range(ncols) if i not in bit_cols and i not in tv_cols]
assert (len(bit_cols), len(u32_cols), len(tv_cols)) == (84, 12, 4)
low = plain[:, :, 0]
assert int(low[bit_cols].max()) == 1 and not bool(plain[bit_cols + u32_cols][:, :, 1:].any())
weights = torch.ones(32, dtype=torch.int64, device="cuda") << torch.arange(32, device="cuda")
bitmaps = (low[bit_cols].reshape(len(bit_cols), n // 32, 32) * weights).sum(-1).to(torch.int32).contiguous()
words32 = low[u32_cols].to(torch.int32).contiguous()
p0 = pasta.FIELDS[field].m & ((1 << 64) - 1)
negative = (plain[tv_cols][:, :, 1:] != 0).any(-1)
words64 = torch.where(negative, low[tv_cols] - (p0 - (1 << 64) if p0 >> 63 else p0), low[tv_cols]).contiguous()
n_negative = int(negative.sum())
del plain, low
out_b = torch.empty_like(out)


def expand():
    witness.columns_from_ints(field, bitmaps, n, out=out_b[:84], kind="bits", live=n)
    witness.columns_from_ints(field, words32, n, out=out_b[84:96], kind="u32")
    witness.columns_from_ints(field, words64, n, out=out_b[96:], kind="i64")


expand()
torch.cuda.synchronize()
order = torch.tensor(bit_cols + u32_cols + tv_cols, device="cuda")
for j in range(ncols):
    assert torch.equal(out_b[j], out[int(order[j])]), f"the two routes differ in column {names[int(order[j])]}"
in_entry, in_expand = 4 * 4 + 4 * R + 1 / 8, 84 / 8 + 12 * 4 + 4 * 8
print(f"k = {k}: m = {m} steps, reg_count = {R}, word_bits = {W} -> {ncols} columns of {n} rows = {ncols * n * 32 / 1e6:.0f} MB; {n_negative} negative cells (shr); "
      f"the expansion of the same words agrees word for word")
print(f"   bytes per row: the entry reads {in_entry:.3f} (pc, inst, a, value, {R} registers, one flag bit) and writes {ncols * 32}; the expansion reads "
      f"{in_expand:.1f} (84 bits, 12 u32, 4 i64) that something has to have computed first")
med = alternate({"entry (validate, verdict, rows)": entry, "entry, refused (validate, verdict)": refused, "tensor.zero_() of the destination": out.zero_,
                 "expand the same columns (3 launches)": expand})
e, r, f, x = (med[key] for key in med)
gb = ncols * n * 32 / 1e6
print(f"   entry / fill = {e / f:.2f}; (entry - refused) / fill = {(e - r) / f:.2f}; expand / fill = {x / f:.2f}; entry / expand = {e / x:.2f}")
print(f"   the entry writes {gb / e:.0f} GB/s end to end, {gb / (e - r):.0f} GB/s behind its verdict; the fill {gb / f:.0f} GB/s; the expansion {gb / x:.0f} GB/s")
