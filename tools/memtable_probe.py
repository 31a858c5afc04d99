"""What the Mem table costs on the device, next to the host route it replaces: tools/memtable_probe.py [reps]
Two shapes at word_bits = 32, no tape:
  reference   the reference's table, full: max_rows = 2^16 rows in columns of 2^18 (k = 18) -- 60000 accesses over 5536 addresses
  large       m = 2^22 accesses over 2^18 addresses, columns of 2^23 rows
Three routes, alternating, medians of `reps` (default 9) after one untimed run each; the device route's columns and the host route's are
compared word for word before anything is timed.
  device, resident    trh_mem_table_dev on log arrays that are already on the device: device events around the call (the entry's two host
                      synchronisations lie inside the window) and wall time to a synchronise
  device, from numpy  memtable.build on numpy arrays: the four uploads, then the same call; wall time
  host                numpy: a stable argsort by address, the Init rows inserted, the carried value by a running maximum of the last Init /
                      Store row, the increments and their halves -- 13 u32 columns -- then witness.columns_from_ints from host memory; wall time"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import torch

from tiny_ram_halo2_amd import api, memtable, witness

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
field, word_bits = "fp", 32
EVEN = np.uint32(0x55555555)


def make_log(rng, m, n_addresses):
    pool = rng.choice(1 << 32, size=n_addresses, replace=False).astype(np.uint32)
    address = np.concatenate([pool, pool[rng.integers(0, n_addresses, size=m - n_addresses)]])
    rng.shuffle(address)
    time_ = np.cumsum(rng.integers(1, max(2, (1 << 32) // (m + 1)), size=m, dtype=np.uint64)).astype(np.uint32)
    is_store = rng.integers(0, 2, size=m).astype(bool)
    value = rng.integers(0, 1 << 32, size=m, dtype=np.uint32)
    return address, time_, value, is_store


def host_columns(address, time_, value, is_store):
    """the 13 columns as u32 arrays of `rows` entries (no tape: every run opens on a synthesized Init row whose value is 0); loads carry the
    table's value, whatever they claim"""
    m = len(address)
    order = np.argsort(address, kind="stable")
    a = address[order]
    head = np.ones(m, dtype=bool)
    head[1:] = a[1:] != a[:-1]
    at = np.arange(m) + np.cumsum(head)          # the row of every access; its run's Init row lies at at - 1 where head
    rows = m + int(head.sum())
    init = np.zeros(rows, dtype=bool)
    init[at[head] - 1] = True
    addr = np.zeros(rows, dtype=np.uint32)
    addr[at] = a
    addr[at[head] - 1] = a[head]
    tm = np.zeros(rows, dtype=np.uint32)
    tm[at] = time_[order]
    store = np.zeros(rows, dtype=bool)
    store[at] = is_store[order]
    own = np.zeros(rows, dtype=np.uint32)
    own[at] = value[order]
    holder = np.maximum.accumulate(np.where(init | store, np.arange(rows), 0))
    carried = own[holder]
    run_head = np.maximum.accumulate(np.where(init, np.arange(rows), 0))
    prev_addr = np.where(run_head > 0, addr[np.maximum(run_head, 1) - 1], 0).astype(np.uint32)
    addr_inc = np.where(addr > prev_addr, addr - prev_addr - np.uint32(1), 0).astype(np.uint32)
    prev_time = np.concatenate([[0], tm[:-1]]).astype(np.uint32)
    time_inc = np.where(init, 0, tm - prev_time).astype(np.uint32)
    one = np.ones(rows, dtype=np.uint32)
    return np.stack([one, addr, tm, init.astype(np.uint32), store.astype(np.uint32), (~init & ~store).astype(np.uint32), carried, addr_inc, time_inc,
                     addr_inc & EVEN, (addr_inc >> 1) & EVEN, time_inc & EVEN, (time_inc >> 1) & EVEN])


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def device_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def alternate(sides):
    """sides: {name: (timer, function)}"""
    for timer, fn in sides.values():
        timer(fn)
    times = {name: [] for name in sides}
    for _ in range(reps):
        for name, (timer, fn) in sides.items():
            times[name].append(timer(fn))
    for name, ts in times.items():
        print(f"   {name:42s}: median {statistics.median(ts):9.3f} ms, min {min(ts):9.3f}, max {max(ts):9.3f}")
    return {name: statistics.median(ts) for name, ts in times.items()}


api.init(0)
for label, m, n_addresses, n, max_rows in (("reference", 60000, 5536, 1 << 18, 1 << 16), ("large", 1 << 22, 1 << 18, 1 << 23, 1 << 23)):
    rng = np.random.default_rng(m)
    address, time_, value, is_store = make_log(rng, m, n_addresses)
    resident = [torch.from_numpy(x.view(np.int32)).cuda() for x in (address, time_, value, witness.pack_bits(is_store))]
    out = torch.empty((13, n, 4), dtype=torch.int64, device="cuda")
    out_host = torch.empty((13, n, 4), dtype=torch.int64, device="cuda")

    def device_resident():
        return memtable.build(field, word_bits, resident[0], resident[1], resident[2], resident[3], out=out, max_rows=max_rows, m=m)

    def device_from_numpy():
        return memtable.build(field, word_bits, address, time_, value, is_store, out=out, max_rows=max_rows)

    def host_route():
        witness.columns_from_ints(field, host_columns(address, time_, value, is_store), n, out=out_host)

    got = device_resident()
    host_route()
    torch.cuda.synchronize()
    assert got.rows == m + n_addresses and torch.equal(out, out_host), "the two routes differ"
    passes, tiles = api.stat("memtable_sort_passes"), api.stat("memtable_tiles")
    print(f"{label}: word_bits = {word_bits}, m = {m} accesses over {n_addresses} addresses -> {got.rows} rows (max_rows {max_rows}) in 13 columns of {n} = "
          f"{13 * n * 32 / 1e6:.0f} MB; {passes} sort passes, {tiles} tiles; {got.n_inconsistent} loads claim another value than the table carries; both routes agree")
    t0 = time.perf_counter()
    host_columns(address, time_, value, is_store)
    print(f"   (of the host route, numpy alone: {(time.perf_counter() - t0) * 1e3:.3f} ms, one run)")
    med = alternate({"device, resident (device events)": (device_ms, device_resident), "device, resident (wall)": (wall_ms, device_resident),
                     "device, from numpy (wall)": (wall_ms, device_from_numpy), "host: numpy + columns_from_ints (wall)": (wall_ms, host_route)})
    print(f"   host / device from numpy = {med['host: numpy + columns_from_ints (wall)'] / med['device, from numpy (wall)']:.2f}; "
          f"the resident call writes its {13 * n * 32 / 1e6:.0f} MB at {13 * n * 32 / med['device, resident (device events)'] / 1e6:.0f} GB/s end to end")
