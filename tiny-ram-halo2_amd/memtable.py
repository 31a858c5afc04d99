"""The memory-consistency table on the device: an access log in execution order -> the 13 sorted, checked columns of the reference's Mem
chip (trh_mem_table_dev; csrc/memtable.hip over csrc/memtable.h).

It is the one table whose rows are no per-row function of the trace: the accesses are grouped by address (stable radix sort, time order kept
inside a run), every run is opened by an Init row (the tape word at that address, or 0), the most recently stored value is carried down the
run, and the two increments between neighbouring rows come with their even-bits halves.  The host hands over four word arrays and the tape.

    COLUMNS                         the 13 column names, in the order of the result
    build(field, word_bits, address, time, value, is_store, tape=(), n=...)  -> MemTable
    witness.AdviceBuilder.mem_table(first_column, ...)                       the same into the builder's column slices

A log that breaks a rule (a word >= 2^word_bits, a time of 0 or one that does not increase) or needs more than max_rows rows is refused
(api.TrhError; MemTableTooLong carries the rows it would need).  Loads that claim another value than the table carries are reported."""
from __future__ import annotations

import ctypes

import numpy as np

from . import api
from .witness import _device, _out, _stream, pack_bits

COLUMNS = ("s_trace", "address", "time", "init", "store", "load", "value", "addr_inc", "time_inc", "addr_inc_even", "addr_inc_odd", "time_inc_even",
           "time_inc_odd")
SORT_TILE = 2048  # csrc/memtable.h: records per workgroup of a sort pass
SCAN_TILE = 1024  # csrc/memtable.h: elements per workgroup of a scan
NO_SOURCE = 0xFFFFFFFF


class MemTableTooLong(api.TrhError):
    """rows > max_rows; .rows is what the table would need"""

    def __init__(self, message, rows):
        super().__init__(message)
        self.rows = rows


class MemTable:
    """columns: device tensor (13, n, 4) of Montgomery words; rows: the live rows; n_inconsistent / first_inconsistent: loads whose claimed
    value differs from the carried one, and the smallest log index among them (the log's length when there is none); src_index: device
    tensor (n,) int32 holding the u32 log index of every row, 0xFFFFFFFF (-1) for Init rows and behind the table"""

    def __init__(self, columns, rows, n_inconsistent, first_inconsistent, src_index):
        self.columns, self.rows, self.n_inconsistent, self.first_inconsistent, self.src_index = columns, rows, n_inconsistent, first_inconsistent, src_index

    def column(self, name):
        return self.columns[COLUMNS.index(name)]


def plan(m: int, t: int, word_bits: int) -> dict:
    """the host-visible part of csrc/memtable.h's plan: sort passes and tile counts"""
    records = m + t
    return {"passes": (word_bits + 7) // 8, "sort_tiles": -(-records // SORT_TILE), "scan_tiles": -(-records // SCAN_TILE)}


def _words(x, dev, what):
    """-> int32 device tensor holding u32 words"""
    import torch
    if torch.is_tensor(x):
        assert x.is_cuda and x.ndim == 1 and x.is_contiguous() and x.element_size() == 4, f"{what}: a contiguous device tensor of 32-bit words"
        return x
    a = np.ascontiguousarray(x)
    if a.dtype != np.uint32:
        assert a.size == 0 or (a.dtype.kind in "ui" and int(a.min()) >= 0 and int(a.max()) < 1 << 32), f"{what}: words of at most 32 bits"
        a = a.astype(np.uint32)
    return torch.from_numpy(a.reshape(-1).view(np.int32)).to(dev)


def build(field: str, word_bits: int, address, time, value, is_store, tape=(), n: int | None = None, max_rows: int | None = None, out=None, stream=None,
          m: int | None = None) -> MemTable:
    """address / time / value: m words each, numpy arrays (uploaded) or device tensors of 32-bit words; is_store: a bool array (packed with
    witness.pack_bits) or a device tensor of ceil(m / 32) bitmap words, which needs m=; tape: the tape's words.  n: rows per column
    (default: out's); max_rows: the table's extent (default n).  out: a (13, n, 4) int64 device tensor to write into."""
    import torch
    dev = _device() if out is None else out.device
    address, time, value = _words(address, dev, "address"), _words(time, dev, "time"), _words(value, dev, "value")
    if torch.is_tensor(is_store):
        assert m is not None, "a packed bitmap needs m="
        store_bits = _words(is_store, dev, "is_store")
    else:
        flags = np.asarray(is_store, dtype=np.bool_).reshape(-1)
        assert m is None or m == flags.size
        m = flags.size
        store_bits = _words(pack_bits(flags) if m else np.zeros(0, dtype=np.uint32), dev, "is_store")
    assert address.numel() >= m and time.numel() >= m and value.numel() >= m and store_bits.numel() >= (m + 31) // 32
    tape = _words(tape, dev, "tape")
    t = tape.numel()
    if n is None:
        assert out is not None, "n= or out="
        n = out.shape[1]
    out = _out(out, (len(COLUMNS), n, 4), dev)
    src_index = torch.empty((n,), dtype=torch.int32, device=dev)
    s = _stream(stream, dev)
    a = api.MemTableArgs(word_bits=word_bits, address=address.data_ptr() if m else None, time=time.data_ptr() if m else None, value=value.data_ptr() if m else None,
                         store_bits=store_bits.data_ptr() if m else None, m=m, tape=tape.data_ptr() if t else None, t=t, dst=out.data_ptr(), n=n,
                         max_rows=n if max_rows is None else max_rows, src_index=src_index.data_ptr(), stream=s)
    rc = api.lib().trh_mem_table_dev(api.FIELD_ID[field], ctypes.byref(a))
    if rc != 0:
        message = f"libtrh error {rc}: {api.lib().trh_last_error().decode()}"
        if a.rows > a.max_rows:
            raise MemTableTooLong(message, int(a.rows))
        raise api.TrhError(message)
    return MemTable(out, int(a.rows), int(a.n_inconsistent), int(a.first_inconsistent), src_index)
