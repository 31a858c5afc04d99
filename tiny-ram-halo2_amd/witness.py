"""Packed witness intake: columns from machine words and flag bits, expanded on the device (trh_columns_from_ints_*, trh_even_odd_split_dev,
trh_even_bits_table_dev; csrc/witness.hip).

Every instance and advice column of the reference's circuit is a flag, a WORD_BITS-bit word or an even-bits half of a word
(replay.column_classes), and a TinyRAM host knows them as machine integers before it wraps them in `F::from(u64)`.  Here it hands over
the integers -- one bit per flag, 1 .. 8 bytes per word, nothing for the halves of a word that is already resident -- and the device makes
the (columns, n, 4) Montgomery tensors that plonk.create_proof and mock.MockProver take.  The host does O(#columns) work, nothing per row.

    pack_bits(flags)                                  bool (cols, live) -> uint32 (cols, ceil(live / 32)), bit r & 31 of word r >> 5
    columns_from_ints(field, src, n)                  numpy array: from host memory (pageable is fine); torch device tensor: resident
    even_odd(field, words, n)                         the even-bits decomposition: w & 0x5555.., (w & 0xAAAA..) >> 1
    even_bits_table(field, word_bits, n)              the lookup table of the decomposition
    AdviceBuilder(field, num_advice, n)               owns the advice tensor; ints / even_odd / full / mem_table write into its column slices

The one table that is no per-row function of the trace, the memory-consistency table, is made from the access log by memtable.build
(AdviceBuilder.mem_table): sorted, scanned and checked on the device.  The Exe table's temporary variables and selectors are derived from
the steps themselves by exetable.build (AdviceBuilder.exe_table), and the Out, changed and sub-chip columns of the same steps by
exetable.build_chips (AdviceBuilder.exe_chips).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import api

BITS, U8, U16, U32, U64, I32, I64 = range(7)  # TRH_INT_*
KINDS = {"bits": BITS, "u8": U8, "u16": U16, "u32": U32, "u64": U64, "i32": I32, "i64": I64}
_KIND_BYTES = {BITS: 4, U8: 1, U16: 2, U32: 4, U64: 8, I32: 4, I64: 8}
_NUMPY_KINDS = {("u", 1): U8, ("u", 2): U16, ("u", 4): U32, ("u", 8): U64, ("i", 4): I32, ("i", 8): I64}


def pack_bits(flags) -> np.ndarray:
    """bool (cols, live) or (live,) -> uint32 (cols, ceil(live / 32)) or (ceil(live / 32),): row r is bit r & 31 of word r >> 5; the bits of
    the last word behind `live` are clear"""
    flags = np.asarray(flags)
    assert flags.dtype == np.bool_ and flags.ndim in (1, 2)
    live = flags.shape[-1]
    words = (live + 31) // 32
    by = np.packbits(flags, axis=-1, bitorder="little")
    pad = [(0, 0)] * (flags.ndim - 1) + [(0, 4 * words - by.shape[-1])]
    return np.ascontiguousarray(np.pad(by, pad)).view("<u4").astype(np.uint32, copy=False)


def _torch_kinds():
    import torch
    kinds = {torch.uint8: U8, torch.int32: I32, torch.int64: I64}
    for name, kind in (("uint16", U16), ("uint32", U32), ("uint64", U64)):
        if hasattr(torch, name):
            kinds[getattr(torch, name)] = kind
    return kinds


def _device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _source(src, kind, live):
    """-> (kind id, address, stride in elements, columns, live rows, is it host memory, one-dimensional, the object that keeps the memory alive)"""
    import torch
    on_host = not torch.is_tensor(src)
    if on_host:
        src = np.asarray(src)
        if src.dtype == np.bool_:
            assert kind is None and live is None, "a bool array is packed here: neither kind nor live applies"
            kind, live, src = "bits", src.shape[-1], pack_bits(src)
        found = _NUMPY_KINDS.get((src.dtype.kind, src.dtype.itemsize))
        item, strides, address = src.dtype.itemsize, src.strides, src.ctypes.data
    else:
        assert src.is_cuda, "a torch source is device memory; pass host data as a numpy array"
        found = _torch_kinds().get(src.dtype)
        item, strides, address = src.element_size(), [s * src.element_size() for s in src.stride()], src.data_ptr()
    kid = found if kind is None else KINDS[kind]
    if kid is None:
        raise TypeError(f"no integer kind for dtype {src.dtype}: u8, u16, u32, u64, i32 or i64 (or name one with kind=)")
    if _KIND_BYTES[kid] != item:
        raise TypeError(f"kind {kid} has {_KIND_BYTES[kid]}-byte elements, dtype {src.dtype} {item}-byte ones")
    assert src.ndim in (1, 2), "one column (rows,) or (columns, rows)"
    one_d = src.ndim == 1
    cols, elems = (1, src.shape[0]) if one_d else src.shape
    if elems > 1 and strides[-1] != item:
        raise ValueError("the rows of a column must be contiguous")
    stride = elems if one_d or cols <= 1 else strides[0] // item
    if not one_d and cols > 1 and (strides[0] % item or strides[0] < 0):
        raise ValueError("columns must lie a whole, non-negative number of elements apart")
    if kid == BITS:
        assert live is not None and (live + 31) // 32 <= elems, "a bitmap needs live=, at most 32 rows per word"
    else:
        assert live is None or live <= elems
        live = elems if live is None else live
    return kid, address, stride, cols, live, on_host, one_d, src


def _out(out, shape, dev):
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.int64, device=dev)
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == tuple(shape), (tuple(out.shape), tuple(shape))
    return out


def _stream(stream, dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream if stream is None else stream


def columns_from_ints(field: str, src, n: int, out=None, stream=None, kind: str | None = None, live: int | None = None):
    """src -> device tensor (columns, n, 4) of Montgomery words -- (n, 4) for a one-dimensional src -- with the values in the first `live`
    rows and zero behind.  src: a numpy array (host memory, staged through the context's pinned ring: trh_columns_from_ints_host) or a torch
    device tensor (trh_columns_from_ints_dev), (rows,) or (columns, rows) with contiguous rows -- a slice `big[:, :live]` keeps its stride.
    The dtype picks the kind (u8, u16, u32, u64, i32, i64); bool arrays are packed first (pack_bits); kind="bits" with live= takes a
    bitmap of u32 words as it is, and kind= names the kind of a tensor whose dtype torch lacks (u32 words held as int32).
    Asynchronous on `stream` (default: torch's current one); the host form returns when src has been read."""
    kid, address, stride, cols, live, on_host, one_d, keep = _source(src, kind, live)
    dev = _device() if on_host else keep.device
    out = _out(out, (n, 4) if one_d else (cols, n, 4), dev)
    a = api.IntsArgs(kind=kid, src=address, src_stride=stride, n_cols=cols, live_rows=live, dst=out.data_ptr(), dst_odd=None, n=n, stream=_stream(stream, dev))
    fn = api.lib().trh_columns_from_ints_host if on_host else api.lib().trh_columns_from_ints_dev
    api._check(fn(api.FIELD_ID[field], ctypes.byref(a)))
    return out


def to_device_words(words):
    """an unsigned numpy array -> (device tensor of the same bytes, kind name): torch lacks most unsigned dtypes, so the words travel as
    the signed dtype of their size and keep their kind by name"""
    import torch
    words = np.ascontiguousarray(words)
    assert words.dtype.kind == "u" and words.dtype.itemsize in (1, 2, 4, 8)
    name = f"u{8 * words.dtype.itemsize}"
    signed = words if words.dtype == np.uint8 else words.view(f"i{words.dtype.itemsize}")
    return torch.from_numpy(signed).to(_device()), name


def even_odd(field: str, src, n: int, out_even=None, out_odd=None, stream=None, kind: str | None = None):
    """the even-bits decomposition of unsigned words (trh_even_odd_split_dev): -> (even, odd), shaped like columns_from_ints' result, with
    even = w & 0x5555.., odd = (w & 0xAAAA..) >> 1, so even + 2 odd = w.  src: a torch device tensor (kind= names an unsigned kind its dtype
    cannot, as in columns_from_ints) or an unsigned numpy array, whose packed words are sent to the device first -- the halves never cross."""
    import torch
    if not torch.is_tensor(src):
        assert kind is None
        src, kind = to_device_words(src)
    kid, address, stride, cols, live, _, one_d, keep = _source(src, kind, None)
    if kid not in (U8, U16, U32, U64):
        raise TypeError("even_odd takes unsigned words (u8, u16, u32, u64)")
    shape = (n, 4) if one_d else (cols, n, 4)
    out_even, out_odd = _out(out_even, shape, keep.device), _out(out_odd, shape, keep.device)
    a = api.IntsArgs(kind=kid, src=address, src_stride=stride, n_cols=cols, live_rows=live, dst=out_even.data_ptr(), dst_odd=out_odd.data_ptr(), n=n,
                     stream=_stream(stream, keep.device))
    api._check(api.lib().trh_even_odd_split_dev(api.FIELD_ID[field], ctypes.byref(a)))
    return out_even, out_odd


def even_bits_table(field: str, word_bits: int, n: int, out=None, stream=None):
    """-> device tensor (n, 4): row i < 2^(word_bits / 2) holds sum_j bit_j(i) 4^j, the rows behind are zero (trh_even_bits_table_dev)"""
    dev = _device() if out is None else out.device
    out = _out(out, (n, 4), dev)
    a = api.EvenBitsTableArgs(word_bits=word_bits, dst=out.data_ptr(), n=n, stream=_stream(stream, dev))
    api._check(api.lib().trh_even_bits_table_dev(api.FIELD_ID[field], ctypes.byref(a)))
    return out


class AdviceBuilder:
    """Owns the (num_advice, n, 4) tensor plonk.create_proof takes and fills it column by column, straight into its slices: no intermediate
    copy of a column exists on either side of the link.  Columns nobody writes stay zero."""

    def __init__(self, field: str, num_advice: int, n: int):
        import torch
        self.field, self.num_advice, self.n = field, num_advice, n
        self._t = torch.zeros((num_advice, n, 4), dtype=torch.int64, device=_device())

    def _slice(self, first: int, count: int):
        assert 0 <= first and first + count <= self.num_advice, (first, count, self.num_advice)
        return self._t[first:first + count]

    def ints(self, first_column: int, array, kind: str | None = None, live: int | None = None) -> None:
        """columns first_column .. from the rows of `array` ((columns, live), or (live,) for one column): see columns_from_ints"""
        import torch
        shape = array.shape if torch.is_tensor(array) else np.shape(array)
        if len(shape) == 1:
            columns_from_ints(self.field, array, self.n, out=self._t[first_column], kind=kind, live=live)
        else:
            columns_from_ints(self.field, array, self.n, out=self._slice(first_column, shape[0]), kind=kind, live=live)

    def even_odd(self, word_array, first_even_column: int, first_odd_column: int, kind: str | None = None) -> None:
        """the halves of the words of `word_array` ((columns, live) or (live,)) into columns first_even_column .. and first_odd_column .."""
        import torch
        shape = word_array.shape if torch.is_tensor(word_array) else np.shape(word_array)
        if len(shape) == 1:
            even_odd(self.field, word_array, self.n, out_even=self._t[first_even_column], out_odd=self._t[first_odd_column], kind=kind)
        else:
            even_odd(self.field, word_array, self.n, out_even=self._slice(first_even_column, shape[0]), out_odd=self._slice(first_odd_column, shape[0]), kind=kind)

    def full(self, column: int, limbs) -> None:
        """a column of full field elements: limbs is (rows <= n, 4) Montgomery words, a uint64 numpy array or a device tensor"""
        import torch
        if not torch.is_tensor(limbs):
            limbs = torch.from_numpy(np.ascontiguousarray(limbs, dtype=np.uint64).view(np.int64))
        assert limbs.ndim == 2 and limbs.shape[1] == 4 and limbs.shape[0] <= self.n
        self._t[column, :limbs.shape[0]].copy_(limbs)

    def mem_table(self, first_column: int, word_bits: int, address, time, value, is_store, tape=(), max_rows: int | None = None, stream=None, m: int | None = None):
        """the memory-consistency table of an access log into the 13 columns first_column .. (memtable.COLUMNS, memtable.build): -> MemTable
        whose .columns is the builder's own slice"""
        from . import memtable
        return memtable.build(self.field, word_bits, address, time, value, is_store, tape=tape, max_rows=max_rows, out=self._slice(first_column, len(memtable.COLUMNS)),
                              stream=stream, m=m)

    def exe_table(self, first_column: int, word_bits: int, reg_count: int, pc, inst, a, regs, flags, value, selection=None, stream=None, m: int | None = None):
        """the Exe table of a trace's steps into the 28 + 9 reg_count columns first_column .. (exetable.columns, exetable.build): -> the
        builder's own slice"""
        from . import exetable
        return exetable.build(self.field, word_bits, reg_count, pc, inst, a, regs, flags, value, selection=selection,
                              out=self._slice(first_column, 28 + 9 * reg_count), stream=stream, m=m)

    def exe_chips(self, first_column: int, word_bits: int, reg_count: int, pc, inst, a, regs, flags, value, selection=None, chips=None, stream=None,
                  m: int | None = None):
        """the sub-chips' columns of the same steps into the 52 + reg_count columns first_column .. (exetable.chip_columns,
        exetable.build_chips): -> the builder's own slice"""
        from . import exetable
        return exetable.build_chips(self.field, word_bits, reg_count, pc, inst, a, regs, flags, value, selection=selection, chips=chips,
                                    out=self._slice(first_column, 52 + reg_count), stream=stream, m=m)

    def tensor(self):
        return self._t
