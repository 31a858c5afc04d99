"""The packed witness intake on the device (tiny_ram_halo2_amd.witness over trh_columns_from_ints_*, trh_even_odd_split_dev and
trh_even_bits_table_dev): machine words and flag bits in, columns of Montgomery words out, bit-exact against oracle/pasta.py.

  kinds        every kind x both fields, three columns a stride of live + 3 apart, live around the word of a bitmap and the 256 elements of
               a workgroup, device and host form, 0xFF-filled destination between two guard columns
  grid         one u32 column longer than one pass of the grid, brought back through the ABI's from_mont
  host = dev   a packed source larger than one ring slot, 70 columns, and three columns that take two staging chunks
  even_odd     the halves and even + 2 odd = word;  even_bits_table against the explicit spread;  every refusal leaves the destination alone
  stream       a source written on a non-default stream, expanded there without a synchronisation in between
  end to end   circuit B (the logic chip) at k = 5 and 10 with its witness handed over as bitmaps and u32 words, the halves and the table
               made on the device: same tensors, same proof bytes as the host-built witness; a flipped source bit is caught
  instances    an instance column as np.uint64 gives the proof of the same values as a Python list
  native       tests/native/witness_test.cpp over include/trh.hpp"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pasta as o
import plonk_circuits as pc
from tiny_ram_halo2_amd import api, mock, plonk, poly, witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, COLS = 1024, 3
LIVES = [0, 1, 31, 32, 33, 255, 256, 257, 1000, 1024]   # the workgroup is 256 elements, a bitmap word 32
EXTREMES = {"u8": [0, 1, 255], "u16": [0, 1, 65535], "u32": [0, 1, (1 << 32) - 1], "u64": [0, 1, (1 << 32) - 1, 1 << 63, (1 << 64) - 1],
            "i32": [0, -1, (1 << 31) - 1, -(1 << 31)], "i64": [0, -1, 1 << 31, -(1 << 31), (1 << 63) - 1, -(1 << 63)]}
PATTERNS = [0, (1 << 64) - 1, int("10" * 32, 2), int("01" * 32, 2)]   # the split's: none, all, odd positions, even positions
DTYPE = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64, "i32": np.int32, "i64": np.int64}
FILL = -1  # every byte 0xFF


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


def oracle_limbs(field, values):
    f = o.FIELDS[field]
    return np.array([f.limbs(int(v) % f.m) for v in values], dtype=np.uint64).reshape(len(values), 4)


def to_dev(field, columns):
    f = o.FIELDS[field]
    return torch.from_numpy(np.array([[f.limbs(v % f.m) for v in col] for col in columns], dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def field_op(field, op, a, b=None):
    out = torch.empty_like(a)
    api._check(api.lib().trh_field_op_dev(api.FIELD_ID[field], api.FIELD_OPS[op], a.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                                          a.numel() // 4, torch.cuda.current_stream().cuda_stream))
    return out


@functools.lru_cache(maxsize=None)
def values_of(kind, patterns=False):
    """(COLS, N) integers of one kind: the extreme values (or the split's patterns, cut to the kind's width) first, random ones behind"""
    bits = int(kind[1:])
    rng = np.random.default_rng(bits + (kind[0] == "i") + 2 * patterns)
    lo, hi = (-(1 << (bits - 1)), 1 << (bits - 1)) if kind[0] == "i" else (0, 1 << bits)
    first = [p & ((1 << bits) - 1) for p in PATTERNS] if patterns else EXTREMES[kind]
    return tuple(tuple(first + [int(v) for v in rng.integers(lo, hi - 1, size=N - len(first), dtype=DTYPE[kind], endpoint=True)]) for _ in range(COLS))


@functools.lru_cache(maxsize=None)
def reference(field, kind, patterns=False, part=None):
    """(COLS, N, 4) limbs of values_of, or of their even / odd parts: computed once, sliced by every test, never written"""
    even = int("01" * 32, 2)
    pick = {None: lambda v: v, "even": lambda v: v & even, "odd": lambda v: (v >> 1) & even}[part]
    ref = np.stack([oracle_limbs(field, [pick(v) for v in col]) for col in values_of(kind, patterns)])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def flag_values():
    return np.random.default_rng(0xB17).integers(0, 2, size=(COLS, N)).astype(bool)


def strided_source(kind, live, patterns=False):
    """-> numpy (COLS, live) view whose columns lie live + 3 elements apart (for u8 .. u32 a column then starts at an odd element offset)"""
    flat = np.full(COLS * (live + 3), 0x5A, dtype=DTYPE[kind])
    view = flat.reshape(COLS, live + 3)[:, :live]
    view[:] = np.array([col[:live] for col in values_of(kind, patterns)], dtype=DTYPE[kind]).reshape(COLS, live)
    assert live == 0 or view.strides[0] == (live + 3) * flat.itemsize
    return view


def device_view(view, kind):
    """the same words, the same stride, in device memory (torch keeps unsigned words as the signed dtype of their size)"""
    live = view.shape[1]
    base = view.base if view.base is not None else view
    flat = np.ascontiguousarray(base).reshape(-1)
    t = torch.from_numpy(flat if flat.dtype == np.uint8 else flat.view(f"i{flat.itemsize}")).cuda()
    return t.reshape(COLS, -1)[:, :live]


def guarded(cols=COLS, n=N):
    buf = torch.full((cols + 2, n, 4), FILL, dtype=torch.int64, device="cuda")
    return buf, buf[1:cols + 1]


def guards_intact(buf):
    return bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all())


# ---- 1. every kind x both fields ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fp", "fq"])
@pytest.mark.parametrize("kind", sorted(EXTREMES))
def test_every_integer_kind(kind, field):
    ref = reference(field, kind)
    for live in LIVES:
        want = np.zeros((COLS, N, 4), dtype=np.uint64)
        want[:, :live] = ref[:, :live]
        src = strided_source(kind, live)
        for form, source in (("host", src), ("dev", device_view(src, kind))):
            buf, out = guarded()
            witness.columns_from_ints(field, source, N, out=out, kind=kind)
            assert (host(out) == want).all(), (kind, field, live, form)
            assert guards_intact(buf), (kind, field, live, form)


@pytest.mark.parametrize("field", ["fp", "fq"])
def test_bitmaps(field):
    one = oracle_limbs(field, [1])[0]
    flags = flag_values()
    for live in LIVES:
        want = np.zeros((COLS, N, 4), dtype=np.uint64)
        want[:, :live][flags[:, :live]] = one
        words = (live + 31) // 32
        flat = np.full(COLS * (words + 3), 0xFFFFFFFF, dtype=np.uint32)      # set bits all around the live ones
        view = flat.reshape(COLS, words + 3)[:, :words]
        packed = witness.pack_bits(flags[:, :live])
        if live % 32:
            packed[:, -1] |= np.uint32((0xFFFFFFFF << (live % 32)) & 0xFFFFFFFF)   # the bits behind `live` in the last word
        view[:] = packed
        for form, source in (("host", view), ("dev", torch.from_numpy(flat.view(np.int32)).cuda().reshape(COLS, words + 3)[:, :words])):
            buf, out = guarded()
            witness.columns_from_ints(field, source, N, out=out, kind="bits", live=live)
            assert (host(out) == want).all(), (field, live, form)
            assert guards_intact(buf), (field, live, form)
        if live:  # a bool array is packed on the way
            assert (host(witness.columns_from_ints(field, flags[:, :live], N)) == want).all(), (field, live)


# ---- 2. past one pass of the grid -----------------------------------------------------------------------------------------------------------
def test_a_column_longer_than_one_pass_of_the_grid():
    field, live, n = "fq", (1 << 20) + 5, 1 << 21
    src = np.random.default_rng(2).integers(0, 1 << 32, size=live, dtype=np.uint32)
    src[:3], src[-1] = [0, 1, (1 << 32) - 1], (1 << 32) - 1
    out = witness.columns_from_ints(field, src, n)
    plain = host(field_op(field, "from_mont", out))
    assert (plain[:live, 0] == src).all() and not plain[:live, 1:].any() and not plain[live:].any()
    got = host(out)
    assert (got[:64] == oracle_limbs(field, src[:64])).all() and (got[live - 64:live] == oracle_limbs(field, src[-64:])).all()


# ---- 3. the host form equals the dev form byte for byte ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["ring slot", "70 columns", "two chunks"])
def test_host_form_equals_dev_form(shape):
    rng = np.random.default_rng(3)
    if shape == "ring slot":     # one column whose packed bytes exceed one 16 MiB slot of the upload ring
        src, n = rng.integers(0, 1 << 32, size=(1, 5 * (1 << 20) + 3), dtype=np.uint32), 5 * (1 << 20) + 3
    elif shape == "70 columns":
        src, n = rng.integers(0, 1 << 16, size=(70, 1000), dtype=np.uint16), 1024
    else:                        # 3 x 24 MiB of packed words: the host form stages 64 MiB at a time, two columns and then one
        src, n = rng.integers(0, 1 << 63, size=(3, 3 * (1 << 20) + 1), dtype=np.uint64), 3 * (1 << 20) + 1
    dev_words, kind = witness.to_device_words(src)
    from_dev = witness.columns_from_ints("fp", dev_words, n, kind=kind)
    from_host = witness.columns_from_ints("fp", src, n)
    torch.cuda.synchronize()
    assert torch.equal(from_host, from_dev)
    for c, r in ((0, 0), (src.shape[0] - 1, src.shape[1] - 1)):
        assert (host(from_host[c, r:r + 1]) == oracle_limbs("fp", [src[c, r]])).all()


# ---- 4. even_odd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fp", "fq"])
@pytest.mark.parametrize("kind", ["u8", "u16", "u32", "u64"])
def test_even_odd(kind, field):
    ref_e, ref_o = reference(field, kind, True, "even"), reference(field, kind, True, "odd")
    for live in LIVES:
        src = device_view(strided_source(kind, live, patterns=True), kind)
        buf_e, even = guarded()
        buf_o, odd = guarded()
        witness.even_odd(field, src, N, out_even=even, out_odd=odd, kind=kind)
        for got, ref in ((even, ref_e), (odd, ref_o)):
            want = np.zeros((COLS, N, 4), dtype=np.uint64)
            want[:, :live] = ref[:, :live]
            assert (host(got) == want).all(), (kind, field, live)
        assert guards_intact(buf_e) and guards_intact(buf_o)
        whole = witness.columns_from_ints(field, src, N, kind=kind)
        e, d = even.contiguous(), odd.contiguous()
        assert torch.equal(field_op(field, "add", e, field_op(field, "add", d, d)), whole), (kind, field, live)
    # host words: sent packed, split on the device
    e2, o2 = witness.even_odd(field, np.array(values_of(kind, True), dtype=DTYPE[kind]), N)
    assert (host(e2) == ref_e).all() and (host(o2) == ref_o).all()


# ---- 5. even_bits_table -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fp", "fq"])
@pytest.mark.parametrize("word_bits", [2, 8, 16])
def test_even_bits_table(word_bits, field):
    entries = 1 << (word_bits // 2)
    spread = [sum(((i >> j) & 1) << (2 * j) for j in range(word_bits // 2)) for i in range(entries)]
    for n in (entries, 4 * entries):
        buf, out = guarded(1, n)
        witness.even_bits_table(field, word_bits, n, out=out[0])
        assert (host(out[0]) == oracle_limbs(field, spread + [0] * (n - entries))).all() and guards_intact(buf)


def test_even_bits_table_refusals():
    lib = api.lib()
    buf, out = guarded(1, 64)
    good = dict(word_bits=8, dst=out.data_ptr(), n=64, stream=None)
    for change in (dict(word_bits=3), dict(word_bits=0), dict(word_bits=66), dict(word_bits=14), dict(dst=None), dict(dst=out.data_ptr() + 8)):
        a = api.EvenBitsTableArgs(**{**good, **change})
        assert lib.trh_even_bits_table_dev(api.FP, ctypes.byref(a)) == -1 and lib.trh_last_error(), change
    a = api.EvenBitsTableArgs(**good)
    assert lib.trh_even_bits_table_dev(7, ctypes.byref(a)) == -1 and b"unknown field id 7" in lib.trh_last_error()
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())


# ---- 6. the refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_alone():
    lib = api.lib()
    words = np.arange(3 * 40, dtype=np.uint32)
    d_words = torch.from_numpy(words.view(np.int32)).cuda()
    buf, out = guarded(6, 64)
    even, odd = out[:3], out[3:]
    good = dict(kind=witness.U32, src_stride=40, n_cols=3, live_rows=40, dst=even.data_ptr(), dst_odd=odd.data_ptr(), n=64, stream=None)
    common = [dict(kind=99), dict(kind=-1), dict(src_stride=39), dict(live_rows=65), dict(dst=None), dict(dst=even.data_ptr() + 8)]
    split_only = [dict(kind=witness.I32), dict(kind=witness.I64), dict(kind=witness.BITS, src_stride=2), dict(dst_odd=None), dict(dst_odd=odd.data_ptr() + 8)]
    entries = [(lib.trh_columns_from_ints_dev, d_words.data_ptr(), common), (lib.trh_columns_from_ints_host, words.ctypes.data, common),
               (lib.trh_even_odd_split_dev, d_words.data_ptr(), common + split_only)]
    refused = 0
    for fn, src, changes in entries:
        for change in changes:
            a = api.IntsArgs(**{**good, "src": src, **change})
            assert fn(api.FQ, ctypes.byref(a)) == -1 and lib.trh_last_error(), change
            refused += 1
        a = api.IntsArgs(**{**good, "src": src})
        assert fn(7, ctypes.byref(a)) == -1 and b"unknown field id 7" in lib.trh_last_error()
    torch.cuda.synchronize()
    assert refused == 23 and bool((buf == FILL).all())
    # nothing to do is no refusal
    for change in (dict(n_cols=0), dict(n=0, live_rows=0)):
        a = api.IntsArgs(**{**good, "src": d_words.data_ptr(), **change})
        assert lib.trh_columns_from_ints_dev(api.FQ, ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())
    # and the good arguments are good
    a = api.IntsArgs(**{**good, "src": d_words.data_ptr()})
    assert lib.trh_even_odd_split_dev(api.FQ, ctypes.byref(a)) == 0
    assert (host(even)[:, :40] == oracle_limbs("fq", words & 0x55555555).reshape(3, 40, 4)).all() and guards_intact(buf)


# ---- 7. a non-default stream ------------------------------------------------------------------------------------------------------------------
def test_on_a_non_default_stream_without_synchronising():
    live, n = 100_000, 1 << 17
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src = ((torch.arange(live, device="cuda", dtype=torch.int64) * 2654435761) & 0xFFFFFFFF).to(torch.int32)   # written on s
        out = witness.columns_from_ints("fp", src, n, kind="u32")                                                 # expanded on s, behind it
        plain = field_op("fp", "from_mont", out)
    s.synchronize()
    want = (np.arange(live, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    got = plain.cpu().numpy().view(np.uint64)
    assert (got[:live, 0] == want).all() and not got[:live, 1:].any() and not got[live:].any()


# ---- 8. circuit B end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 10])
def test_logic_chip_from_words_and_bitmaps(k):
    field, curve, n, u = "fp", "vesta", 1 << k, pc.usable(k)
    circuit = pc.circuit_b(field)
    cs = circuit.system()
    advice_ints, (s_table, table) = pc.witness_b(field, k, used=20 if k == pc.K else None)
    col = dict(zip(pc.ADV_B, advice_ints))
    even_mask = int("01" * 32, 2)
    enabled = [r for r in range(n) if col["s_and"][r] | col["s_xor"][r] | col["s_or"][r]]
    # the witness value by value on the host; the halves are the decomposition of their word on EVERY row (on rows where no chip is
    # enabled the generator leaves them zero: any value satisfies the constraints there)
    host_cols = {name: list(v) for name, v in col.items()}
    for word, even, odd in pc.DECOMPOSED_B:
        host_cols[even] = [w & even_mask for w in col[word]]
        host_cols[odd] = [(w >> 1) & even_mask for w in col[word]]
        assert all(host_cols[even][r] == col[even][r] and host_cols[odd][r] == col[odd][r] for r in enabled)
    host_advice = to_dev(field, [host_cols[name] for name in pc.ADV_B])
    host_fixed = to_dev(field, [s_table, table])

    def build(words):
        b = witness.AdviceBuilder(field, len(pc.ADV_B), n)
        b.ints(0, np.array([col["s_and"][:u], col["s_xor"][:u], col["s_or"][:u]], dtype=bool))                  # three bitmaps
        for word, even, odd in pc.DECOMPOSED_B:
            w = np.array(words[word][:u], dtype=np.uint32)
            b.ints(pc.ADV_B.index(word), w)
            b.even_odd(w, pc.ADV_B.index(even), pc.ADV_B.index(odd))
        b.ints(pc.ADV_B.index("res"), np.array(words["res"][:u], dtype=np.uint32))
        return b.tensor()

    advice = build(col)
    fixed = torch.stack([witness.columns_from_ints(field, np.array(s_table[:u], dtype=bool), n), witness.even_bits_table(field, 8, n)])
    torch.cuda.synchronize()
    assert torch.equal(advice, host_advice) and torch.equal(fixed, host_fixed)

    prover = mock.MockProver(field, k, cs.usable_rows(n), [(f"gate {i}", [g]) for i, g in enumerate(circuit.gates)],
                             [(f"lookup {i}", ins, tabs) for i, (ins, tabs) in enumerate(circuit.lookups)])
    columns = lambda adv: {**{("advice", i): adv[i] for i in range(len(pc.ADV_B))}, ("fixed", 0): fixed[0], ("fixed", 1): fixed[1]}   # noqa: E731
    assert prover.verify(columns(advice)) == []

    params = poly.Params.new(curve, k)
    vk, pk = plonk.keygen(params, cs, fixed, [])
    seed = bytes([7]) * 32
    proof = plonk.create_proof_bytes(params, pk, [], advice, api.Rng(seed))
    assert proof == plonk.create_proof_bytes(params, pk, [], host_advice, api.Rng(seed))
    assert plonk.single_verify(params, plonk.verify_proof_bytes(params, vk, [], proof))

    # one bit of the source word `a` flipped on a row where a chip is enabled, the halves as they were
    row = enabled[len(enabled) // 2]
    bad = advice.clone()
    a_bad = np.array(col["a"][:u], dtype=np.uint32)
    a_bad[row] ^= 4
    witness.columns_from_ints(field, a_bad, n, out=bad[pc.ADV_B.index("a")])
    assert prover.verify(columns(bad)) == [mock.ConstraintNotSatisfied(0, 0, "gate 0", row)]    # gate 0: a_e + 2 a_o - a
    bad_proof = plonk.create_proof_bytes(params, pk, [], bad, api.Rng(seed))
    try:
        accepted = plonk.single_verify(params, plonk.verify_proof_bytes(params, vk, [], bad_proof))
    except plonk.VerifyError:
        accepted = False
    assert not accepted


# ---- 9. instances as arrays -------------------------------------------------------------------------------------------------------------------
def test_an_instance_column_as_an_array():
    """one advice and one instance column, both equality-enabled, row i tied to row i"""
    field, curve, k = "fq", "pallas", 5
    n, u = 1 << k, pc.usable(k)
    cs = plonk.ConstraintSystem(field, 0, 1, 1, [], [], [("advice", 0), ("instance", 0)])
    assert cs.usable_rows(n) == u
    values = np.random.default_rng(9).integers(0, 1 << 63, size=u, dtype=np.uint64)
    values[:3] = [0, 1, (1 << 64) - 1]
    params = poly.Params.new(curve, k)
    vk, pk = plonk.keygen(params, cs, None, [(0, r, 1, r) for r in range(u)])
    advice = witness.columns_from_ints(field, values.reshape(1, u), n)
    seed = bytes([9]) * 32
    as_list = [int(v) for v in values]
    proof = plonk.create_proof_bytes(params, pk, [values], advice, api.Rng(seed))
    assert proof == plonk.create_proof_bytes(params, pk, [as_list], advice, api.Rng(seed))
    for instances in ([values], [as_list]):
        assert plonk.single_verify(params, plonk.verify_proof_bytes(params, vk, instances, proof))
    changed = values.copy()
    changed[5] += np.uint64(1)
    try:
        accepted = plonk.single_verify(params, plonk.verify_proof_bytes(params, vk, [changed], proof))
    except plonk.VerifyError:
        accepted = False
    assert not accepted


# ---- 10. the C++ wrappers -----------------------------------------------------------------------------------------------------------------------
def test_native_wrappers():
    exe = os.path.join(ROOT, "tests", "native", "witness_test")
    assert os.path.exists(exe), "tests/native/witness_test is missing: run `make`"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["test"] == "witness" and rec["checks_failed"] == 0 and rec["checks"] > 1000
