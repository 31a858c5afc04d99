"""The Exe table on the device: the steps of a trace -> the plain trace cells, the four temporary variables a, b, c, d with their
non-deterministic advice, and their one-hot selector cells (trh_exe_table_dev; csrc/exetable.hip over csrc/exetable.h).

Every row is a function of its step and the step behind it.  The host hands over the steps as machine words -- pc, the packed instruction,
the operand, the registers and the flag before the step, the word loaded or stored -- and the device writes 28 + 9 reg_count columns.

    columns(reg_count)                      the column names, in the order of the result
    encode(op, ri, rj, a, a_is_reg)         -> (inst word, a word) of one step
    DEFAULT_SELECTION                       opcode name -> the sources of (a, b, c, d): the reference's table (aux.rs:105-398), with a register
                                            operand's CONTENT as its value and CJmp's d as NONDET(PC_PLUS_ONE) (include/trh.h says why)
    build(field, word_bits, reg_count, pc, inst, a, regs, flags, value, n=...)  -> device tensor (columns, n, 4)
    witness.AdviceBuilder.exe_table(first_column, ...)                          the same into the builder's column slices
    chip_columns(reg_count), DEFAULT_CHIPS, build_chips(...)                    the 52 + reg_count columns of the sub-chips from the same steps
                                            (trh_exe_chips_dev; csrc/exechips.hip): Out, the changed flags, decompositions, signed words,
                                            r, a_shift / a_power, a_flag, lsb_b / b_flag; witness.AdviceBuilder.exe_chips

Which source a variable takes is data: pass selection= to build, a mapping like DEFAULT_SELECTION (opcodes it leaves out are unknown and
refuse the steps that use them).  Steps that break a rule are refused with nothing written (api.TrhError names the first one)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import api
from .memtable import _words
from .witness import _device, _out, _stream, pack_bits

OPCODES = {"and": 0, "or": 1, "xor": 2, "not": 3, "add": 4, "sub": 5, "mull": 6, "umulh": 7, "smulh": 8, "udiv": 9, "umod": 10, "shl": 11, "shr": 12,
           "cmpe": 13, "cmpa": 14, "cmpae": 15, "cmpg": 16, "cmpge": 17, "mov": 18, "cmov": 19, "jmp": 20, "cjmp": 21, "cnjmp": 22, "store.w": 28,
           "load.w": 29, "answer": 31}
ANSWER = OPCODES["answer"]

# TRH_EXE_*: the sources of a temporary variable
UNSET, PC, PC_NEXT, PC_PLUS_ONE, REG_RI, REG_RJ, REG_NEXT_RI, A, VALUE, ZERO, ONE, MAX_WORD = range(12)
# TRH_EXE_RULE_*: the non-deterministic rules
REM, QUOT, CMP_GT, CMP_GE, MUL_HI, MUL_LO, SMUL_LO, XOR, SHL_HI, SHR_LO, RULE_PC_PLUS_ONE = range(11)
UNKNOWN = 0xFFFFFFFF
ROWS_PER_WORKGROUP = 256  # csrc/exetable.h EXE_THREADS


def NONDET(rule: int) -> int:
    return 16 + rule


DEFAULT_SELECTION = {
    "and": (A, REG_RJ, REG_NEXT_RI, UNSET), "or": (A, REG_RJ, REG_NEXT_RI, UNSET), "xor": (A, REG_RJ, REG_NEXT_RI, UNSET),
    "not": (A, MAX_WORD, REG_NEXT_RI, UNSET),
    "add": (A, REG_RJ, REG_NEXT_RI, ZERO), "sub": (A, REG_NEXT_RI, REG_RJ, ZERO),
    "mull": (A, REG_RJ, NONDET(MUL_HI), REG_NEXT_RI), "umulh": (A, REG_RJ, REG_NEXT_RI, NONDET(MUL_LO)), "smulh": (A, REG_RJ, REG_NEXT_RI, NONDET(SMUL_LO)),
    "udiv": (NONDET(REM), REG_NEXT_RI, A, REG_RJ), "umod": (REG_NEXT_RI, NONDET(QUOT), A, REG_RJ),
    "shl": (A, REG_RJ, NONDET(SHL_HI), REG_NEXT_RI), "shr": (A, REG_RJ, REG_NEXT_RI, NONDET(SHR_LO)),
    "cmpe": (A, REG_RI, NONDET(XOR), UNSET),
    "cmpa": (REG_RI, NONDET(CMP_GT), A, ZERO), "cmpae": (REG_RI, NONDET(CMP_GE), A, ONE),
    "cmpg": (REG_RI, NONDET(CMP_GT), A, ZERO), "cmpge": (REG_RI, NONDET(CMP_GE), A, ONE),
    "mov": (A, REG_NEXT_RI, ZERO, UNSET), "cmov": (REG_NEXT_RI, A, ZERO, REG_RI),
    "jmp": (A, PC_NEXT, ZERO, UNSET),
    "cjmp": (PC_NEXT, A, ZERO, NONDET(RULE_PC_PLUS_ONE)),  # the reference: sd_pc AND sd_one, which forces pc = 1
    "cnjmp": (PC_NEXT, PC_PLUS_ONE, ZERO, A),
    "load.w": (VALUE, REG_RI, ZERO, ZERO), "store.w": (VALUE, REG_NEXT_RI, ZERO, ZERO),
    "answer": (A, PC, ZERO, ZERO),
}


def columns(reg_count: int) -> tuple:
    """the 28 + 9 reg_count column names; the first 24 + 9 reg_count are ADVICE of tests/golden/make_exe_gates.py for that reg_count"""
    regs, nexts = [f"reg{i}" for i in range(reg_count)], [f"reg_next{i}" for i in range(reg_count)]
    names = ["s_trace", "pc", "flag"] + regs + ["opcode", "immediate", "value", "tv_a", "tv_b", "tv_c", "tv_d"]
    names += [f"sa_{x}" for x in ["pc_next"] + regs + nexts + ["a", "v_addr"]]
    names += [f"sb_{x}" for x in ["pc", "pc_next", "pc_plus_one"] + regs + nexts + ["a", "max_word"]]
    names += [f"sc_{x}" for x in regs + nexts + ["a", "zero"]]
    names += [f"sd_{x}" for x in ["pc"] + regs + nexts + ["a", "zero", "one"]]
    names += ["sa_non_det", "sb_non_det", "sc_non_det", "sd_non_det"]
    return tuple(names)


def encode(op, ri: int = 0, rj: int = 0, a: int = 0, a_is_reg: bool = False) -> tuple:
    """one step's (inst, a) words: opcode (a name of OPCODES or a number) in bits 0 - 4, ri in bits 8 - 11, rj in bits 12 - 15, "A is a
    register" in bit 16; a is the immediate or the register's number"""
    code = OPCODES[op] if isinstance(op, str) else op
    assert 0 <= code < 32 and 0 <= ri < 16 and 0 <= rj < 16 and 0 <= a < 1 << 32
    return code | ri << 8 | rj << 12 | (1 << 16 if a_is_reg else 0), a


def selection_table(selection) -> list:
    """a mapping opcode (name or number) -> (a, b, c, d) sources into the 32 words of trh_exe_table_args_t.selection"""
    table = [UNKNOWN] * 32
    for op, sources in selection.items():
        sa, sb, sc, sd = sources
        assert all(0 <= s < 256 for s in sources)
        table[OPCODES[op] if isinstance(op, str) else op] = sa | sb << 8 | sc << 16 | sd << 24
    return table


def _steps(word_bits, reg_count, pc, inst, a, regs, flags, value, n, out, m, ncols):
    """the step arrays on out's device (or the current one) and the destination: what build and build_chips share"""
    import torch
    dev = _device() if out is None else out.device
    pc, inst, a, value = _words(pc, dev, "pc"), _words(inst, dev, "inst"), _words(a, dev, "a"), _words(value, dev, "value")
    if m is None:
        m = pc.numel()
    regs = _words(np.asarray(regs).reshape(-1) if not torch.is_tensor(regs) else regs.reshape(-1), dev, "regs")
    if torch.is_tensor(flags):
        flag_bits = _words(flags, dev, "flags")
    else:
        bits = np.asarray(flags, dtype=np.bool_).reshape(-1)
        assert bits.size == m, "one flag per step"
        flag_bits = _words(pack_bits(bits) if m else np.zeros(0, dtype=np.uint32), dev, "flags")
    assert min(pc.numel(), inst.numel(), a.numel(), value.numel()) >= m and regs.numel() >= m * reg_count and flag_bits.numel() >= (m + 31) // 32
    if n is None:
        assert out is not None, "n= or out="
        n = out.shape[1]
    out = _out(out, (ncols, n, 4), dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    keep = (pc, inst, a, value, regs, flag_bits)
    return dict(word_bits=word_bits, reg_count=reg_count, pc=ptr(pc), inst=ptr(inst), a=ptr(a), value=ptr(value), regs=ptr(regs), flag_bits=ptr(flag_bits), m=m,
                dst=out.data_ptr(), n=n), out, dev, keep


def build(field: str, word_bits: int, reg_count: int, pc, inst, a, regs, flags, value, n: int | None = None, selection=None, out=None, stream=None,
          m: int | None = None):
    """pc / inst / a / value: m words each, regs: m x reg_count words (step-major, the registers before the step): numpy arrays (uploaded) or
    device tensors of 32-bit words; flags: a bool array (packed with witness.pack_bits) or a device tensor of ceil(m / 32) bitmap words.  m
    defaults to pc's length.  n: rows per column (default: out's); out: a (columns, n, 4) int64 device tensor to write into.  Asynchronous
    on `stream` once the steps have passed validation."""
    fields, out, dev, keep = _steps(word_bits, reg_count, pc, inst, a, regs, flags, value, n, out, m, 28 + 9 * reg_count)
    args = api.ExeTableArgs(selection=(ctypes.c_uint32 * 32)(*selection_table(DEFAULT_SELECTION if selection is None else selection)), stream=_stream(stream, dev), **fields)
    api._check(api.lib().trh_exe_table_dev(api.FIELD_ID[field], ctypes.byref(args)))
    del keep
    return out


# ---- the chips: Out, the changed flags and the sub-chips' advice (trh_exe_chips_dev) ---------------------------------------------------------
# TRH_CHIP_*: bits 0 - 12 are the reference's Out in Out::new order
AND, XOR_, OR, SUM, PROD, SSUM, SPROD, MOD, SHIFT, FLAG1, FLAG2, FLAG3, FLAG4, B_FLAG, CH_PC, CH_FLAG, CH_REG = (1 << i for i in range(17))
OUT_NAMES = ("and", "xor", "or", "sum", "prod", "ssum", "sprod", "mod", "shift", "flag1", "flag2", "flag3", "flag4")
INVERSE_STRIP = 8  # csrc/exechips_inv.h EXE_CHIPS_STRIP: rows per lane of the inversion kernel

# out.rs:148-349 and the `ch:` fields of aux.rs:109-396
DEFAULT_CHIPS = {
    "and": AND | FLAG1 | FLAG2 | CH_REG | CH_FLAG, "or": OR | FLAG1 | FLAG2 | CH_REG | CH_FLAG, "xor": XOR_ | FLAG1 | FLAG2 | CH_REG | CH_FLAG,
    "not": XOR_ | FLAG1 | FLAG2 | CH_REG | CH_FLAG,
    "add": SUM | CH_REG | CH_FLAG, "sub": SUM | CH_REG | CH_FLAG,
    "mull": PROD | FLAG1 | FLAG2 | CH_REG | CH_FLAG, "umulh": PROD | FLAG1 | FLAG2 | CH_REG | CH_FLAG, "smulh": SPROD | FLAG1 | FLAG2 | CH_REG | CH_FLAG,
    "udiv": MOD | FLAG1 | FLAG2 | FLAG3 | CH_REG | CH_FLAG, "umod": MOD | FLAG1 | FLAG2 | FLAG3 | CH_REG | CH_FLAG,
    "shl": SHIFT | FLAG4 | B_FLAG | CH_REG | CH_FLAG, "shr": SHIFT | FLAG4 | CH_REG | CH_FLAG,
    "cmpe": XOR_ | FLAG1 | FLAG2 | CH_FLAG,
    "cmpa": SUM | CH_FLAG, "cmpae": SUM | CH_FLAG, "cmpg": SSUM | CH_FLAG, "cmpge": SSUM | CH_FLAG,
    "mov": XOR_ | CH_REG, "cmov": MOD | CH_REG,
    "jmp": XOR_ | CH_PC, "cjmp": MOD | CH_PC, "cnjmp": MOD | CH_PC,
    "load.w": CH_REG, "store.w": XOR_, "answer": 0,
}


def chip_columns(reg_count: int) -> tuple:
    """the 52 + reg_count column names of build_chips, in the order of the result"""
    names = [f"out_{x}" for x in OUT_NAMES] + [f"ch_reg{i}" for i in range(reg_count)] + ["ch_pc", "ch_flag"]
    names += [f"{v}_{half}" for v in "abcd" for half in ("even", "odd")]
    names += [f"{s}_{x}" for s in ("es", "os") for x in ("word", "even", "odd")]
    names += [f"sg_{v}_{x}" for v in "abc" for x in ("msb", "sigma", "check", "check_even", "check_odd")]
    names += ["r_word", "r_even", "r_odd", "a_shift", "a_power", "a_flag", "lsb_b", "b_flag"]
    return tuple(names)


def chips_table(chips) -> list:
    """a mapping opcode (name or number) -> TRH_CHIP_* bits into the 32 words of trh_exe_chips_args_t.chips"""
    table = [UNKNOWN] * 32
    for op, bits in chips.items():
        assert 0 <= bits < 1 << 32
        table[OPCODES[op] if isinstance(op, str) else op] = bits
    return table


def build_chips(field: str, word_bits: int, reg_count: int, pc, inst, a, regs, flags, value, n: int | None = None, selection=None, chips=None, out=None,
                stream=None, m: int | None = None):
    """the 52 + reg_count columns of chip_columns from the same steps as build (include/trh.h says what each cell is): -> device tensor
    (columns, n, 4).  chips: a mapping like DEFAULT_CHIPS, which must know exactly the opcodes `selection` knows.  word_bits must be even.
    Asynchronous on `stream` once the steps have passed validation; it reads no column of build's, and the two can run in either order."""
    fields, out, dev, keep = _steps(word_bits, reg_count, pc, inst, a, regs, flags, value, n, out, m, 52 + reg_count)
    args = api.ExeChipsArgs(selection=(ctypes.c_uint32 * 32)(*selection_table(DEFAULT_SELECTION if selection is None else selection)),
                            chips=(ctypes.c_uint32 * 32)(*chips_table(DEFAULT_CHIPS if chips is None else chips)), stream=_stream(stream, dev), **fields)
    api._check(api.lib().trh_exe_chips_dev(api.FIELD_ID[field], ctypes.byref(args)))
    del keep
    return out
