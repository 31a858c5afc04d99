"""No device: the Exe table's integer model, csrc/exetable.h on the host, and the host side of trh_exe_table_dev.

  model              tests/exetable_model.py and its interpreter on the reference's two programs (word_bits 8), a loop with cjmp / cnjmp / jmp and
                     a program that uses every opcode; the rows obey the arithmetic identities the reference's sub-chips impose on the
                     temporary variables (sum, product, division, logic, shifts)
  the gates          the model's columns at W = 16, R = 8, n = 128 satisfy the 90 gates of tests/golden/exe_tempvar_gates.json
                     (pasta.evaluate_gates) on the interpreter's traces and on 100 steps drawn independently; with the reference's literal
                     choice for CJmp's d exactly the CJmp rows fail, in tv.d.pc / tv.d.one; one corrupted tv_b cell fails exactly its row
  exetable_vec_test  the header's decode, rules and exe_row in a stand-alone program under address + undefined sanitizers
                     (tests/native/exetable_vec_test.cpp, built by program() below as `make` builds it; it never loads libtrh), against the
                     model: W = 32 with the words 0 and 0xFFFFFFFF, W = 2, R = 1 and R = 16
  the ABI            exported, TRH_ENODEV without a device, TRH_EINVAL for every refusal the host can see, no stream parameter"""
import atexit
import ctypes
import json
import os
import random
import re
import shutil
import subprocess
import tempfile

import pytest

import exetable_model as em
import pasta as o
from common import expr_from_json as from_json, expr_to_tuple as to_tuple
from tiny_ram_halo2_amd import api, exetable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "exe_tempvar_gates.json")
PROGRAM = [""]  # program()
F = o.FIELDS["fp"]
Y = 0x5EED5EED5EED5EED1234 % F.m
PROGRAMS = {"load_store": (em.reference_load_store, [1]), "load_answer": (em.reference_load_answer, [1]), "loop": (em.loop_program, []),
            "every_opcode": (em.every_opcode_program, [3, 5])}


def program():
    """the stand-alone program, compiled here once per run with the Makefile's command line into a directory of its own (as
    test_memtable_host.py does): the tests without a device then need no build product under tests/"""
    if not os.path.exists(PROGRAM[0]):
        tmp = tempfile.mkdtemp(prefix="exetable_vec_test_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        PROGRAM[0] = os.path.join(tmp, "exetable_vec_test")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "native", "exetable_vec_test.cpp"), "-o", PROGRAM[0]])
    return PROGRAM[0]


def run(lines):
    p = subprocess.run([program()], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]   # a sanitizer report ends the program with a non-zero status
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [[int(x) for x in line.split()] for line in out]


def entry(sources):
    sa, sb, sc, sd = sources
    return sa | sb << 8 | sc << 16 | sd << 24


def inst_word(s):
    return s.op | s.ri << 8 | s.rj << 12 | (1 << 16 if s.a_is_reg else 0)


# ---- the package's tables against the model's -------------------------------------------------------------------------------------------------
def test_the_package_restates_the_model():
    assert exetable.DEFAULT_SELECTION == em.DEFAULT and exetable.OPCODES == em.OPCODES
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    for R in (1, 8, 16):
        assert list(exetable.columns(R)) == em.columns(R) and len(em.columns(R)) == 28 + 9 * R == len(set(em.columns(R)))
    assert em.columns(doc["reg_count"])[:len(doc["advice"])] == doc["advice"] and len(doc["advice"]) == 24 + 9 * doc["reg_count"]
    assert exetable.encode("shr", 3, 15, 9, True) == (12 | 3 << 8 | 15 << 12 | 1 << 16, 9) and exetable.encode(31, a=5) == (31, 5)
    table = exetable.selection_table(exetable.DEFAULT_SELECTION)
    assert len(table) == 32 and table[em.OPCODES["cjmp"]] == entry(em.DEFAULT["cjmp"]) and table[23] == table[30] == exetable.UNKNOWN
    assert sum(e != exetable.UNKNOWN for e in table) == 26
    for name, sources in em.DEFAULT.items():
        for v, src in zip(em.VARS, sources):
            assert src == em.UNSET or src >= em.NONDET0 or src in em.LEGAL[v], (name, v)


# ---- the interpreter and the identities -----------------------------------------------------------------------------------------------------------
def test_the_interpreter_on_the_reference_programs():
    steps, answer = em.run(8, 8, em.reference_load_store(), [1])
    assert answer == 1 and [s.op for s in steps] == [29, 0, 28, 31] and [s.value for s in steps] == [1, 0, 1, 0] and steps[3].regs[:2] == (1, 1)
    steps, answer = em.run(8, 8, em.reference_load_answer(), [1])
    assert answer == 1 and [s.value for s in steps] == [0, 0, 0] and [s.pc for s in steps] == [0, 1, 2]
    steps, answer = em.run(8, 8, em.loop_program())
    assert answer == 0 and len(steps) == 2 + 3 * 5 + 3 and {s.op for s in steps} >= {20, 21, 22}
    steps, answer = em.run(8, 8, em.every_opcode_program(), [3, 5])
    assert answer == 7 and {s.op for s in steps} == set(em.NAMES)


@pytest.mark.parametrize("W", [8, 16, 32])
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_the_rows_obey_the_sub_chips_identities(name, W):
    make, tape = PROGRAMS[name]
    steps, _ = em.run(W, 8, make(), tape)
    assert em.first_violation(W, 8, steps) is None
    two_w, seen = 1 << W, set()
    for i, s in enumerate(steps[:-1]):
        r = em.row(W, 8, em.DEFAULT, s, steps[i + 1])
        ta, tb, tc, td, flag_next = r["tv_a"], r["tv_b"], r["tv_c"], r["tv_d"], int(steps[i + 1].flag)
        op, shift = em.NAMES[s.op], min(em.operand(s), W)
        seen.add(op)
        if op in ("add", "sub", "cmpa", "cmpae"):
            assert ta + tb == tc + two_w * flag_next - td, (i, op)
        elif op in ("mull", "umulh"):
            assert ta * tb == td + two_w * tc, (i, op)
        elif op in ("udiv", "umod"):
            assert flag_next * (tb - td) + td - tb * tc - ta == 0, (i, op)
        elif op in ("and", "or", "xor", "not", "cmpe"):
            assert tc == {"and": ta & tb, "or": ta | tb}.get(op, ta ^ tb), (i, op)
        elif op == "shl":
            assert (tb << shift) == td + two_w * tc, (i, op)
        elif op == "shr":
            assert td == (tb << shift) - two_w * tc, (i, op)
        assert all(0 <= r[f"tv_{v}"] <= two_w for v in "abc") and abs(td) < 1 << 64
    if name == "every_opcode":
        assert seen == set(em.OPCODES) - {"answer"}


# ---- the 90 gates over the model's columns ------------------------------------------------------------------------------------------------------------
N, TABLE_LEN = 128, 110


def fixture():
    with open(FIXTURE) as fh:
        doc = json.load(fh)
    assert doc["reg_count"] == 8 and doc["word_bits"] == 16 and len(doc["gates"]) == 90
    return doc, [from_json(g["expr"]) for g in doc["gates"]]


def gate_columns(doc, cols):
    out = {("advice", i): [v % F.m for v in cols[i]] for i in range(len(doc["advice"]))}
    out[("selector", doc["selectors"].index("first_line"))] = [1] + [0] * (N - 1)
    out[("selector", doc["selectors"].index("s_table"))] = [1] * TABLE_LEN + [0] * (N - TABLE_LEN)
    return out


def failing_rows(gates, cols):
    return [i for i, v in enumerate(o.evaluate_gates(F, [to_tuple(g) for g in gates], cols, Y, N)) if v]


def traces():
    """name -> steps at W = 16, R = 8: the interpreter's four traces and 100 steps drawn independently"""
    out = {name: em.run(16, 8, make(), tape)[0] for name, (make, tape) in PROGRAMS.items()}
    out["random"] = em.random_steps(random.Random(0xE8E7AB1E), 16, 8, 100)
    return out


@pytest.mark.parametrize("name", list(PROGRAMS) + ["random"])
def test_the_models_columns_satisfy_the_gates(name):
    doc, gates = fixture()
    steps = traces()[name]
    if name == "random":  # every opcode with both kinds of operand: the producer does not ask whether a machine ran the steps
        assert len(steps) == 100 and {(s.op, s.a_is_reg) for s in steps} == {(op, kind) for op in em.NAMES for kind in (False, True)}
    cols = em.build(16, 8, steps, N)
    assert failing_rows(gates, gate_columns(doc, cols)) == []


def test_the_references_cjmp_selection_fails_on_exactly_the_cjmp_rows():
    doc, gates = fixture()
    names = [g["name"] for g in doc["gates"]]
    for trace in ("every_opcode", "random"):
        steps = traces()[trace]
        cjmp_rows = [i for i, s in enumerate(steps) if s.op == em.OPCODES["cjmp"]]
        assert cjmp_rows
        cols = gate_columns(doc, em.build(16, 8, steps, N, cjmp_literal=True))
        assert failing_rows(gates, cols) == cjmp_rows
        by_gate = {}
        for name, g in zip(names, gates):
            rows = failing_rows([g], cols)
            if rows:
                by_gate[name] = rows
        assert set(by_gate) == {"tv.d.pc", "tv.d.one"}
        assert by_gate["tv.d.pc"] == cjmp_rows                                           # pc - (pc + 1) is never zero
        assert by_gate["tv.d.one"] == [i for i in cjmp_rows if steps[i].pc != 0]         # 1 - (pc + 1) vanishes for pc = 0 alone


def test_a_corrupted_cell_fails_exactly_its_row():
    doc, gates = fixture()
    steps = traces()["random"]
    cols = em.build(16, 8, steps, N)
    b = em.columns(8).index("tv_b")
    at = next(i for i, s in enumerate(steps) if 2 < i < len(steps) - 1 and em.DEFAULT[em.NAMES[s.op]][1] == em.REG_RJ)
    cols[b][at] += 1
    assert failing_rows(gates, gate_columns(doc, cols)) == [at]


# ---- csrc/exetable.h under the sanitizers, against the model ----------------------------------------------------------------------------------------------
def check_rows_against_the_model(W, R, steps, selection=em.DEFAULT):
    names = em.columns(R)
    lines, want = [], []
    for i, s in enumerate(steps):
        nxt = steps[i + 1] if i + 1 < len(steps) else None
        k = s.a if s.a_is_reg else 0
        lines.append(f"r {W} {R} {entry(selection[em.NAMES[s.op]])} {s.pc} {inst_word(s)} {s.a} {s.value} {s.regs[s.ri]} {s.regs[s.rj]} {s.regs[k]} "
                     f"{nxt.pc if nxt else 0} {nxt.regs[s.ri] if nxt else 0}")
        want.append(em.row(W, R, selection, s, nxt))
    for s, got, r in zip(steps, run(lines), want):
        assert got[:2] == [r["opcode"], r["immediate"]], s
        for v, name in enumerate(em.VARS):
            negative, magnitude, _, hot = got[2 + 4 * v: 6 + 4 * v]
            assert (-magnitude if negative else magnitude) == r[f"tv_{name}"] and not (negative and magnitude == 0), (s, name)
            family = [n for n in names[10 + R:] if n.startswith(f"s{name}_") and r[n]]
            assert family == ([names[hot]] if hot >= 0 else []), (s, name, family, hot)


def test_vec_rows_at_32_bits_with_the_extreme_words():
    steps = em.extreme_steps(8)
    top = 0xFFFFFFFF
    rows = [(em.NAMES[s.op], em.row(32, 8, em.DEFAULT, s, None)) for s in steps]
    assert any(op == "cjmp" and r["tv_d"] == 1 << 32 for op, r in rows) and any(op == "cnjmp" and r["tv_b"] == 1 << 32 for op, r in rows)   # pc + 1 = 2^32
    assert any(op == "mull" and r["tv_c"] == top - 1 for op, r in rows) and any(op == "umulh" and r["tv_d"] == 1 for op, r in rows)        # 0xFFFFFFFF squared
    assert any(op == "shr" and r["tv_d"] == -top * top for op, r in rows)                  # s = 0: RJ - 2^32 RJ, the most negative value
    assert any(op == "shr" and r["tv_d"] == top << 32 for op, r in rows)                   # s = 32: 2^32 RJ - 0, the largest
    assert any(op == "cmpa" and r["tv_a"] == r["tv_c"] == top and r["tv_b"] == 0 for op, r in rows)
    assert any(op == "cmpae" and r["tv_a"] == r["tv_c"] == 0 and r["tv_b"] == top for op, r in rows)
    assert any(op == "udiv" and r["tv_c"] == 0 and r["tv_d"] == top and r["tv_a"] == 0 for op, r in rows)
    check_rows_against_the_model(32, 8, steps)


@pytest.mark.parametrize("W,R", [(2, 8), (32, 1), (32, 16), (16, 16), (2, 1)])
def test_vec_rows_at_the_small_word_and_the_register_counts(W, R):
    if W == 32:
        steps = em.extreme_steps(R)
    else:
        steps = em.random_steps(random.Random(W * 100 + R), W, R, 300)
    check_rows_against_the_model(W, R, steps)


def test_vec_rows_with_another_table():
    """every legal source in every variable, and the reference's literal sources"""
    selection = dict(em.DEFAULT)
    selection["and"] = (em.PC_NEXT, em.PC, em.REG_RI, em.PC)
    selection["or"] = (em.VALUE, em.PC_NEXT, em.ZERO, em.ONE)
    selection["xor"] = (em.REG_RJ, em.PC_PLUS_ONE, em.A, em.A)
    selection["not"] = (em.UNSET, em.UNSET, em.UNSET, em.nd(em.SHR_LO))
    selection["add"] = (em.nd(em.RULE_PC_PLUS_ONE), em.MAX_WORD, em.REG_NEXT_RI, em.ZERO)
    check_rows_against_the_model(16, 8, em.random_steps(random.Random(5), 16, 8, 400), selection)


def test_vec_layout_decode_and_rules():
    for R, got in zip((1, 8, 16), run(["l 1", "l 8", "l 16"])):
        names = em.columns(R)
        assert got == [len(names), names.index("sa_pc_next"), names.index("sb_pc"), names.index("sc_reg0"), names.index("sd_pc"), names.index("sa_non_det"),
                       exetable.ROWS_PER_WORKGROUP]
    words = [0, 0xFFFFFFFF, 31 | 15 << 8 | 15 << 12 | 1 << 16, 12 | 3 << 8 | 9 << 12, 0xFFFE00E0]
    for w, got in zip(words, run([f"d {w}" for w in words])):
        assert got == [w & 31, (w >> 8) & 15, (w >> 12) & 15, (w >> 16) & 1]
    # the table: the default is good; every (variable, source) pair is legal exactly where the model says; unknown entries are skipped
    good = exetable.selection_table(em.DEFAULT)
    lines, want = ["t " + " ".join(str(e) for e in good)], [128]
    for v, name in enumerate(em.VARS):
        for src in list(range(14)) + [15, 16, 26, 27, 255]:
            table = list(good)
            table[9] = (good[9] & ~(0xFF << 8 * v)) | src << 8 * v
            lines.append("t " + " ".join(str(e) for e in table))
            legal = src == em.UNSET or 16 <= src <= 26 or src in em.LEGAL[name]
            want.append(128 if legal else 9 * 4 + v)
    assert [g[0] for g in run(lines)] == want
    # the rule of a step
    e = good[4]
    cases = [((8, 4, e, 255, 4, 255, 255, 0), 1), ((8, 4, e, 256, 4, 0, 0, 0), 0), ((8, 4, e, 0, 4, 256, 0, 0), 0), ((8, 4, e, 0, 4, 0, 256, 0), 0),
             ((8, 4, 0xFFFFFFFF, 0, 4, 0, 0, 0), 0), ((8, 4, e, 0, 4 | 4 << 8, 0, 0, 0), 0), ((8, 4, e, 0, 4 | 3 << 8, 0, 0, 0), 1), ((8, 4, e, 0, 4 | 4 << 12, 0, 0, 0), 0),
             ((8, 4, e, 0, 4 | 1 << 16, 4, 0, 0), 0), ((8, 4, e, 0, 4 | 1 << 16, 3, 0, 0), 1), ((8, 4, e, 0, 4, 0, 0, 1), 0), ((8, 4, e, 0, 31, 0, 0, 1), 1),
             ((32, 16, e, 0xFFFFFFFF, 4 | 15 << 8 | 15 << 12, 0xFFFFFFFF, 0xFFFFFFFF, 0), 1), ((2, 1, e, 3, 4, 3, 3, 0), 1), ((2, 1, e, 4, 4, 0, 0, 0), 0)]
    assert [g[0] for g in run(["s " + " ".join(str(x) for x in c) for c, _ in cases])] == [w for _, w in cases]
    regs = [((8, 3, 255, 0, 255), 1), ((8, 3, 0, 0, 256), 0), ((8, 3, 256, 0, 0), 0), ((32, 16) + (0xFFFFFFFF,) * 16, 1), ((2, 1, 3), 1), ((2, 1, 4), 0)]
    assert [g[0] for g in run(["g " + " ".join(str(x) for x in c) for c, _ in regs])] == [w for _, w in regs]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------
def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _args(**over):
    fields = dict(word_bits=8, reg_count=8, pc=0x1000, inst=0x2000, a=0x3000, value=0x4000, regs=0x5000, flag_bits=0x6000, m=4,
                  selection=(ctypes.c_uint32 * 32)(*exetable.selection_table(exetable.DEFAULT_SELECTION)), dst=0x10000, n=64, stream=None)
    fields.update(over)
    return api.ExeTableArgs(**fields)


def _table(**entries):
    return (ctypes.c_uint32 * 32)(*exetable.selection_table(dict(exetable.DEFAULT_SELECTION, **entries)))


def test_bad_arguments_are_einval():
    """refused before the device is looked for: the pointers are never followed"""
    lib = api.lib()
    assert lib.trh_exe_table_dev(api.FP, None) == -1
    for over, word in ((dict(word_bits=1), "word_bits"), (dict(word_bits=33), "word_bits"), (dict(reg_count=0), "reg_count"), (dict(reg_count=17), "reg_count"),
                       (dict(m=0), "steps"), (dict(m=64), "steps"), (dict(m=65), "steps"), (dict(dst=0x10008), "16-byte"), (dict(dst=None), "16-byte"),
                       (dict(pc=None), "null step"), (dict(inst=None), "null step"), (dict(a=None), "null step"), (dict(value=None), "null step"),
                       (dict(regs=None), "null step"), (dict(flag_bits=None), "null step"), (dict(regs=0x5002), "4-byte"), (dict(flag_bits=0x6001), "4-byte"),
                       (dict(selection=_table(add=(exetable.PC, exetable.REG_RJ, exetable.REG_NEXT_RI, exetable.ZERO))), "selection[4] gives variable a"),
                       (dict(selection=_table(jmp=(exetable.A, exetable.VALUE, exetable.ZERO, exetable.UNSET))), "selection[20] gives variable b"),
                       (dict(selection=_table(mov=(exetable.A, exetable.REG_NEXT_RI, exetable.ONE, exetable.UNSET))), "selection[18] gives variable c"),
                       (dict(selection=_table(answer=(exetable.A, exetable.PC, exetable.ZERO, exetable.MAX_WORD))), "selection[31] gives variable d"),
                       (dict(selection=_table(shr=(exetable.A, exetable.REG_RJ, exetable.REG_NEXT_RI, exetable.NONDET(11)))), "selection[12] gives variable d")):
        a = _args(**over)
        assert lib.trh_exe_table_dev(api.FP, ctypes.byref(a)) == -1, over
        assert word in lib.trh_last_error().decode(), (over, lib.trh_last_error())
    assert lib.trh_exe_table_dev(7, ctypes.byref(_args())) == -1 and "unknown field id 7" in lib.trh_last_error().decode()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_no_device_is_enodev():
    a = _args()
    assert api.lib().trh_exe_table_dev(api.FQ, ctypes.byref(a)) == -2


def test_the_stream_travels_in_the_struct():
    header = open(os.path.join(ROOT, "include", "trh.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    (params,) = re.findall(r"\btrh_exe_table_dev\s*\(([^;{}]*?)\)\s*;", header)
    assert "stream" not in params and params.split(",")[0].strip() == "int field_id"
    assert "trh_exe_table_dev" in api.EXPORTED_SYMBOLS and hasattr(api.lib(), "trh_exe_table_dev")
    assert [name for name, _ in api.ExeTableArgs._fields_][-3:] == ["dst", "n", "stream"]
    assert "TRH_EXE_NONDET = 16" in header and exetable.NONDET(exetable.RULE_PC_PLUS_ONE) == 26
