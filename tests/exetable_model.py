"""The Exe table as Python integers: what trh_exe_table_dev (csrc/exetable.hip) and csrc/exetable.h must compute, written from the entry's
description in include/trh.h, plus a small TinyRAM interpreter that produces traces to feed it.  Both are the tests' own: the package never
imports this file, and nothing here imports the package.

    Step                            one step of a trace: pc, opcode, ri, rj, a, a_is_reg, the registers and the flag BEFORE it, value
    row(W, R, selection, step, nxt) one row as {column name: integer}; SHR_LO's value may be negative (the device stores it mod the field)
    build(W, R, steps, n, ...)      the 28 + 9 R columns as lists of n integers, rows behind the trace zero
    first_violation(W, R, steps)    the first step the entry refuses, or None
    run(W, R, program, tape)        the interpreter: -> (steps, answer)
    reference_load_store / reference_load_answer / loop_program / every_opcode_program   programs as lists of (op, ri, rj, a, a_is_reg)
    random_steps(rnd, W, R, m)      m steps drawn independently (operand, ri, rj, registers), every opcode with both operand kinds: no machine ran them

Nothing here checks the cmpg / cmpge and smulh rules beyond the reference's own formulas (aux.rs:468-499, instructions.rs:323-337): the
identities of tests/test_exetable_host.py cover the unsigned comparisons, the unsigned products, division, logic and the shifts."""
import random
from collections import namedtuple

OPCODES = {"and": 0, "or": 1, "xor": 2, "not": 3, "add": 4, "sub": 5, "mull": 6, "umulh": 7, "smulh": 8, "udiv": 9, "umod": 10, "shl": 11, "shr": 12,
           "cmpe": 13, "cmpa": 14, "cmpae": 15, "cmpg": 16, "cmpge": 17, "mov": 18, "cmov": 19, "jmp": 20, "cjmp": 21, "cnjmp": 22, "store.w": 28,
           "load.w": 29, "answer": 31}
NAMES = {v: k for k, v in OPCODES.items()}
UNSET, PC, PC_NEXT, PC_PLUS_ONE, REG_RI, REG_RJ, REG_NEXT_RI, A, VALUE, ZERO, ONE, MAX_WORD = range(12)
NONDET0 = 16
REM, QUOT, CMP_GT, CMP_GE, MUL_HI, MUL_LO, SMUL_LO, XOR, SHL_HI, SHR_LO, RULE_PC_PLUS_ONE = range(11)
VARS = "abcd"
# the selector columns each variable has, by the source that sets them (registers apart)
LEGAL = {"a": {PC_NEXT, REG_RI, REG_RJ, REG_NEXT_RI, A, VALUE}, "b": {PC, PC_NEXT, PC_PLUS_ONE, REG_RI, REG_RJ, REG_NEXT_RI, A, MAX_WORD},
         "c": {REG_RI, REG_RJ, REG_NEXT_RI, A, ZERO}, "d": {PC, REG_RI, REG_RJ, REG_NEXT_RI, A, ZERO, ONE}}
SELECTOR_OF = {PC: "pc", PC_NEXT: "pc_next", PC_PLUS_ONE: "pc_plus_one", VALUE: "v_addr", ZERO: "zero", ONE: "one", MAX_WORD: "max_word"}


def nd(rule):
    return NONDET0 + rule


# aux.rs:105-398, with CJmp's d as NONDET(pc + 1)
DEFAULT = {
    "and": (A, REG_RJ, REG_NEXT_RI, UNSET), "or": (A, REG_RJ, REG_NEXT_RI, UNSET), "xor": (A, REG_RJ, REG_NEXT_RI, UNSET), "not": (A, MAX_WORD, REG_NEXT_RI, UNSET),
    "add": (A, REG_RJ, REG_NEXT_RI, ZERO), "sub": (A, REG_NEXT_RI, REG_RJ, ZERO), "mull": (A, REG_RJ, nd(MUL_HI), REG_NEXT_RI),
    "umulh": (A, REG_RJ, REG_NEXT_RI, nd(MUL_LO)), "smulh": (A, REG_RJ, REG_NEXT_RI, nd(SMUL_LO)), "udiv": (nd(REM), REG_NEXT_RI, A, REG_RJ),
    "umod": (REG_NEXT_RI, nd(QUOT), A, REG_RJ), "shl": (A, REG_RJ, nd(SHL_HI), REG_NEXT_RI), "shr": (A, REG_RJ, REG_NEXT_RI, nd(SHR_LO)),
    "cmpe": (A, REG_RI, nd(XOR), UNSET), "cmpa": (REG_RI, nd(CMP_GT), A, ZERO), "cmpae": (REG_RI, nd(CMP_GE), A, ONE), "cmpg": (REG_RI, nd(CMP_GT), A, ZERO),
    "cmpge": (REG_RI, nd(CMP_GE), A, ONE), "mov": (A, REG_NEXT_RI, ZERO, UNSET), "cmov": (REG_NEXT_RI, A, ZERO, REG_RI), "jmp": (A, PC_NEXT, ZERO, UNSET),
    "cjmp": (PC_NEXT, A, ZERO, nd(RULE_PC_PLUS_ONE)), "cnjmp": (PC_NEXT, PC_PLUS_ONE, ZERO, A), "load.w": (VALUE, REG_RI, ZERO, ZERO),
    "store.w": (VALUE, REG_NEXT_RI, ZERO, ZERO), "answer": (A, PC, ZERO, ZERO),
}

Step = namedtuple("Step", "pc op ri rj a a_is_reg regs flag value")


def columns(R):
    regs, nexts = [f"reg{i}" for i in range(R)], [f"reg_next{i}" for i in range(R)]
    names = ["s_trace", "pc", "flag"] + regs + ["opcode", "immediate", "value", "tv_a", "tv_b", "tv_c", "tv_d"]
    names += ["sa_" + x for x in ["pc_next"] + regs + nexts + ["a", "v_addr"]]
    names += ["sb_" + x for x in ["pc", "pc_next", "pc_plus_one"] + regs + nexts + ["a", "max_word"]]
    names += ["sc_" + x for x in regs + nexts + ["a", "zero"]]
    names += ["sd_" + x for x in ["pc"] + regs + nexts + ["a", "zero", "one"]]
    return names + ["sa_non_det", "sb_non_det", "sc_non_det", "sd_non_det"]


def signed(W, w):
    return w - (1 << W) if w >> (W - 1) else w


def nondet(rule, W, RI, RJ, Av, pc):
    s = min(Av, W)
    if rule == REM:
        return 0 if Av == 0 else RJ % Av
    if rule == QUOT:
        return 0 if Av == 0 else RJ // Av
    if rule == CMP_GT:
        return (1 << W) - (RI - Av) if RI > Av else Av - RI
    if rule == CMP_GE:
        return (1 << W) - 1 - (RI - Av) if RI >= Av else Av - RI - 1
    if rule == MUL_HI:
        return (RJ * Av) >> W
    if rule == MUL_LO:
        return (RJ * Av) % (1 << W)
    if rule == SMUL_LO:
        return (signed(W, Av) * signed(W, RJ)) % (1 << W)
    if rule == XOR:
        return RI ^ Av
    if rule == SHL_HI:
        return (RJ << s) >> W
    if rule == SHR_LO:
        return (RJ << s) - ((RJ >> s) << W)
    assert rule == RULE_PC_PLUS_ONE
    return pc + 1


def operand(step):
    return step.regs[step.a] if step.a_is_reg else step.a


def row(W, R, selection, step, nxt, cjmp_literal=False):
    """nxt: the successor, None behind the last step (the zero row).  cjmp_literal: CJmp's d as the reference writes it -- sd_pc and sd_one
    both set, the value pc + 1 (aux.rs:1070-1073)"""
    out = {name: 0 for name in columns(R)}
    out.update(s_trace=1, pc=step.pc, flag=int(step.flag), opcode=step.op, immediate=0 if step.a_is_reg else step.a, value=step.value)
    for i in range(R):
        out[f"reg{i}"] = step.regs[i]
    pc_next = nxt.pc if nxt else 0
    next_ri = nxt.regs[step.ri] if nxt else 0
    for v, src in zip(VARS, selection[NAMES[step.op]]):
        if src == UNSET:
            continue
        if src >= NONDET0:
            out[f"tv_{v}"] = nondet(src - NONDET0, W, step.regs[step.ri], step.regs[step.rj], operand(step), step.pc)
            out[f"s{v}_non_det"] = 1
            continue
        assert src in LEGAL[v], (v, src)
        if src in (REG_RI, REG_RJ) or (src == A and step.a_is_reg):
            k = {REG_RI: step.ri, REG_RJ: step.rj, A: step.a}[src]
            out[f"tv_{v}"], out[f"s{v}_reg{k}"] = step.regs[k], 1
        elif src == REG_NEXT_RI:
            out[f"tv_{v}"], out[f"s{v}_reg_next{step.ri}"] = next_ri, 1
        elif src == A:
            out[f"tv_{v}"], out[f"s{v}_a"] = step.a, 1
        else:
            out[f"tv_{v}"] = {PC: step.pc, PC_NEXT: pc_next, PC_PLUS_ONE: step.pc + 1, VALUE: step.value, ZERO: 0, ONE: 1, MAX_WORD: (1 << W) - 1}[src]
            out[f"s{v}_{SELECTOR_OF[src]}"] = 1
    if cjmp_literal and step.op == OPCODES["cjmp"]:
        out.update(tv_d=step.pc + 1, sd_pc=1, sd_one=1, sd_non_det=0)
    return out


def first_violation(W, R, steps, selection=DEFAULT):
    for i, s in enumerate(steps):
        known = s.op in NAMES and NAMES[s.op] in selection
        in_range = s.ri < R and s.rj < R and (not s.a_is_reg or s.a < R)
        words = all(w < 1 << W for w in (s.pc, s.a, s.value) + tuple(s.regs))
        if not (known and in_range and words) or (i == len(steps) - 1 and s.op != OPCODES["answer"]):
            return i
    return None


def build(W, R, steps, n, selection=DEFAULT, cjmp_literal=False):
    """-> 28 + 9 R lists of n integers"""
    assert 0 < len(steps) < n and first_violation(W, R, steps, selection) is None
    names = columns(R)
    cols = [[0] * n for _ in names]
    for i, s in enumerate(steps):
        r = row(W, R, selection, s, steps[i + 1] if i + 1 < len(steps) else None, cjmp_literal)
        for c, name in enumerate(names):
            cols[c][i] = r[name]
    return cols


# ---- the interpreter (trace.rs:378-551) ----------------------------------------------------------------------------------------------------
def run(W, R, program, tape=(), max_steps=4096):
    """program: [(op name, ri, rj, a, a_is_reg)].  Memory is a map from address to word, tape word i at address i * W / 8, 0 where nothing
    was stored.  -> (steps, answer)"""
    mask = (1 << W) - 1
    regs, pc, flag, steps = [0] * R, 0, False, []
    mem = {i * W // 8: w for i, w in enumerate(tape)}
    while len(steps) < max_steps:
        name, ri, rj, a, a_is_reg = program[pc]
        Av = regs[a] if a_is_reg else a
        value = 0
        if name == "load.w":
            value = mem.get(Av, 0)
        elif name == "store.w":
            value = regs[ri]
            mem[Av] = value
        steps.append(Step(pc, OPCODES[name], ri, rj, a, a_is_reg, tuple(regs), flag, value))
        jump = None
        if name in ("and", "or", "xor"):
            regs[ri] = {"and": regs[rj] & Av, "or": regs[rj] | Av, "xor": regs[rj] ^ Av}[name]
            flag = regs[ri] == 0
        elif name == "not":
            regs[ri] = ~Av & mask
            flag = regs[ri] == 0
        elif name == "add":
            r = regs[rj] + Av
            regs[ri], flag = r & mask, r > mask
        elif name == "sub":
            r = regs[rj] + (1 << W) - Av
            regs[ri], flag = r & mask, r <= mask
        elif name == "mull":
            r = regs[rj] * Av
            regs[ri], flag = r & mask, r <= mask
        elif name == "umulh":
            regs[ri] = (regs[rj] * Av) >> W
            flag = regs[ri] == 0
        elif name == "smulh":
            regs[ri] = ((signed(W, Av) * signed(W, regs[rj])) >> W) & mask
            flag = regs[ri] == 0
        elif name == "udiv":
            regs[ri], flag = (0 if Av == 0 else regs[rj] // Av), Av == 0
        elif name == "umod":
            regs[ri], flag = (0 if Av == 0 else regs[rj] % Av), Av == 0
        elif name == "shl":
            regs[ri], flag = (regs[rj] << min(Av, W)) & mask, bool(regs[rj] >> (W - 1))
        elif name == "shr":
            regs[ri], flag = regs[rj] >> min(Av, W), bool(regs[rj] & 1)
        elif name == "cmpe":
            flag = Av == regs[ri]
        elif name == "cmpa":
            flag = regs[ri] > Av
        elif name == "cmpae":
            flag = regs[ri] >= Av
        elif name == "cmpg":
            flag = signed(W, regs[ri]) > signed(W, Av)
        elif name == "cmpge":
            flag = signed(W, regs[ri]) >= signed(W, Av)
        elif name == "mov":
            regs[ri] = Av
        elif name == "cmov":
            if flag:
                regs[ri] = Av
        elif name == "jmp":
            jump = Av
        elif name == "cjmp":
            jump = Av if flag else pc + 1
        elif name == "cnjmp":
            jump = Av if not flag else pc + 1
        elif name == "load.w":
            regs[ri] = value
        elif name == "answer":
            return steps, Av
        else:
            assert name == "store.w", name
        pc = pc + 1 if jump is None else jump
    raise RuntimeError("the program did not answer")


def reference_load_store():  # trace.rs:567-584, run there with word_bits 8 and the tape [1]
    return [("load.w", 0, 0, 0, False), ("and", 1, 0, 1, False), ("store.w", 1, 0, 8, False), ("answer", 0, 0, 1, True)]


def reference_load_answer():  # trace.rs:605-618
    return [("load.w", 0, 0, 16, False), ("and", 1, 0, 128, False), ("answer", 0, 0, 1, False)]


def loop_program():
    """counts r0 up to r1 = 5 with cnjmp, leaves through a taken cjmp and a jmp"""
    return [("mov", 0, 0, 0, False), ("mov", 1, 0, 5, False), ("add", 0, 0, 1, False), ("cmpe", 0, 0, 1, True), ("cnjmp", 0, 0, 2, False), ("cjmp", 0, 0, 7, False),
            ("answer", 0, 0, 1, False), ("jmp", 0, 0, 8, False), ("answer", 0, 0, 0, False)]


def every_opcode_program():
    """every opcode at least once, immediates below 2^8, eight registers; jumps taken and not taken, division by zero, a shift past the word"""
    return [
        ("mov", 0, 0, 200, False), ("mov", 1, 0, 7, False), ("and", 2, 0, 0x0F, False), ("or", 2, 2, 1, True), ("xor", 3, 0, 1, True), ("not", 4, 0, 0, True),
        ("add", 5, 0, 100, False), ("sub", 5, 1, 0, True), ("mull", 6, 0, 0, True), ("umulh", 6, 0, 0, True), ("smulh", 7, 4, 0, True), ("udiv", 2, 0, 1, True),
        ("udiv", 2, 0, 0, False), ("umod", 3, 0, 1, True), ("umod", 3, 0, 0, False), ("shl", 4, 0, 3, False), ("shr", 4, 0, 1, True), ("shl", 4, 0, 40, False),
        ("shr", 4, 0, 40, False), ("cmpe", 0, 0, 200, False), ("cmpa", 0, 0, 1, True), ("cmpae", 1, 0, 7, False), ("cmpg", 4, 0, 0, True), ("cmpge", 0, 0, 0, True),
        ("cmov", 5, 0, 9, False), ("store.w", 0, 0, 4, False), ("load.w", 6, 0, 4, False), ("cmpe", 6, 0, 0, True), ("cjmp", 0, 0, 30, False), ("answer", 0, 0, 1, False),
        ("cnjmp", 0, 0, 33, False), ("jmp", 0, 0, 33, False), ("answer", 0, 0, 1, False), ("cmpe", 0, 0, 0, False), ("cnjmp", 0, 0, 36, False), ("answer", 0, 0, 1, False),
        ("cjmp", 0, 0, 0, False), ("answer", 0, 0, 1, True)]


def random_steps(rnd, W, R, m, words=None):
    """m steps, each drawn on its own: no machine ran them.  The (opcode, operand kind) pairs come in a shuffled order that holds every
    pair once before any repeats (m - 1 >= 52 reaches them all); step 0 starts the trace (pc = 0, flag clear, registers zero) and step
    m - 1 answers.  words: the pool the machine words are drawn from (default: any word)"""
    word = (lambda: rnd.randrange(1 << W)) if words is None else (lambda: rnd.choice(words))
    pairs = []
    while len(pairs) < m - 1:
        deck = [(op, kind) for op in sorted(NAMES) for kind in (False, True)]
        rnd.shuffle(deck)
        pairs += deck
    pairs = pairs[:m - 1] + [(OPCODES["answer"], rnd.random() < 0.5)]
    steps = []
    for i, (op, a_is_reg) in enumerate(pairs):
        regs = tuple(0 if i == 0 else word() for _ in range(R))
        steps.append(Step(0 if i == 0 else word(), op, rnd.randrange(R), rnd.randrange(R), rnd.randrange(R) if a_is_reg else word(), a_is_reg, regs,
                          i > 0 and rnd.random() < 0.5, word() if op in (OPCODES["load.w"], OPCODES["store.w"]) else 0))
    return steps


EXTREME = [0, 0xFFFFFFFF, 1, 2, 31, 32, 33, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFE]


def extreme_steps(R, m=None):
    """W = 32: pc + 1 = 2^32, 0xFFFFFFFF squared, shifts by 0, 31, 32 and more, comparisons of equal words, division by zero and by the
    largest word, with immediates and with register operands; then steps drawn from the same words, the last one an answer.  m: that many
    steps in all, made of the sharpest of the hand-picked ones and a drawn tail (default: all hand-picked ones and 300 drawn)"""
    top = 0xFFFFFFFF
    steps = [Step(top, OPCODES[op], 0, 0, top, False, (top,) * R, True, 0) for op in ("cjmp", "cnjmp", "jmp", "answer")]
    ri, rj, ra = 0, min(1, R - 1), R - 1
    if m is None:
        picks = [(rjv, av, riv, kind) for rjv in (top, 0x80000000, 1, 0) for av in (0, top, 32, 31, 33, 1) for riv in (av, top) for kind in (False, True)]
    else:
        picks = [(top, 0, 0, False), (top, top, top, False), (top, 32, 32, False), (0x80000000, 31, 31, False), (1, 33, 33, False), (0, 0, 0, False), (top, top, top, True)]
    for op in ("mull", "umulh", "smulh", "udiv", "umod", "cmpa", "cmpae", "cmpg", "cmpge", "cmpe", "shl", "shr", "add", "sub", "and", "not"):
        for rjv, av, riv, a_is_reg in picks:
            regs = [5] * R
            regs[ri], regs[rj] = riv, rjv  # with one register ri = rj, with two the operand's register is rj: the later write wins
            if a_is_reg:
                regs[ra] = av
            steps.append(Step(7, OPCODES[op], ri, rj, ra if a_is_reg else av, a_is_reg, tuple(regs), False, 0))
    tail = 300 if m is None else m - len(steps)
    assert tail > 0
    return steps + random_steps(random.Random(32), 32, R, tail, EXTREME)
