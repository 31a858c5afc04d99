"""The Exe chips as Python integers: what trh_exe_chips_dev (csrc/exechips.hip) and csrc/exetable.h's chip_row must compute, written from
the entry's description in include/trh.h over tests/exetable_model.py's row and run -- and the tests' own restatement of every gate those
columns must satisfy.  The tests' own: the package never imports this file, and nothing here imports the package.

    DEFAULT                          opcode name -> TRH_CHIP_* bits: out.rs:148-349 and the `ch:` fields of aux.rs:109-396
    columns(R)                       the 52 + R column names
    chip_row(W, mask, a, b, c, d, flag_next, p)   one row's cells but Out / changed as {name: integer}; a_flag is the inverse mod p
    build(W, R, steps, n, p, ...)    the columns as lists of n integers (negative _word cells as they are: reduce mod p to compare)
    first_bad(selection, chips)      (opcode, fault) of the first entry the host refuses, or None
    flag2_rows(steps, chips)         what trh_stat "exechips_flag2_rows" must report
    System(W, R)                     the gates: tests/golden/chip_gates.json but `Mem`, plus the logic chip (logic.rs:125-185), the even-bits
                                     `decompose` gate (even_bits.rs:146-156) per decomposed word and sprod (sprod.rs:65-92), as
                                     tests/test_gpu_logic_chip.py builds them; bind(exe, chips, n, table_len) -> the columns they read
    pow_table(W)                     the (value, power) pairs of the shift lookup with (W, 2^W) where pow.rs:58-62 has (W, 0)"""
import json
import os

import exetable_model as em

AND, XOR, OR, SUM, PROD, SSUM, SPROD, MOD, SHIFT, FLAG1, FLAG2, FLAG3, FLAG4, B_FLAG, CH_PC, CH_FLAG, CH_REG = (1 << i for i in range(17))
OUT_NAMES = ["and", "xor", "or", "sum", "prod", "ssum", "sprod", "mod", "shift", "flag1", "flag2", "flag3", "flag4"]
UNKNOWN = 0xFFFFFFFF
LOGIC, SIGNED_OPS = AND | XOR | OR, SSUM | SPROD
# which Out bits compute a group of cells
ENABLE = {"a": MOD | LOGIC | SIGNED_OPS, "b": MOD | SUM | SIGNED_OPS | FLAG4 | LOGIC, "c": XOR | PROD | SHIFT | SIGNED_OPS, "d": PROD | SPROD,
          "logic": LOGIC, "sg_a": SIGNED_OPS, "sg_b": SPROD | FLAG4, "sg_c": SIGNED_OPS, "r": FLAG3 | SHIFT}

_RF, _F12 = CH_REG | CH_FLAG, FLAG1 | FLAG2
DEFAULT = {
    "and": AND | _F12 | _RF, "or": OR | _F12 | _RF, "xor": XOR | _F12 | _RF, "not": XOR | _F12 | _RF, "add": SUM | _RF, "sub": SUM | _RF,
    "mull": PROD | _F12 | _RF, "umulh": PROD | _F12 | _RF, "smulh": SPROD | _F12 | _RF, "udiv": MOD | _F12 | FLAG3 | _RF, "umod": MOD | _F12 | FLAG3 | _RF,
    "shl": SHIFT | FLAG4 | B_FLAG | _RF, "shr": SHIFT | FLAG4 | _RF, "cmpe": XOR | _F12 | CH_FLAG, "cmpa": SUM | CH_FLAG, "cmpae": SUM | CH_FLAG,
    "cmpg": SSUM | CH_FLAG, "cmpge": SSUM | CH_FLAG, "mov": XOR | CH_REG, "cmov": MOD | CH_REG, "jmp": XOR | CH_PC, "cjmp": MOD | CH_PC, "cnjmp": MOD | CH_PC,
    "load.w": CH_REG, "store.w": XOR, "answer": 0,
}
SG = ("msb", "sigma", "check", "check_even", "check_odd")


def columns(R):
    names = [f"out_{x}" for x in OUT_NAMES] + [f"ch_reg{i}" for i in range(R)] + ["ch_pc", "ch_flag"]
    names += [f"{v}_{h}" for v in "abcd" for h in ("even", "odd")] + [f"{s}_{x}" for s in ("es", "os") for x in ("word", "even", "odd")]
    names += [f"sg_{v}_{x}" for v in "abc" for x in SG]
    return names + ["r_word", "r_even", "r_odd", "a_shift", "a_power", "a_flag", "lsb_b", "b_flag"]


def halves(w):
    even = odd = 0
    for i in range(0, w.bit_length() + 1, 2):
        even |= ((w >> i) & 1) << i
        odd |= ((w >> (i + 1)) & 1) << i
    assert even + 2 * odd == w
    return even, odd


def is_even_bits(v, W):
    return 0 <= v < 1 << W and all(not (v >> i) & 1 for i in range(1, W, 2))


def chip_row(W, mask, a, b, c, d, flag_next, p):
    out = {name: 0 for name in columns(0)[15:]}
    word = lambda v: 0 <= v < 1 << W  # noqa: E731
    for name, v in zip("abcd", (a, b, c, d)):
        if mask & ENABLE[name] and word(v):
            out[f"{name}_even"], out[f"{name}_odd"] = halves(v)
    if mask & LOGIC and word(a) and word(b):
        for s, k in (("es", 0), ("os", 1)):
            out[f"{s}_word"] = halves(a)[k] + halves(b)[k]
            out[f"{s}_even"], out[f"{s}_odd"] = halves(out[f"{s}_word"])
    for name, v in zip("abc", (a, b, c)):
        if mask & ENABLE[f"sg_{name}"] and word(v):
            msb = v >> (W - 1)
            check = halves(v)[1] + (1 - 2 * msb) * (1 << (W - 2))
            assert check >= 0
            out.update({f"sg_{name}_msb": msb, f"sg_{name}_sigma": abs(em.signed(W, v)), f"sg_{name}_check": check, f"sg_{name}_check_even": halves(check)[0],
                        f"sg_{name}_check_odd": halves(check)[1]})
    if mask & (FLAG3 | SHIFT):
        r = (0 if c == 0 else c - a - 1) if mask & FLAG3 else (0 if a > W else W - a)
        out["r_word"] = r
        if word(r):
            out["r_even"], out["r_odd"] = halves(r)
    if mask & SHIFT:
        out["a_shift"], out["a_power"] = int(a > W), (0 if a < 0 else 1 << min(a, W))
    if mask & FLAG2:
        out["a_flag"] = pow(c + flag_next, -1, p) if (c + flag_next) % p else 0
    if mask & FLAG4:
        out["lsb_b"], out["b_flag"] = b & 1, int(bool(mask & B_FLAG))
    return out


def first_bad(selection, chips):
    """selection, chips: 32 words each"""
    for op in range(32):
        e = chips[op]
        if (e == UNKNOWN) != (selection[op] == UNKNOWN):
            return op, "known"
        if e == UNKNOWN:
            continue
        if e >> 17:
            return op, "bit"
        if e & FLAG3 and e & SHIFT:
            return op, "r"
        if e & B_FLAG and not e & FLAG4:
            return op, "b_flag"
    return None


def row(W, R, selection, chips, step, nxt, p):
    tv = em.row(W, R, selection, step, nxt)
    mask = chips[em.NAMES[step.op]]
    out = {name: 0 for name in columns(R)}
    for i, name in enumerate(OUT_NAMES):
        out[f"out_{name}"] = (mask >> i) & 1
    out["ch_pc"], out["ch_flag"] = int(bool(mask & CH_PC)), int(bool(mask & CH_FLAG))
    if mask & CH_REG:
        out[f"ch_reg{step.ri}"] = 1
    out.update(chip_row(W, mask, tv["tv_a"], tv["tv_b"], tv["tv_c"], tv["tv_d"], int(nxt.flag) if nxt else 0, p))
    return out


def build(W, R, steps, n, p, selection=em.DEFAULT, chips=DEFAULT):
    """-> 52 + R lists of n integers"""
    assert 0 < len(steps) < n and W % 2 == 0 and em.first_violation(W, R, steps, selection) is None
    names = columns(R)
    cols = [[0] * n for _ in names]
    for i, s in enumerate(steps):
        r = row(W, R, selection, chips, s, steps[i + 1] if i + 1 < len(steps) else None, p)
        for c, name in enumerate(names):
            cols[c][i] = r[name]
    return cols


def flag2_rows(steps, chips=DEFAULT):
    return sum(1 for s in steps if chips[em.NAMES[s.op]] & FLAG2)


def pow_table(W):
    return {(i, 1 << i) for i in range(W + 1)}


# ---- the gates --------------------------------------------------------------------------------------------------------------------------------
def _col(name, rot=0):
    return ("col", name, rot)


def _sum(*xs):
    out = xs[0]
    for x in xs[1:]:
        out = ("sum", out, x)
    return out


def _prod(*xs):
    out = xs[0]
    for x in xs[1:]:
        out = ("prod", out, x)
    return out


def _rename(e, f):
    if e[0] == "col":
        return ("col", f(e[1]), e[2])
    if e[0] == "const":
        return e
    if e[0] == "scaled":
        return ("scaled", _rename(e[1], f), e[2])
    return (e[0],) + tuple(_rename(x, f) for x in e[1:])


class System:
    """gates: [(name, expression tuple over column NAMES)] for pasta.evaluate_gates once bind() has produced {name: values}.  Names: the
    exe table's (tests/exetable_model.columns), this entry's (columns), `s_table`, and per signed word v: the fixture's sg_* instance."""
    # the fixture's column names onto the two entries' (a name that maps to itself is the exe table's or this entry's own)
    FIXTURE = {"a": "tv_a", "b": "tv_b", "c": "tv_c", "d": "tv_d", "msb_b": "sg_b_msb", "a_sigma": "sg_a_sigma", "a_msb": "sg_a_msb", "c_sigma": "sg_c_sigma",
               "c_msb": "sg_c_msb", "rs_even": "r_even", "rs_odd": "r_odd"}
    FIXTURE.update({f"s_{x}": f"out_{x}" for x in ("flag1", "flag2", "flag3", "flag4", "mod", "prod", "ssum", "sum", "shift")})
    # the selectors that are sums of Out cells: name -> the Out bits
    SELECTORS = {"s_logic": LOGIC, "s_dec_r": ENABLE["r"], **{f"s_dec_{v}": ENABLE[v] for v in "abcd"}, **{f"s_signed_{v}": ENABLE[f"sg_{v}"] for v in "abc"}}
    # the even-bits lookups: (selector, cell) -- selector * cell must be an even-bits value
    EVEN_LOOKUPS = ([(f"s_dec_{v}", f"{v}_{h}") for v in "abcd" for h in ("even", "odd")] + [("s_logic", f"{s}_{h}") for s in ("es", "os") for h in ("even", "odd")]
                    + [(f"s_signed_{v}", f"sg_{v}_check_{h}") for v in "abc" for h in ("even", "odd")] + [("s_dec_r", "r_even"), ("s_dec_r", "r_odd")])

    @staticmethod
    def out_names(mask):
        return [f"out_{x}" for i, x in enumerate(OUT_NAMES) if mask >> i & 1]

    def __init__(self, W, R, to_tuple, from_json):
        here = os.path.dirname(os.path.abspath(__file__))
        with open(os.path.join(here, "golden", "chip_gates.json")) as fh:
            doc = json.load(fh)
        assert doc["word_bits"] == W and doc["reg_count"] == R
        self.W, self.R = W, R
        adv, sel = doc["advice"], doc["selectors"]

        def named(key):
            kind, i = key
            return sel[i] if kind == "selector" else adv[i]

        self.gates = []
        for g in doc["gates"]:
            if g["name"] == "Mem":
                continue
            e = _rename(to_tuple(from_json(g["expr"])), named)
            if g["name"] == "signed":  # one instance per signed word
                for v in "abc":
                    inst = {"sg_word": f"tv_{v}", "sg_odd": f"{v}_odd", "sg_msb": f"sg_{v}_msb", "sg_sigma": f"sg_{v}_sigma", "sg_check": f"sg_{v}_check",
                            "s_signed": f"s_signed_{v}"}
                    self.gates.append((f"signed.{v}", _rename(e, lambda n: inst.get(n, n))))
            else:
                self.gates.append((g["name"], _rename(e, lambda n: self.FIXTURE.get(n, n))))
        two, table = ("const", 2), _col("s_table")

        def decompose(name, s, word, even, odd):
            self.gates.append((name, _prod(table, _col(s), _sum(_col(even), ("scaled", _col(odd), 2), ("neg", _col(word))))))
        for v in "abcd":
            decompose(f"decompose.{v}", f"s_dec_{v}", f"tv_{v}", f"{v}_even", f"{v}_odd")
        for s in ("es", "os"):
            decompose(f"decompose.{s}", "s_logic", f"{s}_word", f"{s}_even", f"{s}_odd")
        for v in "abc":
            decompose(f"decompose.check_{v}", f"s_signed_{v}", f"sg_{v}_check", f"sg_{v}_check_even", f"sg_{v}_check_odd")
        decompose("decompose.r", "s_dec_r", "r_word", "r_even", "r_odd")
        self.gates.append(("l_add.even", _prod(table, _col("s_logic"), _sum(_col("a_even"), _col("b_even"), ("neg", _col("es_word"))))))
        self.gates.append(("l_add.odd", _prod(table, _col("s_logic"), _sum(_col("a_odd"), _col("b_odd"), ("neg", _col("os_word"))))))
        and_ = _sum(_col("es_odd"), ("scaled", _col("os_odd"), 2))
        xor = _sum(_col("es_even"), ("scaled", _col("os_even"), 2))
        res = ("neg", _col("tv_c"))
        self.gates.append(("and", _prod(table, _col("out_and"), _sum(and_, res))))
        self.gates.append(("xor", _prod(table, _col("out_xor"), _sum(xor, res))))
        self.gates.append(("or", _prod(table, _col("out_or"), _sum(xor, and_, res))))
        sg = lambda v: _sum(("neg", _prod(_col(f"sg_{v}_msb"), two, _col(f"sg_{v}_sigma"))), _col(f"sg_{v}_sigma"))  # noqa: E731
        self.gates.append(("sprod", _prod(table, _col("out_sprod"), _sum(_prod(sg("a"), sg("b")), ("neg", _col("tv_d")), ("neg", ("scaled", sg("c"), 1 << W))))))
        self.names = sorted({n for _, g in self.gates for n in _names(g)})

    def bind(self, exe, chips, n, table_len, p):
        """exe, chips: the two entries' columns (lists of n integers, in em.columns / columns order) -> {name: values mod p}; the r
        decomposition is bound on flag3 rows and on shift rows that are not saturated (r_word is 0 there, as the halves are)"""
        cols = dict(zip(em.columns(self.R), exe))
        cols.update(zip(columns(self.R), chips))
        cols["s_table"] = [1] * table_len + [0] * (n - table_len)
        for name, mask in self.SELECTORS.items():
            cols[name] = [sum(cols[x][r] for x in self.out_names(mask)) for r in range(n)]
        return {name: [x % p for x in cols[name]] for name in self.names}


def _names(e):
    if e[0] == "col":
        return {e[1]}
    if e[0] == "const":
        return set()
    if e[0] == "scaled":
        return _names(e[1])
    return set().union(*(_names(x) for x in e[1:]))
