"""Verdicts do not leak between entries (csrc/verdict.h).

Six entry points report through the SAME words of their context -- sums that kernels add to, minima that kernels lower -- and read them
through the same pinned landing area.  What that makes possible, and separate words did not, is a missing seed: an entry that finds the
count, the minimum or the refusal of the entry before it.  Seven calls run on one context in a row, then in the reverse order; each must
return what the same call returns alone in a fresh context, and what its inputs say it must:

  1. trh_exe_table_dev         refused: step 5 of 70 breaks a rule (a minimum is lowered)
  2. trh_points_decompress_dev 130 valid encodings: reports 130 (no minimum lowered)
  3. trh_perm_check_dev        a satisfied assignment: (0, cells)
  4. trh_expr_check_dev        five outputs, one bad row 64 in one of them: (1, 64) there, (0, usable) in the others
  5. trh_mem_table_dev         refused: record 3 of 40 has a time that does not increase
  6. trh_lookup_check_dev      every input present: (0, usable)
  7. trh_mem_table_dev         a consistent log of 40 records: no inconsistent load, first_inconsistent == 40

The inputs and helpers are those of the entries' own test files."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import encoding_cases as ec
import exetable_model as em
import memtable_model as mm
import mock_cases as mc
import pasta as o
import test_gpu_encoding as t_enc
import test_gpu_exetable as t_exe
import test_gpu_memtable as t_mem
import test_gpu_mock as t_mock
import test_gpu_permkeygen as t_perm
from tiny_ram_halo2_amd import api, mock, permutation


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


@pytest.fixture(scope="module")
def calls():
    """[(name, call, expected)]: call() -> everything the entry returned, comparable with ==; expected: what the inputs demand of it (a
    predicate).  The inputs are made once and never written to."""
    out = []
    # 1. a refused Exe table
    W, R = 16, 4
    steps = list(t_exe.drawn(W, R, 70))
    assert em.first_violation(W, R, steps) is None
    steps[5] = steps[5]._replace(pc=1 << W)
    assert em.first_violation(W, R, steps) == 5

    def exe_refused():
        dst = t_exe.filled(R, 128)
        with pytest.raises(api.TrhError) as e:
            t_exe.device_build("fq", W, R, steps, out=dst)
        return str(e.value), bool((t_exe.host(dst) == t_exe.FILL).all())
    out.append(("exe_refused", exe_refused, lambda r: "step 5 " in r[0] and r[1]))
    # 2. 130 valid encodings
    cv, encs, x = o.CURVES["pallas"], [], 1
    while len(encs) < 130:
        if cv.lift_x(x) is not None:
            encs.append(ec.enc_int(x, len(encs) & 1))
        x += 1
    d_enc = t_enc.dev_bytes(b"".join(encs))

    def decompress():
        d_xy = torch.full((130, 8), -1, dtype=torch.int64, device="cuda")
        first_bad = api.points_decompress_dev("pallas", d_enc, d_xy, 130)
        return first_bad, t_enc.host_u64(d_xy, 8).tolist()
    out.append(("decompress", decompress, lambda r: r[0] == 130))
    # 3. a satisfied permutation
    k, n_columns = 9, 3
    asm = permutation.Assembly("fp", k, n_columns)
    asm.copy_many(t_perm.random_copies(k, n_columns, 200, 0x7E4D))
    values, _ = t_perm.cycle_values(asm.mapping().reshape(-1).astype(np.int64), 0x7E4E)
    cols = t_perm.to_dev(values.reshape(n_columns, 1 << k, 4))
    ptrs = (api._vp * n_columns)(*[cols[j].data_ptr() for j in range(n_columns)])
    cells = n_columns << k

    def perm_check():
        n_bad, first = ctypes.c_uint64(7), ctypes.c_uint64(7)
        api._check(api.lib().trh_perm_check_dev(asm.handle, api.FP, ptrs, ctypes.byref(n_bad), ctypes.byref(first), torch.cuda.current_stream().cuda_stream))
        return n_bad.value, first.value
    out.append(("perm_check", perm_check, lambda r: r == (0, cells)))
    # 4. the five-output gate check of tests/test_gpu_mock.py with one bad row
    field, log_n = "fp", 8
    f, usable = o.FIELDS[field], t_mock.GATE_SIZES[8]
    ints = dict(t_mock.gate_witness(field, log_n))
    ints[("advice", 4)] = list(ints[("advice", 4)])
    ints[("advice", 4)][64] = (ints[("advice", 4)][64] + 1) % f.m              # the value p_0 = s (E_0 - advice 4) expects, queried at rotation 0 only
    assert t_mock.gate_model(f, ints, 1 << log_n, usable) == [[64], [], [], [], []]
    gate_dev = {key: t_mock.to_dev(f, col) for key, col in ints.items()}
    ev = t_mock.gate_evaluator(field)

    def gate_check():
        n_bad, first, words = ev.check(gate_dev, log_n, usable, bitmap=True)
        return [int(v) for v in n_bad], [int(v) for v in first], t_mock.words_of(words).tolist()
    out.append(("gate_check", gate_check, lambda r: r[0] == [1, 0, 0, 0, 0] and r[1] == [64] + [usable] * 4))
    # 5. a refused Mem table, 7. a consistent one
    rng = mm.rng_of(0x7E4F)
    log = t_mem.log_over(rng, 16, [rng.randrange(12) for _ in range(40)], [4, 5])
    table = mm.build(16, log, [4, 5])
    assert table.n_inconsistent == 0
    late = list(log)
    late[3] = (log[3][0], log[2][1], log[3][2], log[3][3])
    with pytest.raises(ValueError, match="record 3$"):
        mm.build(16, late, [4, 5])

    def mem_refused():
        dst = t_mem.filled(90)
        with pytest.raises(api.TrhError) as e:
            t_mem.device_build("fq", 16, late, [4, 5], out=dst)
        return str(e.value), bool((t_mem.host(dst) == t_mem.FILL).all())

    def mem_consistent():
        got = t_mem.device_build("fq", 16, log, [4, 5], 90)
        return got.rows, got.n_inconsistent, got.first_inconsistent, t_mem.host(got.columns).tolist()
    # 6. a lookup with every input present
    l_usable = 300
    inputs, tables = mc.lookup_case("range", 2, l_usable, False)
    assert mc.lookup_model(inputs, tables, l_usable)[:2] == (0, l_usable)
    d_in, d_tab = t_mock.dev_columns(inputs), t_mock.dev_columns(tables)

    def lookup():
        n_bad, first, words = mock.lookup_check("fp", d_in, d_tab, l_usable, bitmap=True)
        # the slots visited are a sum word too; their number depends on which thread claimed a slot first, so it is held to its bounds
        return n_bad, first, t_mock.words_of(words).tolist(), 2 * l_usable <= api.stat("lookup_check_probes") <= mc.PROBE_CAP * 2 * l_usable
    out.append(("mem_refused", mem_refused, lambda r: "log record 3 " in r[0] and r[1]))
    out.append(("lookup", lookup, lambda r: r[:2] == (0, l_usable) and r[3]))
    out.append(("mem_consistent", mem_consistent, lambda r: r[:3] == (len(table.rows), 0, 40)))
    yield out
    asm.destroy()


def test_verdicts_do_not_leak_between_entries(calls):
    alone = {}
    for name, call, demanded in calls:
        fresh = api.Context(0)
        try:
            with fresh:
                alone[name] = call()
        finally:
            fresh.destroy()
        assert demanded(alone[name]), (name, alone[name][:3])
    shared = api.Context(0)
    try:
        with shared:
            for name, call, _ in calls + calls[::-1]:
                assert call() == alone[name], name
    finally:
        shared.destroy()
