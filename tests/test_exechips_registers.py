"""After `make`: scratch and LDS use of the two kernels of trh_exe_chips_dev (csrc/exechips.hip, csrc/exechips_inv.h), read from the metadata
of the built code objects through tools/isa_regs.py -- nothing runs.  The row kernel stores each of a row's 37 cells as chip_cells yields it
(an array of them would live in scratch: 16 bytes a cell); the inversion kernel keeps a strip's denominators and prefix products in
registers, every index a constant.  The VGPR counts are recorded in DESIGN.md; no limit is fixed here."""
import glob
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def registers():
    assert glob.glob(os.path.join(ROOT, "tiny-ram-halo2_amd", "csrc", "*.o")), "no objects in csrc/: run `make`"
    spec = importlib.util.spec_from_file_location("isa_regs", os.path.join(ROOT, "tools", "isa_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(count_instructions=False)


@pytest.mark.parametrize("field", ["Fp", "Fq"])
@pytest.mark.parametrize("kernel", ["exe_chips_rows_kernel", "exe_chips_inverse_kernel"])
def test_no_scratch_and_no_lds(registers, kernel, field):
    name = f"{kernel}<{field}>"
    assert name in registers, f"{name} not found among {len(registers)} kernels"
    r = registers[name]
    print(name, r)
    assert r["scratch"] == 0, f"{name} uses scratch memory: {r}"
    assert r["lds"] == 0, r
