"""After `make`: scratch use of the quotient-terms kernel (csrc/quotient.hip), read from the metadata of the built code objects through
tools/isa_regs.py -- nothing runs.  The kernel keeps l0, l_last, l_active, X, the accumulator and the two running products of a set in
registers for the whole row; a spill of any of them would put a scratch round trip into every one of its ~1 400 multiplications.  The VGPR
count is recorded in DESIGN.md (f4); no limit is fixed here."""
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
def test_no_scratch(registers, field):
    name = f"quotient_terms_kernel<{field}>"
    assert name in registers, f"{name} not found among {len(registers)} kernels"
    r = registers[name]
    print(name, r)
    assert r["scratch"] == 0, f"{name} uses scratch memory: {r}"
    assert r["lds"] == 0 and 0 < r["vgpr"] <= 512, r
