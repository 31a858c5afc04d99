"""After `make`: scratch use of the hash_to_curve kernels (csrc/hashtocurve.hip), read from the metadata of the built code objects through
tools/isa_regs.py -- nothing runs.  Neither kernel may spill or index a local array at run time: BLAKE2b's message schedule must name
registers (csrc/blake2b.h unrolls the rounds for that), and the map's square-root chain keeps two running values instead of the eight stored
powers of fe_sqrt (csrc/fieldsqrt.h fe_sqrt_chain).  The VGPR counts are recorded in DESIGN.md section 4; no limit is fixed here until a
device has measured which occupancy the kernels want."""
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
@pytest.mark.parametrize("kernel", ["h2c_hash_kernel", "h2c_map_kernel"])
def test_no_scratch(registers, kernel, field):
    name = f"{kernel}<{field}>"
    assert name in registers, f"{name} not found among {len(registers)} kernels"
    r = registers[name]
    assert r["scratch"] == 0, f"{name} uses scratch memory: {r}"
    assert r["lds"] == 0 and 0 < r["vgpr"] <= 512, r
