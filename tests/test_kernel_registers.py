"""After `make`: register and scratch counts of the kernels that run the lazy domain's products (csrc/field.h), read from the metadata
of the built code objects through tools/isa_regs.py -- nothing runs.  The accumulation, combine, reduce and NTT-pass kernels must stay
free of scratch, and their VGPR counts must not rise above those of the row-order build (profiles/r06_kernel_stats.md): a VGPR more
than 168 takes the accumulation from three waves per SIMD to two."""
import glob
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGPR_LIMIT = {"msm_accumulate_seg_kernel": 160, "msm_combine_kernel": 155, "msm_reduce_kernel": 201, "ntt_passy_kernel": 98}


@pytest.fixture(scope="module")
def registers():
    assert glob.glob(os.path.join(ROOT, "tiny-ram-halo2_amd", "csrc", "*.o")), "no objects in csrc/: run `make`"
    spec = importlib.util.spec_from_file_location("isa_regs", os.path.join(ROOT, "tools", "isa_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collect(count_instructions=False)


@pytest.mark.parametrize("field", ["Fp", "Fq"])
@pytest.mark.parametrize("kernel", sorted(VGPR_LIMIT))
def test_no_scratch_and_vgprs_not_above_row_order_build(registers, kernel, field):
    name = f"{kernel}<{field}>"
    assert name in registers, f"{name} not found among {len(registers)} kernels"
    r = registers[name]
    assert r["scratch"] == 0, f"{name} spills: {r}"
    assert r["vgpr"] <= VGPR_LIMIT[kernel], f"{name}: {r['vgpr']} VGPRs, row-order build {VGPR_LIMIT[kernel]}"
