"""The whole-bin LDS bucket sort (msm_bin_sort_kernel) at the edges of its capacity, against the closed form (bases P_i = (s0 + i d) G).

At 2^20 pairs (c = 16, 256 level-1 bins of 2^7 buckets each) a bin holds 4096 entries on average and the LDS takes up to
bin_cap = 5120 of them; a window with a bigger bin takes the chunked passes instead.  The scalars below move every window-0 digit of
bins 0 and 255 to a uniform draw over the 254 bins between, then put exactly K digits into bin 0: bin 0 of window 0 holds K entries
(one under the capacity, at it -- every register slot of the sort filled -- or one over it), bin 255 is empty, and every other bin stays
far under the capacity (checked on the digits themselves).  The short top window of 254-bit scalars is oversize in every case (its
bins hold twice the average), so one launch mixes windows sorted in LDS with windows that took the chunked passes; trh_stat
"msm_bin_sorted_windows" tells which path every window took.  The generator of the scalars is tests/msm_sort_cases.py.
"""
import numpy as np
import pytest

import cpu_ref
import pasta as o
from msm_sort_cases import BIN_CAP, LOG_N, canonical as _canonical, lds_windows as _lds_windows
from tiny_ram_halo2_amd import api, synth

pytestmark = pytest.mark.gpu

CURVE = "pallas"


@pytest.fixture(scope="module", autouse=True)
def _init():
    api.init(0)
    yield


@pytest.fixture(scope="module")
def bases():
    return api.Bases.generate(CURVE, synth.BASE_S0, synth.BASE_D, 1 << LOG_N)


def _want(can):
    q = o.CURVES[CURVE].scalar.m
    total = synth.weighted_scalar_sum(can, synth.BASE_S0, synth.BASE_D) % q
    g = np.array(o.CURVES[CURVE].affine_limbs(o.CURVES[CURVE].generator), np.uint64)
    return cpu_ref.to_affine(CURVE, cpu_ref.scalar_mul(CURVE, g, np.array(o.int_to_limbs(total), np.uint64)))


@pytest.mark.parametrize("k,one_bucket", [(BIN_CAP - 1, False), (BIN_CAP, False), (BIN_CAP + 1, False), ((3 << LOG_N) // 4, True)])
def test_msm_bin_sort_capacity_edges(bases, k, one_bucket):
    can = _canonical(0x50B7 + k, k, one_bucket)
    got = bases.msm(cpu_ref.field_op("fq", "to_mont", can))
    assert api.stat("msm_bin_sorted_windows") == _lds_windows(k)
    assert (got[:8] == _want(can)).all()


@pytest.mark.parametrize("batch", [2, 4])
def test_msm_bin_sort_batches(bases, batch):
    """blockIdx.z: items whose window 0 fits (at the capacity, empty bin 0) next to an item whose window 0 does not"""
    n = 1 << LOG_N
    ks = [BIN_CAP, BIN_CAP + 1, 0, BIN_CAP - 1][:batch]
    cans = [_canonical(0xBA7 + i, k) for i, k in enumerate(ks)]
    sc = np.stack([cpu_ref.field_op("fq", "to_mont", c) for c in cans])
    got = bases.msm_batch_dev(api.DeviceBuffer.from_host(sc), n, batch)
    assert api.stat("msm_bin_sorted_windows") == sum(_lds_windows(k) for k in ks)
    for i, c in enumerate(cans):
        assert (got[i, :8] == _want(c)).all(), i
