"""GPU test (-m gpu): the signed 29-bit lazy domain (csrc/field.h Fy, csrc/curve.h XYZZz) on the device at the bounds its comments
state.  On the device the products and reduction rounds of this domain are blocks of v_mad_i64_i32 inline assembly, on the host
plain C++: tests/native/lazy29_dev_test (built by `make` with the library's flags) runs the records of tests/lazy29_gen.py through
both in one binary.  Per operation and field: the device's limbs equal the host branch's, limb for limb, and equal the big-integer
reference (value, documented range, limb form, bool).  One subprocess per case file, under a time limit, never retried."""
import os
import subprocess

import pytest

import lazy29_gen as gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "lazy29_dev_test")
FIELDS = ["fp", "fq"]


@pytest.fixture(scope="module")
def device_results(tmp_path_factory):
    done = {}

    def run(field):
        if field not in done:
            done[field] = None  # a failed run is not started again by the next test of the field
            assert os.path.exists(EXE), "tests/native/lazy29_dev_test is missing: run `make`"
            cs = gen.cases(field)
            d = tmp_path_factory.mktemp("lazy29_dev_" + field)
            src, dst = str(d / "cases.bin"), str(d / "results.bin")
            gen.write_cases(src, cs)
            r = subprocess.run(["timeout", "-k", "10", "120", EXE, src, dst], capture_output=True, text=True)
            assert r.returncode == 0 and "records ok" in r.stdout, f"exit {r.returncode}\n{r.stdout}{r.stderr}"
            res = gen.read_results(dst, len(cs), sets=2)
            done[field] = (cs, res[0], res[1])
        assert done[field] is not None, "the device run of this field failed (see the first test of the field)"
        return done[field]
    return run


@pytest.mark.parametrize("op", gen.OPS)
@pytest.mark.parametrize("field", FIELDS)
def test_device_branch_matches_host_branch_and_bigint_reference(device_results, field, op):
    cs, dev, host = device_results(field)
    rows = gen.rows_of(cs, op)
    differ = [i for i in rows if (dev[i] != host[i]).any()]
    msg = [f"{op}[{field}] {cs[i].tag} (record {i}): device {dev[i].tolist()} != host {host[i].tolist()}; operands {cs[i].slots}" for i in differ[:8]]
    assert not differ, f"{len(differ)} of {len(rows)} records differ between device and host\n" + "\n".join(msg)
    bad = gen.failures(cs, dev, op)
    assert not bad, "\n".join(bad)
