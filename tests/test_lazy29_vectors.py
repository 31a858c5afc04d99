"""CPU test: the signed 29-bit lazy domain (csrc/field.h Fy, csrc/curve.h XYZZz) at the bounds its comments state, through the plain
C++ branch of the headers under -fsanitize=undefined.  tests/lazy29_gen.py places the operands, asserts that each is inside the
stated precondition and computes the references from oracle/pasta.py integers; tests/native/lazy29_vec_test.cpp runs the records.
A worst-case record that overflows a limb or a column stops the run; a result that is not the reference's -- value, documented
range, limb form, bool -- fails its operation's test.  tests/test_gpu_lazy29.py sends the same records through the device branch."""
import os
import subprocess

import pytest

import lazy29_gen as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["fp", "fq"]


@pytest.fixture(scope="module")
def vec_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lazy29") / "lazy29_vec_test")
    subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-w", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "lazy29_vec_test.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def host_results(vec_exe, tmp_path_factory):
    """one run of the host driver per field, shared by the tests of that field"""
    done = {}

    def run(field):
        if field not in done:
            cs = gen.cases(field)  # the generator's self-check runs here: every operand inside its precondition, every reference computed
            d = tmp_path_factory.mktemp("lazy29_" + field)
            src, dst = str(d / "cases.bin"), str(d / "host.bin")
            gen.write_cases(src, cs)
            r = subprocess.run([vec_exe, src, dst], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
            assert r.returncode == 0 and "records ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
            done[field] = (cs, gen.read_results(dst, len(cs))[0])
        return done[field]
    return run


@pytest.mark.parametrize("field", FIELDS)
def test_generator_covers_every_op_and_edge_class(field):
    cs = gen.cases(field)
    assert {c.op for c in cs} == set(gen.OPS)
    per_op = {op: sum(1 for c in cs if c.op == op and c.tag.startswith("random")) for op in gen.OPS}
    assert all(per_op[op] >= gen.RANDOM_PER_OP for op in gen.OPS if not op.startswith("xyzzz")), per_op
    tags = " ".join(t for _, t in gen.edge_classes(cs))
    for word in ("low-limbs-0", "low-limbs-max", "only-limb3-set", "only-limb3-clear", "top=-1", "-16m", "16m", "R''(m-1)", "product-multiple-of-2^261",
                 "round0-r=0", "round8-r=2^29-1", "lazy-all+max", "lazy-all-max", "lazy-alternating", "worst-column", "signs opposed", "sub-top=+max",
                 "sub-top=-max", "twiddle-all--2^28", "twiddle-all-2^28-1", "wide-all+1.5*2^30", "all+(2^31-2^3-1)", "carry-ripples-through-all-limbs",
                 "bit28-flipped", "low-limb-in-window", "2^(30*8)", "2^(29*8)", "2^254", "P + P", "P + (-P)", "identity + P", "P + identity",
                 "y=+2(mod m)", "base-y-negated-limbs", "shift(x+6m,y-3m,zz-1m,zzz+0m)"):
        assert word in tags, word


@pytest.mark.parametrize("op", gen.OPS)
@pytest.mark.parametrize("field", FIELDS)
def test_host_branch_matches_bigint_reference(host_results, field, op):
    cs, res = host_results(field)
    bad = gen.failures(cs, res, op)
    assert not bad, "\n".join(bad)
