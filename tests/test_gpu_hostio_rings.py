"""GPU tests (-m gpu) of the host-pointer staging rings (csrc/hostio.hip, csrc/copypool.h) at slot sizes where they wrap: the cases of
tests/hostio_cases.py under each of its option sets (stage_slot_mb, copy_threads), every result bit for bit against a reference that is
not the code under test -- cpu_ref.best_fft, cpu_ref.EvaluationDomain, the device form of the same transform on the stacked columns, the
closed form of an MSM over generated bases -- and the byte counters of trh_io_stats against the model of hostio_cases (never against
what the library says).  tests/test_hostio_cases.py checks without a GPU that the cases reach the paths they are written for.

Options are fixed while a context exists, so every option set runs in ONE child process (common.run_with_options) that first asserts its
options took effect, runs every case and prints one line per case; the assertions are made here, on those lines.  The hand-over case (a
device group, TRH_FORCE_NO_PEER=1) has a child of its own: trh_init_multi fixes the group for the process."""
import pytest

import hostio_cases as hc
from common import run_with_options

pytestmark = pytest.mark.gpu

CHILD = r"""
import ctypes, time
import numpy as np, torch
import cpu_ref, pasta as o
import hostio_cases as hc
from tiny_ram_halo2_amd import api, poly, synth

api.init(0)
assert api.get_option("stage_slot_mb") == SLOT_MB, api.get_option("stage_slot_mb")
assert api.get_option("copy_threads") == (-1 if THREADS is None else THREADS), api.get_option("copy_threads")
SLOT = SLOT_MB * hc.MiB
TH = min(cpu_ref.hardware_threads(), 16)
lib = api.lib()


def omega(field, log_n):
    f = o.FIELDS[field]
    return np.array(f.limbs(f.omega(log_n)), np.uint64)


def counters():
    io = api.io_stats(reset=True)
    return {k: int(io[k]) for k in ("h2d_bytes", "d2h_bytes", "h2d_zero_bytes")}


def report(name, ok, t0, **kv):
    print("case", name, "ok" if ok else "BAD", *[f"{k}={v}" for k, v in kv.items()], f"ms={(time.perf_counter() - t0) * 1e3:.0f}", flush=True)


def fft(name, field, a, log_n, want):
    work = a.copy()
    api.io_stats(reset=True)
    t0 = time.perf_counter()
    api.best_fft_inplace(field, work, omega(field, log_n), log_n)
    report(name, bool((work == want).all()), t0, **counters())


def oracle_fft(field, a, log_n):
    return cpu_ref.best_fft(field, a, omega(field, log_n), log_n, threads=TH)


# (a) single transfers past several ring turns
for name, field, vec in hc.ring_cases(SLOT_MB):
    a = hc.build(vec)
    log_n = vec.n.bit_length() - 1
    fft(name, field, a, log_n, oracle_fft(field, a, log_n))

# the same uploads behind device work that is not waited for: every DMA queues while the host goes on filling slots
def closed_form(curve, sc):
    cv = o.CURVES[curve]
    can = cpu_ref.field_op({"pallas": "fq", "vesta": "fp"}[curve], "from_mont", sc)
    total = synth.weighted_scalar_sum(can, synth.BASE_S0, synth.BASE_D) % cv.scalar.m
    g = np.array(cv.affine_limbs(cv.generator), np.uint64)
    return cpu_ref.to_affine(curve, cpu_ref.scalar_mul(curve, g, np.array(o.int_to_limbs(total), np.uint64)))


stream = torch.cuda.current_stream().cuda_stream
held = torch.zeros((1 << hc.HELD_LOG_N, 4), dtype=torch.int64, device="cuda")
w_held = omega("fp", hc.HELD_LOG_N)
api.ntt_dev("fp", held, hc.HELD_LOG_N, w_held, stream=stream)   # twiddles and plan exist before the first held case
torch.cuda.synchronize()


def hold():
    for _ in range(hc.HELD_REPEATS):
        api.ntt_dev("fp", held, hc.HELD_LOG_N, w_held, stream=stream)


for name, kind, field, vec in hc.held_cases(SLOT_MB):
    a = np.ascontiguousarray(hc.build(vec))
    if kind == "fft":
        log_n = vec.n.bit_length() - 1
        want, work, w = oracle_fft(field, a, log_n), a.copy(), omega(field, log_n)
        api.best_fft_inplace(field, a.copy(), w, log_n)   # twiddles of this size: nothing but the staging between hold() and the upload
        api.io_stats(reset=True)
        t0 = time.perf_counter()
        hold()
        api.best_fft_inplace(field, work, w, log_n)
        report(name, bool((work == want).all()), t0, **counters())
    else:
        want = closed_form("pallas", a)
        bases = api.Bases.generate("pallas", synth.BASE_S0, synth.BASE_D, vec.n)
        bases.msm(a)
        api.io_stats(reset=True)
        t0 = time.perf_counter()
        hold()
        got = bases.msm(a)
        report(name, bool((got[:8] == want).all()), t0, ranges=api.stat("msm_host_ranges"), **counters())
        bases.destroy()
torch.cuda.synchronize()
del held

# (b) zero elision and speculation
padded = hc.build(hc.elide_vectors()["padded"])
want_padded = {f: oracle_fft(f, padded, hc.ELIDE_LOG_N) for f in ("fp", "fq")}
for name, field, vec, repeat in hc.elide_cases(SLOT_MB):
    a = hc.build(vec)
    want = oracle_fft(field, a, hc.ELIDE_LOG_N)
    fft(name, field, a, hc.ELIDE_LOG_N, want)
    if repeat:   # the restart on rings that are warm from the restart before, and the rings' state after it
        fft(name + "-again", field, a, hc.ELIDE_LOG_N, want)
        fft(name + "-then-padded", field, padded, hc.ELIDE_LOG_N, want_padded[field])

# (c) pipelines
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
to_host = lambda t: t.cpu().numpy().view(np.uint64)
for b in hc.BATCHES:
    n, w, model = 1 << b.log_n, omega(b.field, b.log_n), hc.batch_model(b, SLOT)
    cols, allocs, regs = [], [], []
    try:
        for i in range(b.count):
            src = np.zeros((n, 4), dtype=np.uint64) if i in b.zero else synth.field_elements(0xC300 + (b.log_n << 8) + i, n)
            kind = b.pinned.get(i)
            if kind == "alloc":
                p = ctypes.c_void_p()
                api._check(lib.trh_host_alloc(ctypes.byref(p), src.nbytes))
                allocs.append(p)
                a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n, 4))
                a[:] = src
            else:
                a = np.ascontiguousarray(src.copy())
                if kind == "register":
                    api._check(lib.trh_host_register(a.ctypes.data_as(ctypes.c_void_p), a.nbytes))
                    regs.append(a)
            cols.append(a)
        orig = np.stack(cols)
        d = to_dev(orig)
        api.ntt_dev(b.field, d, b.log_n, w, batch=b.count, stream=stream)
        torch.cuda.synchronize()
        dev = to_host(d).reshape(b.count, n, 4)
        del d
        api.io_stats(reset=True)
        t0 = time.perf_counter()
        api.best_fft_batch(b.field, cols, w, b.log_n)
        io = counters()
        bad = [i for i in range(b.count) if not (cols[i] == dev[i]).all()]
        bad += [i for i in model["edges"] if not (cols[i] == oracle_fft(b.field, orig[i], b.log_n)).all()]
        report(b.name, not bad, t0, bad=",".join(map(str, sorted(set(bad)))) or "-", **io)
    finally:
        for a in regs:
            api._check(lib.trh_host_unregister(a.ctypes.data_as(ctypes.c_void_p)))
        cols = None
        for p in allocs:
            api._check(lib.trh_host_free(p))

dm = hc.DOMAIN
dom = poly.EvaluationDomain(dm["field"], dm["j"], dm["k"])
cd = cpu_ref.EvaluationDomain(dm["field"], dm["j"], dm["k"], threads=TH)
n, N, D = 1 << dm["k"], 1 << dom.extended_k, dm["j"] - 1
stride = N // n
orig = [np.ascontiguousarray(synth.field_elements(0xC700 + i, n)) for i in range(dm["count"])]
want = [np.asarray(cd.coeff_to_extended(c)).reshape(N, 4) for c in orig]
api.io_stats(reset=True)
t0 = time.perf_counter()
ext = dom.coeff_to_extended_host(orig)
io = counters()
report("domain-extended", all(e.shape == (N, 4) and (e == w_).all() for e, w_ in zip(ext, want)) and len(ext) == len(want), t0, ratio=N // n, **io)
del ext
t0 = time.perf_counter()
blk = dom.coeff_to_extended_blocks_host(orig, D)
io = counters()
report("domain-blocks", len(blk) == len(want) and all((blk[i][r] == want[i][r::stride]).all() for i in range(len(want)) for r in range(D)), t0, **io)
del blk, want

# (d) MSM uploads: generated bases P_i = (s0 + i d) G, so the sum is (sum_i s_i (s0 + i d)) G (closed_form above)
resident, host_bases = {}, {}
for name, vec, on_host in hc.msm_cases(SLOT_MB, THREADS):
    sc = np.ascontiguousarray(hc.build(vec))
    want = closed_form("pallas", sc)
    if vec.n not in resident:
        resident[vec.n] = api.Bases.generate("pallas", synth.BASE_S0, synth.BASE_D, vec.n)
    if on_host and vec.n not in host_bases:
        host_bases[vec.n] = np.ascontiguousarray(resident[vec.n].download())   # downloaded once
    api.io_stats(reset=True)
    t0 = time.perf_counter()
    got = api.best_multiexp("pallas", sc, host_bases[vec.n]) if on_host else resident[vec.n].msm(sc)
    report(name, bool((got[:8] == want).all()), t0, ranges=api.stat("msm_host_ranges"), **counters())
host_bases.clear()
for b in resident.values():
    b.destroy()

cm = hc.COMMIT
n = cm["n"]
b = api.Bases.generate(cm["curve"], synth.BASE_S0, synth.BASE_D, n + 1)
for batch in cm["batches"]:
    cols = [np.ascontiguousarray(synth.field_elements(0xE800 + i, n)) for i in range(batch)]
    blinds = synth.field_elements(0xE8FF, batch)
    api.io_stats(reset=True)
    t0 = time.perf_counter()
    got = b.commit_batch_host(cols, blinds)
    io = counters()
    ok = all((got[i] == b.msm(np.concatenate([cols[i], blinds[i][None]]))).all() for i in range(batch))
    ok = ok and (got[0][:8] == closed_form(cm["curve"], np.concatenate([cols[0], blinds[0][None]]))).all()
    report(f"commit-{batch}", bool(ok), t0, **io)
api.shutdown()
print("done")
"""

HANDOVER_CHILD = r"""
import time
import numpy as np, torch
import cpu_ref, pasta as o
import hostio_cases as hc
from tiny_ram_halo2_amd import api, synth

h = hc.HANDOVER
assert api.lib().trh_device_count() >= 1
api.init_multi(h["group"])
assert api.get_option("stage_slot_mb") == h["options"][0] and api.get_option("copy_threads") == -1 and api.get_option("force_no_peer") == 1
assert api.group_size() == len(h["group"]) and api.lib().trh_group_peer_access() == 0
curve, n = "pallas", h["n"]
d = torch.from_numpy(synth.field_elements(0xE900, n).view(np.int64)).cuda()
api.set_shard_min(1 << 62)
one = api.Bases.generate(curve, synth.BASE_S0, synth.BASE_D, n)
assert one.shards() == 1
want = one.msm_dev(d, n)          # one context: no hand-over
one.destroy()
api.set_shard_min(1 << 12)
b = api.Bases.generate(curve, synth.BASE_S0, synth.BASE_D, n)
assert b.shards() == len(h["group"])
log_n = h["fft_log_n"]
f = o.FIELDS["fp"]
w = np.array(f.limbs(f.omega(log_n)), np.uint64)
a = synth.field_elements(0xE901, 1 << log_n)
want_fft = cpu_ref.best_fft("fp", a, w, log_n, threads=min(cpu_ref.hardware_threads(), 16))
api.io_stats(reset=True)
t0 = time.perf_counter()
got = b.msm_dev(d, n)             # every shard's scalars through its context's pinned download ring
io = api.io_stats(reset=True)     # shard 0 is the default context
work = a.copy()
api.best_fft_inplace("fp", work, w, log_n)   # the next stage_d2h meets the events the hand-over left on the slots
io2 = api.io_stats(reset=True)
print("case handover-msm", "ok" if (got == want).all() else "BAD", f"h2d_bytes={int(io['h2d_bytes'])} d2h_bytes={int(io['d2h_bytes'])}")
print("case handover-then-fft", "ok" if (work == want_fft).all() else "BAD", f"h2d_bytes={int(io2['h2d_bytes'])} d2h_bytes={int(io2['d2h_bytes'])} h2d_zero_bytes={int(io2['h2d_zero_bytes'])}")
again = b.msm_dev(d, n)           # and the hand-over meets the events the download left
print("case handover-again", "ok" if (again == want).all() else "BAD")
print("done")
"""


def run_child(script, header, env):
    text = run_with_options(header + script, env, timeout=300)
    print(text)
    assert text.rstrip().endswith("done"), text[-2000:]
    lines = {}
    for ln in text.splitlines():
        if ln.startswith("case "):
            _, name, verdict, *kv = ln.split()
            assert name not in lines, name
            lines[name] = (verdict, dict(p.split("=", 1) for p in kv))
    return lines


def expected(slot_mb, threads):
    """name -> the counters the model of hostio_cases gives the case (only the keys it speaks about)"""
    slot, want = slot_mb * hc.MiB, {}
    for name, _, vec in hc.ring_cases(slot_mb):
        nbytes = vec.n * hc.ROW
        want[name] = {"h2d_bytes": nbytes, "d2h_bytes": nbytes, "h2d_zero_bytes": 0}
    for name, kind, _, vec in hc.held_cases(slot_mb):
        nbytes = vec.n * hc.ROW
        want[name] = {"h2d_bytes": nbytes, "h2d_zero_bytes": 0, **({"d2h_bytes": nbytes} if kind == "fft" else {"ranges": 1})}
    padded = hc.best_fft_model(hc.elide_vectors()["padded"].rows, hc.ELIDE_LOG_N, slot)
    for name, _, vec, repeat in hc.elide_cases(slot_mb):
        m = hc.best_fft_model(vec.rows, hc.ELIDE_LOG_N, slot)
        want[name] = {k: m[k] for k in ("h2d_bytes", "d2h_bytes", "h2d_zero_bytes")}   # a dropped pass is counted once
        if repeat:
            want[name + "-again"] = want[name]
            want[name + "-then-padded"] = {k: padded[k] for k in ("h2d_bytes", "d2h_bytes", "h2d_zero_bytes")}
    for b in hc.BATCHES:
        m = hc.batch_model(b, slot)
        want[b.name] = {k: m[k] for k in ("h2d_bytes", "d2h_bytes", "h2d_zero_bytes")}
    d = hc.DOMAIN
    col = hc.ROW << d["k"]
    want["domain-extended"] = {"ratio": 8, "h2d_bytes": d["count"] * col, "d2h_bytes": d["count"] * col * 8, "h2d_zero_bytes": 0}
    want["domain-blocks"] = {"h2d_bytes": d["count"] * col, "d2h_bytes": d["count"] * col * (d["j"] - 1), "h2d_zero_bytes": 0}
    for name, vec, host_bases in hc.msm_cases(slot_mb, threads):
        m = hc.msm_model(vec.rows, vec.n, slot, host_bases)
        want[name] = {"ranges": m["ranges"], "h2d_bytes": m["h2d_bytes"], "h2d_zero_bytes": m["h2d_zero_bytes"]}
    for batch in hc.COMMIT["batches"]:
        want[f"commit-{batch}"] = {"h2d_bytes": batch * (hc.COMMIT["n"] + 1) * hc.ROW, "h2d_zero_bytes": 0}
    assert list(want) == hc.case_names(slot_mb, threads)
    return want


@pytest.mark.parametrize("slot_mb,threads", hc.OPTION_SETS, ids=[hc.option_id(*o) for o in hc.OPTION_SETS])
def test_rings_under_option_set(slot_mb, threads):
    """every case of hostio_cases under one option set: right bit for bit, and the counters the model's"""
    want = expected(slot_mb, threads)
    lines = run_child(CHILD, f"SLOT_MB, THREADS = {slot_mb!r}, {threads!r}\n", hc.option_env(slot_mb, threads))
    assert sorted(lines) == sorted(want)   # the child ran every case, and nothing else
    wrong = [name for name in want if lines[name][0] != "ok"]
    assert not wrong, wrong
    off = {name: (k, v, lines[name][1].get(k)) for name, w in want.items() for k, v in w.items() if lines[name][1].get(k) != str(v)}
    assert not off, off


def test_down_ring_shared_with_the_hand_over():
    """option force_no_peer = 1 and a group of two contexts on device 0: one trh_msm_dev on 2^20 device-resident scalars sends each
    shard's half (16 MiB) through the destination context's 1 MiB download ring, four turns deep, by events alone; the point is the
    one-context point.  The best_fft that follows downloads through the same slots behind the events the hand-over left on them, and
    the hand-over after it behind the download's."""
    h = hc.HANDOVER
    env = dict(hc.option_env(*h["options"]), TRH_FORCE_NO_PEER="1")
    lines = run_child(HANDOVER_CHILD, "", env)
    assert sorted(lines) == ["handover-again", "handover-msm", "handover-then-fft"]
    assert all(v == "ok" for v, _ in lines.values()), lines
    share = h["n"] // len(h["group"]) * hc.ROW
    assert share // (h["options"][0] * hc.MiB) >= hc.RING_TURNS
    kv = lines["handover-msm"][1]
    # shard 0 is the default context, whose counters the child reads: exactly its share went down into its ring and up out of it
    assert kv == {"h2d_bytes": str(share), "d2h_bytes": str(share)}, kv
    nbytes = hc.ROW << h["fft_log_n"]
    assert lines["handover-then-fft"][1] == {"h2d_bytes": str(nbytes), "d2h_bytes": str(nbytes), "h2d_zero_bytes": "0"}
