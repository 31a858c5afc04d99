"""The cases of tests/hostio_cases.py, without a GPU: the Python restatement of chunk_plan against the real one (csrc/copypool.h through
tests/native/chunkplan_dump.cpp), and the conditions each case has to meet on its inputs -- how often it turns the ring, where its zero
chunks lie, where its hidden elements sit relative to the lines probe_zero reads -- computed from the model for every option set, so
that tests/test_gpu_hostio_rings.py cannot pass without having gone there.  These are conditions on the inputs, not measurements."""
import os
import subprocess
import tempfile

import pytest

import hostio_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = hc.MiB
OPTS = pytest.mark.parametrize("slot_mb,threads", hc.OPTION_SETS, ids=[hc.option_id(*o) for o in hc.OPTION_SETS])


def plan_tuples():
    """every (bytes, slot, head, tail, tiny_tail) the cases put to chunk_plan, and a sweep around the sizes at which a plan changes"""
    out = set()
    for slot_mb, threads in hc.OPTION_SETS:
        slot = slot_mb * MiB
        for _, _, vec in hc.ring_cases(slot_mb):
            out |= {(vec.n * hc.ROW, slot, 1, 1, hc.TINY_TAIL), (vec.n * hc.ROW, slot, 0, 1, 0)}
        out |= {(hc.ROW << hc.ELIDE_LOG_N, slot, 1, 1, hc.TINY_TAIL), (hc.ROW << hc.ELIDE_LOG_N, slot, 0, 1, 0)}
        for b in hc.BATCHES:
            out.add((hc.ROW << b.log_n, slot, 0, 0, 0))
        for _, vec, host_bases in hc.msm_cases(*hc.SPLIT_OPTIONS) + hc.msm_cases(slot_mb, threads):
            cuts = hc.msm_host_cuts(host_bases, vec.n)
            for t, (a, b) in enumerate(zip(cuts, cuts[1:])):
                out.add(((b - a) * hc.ROW, slot, int(t == 0), int(t == 0 and len(cuts) == 2 and not host_bases), hc.TINY_TAIL if t == 0 else 0))
                out.add(((b - a) * 2 * hc.ROW, slot, 0, 0, 0))
    for slot_mb in (1, 2, 3, 6, 7, 16):
        for nbytes in (32, hc.TINY_TAIL, 4 * hc.TINY_TAIL, 4 * hc.TINY_TAIL + 32, MiB, 4 * MiB, 4 * MiB + 32, 8 * MiB, 8 * MiB + 32, 14 * MiB + 32, 33 * MiB + 64):
            for ht in range(4):
                for tiny in (0, hc.TINY_TAIL):
                    out.add((nbytes, slot_mb * MiB, ht & 1, ht >> 1, tiny))
    return sorted(out)


def test_chunk_plan_model_matches_copypool_h():
    src = os.path.join(ROOT, "tests", "native", "chunkplan_dump.cpp")
    tuples = plan_tuples()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "chunkplan_dump")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe, "-pthread"])
        r = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % t for t in tuples), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(tuples)
    for t, line in zip(tuples, lines):
        assert [int(v) for v in line.split()[1:]] == hc.chunk_plan(t[0], t[1], bool(t[2]), bool(t[3]), t[4]), t


def test_option_sets_grade_the_plans_as_claimed():
    """1 MiB: ungraded; 3 MiB: the 2 MiB pieces only; 7 MiB: the 6 MiB pieces too; and the parts of CopyPool::copy"""
    assert hc.OPTION_SETS == ((1, 0), (1, None), (3, 1), (7, 62))
    big = 64 * MiB
    assert set(hc.chunk_plan(big, 1 * MiB, True, True)) == {MiB}
    p3 = hc.chunk_plan(big, 3 * MiB, True, True)
    assert p3[0] == p3[-1] == hc.SMALL and hc.MID not in p3
    p7 = hc.chunk_plan(big, 7 * MiB, True, True)
    assert p7[:2] == [hc.SMALL, hc.MID] and p7[-2:] == [hc.MID, hc.SMALL]
    # (parts are whole 4 KiB pages: 7 MiB over 63 parts leaves the last one empty)
    assert [len(hc.pool_parts(63 * 5 * 4096, t)) for t in (0, 1, 4, 62)] == [1, 2, 5, 63] and len(hc.pool_parts(7 * MiB, 62)) == 62
    assert len(hc.pool_parts(MiB - 32, 62)) == 1


def test_down_ring_model_keeps_ns_chunks_ahead():
    """a slot is given to chunk i + NS only after chunk i was copied out of it, and never later than needed to keep NS in flight"""
    for nbytes, slot in ((8 * MiB, MiB), (32 * MiB, 3 * MiB), (64 * MiB, 7 * MiB), (3 * MiB, MiB)):
        plan, steps = hc.d2h_schedule(nbytes, slot)
        holder = {}
        for what, chunk, sl in steps:
            if what == "issue":
                assert sl not in holder and sl == chunk % hc.NS
                holder[sl] = chunk
            else:
                assert holder.pop(sl) == chunk
                assert len(holder) == min(hc.NS, len(plan) - chunk) - 1
        assert not holder and sum(plan) == nbytes


@OPTS
def test_ring_cases_turn_the_rings_they_are_for(slot_mb, threads):
    """(a): every case turns exactly the rings RING_STRESS names for it at least twice (2 * NS + 1 chunks); under every option set and for
    both fields some case does so for the upload ring and some for the download ring; a full random vector elides nothing"""
    slot = slot_mb * MiB
    turned = {}
    for name, field, vec in hc.ring_cases(slot_mb):
        log_n = vec.n.bit_length() - 1
        m = hc.best_fft_model(vec.rows, log_n, slot)
        assert m["h2d_zero_bytes"] == 0 and not m["restart"] and m["guessed"] == 0 and m["used"] == len(m["final"])
        assert [c.slot for c in m["final"]] == [i % hc.NS for i in range(m["used"])]
        got = tuple(d for d, chunks in (("up", m["used"]), ("down", len(m["down"]))) if chunks >= hc.RING_TURNS)
        assert got == hc.RING_STRESS[slot_mb, log_n], (name, m["used"], len(m["down"]))
        turned.setdefault(field, set()).update(got)
    assert turned == {"fp": {"up", "down"}, "fq": {"up", "down"}}
    assert sorted(k[1] for k in hc.RING_STRESS if k[0] == slot_mb) == sorted(hc.ring_log_ns(slot_mb))
    assert 18 in hc.ring_log_ns(slot_mb) and (slot_mb == 1 or 20 in hc.ring_log_ns(slot_mb))
    if slot_mb > 1:   # graded heads and tails appear with the ring still wrapping
        m = hc.best_fft_model(hc.FULL, max(hc.ring_log_ns(slot_mb)), slot)
        sizes = [c.size for c in m["final"]]
        assert sizes[0] == hc.SMALL and sizes[-1] == hc.TINY_TAIL and sizes[-2] == hc.SMALL and m["down"][-1] == hc.SMALL
        assert (hc.MID in sizes and hc.MID in m["down"]) == (slot_mb == 7)


@OPTS
def test_held_cases_reuse_a_slot_while_the_stream_waits(slot_mb, threads):
    """the held cases: the upload puts at least NS + 1 chunks through slots (the transforms turn the ring twice), so with the stream held
    back a slot comes round again before its DMA has run; the work that holds the stream is far longer than filling the ring"""
    slot = slot_mb * MiB
    kinds = []
    for name, kind, field, vec in hc.held_cases(slot_mb):
        kinds.append((kind, field))
        if kind == "fft":
            m = hc.best_fft_model(vec.rows, vec.n.bit_length() - 1, slot)
            assert m["used"] >= hc.RING_TURNS and m["h2d_zero_bytes"] == 0, name
        else:
            m = hc.msm_model(vec.rows, vec.n, slot, False)
            assert m["ranges"] == 1 and m["used"] >= hc.NS + 1 and m["h2d_zero_bytes"] == 0, name
            assert [c.slot for c in m["transfers"][0][1]] == [i % hc.NS for i in range(m["used"])]
    assert sorted(kinds, key=str) == sorted([("fft", "fp"), ("fft", "fq"), ("msm", None)], key=str)
    # 2^24 elements are 512 MiB read and written several times: milliseconds, against well under one for (NS + 1) slots of host copies
    assert (hc.ROW << hc.HELD_LOG_N) * hc.HELD_REPEATS >= 64 * (hc.NS + 1) * slot


@OPTS
def test_elision_cases_reach_what_they_are_for(slot_mb, threads):
    """(b), the vectors that are not hidden ones.  A vector whose data is followed by zeros to its end (padded, zero) cannot have an elided
    chunk BETWEEN two used ones; the two with blinding rows at the very end must, under every option set: the ring index then stands
    still while the transfer moves on.  `ragged` must also have a mixed chunk (data, then zeros) under every option set, and under every
    option set with copy threads some vector has a mixed chunk in which CopyPool::copy skips a part as zero and copies another."""
    slot = slot_mb * MiB
    vecs = hc.elide_vectors()
    model = {k: hc.best_fft_model(v.rows, hc.ELIDE_LOG_N, slot) for k, v in vecs.items()}
    assert hc.ROW << hc.ELIDE_LOG_N == hc.GUESS_MIN_BYTES
    for k, m in model.items():
        assert not m["restart"], k
        assert m["h2d_zero_bytes"] == sum(c.size for c in m["final"] if not vecs[k].rows.any(c.off, c.off + c.size)), k   # nothing guessed that a scan would not elide
    assert model["zero"]["used"] == 0 and model["zero"]["h2d_zero_bytes"] == hc.ROW << hc.ELIDE_LOG_N
    assert model["padded"]["guessed"] >= 1 and not model["padded"]["between"]
    for k in ("blinded", "ragged"):
        m = model[k]
        assert m["between"] and m["guessed"] >= 1 and m["final"][-1].size == hc.TINY_TAIL and m["final"][-1].kind == "copy", k
        # the padding in front of the tiny tail elides whole: that is what the tiny tail is for
        assert m["final"][-2].kind != "copy", k
    mixed = {k: hc.mixed_chunks(vecs[k].rows, model[k]["final"], 4 if threads is None else threads) for k in vecs}
    assert mixed["ragged"], "no chunk with data, then zeros"
    if threads != 0:
        assert any(skipped for k in mixed for _, skipped in mixed[k]), "no mixed chunk in which the pool skips a part"


@OPTS
def test_hidden_elements_are_off_every_probed_line(slot_mb, threads):
    """(b), the hidden ones: each sits in the padding, off every line probe_zero reads in the chunk that holds it; the three kinds next to
    probed lines sit in a chunk that probes as zero and so defeat the speculation; the other two sit in chunks that are never probed
    (below 1 MiB) and are found by the scan"""
    slot = slot_mb * MiB
    rows = hc.hidden_rows(slot_mb)
    padded = hc.elide_vectors()["padded"]
    first = hc.best_fft_model(padded.rows, hc.ELIDE_LOG_N, slot)["first"]
    want = set(hc.HIDDEN_KINDS) - ({"unprobed"} if slot_mb == 7 else set())   # 8 MiB in 7 MiB slots has no chunk below 1 MiB but the tiny tail
    assert set(rows) == want and len(set(rows.values())) == len(rows)
    for kind, row in rows.items():
        byte = row * hc.ROW
        assert not padded.rows.any(byte, byte + hc.ROW), kind
        (c,) = [c for c in first if c.off <= byte < c.off + c.size]
        rel = byte - c.off
        lines = hc.probe_lines(c.size)
        m = hc.best_fft_model(hc.hidden_vectors(slot_mb)[kind].rows, hc.ELIDE_LOG_N, slot)
        assert m["h2d_bytes"] == hc.ROW << hc.ELIDE_LOG_N
        if kind in ("after-line", "before-line", "block-end"):
            assert c.kind == "guess" and c.size >= hc.GUESS_MIN_CHUNK and m["restart"], kind
            assert all(not (l <= rel < l + hc.LINE) for l in lines), kind
            line = {"after-line": rel - hc.LINE, "before-line": rel + hc.ROW, "block-end": rel + hc.ROW}[kind]
            assert line in lines and line % hc.PROBE_STRIDE == 0 and line not in (0, c.size - hc.LINE), kind
            if kind == "block-end":
                assert line == c.size - hc.PROBE_STRIDE
            # the plain pass finds it: the chunk that holds it goes through a slot
            (after,) = [d for d in m["final"] if d.off <= byte < d.off + d.size]
            assert after.kind == "copy"
        else:
            assert c.size < hc.GUESS_MIN_CHUNK and c.kind == "zero" and not m["restart"], kind
            assert (c.size == hc.TINY_TAIL and c is first[-1]) == (kind == "tiny-tail")
            (after,) = [d for d in m["first"] if d.off <= byte < d.off + d.size]
            assert after.kind == "copy"
    # restated here once more, independently of probe_lines: the first and last 64 bytes and 64 bytes at every multiple of 64 KiB
    assert hc.probe_lines(MiB) == [0] + [k << 16 for k in range(1, 16)] + [MiB - 64]
    assert hc.probe_lines(768 << 10)[-2:] == [704 << 10, (768 << 10) - 64]


@OPTS
def test_batch_cases_reach_what_they_are_for(slot_mb, threads):
    """(c): log_n = 17 makes four pipeline items (the three-deep device ring is reused) with a ragged last one, segments longer than a
    slot at 1 and 3 MiB, and the three pinned columns at the first, a middle and the last position of ONE item that also holds pageable
    ones; log_n = 12 makes two full groups of 64 and a ragged one, far below a slot"""
    slot = slot_mb * MiB
    b17, b12 = hc.BATCHES
    m = hc.batch_model(b17, slot)
    assert m["group"] == 8 and [len(i) for i in m["items"]] == [8, 8, 8, 5]
    (item,) = [i for i in m["items"] if set(b17.pinned) & set(i)]
    assert set(b17.pinned) <= set(item) and item[0] in b17.pinned and item[-1] in b17.pinned and any(c in b17.pinned for c in item[1:-1])
    assert sorted(b17.pinned.values()) == ["alloc", "alloc", "register"] and len(set(item) - set(b17.pinned)) >= 1
    assert len(b17.zero) == 1 and b17.zero[0] not in b17.pinned
    per_segment = -(-(hc.ROW << 17) // slot)
    assert per_segment == {1: 4, 3: 2, 7: 1}[slot_mb]
    assert sum(m["down_chunks"][m["items"].index(item)]) == 3 + 5 * per_segment   # direct and ring chunks share one counter
    m = hc.batch_model(b12, slot)
    assert m["group"] == 64 and [len(i) for i in m["items"]] == [64, 64, 3] and (hc.ROW << 12) * 64 < 32 * MiB + 1
    d = hc.DOMAIN
    assert hc.group_for(hc.ROW << d["k"]) == 64 and d["count"] > 64 and d["count"] % 64


@OPTS
def test_msm_cases_reach_what_they_are_for(slot_mb, threads):
    """(d): the zero runs elide what the model says; at 1 MiB slots the aligned run is whole chunks, the mid-chunk run leaves a mixed
    chunk in front of it, and the run to the last 8 scalars leaves the tiny tail alone; the split case has three ranges"""
    slot = slot_mb * MiB
    names = [c[0] for c in hc.msm_cases(slot_mb, threads)]
    assert len(set(names)) == len(names)
    for name, vec, host_bases in hc.msm_cases(slot_mb, threads):
        m = hc.msm_model(vec.rows, vec.n, slot, host_bases)
        assert m["h2d_bytes"] == vec.n * (96 if host_bases else 32)
        if vec.name == "random":
            assert m["h2d_zero_bytes"] == 0 and m["ranges"] == 1
        if vec.name == "run-to-last-8":
            (sc,) = [t for kind, t in m["transfers"] if kind == "scalars"]
            assert [c.kind for c in sc] == ["zero"] * (len(sc) - 1) + ["copy"] and sc[-1].size == hc.TINY_TAIL
            assert m["h2d_zero_bytes"] == vec.n * hc.ROW - hc.TINY_TAIL
        if vec.name in ("run-aligned", "run-mid-chunk"):
            sc = m["transfers"][0][1]
            # an elided chunk between two used ones: 2^18 with the mid-chunk run at every slot size, with the aligned run where the run is
            # whole chunks (1 and 3 MiB); 2^16 is two or three chunks, and only the aligned run at 1 MiB elides the middle one
            want = {(1 << 18, "run-mid-chunk"): (1, 3, 7), (1 << 18, "run-aligned"): (1, 3), (1 << 16, "run-aligned"): (1,), (1 << 16, "run-mid-chunk"): ()}
            assert hc.summary(sc)["between"] == (slot_mb in want[vec.n, vec.name]), name
            if slot_mb == 1 and vec.name == "run-aligned":
                zero_rows = vec.n - sum(b - a for a, b in vec.ranges)
                assert m["h2d_zero_bytes"] == zero_rows * hc.ROW    # the run is whole chunks
            if vec.name == "run-mid-chunk" and (slot_mb == 1 or vec.n == 1 << 18):   # 2 MiB in larger slots: one chunk with data at both ends
                assert hc.mixed_chunks(vec.rows, sc, 4 if threads is None else threads)
        if name == "multiexp-split":
            assert m["ranges"] == 3 and len(vec.ranges) == 1 << 12
            cuts = hc.msm_host_cuts(True, vec.n)
            for a, b in zip(cuts, cuts[1:]):     # scattered over all three ranges
                assert sum(a <= r < b for r, _ in vec.ranges) >= 1 << 10
            later = [t for kind, t in m["transfers"][2:] if kind == "scalars"]
            assert all(hc.summary(t)["between"] for t in later)   # zero chunks inside a range that is part of a batch
            assert m["used"] >= 16 * hc.RING_TURNS
    assert ("multiexp-split" in names) == ((slot_mb, threads) == hc.SPLIT_OPTIONS)
    # the range boundaries restated in hostio_cases against the named sizes of tests/native/hostplan_test.cpp
    assert hc.msm_host_cuts(True, 1 << 21) == [0, 1 << 21] and hc.msm_host_cuts(True, (1 << 21) + 1) == [0, 699051, 1398102, (1 << 21) + 1]
    assert hc.msm_host_cuts(False, 3 << 21) == [0, 3 << 21] and hc.msm_host_cuts(False, (3 << 21) + 5) == [0, 1 << 21, 3 << 21, (3 << 21) + 5]


def test_vectors_are_what_their_description_says():
    """build() makes the array from the ranges; the model only ever sees the ranges"""
    import numpy as np
    for vec in list(hc.elide_vectors().values()) + list(hc.hidden_vectors(3).values()) + hc.msm_vectors(16) + [hc.split_vector()]:
        a = hc.build(vec)
        nz = a.any(axis=1)
        assert a.shape == (vec.n, 4) and int(nz.sum()) == sum(b - a_ for a_, b in vec.ranges)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], nz.astype(np.int8), [0]])))
        merged = []
        for lo, hi in vec.ranges:
            if merged and merged[-1][1] == lo:
                merged[-1][1] = hi
            else:
                merged.append([lo, hi])
        assert edges.reshape(-1, 2).tolist() == merged


def test_case_names_are_unique_per_option_set():
    for opts in hc.OPTION_SETS:
        names = hc.case_names(*opts)
        assert len(set(names)) == len(names) and len(names) > 30
