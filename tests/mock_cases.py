"""Inputs of the lookup check (trh_lookup_check_dev / csrc/tuplehash.h) and their expected verdicts, shared by tests/test_mock_host.py (the
set built sequentially on the host by tests/native/tuplehash_test.cpp) and tests/test_gpu_mock.py (the device kernels): both must answer
these very inputs alike, and both must stay within the probe cap on them.

An element is four u64 words compared as they are, so the cases write stored words directly: element(v, top) = words (v, 0, 0, top << 32),
which is below both moduli for top < 2^30.  Expected verdicts come from a Python set of tuples, never from the code under test."""
import numpy as np

SIZES = (1, 63, 64, 65, (1 << 10) - 6)                  # usable_rows: one row; below, at and above one wave; several workgroups with a masked last wave
PADDED = (1 << 16) + 3                                  # and the padded table ("same") at a size where a chain of duplicates would show
TABLES = ("range", "same", "topword")
EXTRA = 6                                               # rows behind usable_rows: a table tuple that only lives there, garbage inputs
PROBE_CAP = 4                                           # slots visited <= PROBE_CAP * (table rows + input rows): a condition, not a measurement --
                                                        # Knuth, linear probing at load 1/2: 2.5 expected probes per unsuccessful search, 1.5 per hit


def sizes(kind: str):
    return SIZES + (PADDED,) if kind == "same" else SIZES


def elements(values, tops=None):
    """-> (len, 4) uint64 stored words"""
    values = np.asarray(values, dtype=np.uint64)
    out = np.zeros((values.shape[0], 4), dtype=np.uint64)
    out[:, 0] = values
    if tops is not None:
        out[:, 3] = np.asarray(tops, dtype=np.uint64) << np.uint64(32)
    return out


def table_columns(kind: str, width: int, usable: int) -> np.ndarray:
    """(width, usable + EXTRA, 4): the table.  Rows behind `usable` hold tuples that no usable row holds"""
    rows = usable + EXTRA
    t = np.arange(rows, dtype=np.uint64)
    behind = t >= usable
    cols = []
    for j in range(width):
        if kind == "range":       # row t = (t, t + K, t + 2 K, ..): no two rows share a column value, so mixing two rows leaves the table
            col = elements(t + np.uint64(j * 1000003))
        elif kind == "same":      # a padded table: every usable row is the same tuple
            col = elements(np.where(behind, t + np.uint64(1000), np.uint64(7 + j)))
        elif kind == "topword":   # rows differ only in the top word of the last column
            last = j == width - 1
            col = elements(np.full(rows, 5 + j, dtype=np.uint64), tops=t + np.uint64(1) if last else None)
        else:
            raise ValueError(kind)
        cols.append(col)
    return np.stack(cols)


def lookup_case(kind: str, width: int, usable: int, bad: bool):
    """-> (inputs, tables): two (width, usable + EXTRA, 4) uint64 arrays.  Every usable input row repeats some usable table row; with
    bad=True misses are planted: at row 0 and at row usable - 1 (a value that is in no table row), and -- where the shape has room -- a tuple
    that mixes the columns of two table rows, a table tuple with its first two columns swapped, and a tuple that only table rows behind
    usable_rows hold.  The input rows behind usable_rows are garbage in either variant"""
    tables = table_columns(kind, width, usable)
    rows = usable + EXTRA
    pick = (np.arange(rows, dtype=np.int64) * 7 + 3) % usable
    inputs = tables[:, pick, :].copy()
    inputs[:, usable:, :] = elements(np.arange(EXTRA, dtype=np.uint64) + np.uint64(0xDEAD0000), tops=np.full(EXTRA, 77))   # garbage, never read
    if bad:
        miss = elements([0xBAD0BAD], tops=[123])[0]
        inputs[0, 0] = miss
        inputs[width - 1, usable - 1] = miss
        if usable >= 63:
            inputs[:, 20, :] = tables[:, usable + 2, :]                  # present only behind usable_rows
            if width >= 2 and kind == "range":
                inputs[:, 30, :] = tables[:, 11, :]
                inputs[1, 30] = tables[1, 12]                            # columns of two different rows
                inputs[:, 40, :] = tables[:, 13, :]
                inputs[0, 40], inputs[1, 40] = tables[1, 13].copy(), tables[0, 13].copy()   # two columns swapped
    return inputs, tables


def row_tuples(cols: np.ndarray, rows: int):
    """the first `rows` rows of (width, n, 4) columns as tuples of 4 * width ints"""
    return [tuple(r) for r in np.ascontiguousarray(cols[:, :rows, :].transpose(1, 0, 2)).reshape(rows, -1).tolist()]


def lookup_model(inputs: np.ndarray, tables: np.ndarray, usable: int):
    """-> (n_bad, first_bad_row, bitmap words as uint64): membership in a Python set of the usable table rows' tuples"""
    table = set(row_tuples(tables, usable))
    bad = [r for r, t in enumerate(row_tuples(inputs, usable)) if t not in table]
    words = np.zeros((usable + 63) // 64, dtype=np.uint64)
    for r in bad:
        words[r // 64] |= np.uint64(1) << np.uint64(r % 64)
    return len(bad), (bad[0] if bad else usable), words


def bitmap_hex(words) -> str:
    return "".join(f"{int(w):016x}" for w in np.asarray(words).reshape(-1).view(np.uint64))
