#!/usr/bin/env python3
"""Times the permutation and lookup terms of h(X) (trh_quotient_terms_dev, csrc/quotient.hip) at the reference's shape -- k = 18, Fp, 188
equality-enabled columns in sets of 4, 31 lookups, 5 of 8 coset blocks -- against what the library could do before it: the same terms
compiled as an `Expression` program for the stack machine (trh_expr_eval_blocks_dev), with X as one more resident column.
    tools/quotient_probe.py [--k 18] [--out profiles/quotient_probe.txt]
The two outputs are compared bit for bit first; then five alternating calls of each, after a warm-up, timed with device events.  Bytes:
what each path queries (32 B per column read and row; a rotated query of a column already read counts again) and the distinct columns
behind that, both computed from the shape; the share of HBM peak is distinct bytes / time over 8 TB/s."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
N_COLUMNS, CHUNK, N_LOOKUPS, BLINDING, J, N_BLOCKS = 188, 4, 31, 5, 6, 5
BETA, GAMMA, Y = 0xBE7A ** 9, 0x6A33A ** 9, 0x5EED ** 9


def argument_terms(field, n_columns, chunk, n_lookups, blinding, beta, gamma):
    """the terms as Expressions over advice columns in the entry's order (values, sigmas, product columns, lookups x 5, l0, l_blind, l_last)
    plus X as the last column"""
    from tiny_ram_halo2_amd import expr, permutation
    from tiny_ram_halo2_amd.poly import _MODULUS
    m, delta = _MODULUS[field], permutation.delta(field)
    n_sets = -(-n_columns // chunk)
    A = expr.Advice
    v0, s0, z0, k0 = 0, n_columns, 2 * n_columns, 2 * n_columns + n_sets
    f0 = k0 + 5 * n_lookups
    l0, l_blind, l_last, X = A(f0), A(f0 + 1), A(f0 + 2), A(f0 + 3)
    active = 1 - (l_last + l_blind)
    terms = []
    if n_sets:
        terms.append(l0 * (1 - A(z0)))
        zl = A(z0 + n_sets - 1)
        terms.append(l_last * (zl * zl - zl))
        for s in range(1, n_sets):
            terms.append(l0 * (A(z0 + s) - A(z0 + s - 1, -(blinding + 1))))
        for s in range(n_sets):
            left, right = A(z0 + s, 1), A(z0 + s)
            for j in range(s * chunk, min((s + 1) * chunk, n_columns)):
                left = left * (A(v0 + j) + A(s0 + j) * beta + gamma)
                right = right * (A(v0 + j) + X * (beta * pow(delta, j, m) % m) + gamma)
            terms.append(active * (left - right))
    for i in range(n_lookups):
        a, s_, ap, sp, z = (k0 + 5 * i + c for c in range(5))
        terms.append(l0 * (1 - A(z)))
        terms.append(l_last * (A(z) * A(z) - A(z)))
        terms.append(active * (A(z, 1) * (A(ap) + beta) * (A(sp) + gamma) - A(z) * (A(a) + beta) * (A(s_) + gamma)))
        terms.append(l0 * (A(ap) - A(sp)))
        terms.append(active * ((A(ap) - A(sp)) * (A(ap) - A(ap, -1))))
    return terms, f0 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quotient_probe.txt"))
    a = ap.parse_args()
    import torch
    from tiny_ram_halo2_amd import api, expr, quotient
    from tiny_ram_halo2_amd.poly import _MODULUS, EvaluationDomain
    field, k = "fp", a.k
    m, n = _MODULUS[field], 1 << a.k
    api.init(0)
    dom = EvaluationDomain(field, J, k)
    rows = N_BLOCKS * n
    n_sets = -(-N_COLUMNS // CHUNK)
    n_arg = 2 * N_COLUMNS + n_sets + 5 * N_LOOKUPS
    beta, gamma, y = BETA % m, GAMMA % m, Y % m
    st = torch.cuda.current_stream().cuda_stream

    # the argument columns: random stored words below 2^254 (valid elements of either field); l0 / l_blind / l_last and X as they are
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x9007)
    cols = torch.randint(0, 1 << 62, (n_arg, rows, 4), dtype=torch.int64, device="cuda", generator=gen)
    ls = quotient.lagrange_basis_columns(dom, BLINDING, N_BLOCKS).reshape(3, rows, 4)
    X = torch.empty((N_BLOCKS, n, 4), dtype=torch.int64, device="cuda")
    for r in range(N_BLOCKS):  # block r, row q: zeta extended_omega^r omega^q
        api.powers_dev(field, X[r], n, expr._limbs(field, dom.omega), stream=st)
        api.field_scale_dev(field, X[r], n, expr._limbs(field, dom.g_coset * pow(dom.extended_omega, r, m) % m), stream=st)
    X = X.reshape(rows, 4)

    split = [cols[i] for i in range(n_arg)]
    values, sigmas, zs = split[:N_COLUMNS], split[N_COLUMNS:2 * N_COLUMNS], split[2 * N_COLUMNS:2 * N_COLUMNS + n_sets]
    lookups = [split[2 * N_COLUMNS + n_sets + 5 * i:2 * N_COLUMNS + n_sets + 5 * i + 5] for i in range(N_LOOKUPS)]
    qt = quotient.QuotientTerms(dom, N_COLUMNS, CHUNK, N_LOOKUPS, BLINDING)
    acc = torch.zeros((rows, 4), dtype=torch.int64, device="cuda")

    def dedicated():
        acc.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        qt.eval(acc, values, sigmas, zs, lookups, ls[0], ls[1], ls[2], beta, gamma, y, n_blocks=N_BLOCKS)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    terms, n_prog_columns = argument_terms(field, N_COLUMNS, CHUNK, N_LOOKUPS, BLINDING, beta, gamma)
    prog = expr.compile_gates(field, terms, y=y)
    assert len(prog.columns) == n_prog_columns
    every = split + [ls[0], ls[1], ls[2], X]
    resident = {key: every[key[1]] for key in prog.columns}
    gev = expr.GateEvaluator(prog)
    out = torch.empty((1, rows, 4), dtype=torch.int64, device="cuda")

    def generic():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gev.eval_blocks(resident, k, N_BLOCKS, out=out)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    dedicated(); generic()  # warm-up, and the comparison
    same = bool((acc == out.reshape(rows, 4)).all())
    t_new, t_old = [], []
    for _ in range(5):
        t_new.append(dedicated())
        t_old.append(generic())
    queries_old = int((prog.insns[:, 0] == expr.OP["PUSH_COLUMN"]).sum())
    queries_new = 2 * N_COLUMNS + (2 + 2 * (n_sets - 1) + 2 * n_sets) + 7 * N_LOOKUPS + 3 + 1
    distinct_new, distinct_old = n_arg + 4, n_prog_columns
    col_bytes = rows * 32
    lines = [f"quotient_probe: k = {k}, {field}, {N_COLUMNS} columns / chunk {CHUNK} / {N_LOOKUPS} lookups, {N_BLOCKS} blocks of 2^{k} rows ({rows} rows)",
             f"outputs identical bit for bit: {same}"]
    for name, ts, q, d in (("trh_quotient_terms_dev (csrc/quotient.hip)", t_new, queries_new, distinct_new),
                           (f"Expression program, {len(prog.insns)} instructions, {gev.lds_slots()} LDS slots (trh_expr_eval_blocks_dev)", t_old, queries_old, distinct_old)):
        best, med = min(ts), sorted(ts)[len(ts) // 2]
        lines.append(f"{name}:")
        lines.append("  ms per call: " + " ".join(f"{t:.3f}" for t in ts) + f"   (best {best:.3f}, median {med:.3f})")
        lines.append(f"  column queries {q} = {q * col_bytes / 1e9:.2f} GB; distinct columns {d} = {d * col_bytes / 1e9:.2f} GB read + {col_bytes / 1e9:.3f} GB written")
        lines.append(f"  distinct bytes / median time = {d * col_bytes / (med * 1e-3) / 1e12:.2f} TB/s = {100 * d * col_bytes / (med * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak")
    lines.append(f"generic / dedicated (medians): {sorted(t_old)[2] / sorted(t_new)[2]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
