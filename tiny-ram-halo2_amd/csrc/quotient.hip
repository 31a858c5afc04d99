// The permutation and lookup terms of the quotient's numerator over resident extended columns: what halo2_proofs 0.2.0
// plonk/permutation/prover.rs `Committed::construct` and plonk/lookup/prover.rs `Committed::construct` contribute to h(X) in
// `plonk::create_proof`, folded with the challenge y behind the custom gates (expr.hip).  Recalled from the crate's sources, not
// pinned against the fork the reference builds with.
//
// Per row of the extended domain, every term t folded as acc = acc * y + t, in this order
// (l_active = 1 - (l_last + l_blind), `last` = Rotation(-(blinding_factors + 1)), X the domain point of the row):
//   permutation, n_sets = ceil(n_columns / chunk_len) sets (nothing when n_columns = 0)
//     1  l0 (1 - z_0)
//     2  l_last (z_last^2 - z_last)                                   z_last: the last set's column
//     3  l0 (z_s - z_(s-1)(last))                                     s = 1 .. n_sets - 1
//     4  l_active (z_s(+1) prod_j (v_j + beta sigma_j + gamma) - z_s prod_j (v_j + beta delta^j X + gamma))     s = 0 .. n_sets - 1,
//                                                                     j over the set's columns, delta^j by the global column index
//   every lookup (A, S the compressed input / table, A', S' the permuted columns, z its product column)
//     5  l0 (1 - z)
//     6  l_last (z^2 - z)
//     7  l_active (z(+1) (A' + beta) (S' + gamma) - z (A + beta) (S + gamma))
//     8  l0 (A' - S')
//     9  l_active (A' - S') (A' - A'(-1))
//
// One thread per row, no LDS, no scratch.  Both layouts of expr.hip: the flat one (2^extended_k rows, Rotation(r) = r 2^(extended_k - k)
// rows, cyclic) and coset blocks (n_blocks x 2^k rows, Rotation(r) = row (q + r) mod 2^k of the same block).  In both the row's point is
// X = zeta extended_omega^e -- e the row itself (flat) or r + q 2^(extended_k - k) (block r, row q) -- and comes from three tables of 512
// powers each, kept in the handle: X = T0[e mod 512] T1[(e / 512) mod 512] T2[e / 2^18], T0[i] = zeta w^i, T1[i] = w^(512 i),
// T2[i] = w^(2^18 i) (e < 2^27): two multiplications per row, nothing read from a resident column.  beta delta^j is prepared on the host
// once per call (one constant per column), so the right-hand product costs the same two multiplications per column as the left.
//
// Arithmetic: the signed 29-bit lazy domain of field.h, as in expr.hip (column words read five bits lower = 32 x, constants stored as
// c 2^261 mod m, the result out through fy_to_fe: canonical Montgomery words, bit-exact).  Magnitude bounds, in units of m, against the
// limits trh_expr_create works with (a sum 250, an operand or result of a product 500, a stored value 15); a product of operands
// bounded by a and b is bounded by a b / 128 + 1 (fy_mul: |a b| / 2^261 + m, m / 2^261 < 2^-7):
//   a loaded column          [0, 32)
//   a constant (beta, gamma, y, beta delta^j, a table entry, one)   [0, 1)
//   X                        1/128 + 1, then (1/128 + 1)/128 + 1 < 1.01
//   l_active                 1 - (l_last + l_blind) in (-64, 1): 64
//   the difference of two loaded columns, 1 - z                     32 resp. 33
//   z^2 - z                  32^2/128 + 1 = 9, minus a column: 41
//   terms 1, 5: 32 * 33/128 + 1 = 9.25;  2, 6: 32 * 41/128 + 1 = 11.25;  3, 8: 32 * 32/128 + 1 = 9
//   a factor of term 4       v + beta sigma + gamma: 32 + (32/128 + 1) + 1 = 34.25;  v + (beta delta^j) X + gamma: 32 + (1.01/128 + 1) + 1 < 34.02
//   a running product        from 32 (z): 32 * 34.25/128 + 1 = 9.57, then x -> x * 34.25/128 + 1 falls towards 1.37: never above 9.57,
//                            whatever chunk_len is
//   term 4                   64 * (2 * 9.57)/128 + 1 = 10.57
//   term 7                   32 * 33/128 + 1 = 9.25, * 33/128 + 1 = 3.39 each side; 64 * 6.78/128 + 1 = 4.39
//   term 9                   32 * 32/128 + 1 = 9, 64 * 9/128 + 1 = 5.5
//   acc                      enters as a loaded column (32); acc * y: 32/128 + 1 = 1.25; with the largest term 12.5 after the first fold, and
//                            from then on at most 12.5/128 + 1 + 11.25 < 12.35
// No sum reaches 250, no product 500, and acc is stored from below 15: the kernel holds no reduction of its own.  (With no term at all acc
// would be stored from 32: the entry returns before the launch, acc stays as it is.)
// Sums and differences that feed exactly one multiplication are the limb-wise forms (fy_add_lazy / fy_sub_lazy: limbs below 2^30, the
// other operand normalised); a three-term factor is one carry chain and one limb-wise addition on top (limbs below 2^29 + 2^29).
#include <string.h>

#include <mutex>
#include <vector>

#include "ctx.h"
#include "devmem.h"

namespace trh {
void domain_shape(const trh_domain* d, int* field, u32* j, u32* k, u32* extended_k);  // domain.hip
}

struct trh_quotient {
    int field;
    uint32_t k, extended_k, n_columns, chunk_len, n_sets, n_lookups, blinding_factors;
    void* d_ptrs = nullptr;    // 2 n_columns + n_sets + 5 n_lookups device pointers, refreshed per call
    void* d_consts = nullptr;  // beta, gamma, y, then beta delta^j per column: lazy-domain words, refreshed per call
    void* d_xtab = nullptr;    // 3 x 512 powers of extended_omega (the first table times zeta), lazy-domain words
    std::vector<const void*> h_ptrs;
    std::vector<uint64_t> h_consts;  // the staging copy of d_consts
    std::vector<uint64_t> delta;     // delta^j, canonical Montgomery words
    std::mutex mu;  // a call stages pointers and constants in the handle: one call at a time, whichever context calls
};

namespace trh {
namespace {

constexpr int Q_THREADS = 256;
constexpr u32 XTAB = 512, XTAB_LOG = 9;
constexpr u32 C_BETA = 0, C_GAMMA = 1, C_Y = 2, C_COLUMNS = 3;

struct QuotientArgs {
    const uint4* const* ptrs;  // values[n_columns], sigmas[n_columns], z[n_sets], lookups[n_lookups][5]
    const uint4* consts;
    const uint4* xtab;
    const uint4 *l0, *l_blind, *l_last;
    uint4* acc;
    u32 n_columns, chunk_len, n_sets, n_lookups;
    u32 log_n, rot_step, n_blocks, shift;  // rows of one cyclic domain, rows per Rotation(1), blocks (0: flat), extended_k - k
    i32 last;                              // -(blinding_factors + 1)
};

// column word -> the lazy domain, as expr.hip's ldg_column (kept with its kernel family, devmem.h)
template <class F>
__device__ __forceinline__ Fy<F> q_column(const uint4* p) {
    const uint4 a = p[0], b = p[1];
    const u32 M = (u32)YMASK;
    Fy<F> r;
    r.l[0] = (i32)((a.x << 5) & M);
    r.l[1] = (i32)(((a.x >> 24) | (a.y << 8)) & M);
    r.l[2] = (i32)(((a.y >> 21) | (a.z << 11)) & M);
    r.l[3] = (i32)(((a.z >> 18) | (a.w << 14)) & M);
    r.l[4] = (i32)(((a.w >> 15) | (b.x << 17)) & M);
    r.l[5] = (i32)(((b.x >> 12) | (b.y << 20)) & M);
    r.l[6] = (i32)(((b.y >> 9) | (b.z << 23)) & M);
    r.l[7] = (i32)(((b.z >> 6) | (b.w << 26)) & M);
    r.l[8] = (i32)(b.w >> 3);
    return r;
}

template <class F>
__global__ void __launch_bounds__(Q_THREADS) quotient_terms_kernel(const QuotientArgs a) {
    const size_t N = (size_t)1 << a.log_n, total = a.n_blocks ? (size_t)a.n_blocks << a.log_n : N;
    const size_t gid = (size_t)blockIdx.x * Q_THREADS + threadIdx.x;
    const size_t row = gid < total ? gid : gid & (N - 1);  // surplus lanes of the last workgroup repeat rows, their store is masked
    const bool live = gid < total;
    const size_t row_base = row & ~(N - 1), q = row & (N - 1);
    auto at = [&](const uint4* col, i32 rot) {
        const size_t r = row_base | ((q + (size_t)((long long)rot * (long long)a.rot_step)) & (N - 1));
        return q_column<F>(col + 2 * r);
    };
    const uint4* const* values = a.ptrs;
    const uint4* const* sigmas = values + a.n_columns;
    const uint4* const* zs = sigmas + a.n_columns;
    const uint4* const* lookups = zs + a.n_sets;

    const Fy<F> one = fy_one<F>();
    const Fy<F> beta = load_fy<F>(a.consts + 2 * C_BETA), gamma = load_fy<F>(a.consts + 2 * C_GAMMA), y = load_fy<F>(a.consts + 2 * C_Y);
    const Fy<F> l0 = at(a.l0, 0), l_last = at(a.l_last, 0);
    const Fy<F> l_active = fy_sub(fy_sub(one, l_last), at(a.l_blind, 0));
    Fy<F> acc = at(a.acc, 0);
    auto fold = [&](const Fy<F>& t) { acc = fy_add(fy_mul(acc, y), t); };

    if (a.n_sets) {
        fold(fy_mul(l0, fy_sub_lazy(one, at(zs[0], 0))));
        const Fy<F> z_last = at(zs[a.n_sets - 1], 0);
        fold(fy_mul(l_last, fy_sub_lazy(fy_sqr(z_last), z_last)));
        for (u32 s = 1; s < a.n_sets; ++s) fold(fy_mul(l0, fy_sub_lazy(at(zs[s], 0), at(zs[s - 1], a.last))));
        // X = zeta extended_omega^e
        const size_t e = a.n_blocks ? (row >> a.log_n) + (q << a.shift) : row;
        const Fy<F> X = fy_mul(fy_mul(load_fy<F>(a.xtab + 2 * (e & (XTAB - 1))), load_fy<F>(a.xtab + 2 * (XTAB + ((e >> XTAB_LOG) & (XTAB - 1))))),
                               load_fy<F>(a.xtab + 2 * (2 * XTAB + (e >> (2 * XTAB_LOG)))));
        u32 j = 0;
        for (u32 s = 0; s < a.n_sets; ++s) {
            Fy<F> left = at(zs[s], 1), right = at(zs[s], 0);
            const u32 end = a.n_columns - j < a.chunk_len ? a.n_columns : j + a.chunk_len;
            for (; j < end; ++j) {
                const Fy<F> v = at(values[j], 0);
                left = fy_mul(left, fy_add_lazy(fy_add(v, fy_mul(at(sigmas[j], 0), beta)), gamma));
                right = fy_mul(right, fy_add_lazy(fy_add(v, fy_mul(X, load_fy<F>(a.consts + 2 * (size_t)(C_COLUMNS + j)))), gamma));
            }
            fold(fy_mul(l_active, fy_sub_lazy(left, right)));
        }
    }
    for (u32 i = 0; i < a.n_lookups; ++i) {
        const uint4* const* L = lookups + 5 * (size_t)i;
        const Fy<F> z = at(L[4], 0), Ap = at(L[2], 0), Sp = at(L[3], 0);
        fold(fy_mul(l0, fy_sub_lazy(one, z)));
        fold(fy_mul(l_last, fy_sub_lazy(fy_sqr(z), z)));
        const Fy<F> left = fy_mul(fy_mul(at(L[4], 1), fy_add_lazy(Ap, beta)), fy_add_lazy(Sp, gamma));
        const Fy<F> right = fy_mul(fy_mul(z, fy_add_lazy(at(L[0], 0), beta)), fy_add_lazy(at(L[1], 0), gamma));
        fold(fy_mul(l_active, fy_sub_lazy(left, right)));
        const Fy<F> d = fy_sub(Ap, Sp);
        fold(fy_mul(l0, d));
        fold(fy_mul(l_active, fy_mul(d, fy_sub_lazy(Ap, at(L[2], -1)))));
    }
    if (live) store_fe(a.acc + 2 * row, fy_to_fe(acc));
}

// canonical Montgomery words of c -> the words of 32 c mod m = c 2^261 mod m (what load_fy reads as a constant of the lazy domain)
template <class F>
void to_domain(const Fe<F>& c, uint64_t out[4]) {
    Fe<F> v = c;
    for (int i = 0; i < 5; ++i) v = fe_dbl(v);
    u32 w[8];
    fe_store(v, w);
    memcpy(out, w, 32);
}
// a caller's Montgomery words (below 2^256 < 5 m) -> the canonical element
template <class F>
Fe<F> from_words(const uint64_t in[4]) {
    u64 m[4], v[4];
    for (int i = 0; i < 4; ++i) { m[i] = (u64)F::MOD[2 * i] | ((u64)F::MOD[2 * i + 1] << 32); v[i] = in[i]; }
    auto geq = [&]() { for (int i = 3; i >= 0; --i) { if (v[i] != m[i]) return v[i] > m[i]; } return true; };
    while (geq()) {
        u64 borrow = 0;
        for (int i = 0; i < 4; ++i) {
            const u64 t = v[i] - m[i], b1 = v[i] < m[i] ? 1u : 0u, t2 = t - borrow, b2 = t < borrow ? 1u : 0u;
            v[i] = t2; borrow = b1 | b2;
        }
    }
    u32 w[8];
    memcpy(w, v, 32);
    return fe_load<F>(w);
}

// the three power tables of X and delta^j for j < n_columns
template <class F>
void build_tables(const uint64_t zeta[4], const uint64_t ext_omega[4], uint32_t n_columns, std::vector<uint64_t>& xtab, std::vector<uint64_t>& delta) {
    xtab.resize((size_t)3 * XTAB * 4);
    Fe<F> step = from_words<F>(ext_omega);
    Fe<F> first = from_words<F>(zeta);
    for (int level = 0; level < 3; ++level) {
        Fe<F> cur = first;
        for (u32 i = 0; i < XTAB; ++i) {
            to_domain<F>(cur, xtab.data() + ((size_t)level * XTAB + i) * 4);
            cur = fe_mul(cur, step);
        }
        for (u32 i = 0; i < XTAB_LOG; ++i) step = fe_sqr(step);
        first = fe_one<F>();
    }
    // delta = 5^(2^32) (pasta_curves DELTA, as permutation.hip derives it)
    const Fe<F> one = fe_one<F>();
    Fe<F> d = fe_add(fe_dbl(fe_dbl(one)), one);
    for (int i = 0; i < 32; ++i) d = fe_sqr(d);
    delta.resize((size_t)n_columns * 4);
    Fe<F> cur = one;
    for (uint32_t j = 0; j < n_columns; ++j) {
        u32 w[8];
        fe_store(cur, w);
        memcpy(delta.data() + (size_t)j * 4, w, 32);
        cur = fe_mul(cur, d);
    }
}

}  // namespace
}  // namespace trh

using namespace trh;

extern "C" {

int trh_quotient_create(trh_domain* d, uint32_t n_perm_columns, uint32_t chunk_len, uint32_t n_lookups, uint32_t blinding_factors, trh_quotient** out) {
    TRH_TRY(require_init());
    if (!d || !out) { set_error("quotient_create: null pointer"); return TRH_EINVAL; }
    if (chunk_len == 0) { set_error("quotient_create: chunk_len is 0"); return TRH_EINVAL; }
    int field = 0;
    u32 j = 0, k = 0, ek = 0;
    domain_shape(d, &field, &j, &k, &ek);
    if ((uint64_t)blinding_factors + 2 > ((uint64_t)1 << k)) {
        set_error("quotient_create: blinding_factors %u + 2 rows do not fit the 2^%u rows of the domain", blinding_factors, k);
        return TRH_EINVAL;
    }
    if (n_perm_columns > (1u << 20) || n_lookups > (1u << 20)) { set_error("quotient_create: more than 2^20 columns / lookups"); return TRH_EINVAL; }
    TRH_ENTER(0);
    Range range("trh_quotient_create");
    trh_quotient* h = new trh_quotient();
    h->field = field; h->k = k; h->extended_k = ek;
    h->n_columns = n_perm_columns; h->chunk_len = chunk_len; h->n_sets = (n_perm_columns + chunk_len - 1) / chunk_len;
    h->n_lookups = n_lookups; h->blinding_factors = blinding_factors;
    const size_t n_ptrs = 2 * (size_t)n_perm_columns + h->n_sets + 5 * (size_t)n_lookups;
    h->h_ptrs.resize(n_ptrs ? n_ptrs : 1);
    h->h_consts.resize((C_COLUMNS + (size_t)n_perm_columns) * 4);
    uint64_t zeta[4], ext_omega[4];
    (void)trh_domain_constant(d, 6, zeta);
    (void)trh_domain_constant(d, 2, ext_omega);
    std::vector<uint64_t> xtab;
    with_field(field, [&](auto f) { build_tables<decltype(f)>(zeta, ext_omega, n_perm_columns, xtab, h->delta); });
    hipError_t err = hipMalloc(&h->d_ptrs, h->h_ptrs.size() * sizeof(void*));
    if (err == hipSuccess) err = hipMalloc(&h->d_consts, h->h_consts.size() * 8);
    if (err == hipSuccess) err = hipMalloc(&h->d_xtab, xtab.size() * 8);
    if (err == hipSuccess) err = hipMemcpy(h->d_xtab, xtab.data(), xtab.size() * 8, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        set_error("quotient_create: %s", hipGetErrorString(err));
        trh_quotient_destroy(h);
        return TRH_EHIP;
    }
    *out = h;
    return TRH_OK;
}

void trh_quotient_destroy(trh_quotient* h) {
    if (!h) return;
    if (h->d_ptrs) (void)hipFree(h->d_ptrs);
    if (h->d_consts) (void)hipFree(h->d_consts);
    if (h->d_xtab) (void)hipFree(h->d_xtab);
    delete h;
}

int trh_quotient_terms_dev(trh_quotient* h, const trh_quotient_args_t* args) {
    TRH_TRY(require_init());
    if (!h || !args) { set_error("quotient_terms: null pointer"); return TRH_EINVAL; }
    const uint32_t max_blocks = 1u << (h->extended_k - h->k);
    if (args->n_blocks > max_blocks) { set_error("quotient_terms: %u blocks, the extended domain has %u", args->n_blocks, max_blocks); return TRH_EINVAL; }
    if (h->n_columns && (!args->perm_values || !args->perm_sigmas || !args->perm_z)) { set_error("quotient_terms: null permutation array"); return TRH_EINVAL; }
    if (h->n_lookups && !args->lookups) { set_error("quotient_terms: null lookup array"); return TRH_EINVAL; }
    if (!args->acc || !args->l0 || !args->l_blind || !args->l_last) { set_error("quotient_terms: null acc / l0 / l_blind / l_last"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(h->mu);
    size_t n = 0;
    for (uint32_t i = 0; i < h->n_columns; ++i) h->h_ptrs[n++] = args->perm_values[i];
    for (uint32_t i = 0; i < h->n_columns; ++i) h->h_ptrs[n++] = args->perm_sigmas[i];
    for (uint32_t i = 0; i < h->n_sets; ++i) h->h_ptrs[n++] = args->perm_z[i];
    for (size_t i = 0; i < 5 * (size_t)h->n_lookups; ++i) h->h_ptrs[n++] = args->lookups[i];
    const void* fixed[3] = {args->l0, args->l_blind, args->l_last};
    for (size_t i = 0; i < n + 3; ++i) {
        const void* p = i < n ? h->h_ptrs[i] : fixed[i - n];
        if (!p) { set_error("quotient_terms: input column %zu is null", i); return TRH_EINVAL; }
        if (((uintptr_t)p & 15) != 0) { set_error("quotient_terms: input column %zu: elements must be 16-byte aligned", i); return TRH_EINVAL; }
        if (p == args->acc) { set_error("quotient_terms: acc is also input column %zu (a rotated read would see rows already folded)", i); return TRH_EINVAL; }
    }
    if (((uintptr_t)args->acc & 15) != 0) { set_error("quotient_terms: acc must be 16-byte aligned"); return TRH_EINVAL; }
    if (n == 0) return TRH_OK;  // no term: acc stays as it is
    // beta, gamma, y and beta delta^j in the lazy domain's form
    with_field(h->field, [&](auto f) {
        typedef decltype(f) F;
        const Fe<F> beta = from_words<F>(args->beta);
        to_domain<F>(beta, h->h_consts.data() + 4 * C_BETA);
        to_domain<F>(from_words<F>(args->gamma), h->h_consts.data() + 4 * C_GAMMA);
        to_domain<F>(from_words<F>(args->y), h->h_consts.data() + 4 * C_Y);
        for (uint32_t j = 0; j < h->n_columns; ++j) {
            u32 w[8];
            memcpy(w, h->delta.data() + 4 * (size_t)j, 32);
            to_domain<F>(fe_mul(beta, fe_load<F>(w)), h->h_consts.data() + 4 * (size_t)(C_COLUMNS + j));
        }
    });
    TRH_ENTER(args->stream);
    Range range("trh_quotient_terms_dev");
    hipStream_t s = (hipStream_t)args->stream;
    TRH_HIP_TRY(hipMemcpyAsync(h->d_ptrs, h->h_ptrs.data(), n * sizeof(void*), hipMemcpyHostToDevice, s));
    TRH_HIP_TRY(hipMemcpyAsync(h->d_consts, h->h_consts.data(), h->h_consts.size() * 8, hipMemcpyHostToDevice, s));
    QuotientArgs a;
    a.ptrs = (const uint4* const*)h->d_ptrs; a.consts = (const uint4*)h->d_consts; a.xtab = (const uint4*)h->d_xtab;
    a.l0 = (const uint4*)args->l0; a.l_blind = (const uint4*)args->l_blind; a.l_last = (const uint4*)args->l_last; a.acc = (uint4*)args->acc;
    a.n_columns = h->n_columns; a.chunk_len = h->chunk_len; a.n_sets = h->n_sets; a.n_lookups = h->n_lookups;
    a.shift = h->extended_k - h->k; a.n_blocks = args->n_blocks;
    a.log_n = args->n_blocks ? h->k : h->extended_k;
    a.rot_step = args->n_blocks ? 1u : 1u << a.shift;
    a.last = -(i32)(h->blinding_factors + 1);
    const size_t rows = args->n_blocks ? (size_t)args->n_blocks << h->k : (size_t)1 << h->extended_k;
    const unsigned blocks = (unsigned)((rows + Q_THREADS - 1) / Q_THREADS);
    with_field(h->field, [&](auto f) { hipLaunchKernelGGL((quotient_terms_kernel<decltype(f)>), dim3(blocks), dim3(Q_THREADS), 0, s, a); });
    TRH_HIP_TRY(hipGetLastError());
    TRH_HIP_TRY(hipStreamSynchronize(s));  // the staging copies in the handle are reused by the next call
    return TRH_OK;
}

}  // extern "C"
