// Permutation keygen on the device: trh_perm_* (include/trh.h) over csrc/permkeygen.h.
// halo2_proofs 0.2.0 plonk/permutation/keygen.rs builds, on the host, a table deltaomega[c][r] = delta^c omega^r for every equality-enabled column
// (1.5 GB at the reference's 188 columns x 2^18 rows) and gathers sigma[c][r] = deltaomega[mapping[c][r]] from it.  Here the assembly (the
// copies, the mapping) stays on the host, where the circuit's synthesis calls it cell by cell, and the columns are made where the proving key
// lives: the mapping goes up once as one u32 per cell, the two factors come from an n-element table of omega^r and an n_columns-element
// table of delta^c, and every cell costs one Montgomery product, one 32-byte gather and one 32-byte store.
// perm_check_kernel answers what MockProver::verify asks of the permutation: is value[cell] == value[mapping[cell]] for every cell.
// The handle is host memory like trh_rng_t; its device copy of the mapping is kept per context and dropped by the next copy().
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "ctx.h"
#include "devmem.h"
#include "permkeygen.h"
#include "verdict.h"

struct trh_perm_s {
    std::mutex mu;  // guards the assembly and the device copies; taken INSIDE a context's lock by the device entries
    trh::PermAssembly a;
    struct DevCopy {
        trh::Ctx* ctx;  // the context whose calls the copy is ordered with
        int device;
        void* d_mapping;  // cells x u32
        bool valid;
    };
    std::vector<DevCopy> dev;
};

namespace trh {
namespace {

constexpr unsigned PERM_BLOCK = 256;

// sigma[i] = delta^(m >> k) omega^(m & (n - 1)), m = mapping[first_cell + i], i < count_cells.  delta_tab covers ALL columns: a cell of the
// window may map to any column.
template <class F>
__global__ void __launch_bounds__(PERM_BLOCK) perm_sigma_kernel(const u32* __restrict__ mapping, size_t first_cell, size_t count_cells, u32 k,
                                                                const uint4* __restrict__ omega_tab, const uint4* __restrict__ delta_tab, uint4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count_cells) return;
    const u32 m = mapping[first_cell + i];
    const u32 col = m >> k, row = m & (((u32)1 << k) - 1u);
    store_fe(out + 2 * i, fe_mul(load_fe<F>(delta_tab + 2 * (size_t)col), load_fe<F>(omega_tab + 2 * (size_t)row)));
}

// *n_bad += cells with value[cell] != value[mapping[cell]], *first_bad = min(*first_bad, smallest such cell).  Columns hold canonical stored
// forms, so the eight words are compared as they are.  Lanes hold consecutive cells, so the kernel ends in verdict.h's ballot tail.
__global__ void __launch_bounds__(PERM_BLOCK) perm_check_kernel(const u32* __restrict__ mapping, size_t cells, u32 k, const uint4* const* __restrict__ columns,
                                                                unsigned long long* __restrict__ n_bad, unsigned long long* __restrict__ first_bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < cells) {
        const u32 mask = ((u32)1 << k) - 1u;
        const u32 m = mapping[i];
        const uint4* a = columns[i >> k] + 2 * (size_t)((u32)i & mask);
        const uint4* b = columns[m >> k] + 2 * (size_t)(m & mask);
        const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
        bad = ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w)) != 0;
    }
    wave_verdict(bad, i, n_bad, first_bad);
}

int perm_grid(const char* who, size_t cells, unsigned* blocks) {
    const size_t b = (cells + PERM_BLOCK - 1) / PERM_BLOCK;
    if (b > 0x7fffffffu) { set_error("%s: %zu cells exceed one launch", who, cells); return TRH_EINVAL; }
    *blocks = (unsigned)b;
    return TRH_OK;
}

// The calling context's device copy of the mapping, uploaded if the context has none or a copy() came since (p->mu held).  The upload is
// complete when this returns: the host arrays may change under the next copy() while kernels read the device copy.
int perm_device_mapping(trh_perm_s* p, hipStream_t s, const u32** out) {
    Ctx& c = ctx();
    trh_perm_s::DevCopy* e = nullptr;
    for (auto& d : p->dev) if (d.ctx == &c && d.device == c.device) e = &d;
    if (!e) {
        try { p->dev.push_back({&c, c.device, nullptr, false}); } catch (const std::bad_alloc&) { set_error("perm: out of memory"); return TRH_ENOMEM; }
        e = &p->dev.back();
    }
    const size_t bytes = p->a.cells * sizeof(u32);
    if (!e->d_mapping) {
        hipError_t err = hipMalloc(&e->d_mapping, bytes);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            pool_trim();
            err = hipMalloc(&e->d_mapping, bytes);
        }
        if (err != hipSuccess) { (void)hipGetLastError(); e->d_mapping = nullptr; set_error("perm: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err)); return TRH_ENOMEM; }
        e->valid = false;
    }
    if (!e->valid) {
        TRH_HIP_TRY(hipMemcpyAsync(e->d_mapping, p->a.mapping.data(), bytes, hipMemcpyHostToDevice, s));
        TRH_HIP_TRY(hipStreamSynchronize(s));
        e->valid = true;
    }
    *out = (const u32*)e->d_mapping;
    return TRH_OK;
}

// omega = ROOT_OF_UNITY^(2^(S - k)), the 2^k-th root EvaluationDomain uses; delta = 5^(2^S) (pasta_curves DELTA), S = 32
template <class F>
void perm_constants(u32 k, u64 omega[4], u64 delta[4]) {
    Fe<F> w = fe_load<F>(F::ROOT_OF_UNITY);
    for (u32 i = k; i < 32; ++i) w = fe_sqr(w);
    const Fe<F> one = fe_one<F>();
    Fe<F> d = fe_add(fe_dbl(fe_dbl(one)), one);
    for (int i = 0; i < 32; ++i) d = fe_sqr(d);
    u32 buf[8];
    fe_store(w, buf); memcpy(omega, buf, 32);
    fe_store(d, buf); memcpy(delta, buf, 32);
}

}  // namespace
}  // namespace trh

using namespace trh;

extern "C" {

int trh_perm_create(uint32_t n_columns, uint32_t k, trh_perm_t* out) {
    if (!out) { set_error("perm_create: null pointer"); return TRH_EINVAL; }
    if (!PermAssembly::shape_ok(n_columns, k)) {
        set_error("perm_create: %u columns of 2^%u rows: need n_columns >= 1, k <= 27 and n_columns * 2^k <= 2^32 (a cell is one u32)", n_columns, k);
        return TRH_EINVAL;
    }
    trh_perm_s* p = new (std::nothrow) trh_perm_s;
    if (!p) { set_error("perm_create: out of memory"); return TRH_ENOMEM; }
    const int rc = p->a.init(n_columns, k);
    if (rc != TRH_OK) {
        delete p;
        set_error("perm_create: out of memory (%u columns of 2^%u rows)", n_columns, k);
        return rc;
    }
    *out = p;
    return TRH_OK;
}

void trh_perm_destroy(trh_perm_t p) {
    if (!p) return;
    for (auto& d : p->dev) {
        if (!d.d_mapping) continue;
        int prev = -1;
        (void)hipGetDevice(&prev);
        if (prev != d.device) (void)hipSetDevice(d.device);
        (void)hipFree(d.d_mapping);  // waits for the kernels that still read it
        if (prev >= 0 && prev != d.device) (void)hipSetDevice(prev);
    }
    delete p;
}

int trh_perm_copy(trh_perm_t p, uint32_t left_column, uint32_t left_row, uint32_t right_column, uint32_t right_row) {
    if (!p) { set_error("perm_copy: null handle"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->a.copy(left_column, left_row, right_column, right_row) != TRH_OK) {
        set_error("perm_copy: cell (%u, %u) or (%u, %u) is outside %u columns of %zu rows", left_column, left_row, right_column, right_row, p->a.n_columns, p->a.n);
        return TRH_EINVAL;
    }
    for (auto& d : p->dev) d.valid = false;
    return TRH_OK;
}

int trh_perm_copy_batch(trh_perm_t p, const uint32_t* quads, size_t count) {
    if (!p || (count && !quads)) { set_error("perm_copy_batch: null pointer"); return TRH_EINVAL; }
    if (!count) return TRH_OK;
    std::lock_guard<std::mutex> lk(p->mu);
    for (auto& d : p->dev) d.valid = false;
    for (size_t i = 0; i < count; ++i) {
        const uint32_t* q = quads + 4 * i;
        if (p->a.copy(q[0], q[1], q[2], q[3]) != TRH_OK) {
            set_error("perm_copy_batch: copy %zu: cell (%u, %u) or (%u, %u) is outside %u columns of %zu rows (the copies before it were made)", i, q[0], q[1], q[2], q[3],
                      p->a.n_columns, p->a.n);
            return TRH_EINVAL;
        }
    }
    return TRH_OK;
}

int trh_perm_mapping(trh_perm_t p, uint32_t first_column, uint32_t count, uint32_t* out_cells) {
    if (!p) { set_error("perm_mapping: null handle"); return TRH_EINVAL; }
    if (first_column > p->a.n_columns || count > p->a.n_columns - first_column) {
        set_error("perm_mapping: columns [%u, %u + %u) of %u", first_column, first_column, count, p->a.n_columns);
        return TRH_EINVAL;
    }
    if (!count) return TRH_OK;
    if (!out_cells) { set_error("perm_mapping: null pointer"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(p->mu);
    memcpy(out_cells, p->a.mapping.data() + ((size_t)first_column << p->a.k), ((size_t)count << p->a.k) * sizeof(uint32_t));
    return TRH_OK;
}

int trh_perm_sigma_dev(trh_perm_t p, int field, uint32_t first_column, uint32_t count, void* out_dev, void* stream) {
    if (!p) { set_error("perm_sigma_dev: null handle"); return TRH_EINVAL; }
    TRH_TRY(require_init());
    TRH_TRY(check_field(field));
    if (first_column > p->a.n_columns || count > p->a.n_columns - first_column) {
        set_error("perm_sigma_dev: columns [%u, %u + %u) of %u", first_column, first_column, count, p->a.n_columns);
        return TRH_EINVAL;
    }
    if (count && !out_dev) { set_error("perm_sigma_dev: null pointer"); return TRH_EINVAL; }
    if (((uintptr_t)out_dev & 15) != 0) { set_error("perm_sigma_dev: elements must be 16-byte aligned"); return TRH_EINVAL; }
    if (!count) return TRH_OK;
    TRH_ENTER(stream);
    Range range("trh_perm_sigma_dev");
    Ctx& c = ctx();
    const hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(p->mu);
    const PermAssembly& a = p->a;
    const size_t count_cells = (size_t)count << a.k;
    unsigned blocks = 0;
    TRH_TRY(perm_grid("perm_sigma_dev", count_cells, &blocks));
    const u32* d_mapping = nullptr;
    TRH_TRY(perm_device_mapping(p, s, &d_mapping));
    // omega^r, r < n, then delta^c, c < n_columns, in the context's scan scratch (ordered with every other user by the context's stream order)
    TRH_TRY(c.scan.ensure((a.n + (size_t)a.n_columns) * 32));
    uint4* omega_tab = c.scan.as<uint4>();
    uint4* delta_tab = omega_tab + 2 * a.n;
    u64 omega[4], delta[4];
    with_field(field, [&](auto f) { perm_constants<decltype(f)>(a.k, omega, delta); });
    TRH_TRY(field_powers_device(field, omega_tab, a.n, omega, s));
    TRH_TRY(field_powers_device(field, delta_tab, a.n_columns, delta, s));
    with_field(field, [&](auto f) {
        hipLaunchKernelGGL((perm_sigma_kernel<decltype(f)>), dim3(blocks), dim3(PERM_BLOCK), 0, s, d_mapping, (size_t)first_column << a.k, count_cells, (u32)a.k,
                           (const uint4*)omega_tab, (const uint4*)delta_tab, (uint4*)out_dev);
    });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

int trh_perm_check_dev(trh_perm_t p, int field, const void* const* columns_dev, uint64_t* n_bad, uint64_t* first_bad_cell, void* stream) {
    if (!p) { set_error("perm_check_dev: null handle"); return TRH_EINVAL; }
    TRH_TRY(require_init());
    TRH_TRY(check_field(field));  // both fields store an element in the same eight words: the id only has to be a known one
    if (!columns_dev || !n_bad || !first_bad_cell) { set_error("perm_check_dev: null pointer"); return TRH_EINVAL; }
    for (uint32_t j = 0; j < p->a.n_columns; ++j) {
        if (!columns_dev[j]) { set_error("perm_check_dev: column %u is a null pointer", j); return TRH_EINVAL; }
        if (((uintptr_t)columns_dev[j] & 15) != 0) { set_error("perm_check_dev: column %u: elements must be 16-byte aligned", j); return TRH_EINVAL; }
    }
    TRH_ENTER(stream);
    Range range("trh_perm_check_dev");
    Ctx& c = ctx();
    const hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(p->mu);
    const PermAssembly& a = p->a;
    unsigned blocks = 0;
    TRH_TRY(perm_grid("perm_check_dev", a.cells, &blocks));
    const u32* d_mapping = nullptr;
    TRH_TRY(perm_device_mapping(p, s, &d_mapping));
    // scratch: the column pointers
    const size_t ptr_bytes = (size_t)a.n_columns * sizeof(void*);
    TRH_TRY(c.scan.ensure(ptr_bytes));
    const uint4** d_columns = c.scan.as<const uint4*>();
    unsigned long long *d_sum, *d_min;
    TRH_TRY(verdict_begin(c, 1, 1, s, &d_sum, &d_min));
    TRH_HIP_TRY(hipMemcpyAsync(d_columns, columns_dev, ptr_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(perm_check_kernel, dim3(blocks), dim3(PERM_BLOCK), 0, s, d_mapping, a.cells, (u32)a.k, (const uint4* const*)d_columns, d_sum, d_min);
    TRH_HIP_TRY(hipGetLastError());
    const u64 *sum, *min;
    TRH_TRY(verdict_read(c, s, &sum, &min));  // the synchronisation: the caller's pointer array has been read by now
    *n_bad = sum[0];
    *first_bad_cell = min_or(min[0], a.cells);
    return TRH_OK;
}

}  // extern "C"
