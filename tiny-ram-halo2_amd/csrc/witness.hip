// Packed witness intake: trh_columns_from_ints_*, trh_even_odd_split_dev and trh_even_bits_table_dev (include/trh.h) over csrc/witness.h.
// What they serve: the witness was the one thing that still reached the device at 32 bytes per cell, although every instance and advice
// column of the reference's circuit is a flag, a machine word or an even-bits half of one (replay.column_classes).  Here the host hands
// over bitmaps and words and the device expands them: one lane per element -- one load of 1 .. 8 bytes (none behind the live rows), at most
// one multiplication by R^2, two 16-byte stores, so a wave writes 2 KiB in one piece.  A store-bound pass: no LDS, no scratch memory, no
// cross-lane work.  blockIdx.y walks the columns and blockIdx.x the rows, both with a stride, so no lane divides.
#include <type_traits>

#include "ctx.h"
#include "devmem.h"
#include "witness.h"

namespace trh {
namespace {

constexpr unsigned WIT_BLOCK = 256;
// a memory-bound pass: about 16 workgroups per compute unit and strides for the rest.  blockIdx.x covers at most 2^19 rows of a column per
// pass (longer columns take further passes), blockIdx.y as many columns as keep the grid near WIT_GRID_BLOCKS
constexpr unsigned WIT_GRID_X = 2048;
constexpr unsigned WIT_GRID_BLOCKS = 4096;
// trh_columns_from_ints_host stages whole columns, as many as fit this many bytes (one column if a single one is larger): its scratch
// is max(WIT_STAGE_BYTES, one packed column) -- at most a quarter of the destination it fills
constexpr size_t WIT_STAGE_BYTES = (size_t)64 << 20;

template <class F, class T>
__device__ __forceinline__ Fe<F> fe_from_int(T v) {
    if constexpr (std::is_signed<T>::value) return fe_from_i64<F>((i64)v);
    else return fe_from_u64<F>((u64)v);
}

// dst[c][r] = src[c * stride + r] for r < live, zero for live <= r < n
template <class F, class T>
__global__ void __launch_bounds__(WIT_BLOCK) columns_from_ints_kernel(const T* __restrict__ src, size_t stride, size_t n_cols, size_t live, uint4* __restrict__ dst, size_t n) {
    for (size_t c = blockIdx.y; c < n_cols; c += gridDim.y) {
        const T* col = src + c * stride;
        uint4* out = dst + 2 * c * n;
        for (size_t r = (size_t)blockIdx.x * WIT_BLOCK + threadIdx.x; r < n; r += (size_t)gridDim.x * WIT_BLOCK) {
            if (r < live) store_fe(out + 2 * r, fe_from_int<F, T>(col[r]));
            else store_zero(out + 2 * r);
        }
    }
}

// dst[c][r] = bit (r & 31) of src[c * stride + (r >> 5)] for r < live: R mod m or zero, no multiplication
template <class F>
__global__ void __launch_bounds__(WIT_BLOCK) columns_from_bits_kernel(const u32* __restrict__ src, size_t stride, size_t n_cols, size_t live, uint4* __restrict__ dst, size_t n) {
    u32 one[8];
    fe_store(fe_one<F>(), one);
    for (size_t c = blockIdx.y; c < n_cols; c += gridDim.y) {
        const u32* col = src + c * stride;
        uint4* out = dst + 2 * c * n;
        for (size_t r = (size_t)blockIdx.x * WIT_BLOCK + threadIdx.x; r < n; r += (size_t)gridDim.x * WIT_BLOCK) {
            u32 mask = 0;
            if (r < live) mask = 0u - ((col[r >> 5] >> (r & 31)) & 1u);
            out[2 * r] = make_uint4(one[0] & mask, one[1] & mask, one[2] & mask, one[3] & mask);
            out[2 * r + 1] = make_uint4(one[4] & mask, one[5] & mask, one[6] & mask, one[7] & mask);
        }
    }
}

// even[c][r] = even_part(w), odd[c][r] = odd_part(w), w = src[c * stride + r] for r < live; zero behind
template <class F, class T>
__global__ void __launch_bounds__(WIT_BLOCK) even_odd_split_kernel(const T* __restrict__ src, size_t stride, size_t n_cols, size_t live, uint4* __restrict__ even,
                                                                   uint4* __restrict__ odd, size_t n) {
    for (size_t c = blockIdx.y; c < n_cols; c += gridDim.y) {
        const T* col = src + c * stride;
        uint4* out_e = even + 2 * c * n;
        uint4* out_o = odd + 2 * c * n;
        for (size_t r = (size_t)blockIdx.x * WIT_BLOCK + threadIdx.x; r < n; r += (size_t)gridDim.x * WIT_BLOCK) {
            if (r < live) {
                const u64 w = (u64)col[r];
                store_fe(out_e + 2 * r, fe_from_u64<F>(even_part(w)));
                store_fe(out_o + 2 * r, fe_from_u64<F>(odd_part(w)));
            } else {
                store_zero(out_e + 2 * r);
                store_zero(out_o + 2 * r);
            }
        }
    }
}

// dst[i] = spread_bits(i) for i < entries (<= 2^32), zero for entries <= i < n
template <class F>
__global__ void __launch_bounds__(WIT_BLOCK) even_bits_table_kernel(uint4* __restrict__ dst, size_t entries, size_t n) {
    for (size_t r = (size_t)blockIdx.x * WIT_BLOCK + threadIdx.x; r < n; r += (size_t)gridDim.x * WIT_BLOCK) {
        if (r < entries) store_fe(dst + 2 * r, fe_from_u64<F>(spread_bits((u32)r)));
        else store_zero(dst + 2 * r);
    }
}

dim3 wit_grid(size_t n_cols, size_t n) {
    const size_t blocks = (n + WIT_BLOCK - 1) / WIT_BLOCK;
    const unsigned bx = (unsigned)(blocks < WIT_GRID_X ? blocks : WIT_GRID_X), by = WIT_GRID_BLOCKS / bx;
    return dim3(bx, (unsigned)(n_cols < by ? n_cols : by));
}

// bytes of one source element (BITS: of one bitmap word); 0 for an unknown kind
size_t int_kind_size(int kind) {
    switch (kind) {
        case TRH_INT_BITS: case TRH_INT_U32: case TRH_INT_I32: return 4;
        case TRH_INT_U8: return 1;
        case TRH_INT_U16: return 2;
        case TRH_INT_U64: case TRH_INT_I64: return 8;
        default: return 0;
    }
}
// source elements one column's live rows take
size_t int_kind_elems(int kind, size_t live) { return kind == TRH_INT_BITS ? live / 32 + (live % 32 != 0) : live; }

// every refusal of the three array entries, before anything is entered or written
int check_ints(const char* who, int field, const trh_ints_args_t* a, bool split) {
    if (!a) { set_error("%s: null arguments", who); return TRH_EINVAL; }
    TRH_TRY(check_field(field));
    const size_t esz = int_kind_size(a->kind);
    if (!esz) { set_error("%s: unknown kind %d", who, a->kind); return TRH_EINVAL; }
    if (split && (a->kind < TRH_INT_U8 || a->kind > TRH_INT_U64)) { set_error("%s: kind %d is not an unsigned word (TRH_INT_U8 .. TRH_INT_U64)", who, a->kind); return TRH_EINVAL; }
    if (a->live_rows > a->n) { set_error("%s: %zu live rows in columns of %zu", who, a->live_rows, a->n); return TRH_EINVAL; }
    const size_t need = int_kind_elems(a->kind, a->live_rows);
    if (a->src_stride < need) { set_error("%s: a stride of %zu elements is too small for %zu live rows (%zu elements)", who, a->src_stride, a->live_rows, need); return TRH_EINVAL; }
    const size_t lim = (size_t)-1 >> 5;  // 32-byte elements: every byte offset below fits a size_t
    if ((a->n && a->n_cols > lim / a->n) || (a->src_stride && a->n_cols > lim / a->src_stride)) { set_error("%s: n_cols x n out of range", who); return TRH_EINVAL; }
    const bool empty = !a->n_cols || !a->n;
    if ((!a->dst && !empty) || ((uintptr_t)a->dst & 15) != 0) { set_error("%s: dst must be a 16-byte aligned device pointer", who); return TRH_EINVAL; }
    if (split && ((!a->dst_odd && !empty) || ((uintptr_t)a->dst_odd & 15) != 0)) { set_error("%s: dst_odd must be a 16-byte aligned device pointer", who); return TRH_EINVAL; }
    if ((!a->src && !empty && need) || ((uintptr_t)a->src & (esz - 1)) != 0) { set_error("%s: src must be aligned to its %zu-byte elements", who, esz); return TRH_EINVAL; }
    return TRH_OK;
}

template <class F, class T>
void launch_ints(const void* src, size_t stride, size_t n_cols, size_t live, void* dst, size_t n, hipStream_t s) {
    hipLaunchKernelGGL((columns_from_ints_kernel<F, T>), wit_grid(n_cols, n), dim3(WIT_BLOCK), 0, s, (const T*)src, stride, n_cols, live, (uint4*)dst, n);
}
template <class F, class T>
void launch_split(const void* src, size_t stride, size_t n_cols, size_t live, void* even, void* odd, size_t n, hipStream_t s) {
    hipLaunchKernelGGL((even_odd_split_kernel<F, T>), wit_grid(n_cols, n), dim3(WIT_BLOCK), 0, s, (const T*)src, stride, n_cols, live, (uint4*)even, (uint4*)odd, n);
}

// src: device memory
int expand_device(int field, int kind, const void* src, size_t stride, size_t n_cols, size_t live, void* dst, size_t n, hipStream_t s) {
    with_field(field, [&](auto f) {
        typedef decltype(f) F;
        switch (kind) {
            case TRH_INT_BITS:
                hipLaunchKernelGGL((columns_from_bits_kernel<F>), wit_grid(n_cols, n), dim3(WIT_BLOCK), 0, s, (const u32*)src, stride, n_cols, live, (uint4*)dst, n);
                break;
            case TRH_INT_U8: launch_ints<F, uint8_t>(src, stride, n_cols, live, dst, n, s); break;
            case TRH_INT_U16: launch_ints<F, uint16_t>(src, stride, n_cols, live, dst, n, s); break;
            case TRH_INT_U32: launch_ints<F, uint32_t>(src, stride, n_cols, live, dst, n, s); break;
            case TRH_INT_U64: launch_ints<F, uint64_t>(src, stride, n_cols, live, dst, n, s); break;
            case TRH_INT_I32: launch_ints<F, int32_t>(src, stride, n_cols, live, dst, n, s); break;
            default: launch_ints<F, int64_t>(src, stride, n_cols, live, dst, n, s); break;
        }
    });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

}  // namespace
}  // namespace trh

using namespace trh;

extern "C" {

int trh_columns_from_ints_dev(int field, const trh_ints_args_t* a) {
    TRH_TRY(check_ints("columns_from_ints_dev", field, a, false));
    TRH_ENTER(a->stream);
    if (!a->n_cols || !a->n) return TRH_OK;
    Range range("trh_columns_from_ints_dev");
    return expand_device(field, a->kind, a->src, a->src_stride, a->n_cols, a->live_rows, a->dst, a->n, (hipStream_t)a->stream);
}

int trh_columns_from_ints_host(int field, const trh_ints_args_t* a) {
    TRH_TRY(check_ints("columns_from_ints_host", field, a, false));
    TRH_ENTER(a->stream);
    if (!a->n_cols || !a->n) return TRH_OK;
    Range range("trh_columns_from_ints_host");
    hipStream_t s = (hipStream_t)a->stream;
    const size_t esz = int_kind_size(a->kind), need = int_kind_elems(a->kind, a->live_rows);
    if (!need) return expand_device(field, a->kind, nullptr, a->src_stride, a->n_cols, 0, a->dst, a->n, s);  // no live row: nothing to stage, nothing is read
    Ctx& c = ctx();
    const size_t col_bytes = a->src_stride * esz;
    size_t per_chunk = WIT_STAGE_BYTES / col_bytes;
    if (!per_chunk) per_chunk = 1;
    if (per_chunk > a->n_cols) per_chunk = a->n_cols;
    // the last column of a chunk ends with its live rows: the source need not hold a whole stride behind it
    TRH_TRY(c.io.ensure((per_chunk - 1) * col_bytes + need * esz));
    for (size_t c0 = 0; c0 < a->n_cols; c0 += per_chunk) {
        const size_t cnt = a->n_cols - c0 < per_chunk ? a->n_cols - c0 : per_chunk;
        // the staging copy and the kernel share the stream: the next chunk's copy into the scratch waits for this chunk's kernel
        TRH_TRY(stage_h2d(c, c.io.p, (const char*)a->src + c0 * col_bytes, (cnt - 1) * col_bytes + need * esz, s, c0 + cnt < a->n_cols));
        TRH_TRY(expand_device(field, a->kind, c.io.p, a->src_stride, cnt, a->live_rows, (char*)a->dst + c0 * a->n * 32, a->n, s));
    }
    return TRH_OK;
}

int trh_even_odd_split_dev(int field, const trh_ints_args_t* a) {
    TRH_TRY(check_ints("even_odd_split_dev", field, a, true));
    TRH_ENTER(a->stream);
    if (!a->n_cols || !a->n) return TRH_OK;
    Range range("trh_even_odd_split_dev");
    hipStream_t s = (hipStream_t)a->stream;
    with_field(field, [&](auto f) {
        typedef decltype(f) F;
        switch (a->kind) {
            case TRH_INT_U8: launch_split<F, uint8_t>(a->src, a->src_stride, a->n_cols, a->live_rows, a->dst, a->dst_odd, a->n, s); break;
            case TRH_INT_U16: launch_split<F, uint16_t>(a->src, a->src_stride, a->n_cols, a->live_rows, a->dst, a->dst_odd, a->n, s); break;
            case TRH_INT_U32: launch_split<F, uint32_t>(a->src, a->src_stride, a->n_cols, a->live_rows, a->dst, a->dst_odd, a->n, s); break;
            default: launch_split<F, uint64_t>(a->src, a->src_stride, a->n_cols, a->live_rows, a->dst, a->dst_odd, a->n, s); break;
        }
    });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

int trh_even_bits_table_dev(int field, const trh_even_bits_table_args_t* a) {
    if (!a) { set_error("even_bits_table_dev: null arguments"); return TRH_EINVAL; }
    TRH_TRY(check_field(field));
    if (a->word_bits < 2 || a->word_bits > 64 || (a->word_bits & 1)) { set_error("even_bits_table_dev: word_bits %u is not an even number in 2 .. 64", a->word_bits); return TRH_EINVAL; }
    const size_t entries = (size_t)1 << (a->word_bits / 2);
    if (entries > a->n) { set_error("even_bits_table_dev: the table of %u-bit words has %zu rows, the column %zu", a->word_bits, entries, a->n); return TRH_EINVAL; }
    if (a->n > ((size_t)-1 >> 5)) { set_error("even_bits_table_dev: n out of range"); return TRH_EINVAL; }
    if (!a->dst || ((uintptr_t)a->dst & 15) != 0) { set_error("even_bits_table_dev: dst must be a 16-byte aligned device pointer"); return TRH_EINVAL; }
    TRH_ENTER(a->stream);
    Range range("trh_even_bits_table_dev");
    with_field(field, [&](auto f) {
        hipLaunchKernelGGL((even_bits_table_kernel<decltype(f)>), wit_grid(1, a->n), dim3(WIT_BLOCK), 0, (hipStream_t)a->stream, (uint4*)a->dst, entries, a->n);
    });
    TRH_HIP_TRY(hipGetLastError());
    return TRH_OK;
}

}  // extern "C"
