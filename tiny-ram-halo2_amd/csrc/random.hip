// The prover's random scalars, drawn where they are used: trh_rng_* (include/trh.h) over csrc/chacha.h.
// What they serve: halo2_proofs 0.2.0 fills the vanishing argument's random polynomial, the opening's s(X) and the blinding rows of every
// advice / permuted / product column with one `Scalar::random(&mut rng)` per value on the host; a prover whose columns are resident would have
// to make them there and push 32 bytes per value over the link.  Here the host seeds a handle with 32 bytes of its own rng and the device
// expands the stream in place: one thread per element, one ChaCha20 block and one wide reduction each, two 16-byte stores.  No LDS, no
// cross-lane work, no table: the key travels in the launch's arguments.
// The handle is host memory and belongs to no context: its position (a block number) is shared by host draws and device fills, so that
// they interleave like calls on one Rust rng.
#include <string.h>

#include <mutex>
#include <new>

#include "chacha.h"
#include "ctx.h"
#include "devmem.h"

struct trh_rng {
    std::mutex mu;  // guards pos / at_end; taken INSIDE a context's lock by the device entries (the opening's rng callback runs with the context locked)
    trh::ChaChaKey key;
    uint64_t stream_id;
    uint64_t pos;         // the next element's block number
    bool at_end = false;  // the position is 2^64: the draw that ended on the last block succeeded, nothing more can be drawn before a seek
};

namespace trh {
namespace {

constexpr unsigned RNG_BLOCK = 256;

// out[i] = element pos + i
template <class F>
__global__ void __launch_bounds__(RNG_BLOCK) random_fill_kernel(uint4* __restrict__ out, size_t n, ChaChaKey key, u64 stream_id, u64 pos) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fe(out + 2 * i, chacha_field_element<F>(key.w, stream_id, pos + i));
}

// `rows` columns of row_len elements back to back: cell (r, first + c), c < count, = element pos + r * count + c; nothing else is written
template <class F>
__global__ void __launch_bounds__(RNG_BLOCK) random_fill_rows_kernel(uint4* __restrict__ cols, size_t cells, size_t row_len, size_t first, size_t count,
                                                                     ChaChaKey key, u64 stream_id, u64 pos) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cells) return;
    const size_t r = t / count, c = t - r * count;
    store_fe(cols + 2 * (r * row_len + first + c), chacha_field_element<F>(key.w, stream_id, pos + t));
}

// positions [pos, pos + elems) must exist: pos + elems <= 2^64 (rand_chacha would wrap to block 0 and repeat the stream; refused here)
int rng_reserve(const trh_rng* r, const char* who, size_t elems) {
    if (!elems) return TRH_OK;
    if (r->at_end || (u64)elems - 1 > ~(u64)0 - r->pos) {
        if (r->at_end) set_error("%s: %zu elements from position 2^64 pass the end of the stream (2^64 blocks)", who, elems);
        else set_error("%s: %zu elements from position %llu pass the end of the stream (2^64 blocks)", who, elems, (unsigned long long)r->pos);
        return TRH_EINVAL;
    }
    return TRH_OK;
}
void rng_advance(trh_rng* r, size_t elems) {
    if (!elems) return;
    const u64 next = r->pos + (u64)elems;  // wraps to 0 exactly when the draw ended on the last block
    r->at_end = next == 0;
    r->pos = next;
}

// one thread per element: the grid is ceil(elems / RNG_BLOCK) blocks
int rng_grid(const char* who, size_t elems, unsigned* blocks) {
    const size_t b = (elems + RNG_BLOCK - 1) / RNG_BLOCK;
    if (b > 0x7fffffffu) { set_error("%s: %zu elements exceed one launch", who, elems); return TRH_EINVAL; }
    *blocks = (unsigned)b;
    return TRH_OK;
}

}  // namespace
}  // namespace trh

using namespace trh;

extern "C" {

int trh_rng_create(const uint8_t seed[32], uint64_t stream_id, trh_rng_t* out) {
    if (!seed || !out) { set_error("rng_create: null pointer"); return TRH_EINVAL; }
    trh_rng* r = new (std::nothrow) trh_rng;
    if (!r) { set_error("rng_create: out of memory"); return TRH_ENOMEM; }
    for (int i = 0; i < 8; ++i) r->key.w[i] = (u32)seed[4 * i] | (u32)seed[4 * i + 1] << 8 | (u32)seed[4 * i + 2] << 16 | (u32)seed[4 * i + 3] << 24;
    r->stream_id = stream_id;
    r->pos = 0;
    *out = r;
    return TRH_OK;
}

void trh_rng_destroy(trh_rng_t r) {
    if (!r) return;
    volatile u32* k = r->key.w;  // volatile: the stores are not dead to the compiler
    for (int i = 0; i < 8; ++i) k[i] = 0;
    delete r;
}

int trh_rng_seek(trh_rng_t r, uint64_t block) {
    if (!r) { set_error("rng_seek: null handle"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(r->mu);
    r->pos = block;
    r->at_end = false;
    return TRH_OK;
}

int trh_rng_position(trh_rng_t r, uint64_t* block) {
    if (!r || !block) { set_error("rng_position: null pointer"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(r->mu);
    if (r->at_end) { set_error("rng_position: the stream is exhausted (position 2^64)"); return TRH_EINVAL; }
    *block = r->pos;
    return TRH_OK;
}

int trh_rng_next_scalar(trh_rng_t r, int field, uint64_t out_mont[4]) {
    if (!r || !out_mont) { set_error("rng_next_scalar: null pointer"); return TRH_EINVAL; }
    TRH_TRY(check_field(field));
    std::lock_guard<std::mutex> lk(r->mu);
    TRH_TRY(rng_reserve(r, "rng_next_scalar", 1));
    u32 w[8];
    with_field(field, [&](auto f) { fe_store(chacha_field_element<decltype(f)>(r->key.w, r->stream_id, r->pos), w); });
    memcpy(out_mont, w, 32);
    rng_advance(r, 1);
    return TRH_OK;
}

int trh_rng_fill_dev(trh_rng_t r, int field, void* out_dev, size_t n, void* stream) {
    if (!r) { set_error("rng_fill_dev: null handle"); return TRH_EINVAL; }
    TRH_TRY(check_field(field));
    if (n && !out_dev) { set_error("rng_fill_dev: null pointer"); return TRH_EINVAL; }
    if (((uintptr_t)out_dev & 15) != 0) { set_error("rng_fill_dev: elements must be 16-byte aligned"); return TRH_EINVAL; }
    if (n > ((size_t)-1 >> 5)) { set_error("rng_fill_dev: n out of range"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    if (!n) return TRH_OK;
    unsigned blocks = 0;
    TRH_TRY(rng_grid("rng_fill_dev", n, &blocks));
    std::lock_guard<std::mutex> lk(r->mu);
    TRH_TRY(rng_reserve(r, "rng_fill_dev", n));
    Range range("trh_rng_fill_dev");
    with_field(field, [&](auto f) {
        hipLaunchKernelGGL((random_fill_kernel<decltype(f)>), dim3(blocks), dim3(RNG_BLOCK), 0, (hipStream_t)stream, (uint4*)out_dev, n, r->key, (u64)r->stream_id, (u64)r->pos);
    });
    TRH_HIP_TRY(hipGetLastError());
    rng_advance(r, n);
    return TRH_OK;
}

int trh_rng_fill_rows_dev(trh_rng_t r, int field, void* cols_dev, size_t rows, size_t row_len, size_t first, size_t count, void* stream) {
    if (!r) { set_error("rng_fill_rows_dev: null handle"); return TRH_EINVAL; }
    TRH_TRY(check_field(field));
    if (first > row_len || count > row_len - first) { set_error("rng_fill_rows_dev: cells [%zu, %zu + %zu) do not fit a row of %zu", first, first, count, row_len); return TRH_EINVAL; }
    const size_t lim = (size_t)-1 >> 5;  // 32-byte elements: every byte offset below fits a size_t
    if ((rows && row_len > lim / rows) || (count && rows > lim / count)) { set_error("rng_fill_rows_dev: rows x row_len out of range"); return TRH_EINVAL; }
    const size_t cells = rows * count;
    if (cells && !cols_dev) { set_error("rng_fill_rows_dev: null pointer"); return TRH_EINVAL; }
    if (((uintptr_t)cols_dev & 15) != 0) { set_error("rng_fill_rows_dev: elements must be 16-byte aligned"); return TRH_EINVAL; }
    TRH_ENTER(stream);
    if (!cells) return TRH_OK;
    unsigned blocks = 0;
    TRH_TRY(rng_grid("rng_fill_rows_dev", cells, &blocks));
    std::lock_guard<std::mutex> lk(r->mu);
    TRH_TRY(rng_reserve(r, "rng_fill_rows_dev", cells));
    Range range("trh_rng_fill_rows_dev");
    with_field(field, [&](auto f) {
        hipLaunchKernelGGL((random_fill_rows_kernel<decltype(f)>), dim3(blocks), dim3(RNG_BLOCK), 0, (hipStream_t)stream, (uint4*)cols_dev, cells, row_len, first, count, r->key,
                           (u64)r->stream_id, (u64)r->pos);
    });
    TRH_HIP_TRY(hipGetLastError());
    rng_advance(r, cells);
    return TRH_OK;
}

}  // extern "C"
