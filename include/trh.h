/* trh.h -- C ABI of libtrh.so, the MI355X (gfx950) backend for the MSM / NTT / IPA-commitment
 * hot path of halo2_proofs as driven by the tiny-ram-halo2 TinyRAM circuit.
 *
 * The reference has no FFI of its own: the seam is the set of Rust functions that
 * `halo2_proofs::plonk::create_proof` calls (reference call sites
 * /root/reference/src/test_utils.rs:21, 23-25, 41-49, 89-104; crate pinned at
 * /root/reference/Cargo.lock:619-621, pasta_curves at :847-858).  Each entry point below names
 * the Rust interface it replaces.  INTEGRATION.md shows the `extern "C"` block a maintainer
 * adds to the halo2_proofs fork.
 *
 * Data formats (identical to the Rust in-memory layout, so slices cross without repacking):
 *   field element  4 x u64 little-endian limbs, Montgomery form (R = 2^256), fully reduced
 *                  -- `pasta_curves::Fp` / `Fq`.
 *   affine base    8 x u64: x[4], y[4]; the all-zero pattern is the identity.  (pasta's
 *                  `Affine` carries a separate flag: the Rust shim repacks, see INTEGRATION.md.)
 *   point result   12 x u64: Jacobian X[4], Y[4], Z[4] as in pasta's `Point`, normalised to
 *                  Z = 1; the identity is all-zero.
 * Curves: pallas (base Fp, scalar Fq), vesta (base Fq, scalar Fp; `EqAffine`, the curve the
 * reference proves over).  Fields: fp, fq.
 *
 * Errors: every function returns 0 on success or a negative TRH_E* code; the message is
 * available from trh_last_error() (thread-local).  Nothing aborts or throws across the ABI;
 * the Rust shim maps a non-zero return to the panic the reference would raise.
 * Threading and contexts: a CONTEXT is bound to one GPU and owns every scratch buffer, table cache and
 * in-flight state, behind one lock.  trh_init() makes the process default; every entry point may be
 * called from any host thread (it makes the context's device current for the calling thread itself --
 * hipSetDevice is per thread) and calls on one context are serialised, on the host by its lock and on
 * the device by ordering each call's stream behind the stream of the previous call (they share the
 * scratch).  One MSM may be in flight per context (trh_msm_dev_enqueue .. _finish); a second enqueue
 * returns TRH_EBUSY.  Threads that want to OVERLAP work (an MSM beside an NTT, two MSMs) give each
 * thread its own context: trh_ctx_create + trh_ctx_set_current (thread-local binding; several contexts
 * per GPU are fine).  Handles (trh_bases_t, trh_domain_t, trh_expr_t) are device memory: usable from
 * every context of the device they were created on.  Callbacks (trh_ipa_create_proof's transcript /
 * rng) run with the context locked: they may call host-side helpers (trh_point_sum, trh_rng_next_scalar, trh_last_error)
 * but must not start device work on the same context.
 * Multi-GPU: trh_init_multi() binds a device group; base sets of at least trh_set_shard_min() points
 * created afterwards are range-sharded over the group and trh_msm / trh_msm_dev / trh_best_multiexp_*
 * run one local Pippenger per GPU and add the partial points on the host.
 * There is no CPU fallback: without a usable HIP device trh_init() fails and every compute
 * entry point returns TRH_ENODEV.
 */
#ifndef TRH_H
#define TRH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRH_OK 0
#define TRH_EINVAL (-1)   /* bad argument (the Rust side panics on these: length mismatch, n != 1<<log_n) */
#define TRH_ENODEV (-2)   /* no HIP device / trh_init not called */
#define TRH_EHIP (-3)     /* HIP runtime error */
#define TRH_ENOMEM (-4)
#define TRH_EBUSY (-5)    /* the context already has an MSM in flight; trh_set_option while a context exists */
#define TRH_ESELFTEST (-6) /* trh_init: the known-answer self-test of the device arithmetic failed (trh_last_error() names the primitive) */

#define TRH_PALLAS 0
#define TRH_VESTA 1
#define TRH_FP 0
#define TRH_FQ 1

/* ---- lifecycle ------------------------------------------------------------------------ */
int trh_init(int device);            /* creates the process-default context on one GPU; idempotent */
void trh_shutdown(void);             /* destroys the default context / the device group (not contexts made by trh_ctx_create) */
const char* trh_last_error(void);
int trh_device_count(void);
const char* trh_version(void);       /* "trh <version> (gfx950, build <hash of the sources>)" */
/* The library's switches.  Each has an environment variable TRH_<NAME IN UPPER CASE> that is read ONCE (at the first trh_init /
 * trh_set_option); trh_set_option overrides it for hosts that must not touch the environment (a multi-threaded prover: getenv racing a
 * setenv elsewhere in the process is undefined behaviour, so no entry point of this library calls getenv after that).  Options are
 * process-wide and fixed while any context exists: call before trh_init, or after trh_shutdown (TRH_EBUSY otherwise).  Values are
 * decimal integers.  Names (defaults): pool_mb (4096), stage_slot_mb (16), copy_threads (-1 = by core count), bases_cache (0),
 * force_no_peer (0), ipa_fold (1 = the library's choice of the round after which an opening collapses its generators; 0 never), trace (0; bit 0
 * host-pointer entries, bit 1 IPA rounds), msm_chunk_gb (4), sparse (1), reduce_q4 (1), bin_sort (1), selftest (1) -- DESIGN.md section 8.   */
int trh_set_option(const char* name, const char* value);
int trh_get_option(const char* name, long* value);

/* ---- device group: the MSM range-sharded over the GPUs of one node (one host process, as the reference's prover is:
 * /root/reference/src/test_utils.rs:37-54).  devices[0] becomes the process default, exactly as trh_init(devices[0]);
 * a device may be listed more than once (logical shards on one GPU).  Base sets with at least trh_set_shard_min()
 * points (default 2^20) created afterwards by trh_bases_create_* / trh_bases_generate / trh_best_multiexp_* hold
 * shard g = points [g * ceil(n / G), ...) on devices[g]; MSMs over them enqueue one local Pippenger per device on that
 * device's own stream from the calling thread, copy the G partial points (96 B each) device-to-host and add them on
 * the host.  Device-resident scalars (trh_msm_dev) are handed to the other GPUs with peer copies.                    */
int trh_init_multi(const int* devices, int n_devices);
int trh_group_size(void);
int trh_group_peer_access(void);  /* 1: every pair of distinct group devices has peer access; 0: some pair has not (trh_last_error() after trh_init_multi names the first) */
int trh_set_shard_min(size_t n_points);

/* ---- explicit contexts (see "Threading and contexts" above) ------------------------------------------------------- */
typedef struct trh_ctx* trh_ctx_t;
int trh_ctx_create(int device, trh_ctx_t* out);
void trh_ctx_destroy(trh_ctx_t ctx);
int trh_ctx_set_current(trh_ctx_t ctx_or_null);  /* binds the calling THREAD; NULL = back to the process default */
int trh_ctx_device(trh_ctx_t ctx_or_null);       /* device index of the context (NULL: of the calling thread's), -1 if none */
/* the context's own non-blocking stream (a hipStream_t), for hosts without a HIP toolchain of their own (the Rust shim, the C++ driver):
 * pass it as the `stream` argument of the *_dev entries so that two contexts' work overlaps instead of meeting on the null stream */
void* trh_ctx_stream(trh_ctx_t ctx_or_null);

/* ---- halo2_proofs::arithmetic::best_multiexp(coeffs, bases) -> C::Curve ------------------
 * coeffs: n x 4 u64 (scalar field, Montgomery -- the memory image of `&[C::Scalar]`),
 * bases: n x 8 u64 affine, out: 12 u64.  Host pointers: the pairs cross PCIe in ranges, range t + 1 while range t is
 * computed (96 B per pair: bound by the link, 2^24 pairs in ~max(link, 17 ms)).             */
int trh_best_multiexp_pallas(const uint64_t* coeffs, const uint64_t* bases, size_t n, uint64_t out_xyz[12]);
int trh_best_multiexp_vesta(const uint64_t* coeffs, const uint64_t* bases, size_t n, uint64_t out_xyz[12]);

/* ---- halo2_proofs::arithmetic::best_fft(a, omega, log_n) ---------------------------------
 * a: 2^log_n x 4 u64 in place, natural order in and out; omega: 4 u64 Montgomery, must be a
 * primitive 2^log_n-th root of unity (what EvaluationDomain passes).  Host pointers.       */
int trh_best_fft_fp(uint64_t* a, const uint64_t omega[4], uint32_t log_n);
int trh_best_fft_fq(uint64_t* a, const uint64_t omega[4], uint32_t log_n);

/* the same for `count` host slices with one omega (one pointer per column): the uploads, transforms and downloads of
 * consecutive columns overlap on three streams (the link carries both directions at once); results as `count` single calls */
int trh_best_fft_batch_fp(uint64_t* const* a, size_t count, const uint64_t omega[4], uint32_t log_n);
int trh_best_fft_batch_fq(uint64_t* const* a, size_t count, const uint64_t omega[4], uint32_t log_n);

/* ---- host memory of the host-pointer entry points.  A pageable slice crosses PCIe through the library's pinned rings
 * (csrc/hostio.hip).  A caller that keeps long-lived buffers (Params.g_lagrange, a polynomial arena) may page-lock them once --
 * trh_host_register on memory it owns, or trh_host_alloc -- and the DMA engine then reads / writes them directly.
 * trh_io_stats: bytes moved by the host-pointer entry points on the calling thread's context and the host seconds spent in
 * the copies, per direction (overlapping copies each count their own time); reset != 0 clears the counters.              */
int trh_host_register(void* host, size_t bytes);
int trh_host_unregister(void* host);
int trh_host_alloc(void** host, size_t bytes);
int trh_host_free(void* host);
typedef struct trh_io_stats {
    double h2d_bytes, d2h_bytes, h2d_seconds, d2h_seconds;
    double h2d_zero_bytes; /* of h2d_bytes: pinned slots that were zero throughout (the padding of trh_best_fft's zero-padded vectors)
                              and were cleared on the device instead of crossing the link */
} trh_io_stats_t;
int trh_io_stats(trh_io_stats_t* out, int reset);

/* ---- device-resident base sets: poly::commitment::Params { g, g_lagrange, w } -------------
 * `Params::commit` / `commit_lagrange` run hundreds of MSMs over the same bases; upload once. */
typedef struct trh_bases* trh_bases_t;
int trh_bases_create_pallas(const uint64_t* xy_host, size_t n, trh_bases_t* out);
int trh_bases_create_vesta(const uint64_t* xy_host, size_t n, trh_bases_t* out);
/* wrap n bases already in device memory (no copy, not owned) */
int trh_bases_wrap_device(int curve, const void* xy_dev, size_t n, trh_bases_t* out);
/* synthetic set P_i = (s0 + (first + i) * d) * G, G = (-1, 2), generated on the device */
int trh_bases_generate(int curve, uint64_t s0, uint64_t d, uint64_t first, size_t n, trh_bases_t* out);
int trh_bases_download(trh_bases_t b, size_t offset, size_t n, uint64_t* xy_host);
const void* trh_bases_device_ptr(trh_bases_t b);
size_t trh_bases_len(trh_bases_t b);
int trh_bases_shards(trh_bases_t b);  /* devices the set is range-sharded over (trh_init_multi); 1 for a single-device set */
void trh_bases_destroy(trh_bases_t b);
/* Fixed-base tables for an owned set (Params.g / g_lagrange serve ~500 commitments per proof): stores
 * 2^(c j) * P_i for every window j (W x n x 128 B of HBM), after which a full-range MSM over the handle puts the
 * digits of all windows into ONE bucket set -- one bucket reduction per MSM instead of W, wider windows, no
 * Horner pass over windows.  window_bits 0 = automatic (<= 17); requires W * n <= 2^24.  Results are the same
 * group elements; MSMs over a sub-range (offset != 0 or n < len) keep using the per-window path.           */
int trh_bases_precompute(trh_bases_t b, int window_bits);   /* must not run while an MSM over `b` is in flight on another context; the same holds for trh_bases_destroy */
int trh_bases_precomputed_window_bits(trh_bases_t b); /* 0 when no table is attached */
/* sizes the calling context's MSM scratch for batches of `batch` MSMs (commitments) over the first n bases of the set, without running one:
 * setup-time, so that the first commitment batch of a process allocates nothing (see trh_domain_reserve).  A lone MSM beyond 2^25 pairs runs as
 * range tiles: the scratch of one tile is reserved */
int trh_bases_reserve(trh_bases_t b, size_t n, size_t batch);

/* MSM over bases[offset .. offset+n) with host scalars (Params::commit / commit_lagrange) */
int trh_msm(trh_bases_t bases, size_t offset, const uint64_t* scalars_host, size_t n,
            int scalars_are_montgomery, uint64_t out_xyz[12]);
/* same with scalars already in device memory, enqueued on `stream` (a hipStream_t, may be 0);
 * synchronises the stream before returning the point to the host.                           */
int trh_msm_dev(trh_bases_t bases, size_t offset, const void* scalars_dev, size_t n,
                int scalars_are_montgomery, void* stream, uint64_t out_xyz[12]);
/* asynchronous halves of trh_msm_dev: enqueue leaves the per-window sums on the device,
 * finish synchronises, folds the windows on the host and returns the point.  One MSM in flight per
 * context (TRH_EBUSY otherwise); finish must name the base set and be called on the context of its enqueue.
 * Over a base set WITH fixed-base tables (trh_bases_precompute) the enqueue is not fully asynchronous: a sampler reads ~1024 scalars
 * and votes on the flag-like unit path, which synchronises `stream` once (everything queued on it before the call completes first);
 * option sparse = 0 (or a set without tables) keeps the enqueue free of host synchronisations.  With trh_set_timing(1) such an MSM
 * reports zero phase times (trh_last_timing): the sampler's paths are not timed phase by phase.                                  */
int trh_msm_dev_enqueue(trh_bases_t bases, size_t offset, const void* scalars_dev, size_t n,
                        int scalars_are_montgomery, void* stream);
int trh_msm_dev_finish(trh_bases_t bases, void* stream, uint64_t out_xyz[12]);
/* batch of MSMs over the same bases (one per column): scalars_dev holds batch x n x 4 u64.  Batches of >= 8 items run in chunks
 * of <= 64 and synchronise `stream` once or twice per chunk (a sampler's vote decides whether the chunk is flag-like and its +-1 digits
 * are summed straight from the table; the entry counts of the chunk are read back to size the accumulation's segments for sparse --
 * witness-shaped -- columns), so the call is not fully asynchronous even before the final hand-over of the points. */
int trh_msm_batch_dev(trh_bases_t bases, size_t offset, const void* scalars_dev, size_t n, size_t batch,
                      int scalars_are_montgomery, void* stream, uint64_t* out_xyz /* batch x 12 */);
/* Params::commit / commit_lagrange for `batch` polynomials already in device memory (batch x n x 4 u64, back to back):
 * item b is the MSM of polys[b] || blinds[b] over the handle's n + 1 bases (g or g_lagrange followed by w) -- the blind
 * is read from its own small array, so the polynomials are not copied to make room for it.  blinds: batch x 4 u64, host. */
int trh_commit_batch_dev(trh_bases_t bases, const void* polys_dev, size_t n, size_t batch, const uint64_t* blinds_host,
                         void* stream, uint64_t* out_xyz /* batch x 12 */);
/* the same for polynomials in HOST memory (polys_host[b]: n scalars, Montgomery): the columns cross PCIe in chunks, chunk
 * j + 1 while the batched MSM of chunk j runs */
int trh_commit_batch_host(trh_bases_t bases, const uint64_t* const* polys_host, size_t n, size_t batch, const uint64_t* blinds_host,
                          uint64_t* out_xyz /* batch x 12 */);
/* window width override for tuning (0 = automatic) */
int trh_msm_set_window_bits(int c); /* 0 or 2..18 */

/* sum of `count` points (Jacobian 12 x u64 each) on the host: combines the per-GPU partial
 * results of a range-sharded MSM after the all-gather.                                       */
int trh_point_sum(int curve, const uint64_t* points_xyz, size_t count, uint64_t out_xyz[12]);

/* ---- NTT on device memory (EvaluationDomain call sites) ----------------------------------- */
int trh_ntt_dev(int field, void* a_dev, uint32_t log_n, const uint64_t omega[4], size_t batch, void* stream);
/* a[i] *= factor (e.g. n^-1 after an inverse transform), device memory */
int trh_field_scale_dev(int field, void* a_dev, size_t n, const uint64_t factor[4], void* stream);
/* a[i] *= factors[i % period] (factors: period x 4 u64, host memory, period <= 64).  Covers
 * halo2's `distribute_powers_zeta` coset shift (period 3: 1, zeta, zeta^2) and
 * `divide_by_vanishing_poly` (period 2^(extended_k - k) table of (X^n - 1)^-1 values).        */
int trh_field_scale_periodic_dev(int field, void* a_dev, size_t n, const uint64_t* factors, uint32_t period, void* stream);
/* same for `rows` polynomials stored back to back (row_len elements each): only the first
 * active_len elements of each row are scaled and the period restarts with each row, i.e.
 * a[r][c] *= factors[c % period] for c < active_len (a batch of coeff_to_extended inputs).     */
int trh_field_scale_rows_dev(int field, void* a_dev, size_t rows, size_t row_len, size_t active_len,
                             const uint64_t* factors, uint32_t period, void* stream);

/* ---- halo2_proofs::poly::EvaluationDomain on device polynomials -------------------------------
 * trh_domain_create(field, j, k) mirrors EvaluationDomain::new(j, k): quotient_poly_degree = j - 1,
 * extended_k = smallest e with 2^e >= 2^k (j - 1); omega / extended_omega from ROOT_OF_UNITY, coset
 * generator ZETA, t_evaluations = (X^n - 1)^-1 on the coset.  Polynomials are `batch` rows of 2^k
 * (or 2^extended_k) field elements stored back to back in device memory.                        */
typedef struct trh_domain* trh_domain_t;
int trh_domain_create(int field, uint32_t j, uint32_t k, trh_domain_t* out);
/* Setup-time sizing, so that the FIRST proof of a process runs like every later one (the reference proves 1 - 10 circuits per process,
 * /root/reference/src/test_utils.rs:37-54, and its user waits for the first): the transforms' twiddle / coset-block tables (also built by
 * trh_domain_create) and their scratch for batches of `batch` polynomials, on the calling thread's context.                              */
int trh_domain_reserve(trh_domain_t d, size_t batch);
void trh_domain_destroy(trh_domain_t d);
uint32_t trh_domain_extended_k(trh_domain_t d);
/* which: 0 omega, 1 omega_inv, 2 extended_omega, 3 extended_omega_inv, 4 ifft_divisor,
 *        5 extended_ifft_divisor, 6 g_coset (zeta), 7 g_coset_inv (zeta^2); Montgomery limbs */
int trh_domain_constant(trh_domain_t d, int which, uint64_t out[4]);
int trh_domain_lagrange_to_coeff(trh_domain_t d, void* a_dev, size_t batch, void* stream);            /* in place */
int trh_domain_coeff_to_extended(trh_domain_t d, const void* coeff_dev, void* ext_dev, size_t batch, void* stream);
int trh_domain_extended_to_coeff(trh_domain_t d, void* a_dev, size_t batch, void* stream);            /* in place; caller truncates */
int trh_domain_divide_by_vanishing_poly(trh_domain_t d, void* a_dev, size_t batch, void* stream);     /* in place */

/* The extended domain as coset blocks: its 2^extended_k points zeta * extended_omega^i, i = q * 2^(extended_k - k) + r, are the
 * 2^(extended_k - k) cosets (zeta extended_omega^r) * omega^q of the size-2^k subgroup.  coeff_to_extended_blocks writes, for each
 * of `batch` polynomials, blocks r = 0 .. n_blocks - 1 (2^k values each, back to back): entry q of block r is entry
 * q * 2^(extended_k - k) + r of coeff_to_extended's output.  A block is a size-2^k transform (two passes at k = 18 instead of the
 * three of the zero-padded 2^21 one), Rotation(1) is q + 1 inside a block (trh_expr_eval_blocks_dev), and the quotient h(X) --
 * degree < (j - 1) 2^k -- is determined by j - 1 = trh_domain_quotient_blocks() blocks (5 of 8 for the reference's circuit), so the
 * prover needs only those of every column.  blocks_to_quotient: (j - 1) x 2^k values of the numerator on blocks 0 .. j - 2
 * (overwritten) -> the (j - 1) x 2^k coefficients of h(X) = numerator / (X^(2^k) - 1) (divide_by_vanishing = 1; with 0 the input
 * is taken as h's own values): what extended_to_coeff(divide_by_vanishing_poly(.)) returns, truncated to (j - 1) 2^k, whenever the
 * vanishing polynomial divides the numerator (it does in create_proof).                                                          */
uint32_t trh_domain_quotient_blocks(trh_domain_t d);
int trh_domain_coeff_to_extended_blocks(trh_domain_t d, const void* coeff_dev, void* ext_dev, size_t batch, uint32_t n_blocks, void* stream);
int trh_domain_blocks_to_quotient(trh_domain_t d, void* num_blocks_dev, void* h_coeff_dev, int divide_by_vanishing, void* stream);

/* the same on HOST polynomials (one pointer per column; what the Rust EvaluationDomain's methods take), pipelined over PCIe:
 * lagrange_to_coeff in place; coeff_to_extended reads 2^k coefficients and writes 2^extended_k values (only the non-zero
 * coefficients go up); extended_to_coeff in place on one polynomial of 2^extended_k values, optionally preceded by
 * divide_by_vanishing_poly (the two steps create_proof applies to h(X))                                                     */
int trh_domain_lagrange_to_coeff_host(trh_domain_t d, uint64_t* const* a, size_t count);
int trh_domain_coeff_to_extended_host(trh_domain_t d, const uint64_t* const* coeff, uint64_t* const* ext, size_t count);
int trh_domain_extended_to_coeff_host(trh_domain_t d, uint64_t* a, int divide_by_vanishing_first);
/* the coset-block forms on host polynomials, for a host-side h(X) evaluation that has adopted the block layout: n_blocks x 2^k values
 * per column come down instead of 2^extended_k (5/8 of the bytes when n_blocks = trh_domain_quotient_blocks()), the quotient's numerator
 * goes up as (j - 1) x 2^k values and h(X)'s (j - 1) x 2^k coefficients come back                                                     */
int trh_domain_coeff_to_extended_blocks_host(trh_domain_t d, const uint64_t* const* coeff, uint64_t* const* ext, size_t count, uint32_t n_blocks);
int trh_domain_blocks_to_quotient_host(trh_domain_t d, const uint64_t* num_blocks, uint64_t* h_coeff, int divide_by_vanishing);

/* ---- IPA opening rounds: poly::commitment::prover::create_proof (device memory) ---------------
 * The two half-size MSMs of a round run through trh_msm_dev on the live G' buffer
 * (trh_bases_wrap_device + offset); these are the remaining per-round primitives.            */
/* halo2_proofs::arithmetic::compute_inner_product(a, b): sum a[i] * b[i] -> out (Montgomery) */
int trh_field_inner_product_dev(int field, const void* a_dev, const void* b_dev, size_t n, void* stream, uint64_t out[4]);
/* halo2_proofs::arithmetic::eval_polynomial for `batch` polynomials (n coefficients each, back to back in device memory)
 * at one point -- the evaluations create_proof sends before the multiopen argument; out: batch x 4 u64 on the host */
int trh_poly_eval_batch_dev(int field, const void* polys_dev, size_t n, size_t batch, const uint64_t point[4], void* stream, uint64_t* out);
/* y[i] += c * x[i]: the folds p'[i] += u^-1 p'[i + half], b[i] += u b[i + half] */
int trh_field_axpy_dev(int field, void* y_dev, const void* x_dev, size_t n, const uint64_t c_mont[4], void* stream);
/* out[i] = x^i for i < n: the evaluation vector b = (1, x3, x3^2, ...) */
int trh_field_powers_dev(int field, void* out_dev, size_t n, const uint64_t x_mont[4], void* stream);
/* parallel_generator_collapse: g_lo[i] = g_lo[i] + u * g_hi[i], normalised to affine (u: scalar
 * field element, Montgomery; g_*: `half` 64-byte affine PODs)                                   */
int trh_bases_fold_dev(int curve, void* g_lo_dev, const void* g_hi_dev, size_t half, const uint64_t u_mont[4], void* stream);

/* The whole opening in one call: poly::commitment::prover::create_proof(params, rng, transcript,
 * p_poly, p_blind, x_3).  p', b and G' never leave the device; per round only L_j, R_j and the
 * challenge cross the boundary, through the caller's transcript (BLAKE2b on the Rust side) and
 * randomness callbacks.  g_w: resident bases g (2^k points) followed by w -- or g, w and u (2^k + 2 points; the last one must
 * equal u_xy): with fixed-base tables attached to that set (trh_bases_precompute, once per Params) every MSM of the opening runs
 * in fixed-base mode (k = 18: 20 -> 15.5 ms).  u_xy: Params.u;
 * p_poly_dev / s_poly_dev: 2^k coefficients in device memory (s_poly: the caller's random polynomial,
 * its constant term is adjusted here so that s(x3) = 0); scalars are Montgomery limbs.
 * Writes to the transcript exactly what the Rust prover writes: S, then L_j, R_j per round, then c, f.
 * A zero round challenge (the Rust prover's `u_j.invert().unwrap()` panics) returns TRH_EINVAL.          */
typedef struct trh_transcript {
    void* ctx;
    void (*write_point)(void* ctx, const uint64_t xyz[12]);           /* normalised Jacobian, Z = 1 */
    void (*write_scalar)(void* ctx, const uint64_t s_mont[4]);
    void (*squeeze_challenge_scalar)(void* ctx, uint64_t out_mont[4]);
} trh_transcript_t;
typedef void (*trh_rng_scalar_fn)(void* ctx, uint64_t out_mont[4]);    /* C::Scalar::random(rng) */
int trh_ipa_create_proof(trh_bases_t g_w, const uint64_t u_xy[8], uint32_t k, const void* p_poly_dev,
                         const uint64_t p_blind[4], const uint64_t x3[4], const void* s_poly_dev,
                         const uint64_t s_blind[4], const trh_transcript_t* transcript,
                         trh_rng_scalar_fn rng, void* rng_ctx, void* stream,
                         uint64_t out_c[4], uint64_t out_f[4]);
/* The generator collapse of that opening on its own (csrc/ipafold.hip), for tests and for callers that keep their own round loop:
 * G''[i] = sum over t < 2^r of s_t G[i + t 2^(k-r)], i < 2^(k-r), s_t = the product of u_j over the set bits (r - 1 - j) of t -- what r
 * rounds of parallel_generator_collapse leave of the first 2^k points of `bases`.  bases: a set on one device of at least 2^k points
 * with a fixed-base table attached (trh_bases_precompute); the table's rows are as long as the set, so a g || w || u set collapses as
 * in the opening.  Supported shapes: table windows of 10 .. 18 bits, 2 <= r <= 10, k >= r + 8; anything else is TRH_EINVAL.
 * u_mont: r x 4 Montgomery words in round order, host memory.  out_xy_dev: 2^(k-r) 64-byte affine points (identity: all zero);
 * out_rec_dev: the same points as 128-byte records of the MSM's accumulation (x, y, -y in the signed 29-bit limbs; identity: all zero).
 * Returns with the stream synchronised.                                                                                            */
int trh_ipa_collapse_generators_dev(trh_bases_t bases, uint32_t k, uint32_t r, const uint64_t* u_mont, void* out_xy_dev, void* out_rec_dev, void* stream);

/* ---- IPA verifier accumulator: poly::commitment::msm::MSM and verifier::Guard::use_challenges (halo2_proofs 0.2.0
 *      poly/commitment/{msm.rs, verifier.rs}; reached from plonk::verify_proof / BatchVerifier::finalize after the proofs are made,
 *      reference call site /root/reference/src/test_utils.rs:52-68) ----------------------------------------------------------
 * The transcript, the challenges, compute_b and the multiopen verifier stay on the host; these entries hold MSM's arithmetic.
 * g_w_u: the opening's resident set, g || w (2^k + 1 points) or g || w || u (2^k + 2; the last point must equal u_xy) -- with
 * fixed-base tables attached, eval's MSM uses them.  The g scalars live on the device (2^k Montgomery words, fully reduced) and
 * are absent, as halo2's `g_scalars: Option<Vec<_>>`, until add_constant_term / add_to_g_scalars_dev / use_challenges first sets them;
 * w, u and the appended terms stay on the host.  Scalars are Montgomery words, points 8-word affine (all-zero = identity).
 * Every call on an accumulator must come from the context that created it (trh_ctx_set_current); the stream arguments order the
 * device work as elsewhere (add_constant_term enqueues on the stream of the accumulator's previous call).                      */
typedef struct trh_ipa_msm* trh_ipa_msm_t;
int trh_ipa_msm_create(trh_bases_t g_w_u, uint32_t k, const uint64_t u_xy[8], trh_ipa_msm_t* out);   /* Params::empty_msm (k >= 1) */
void trh_ipa_msm_destroy(trh_ipa_msm_t m);
int trh_ipa_msm_append_term(trh_ipa_msm_t m, const uint64_t scalar[4], const uint64_t point_xy[8]);   /* MSM::append_term */
int trh_ipa_msm_add_constant_term(trh_ipa_msm_t m, const uint64_t c[4]);                              /* MSM::add_constant_term: g[0] += c */
int trh_ipa_msm_add_to_w_scalar(trh_ipa_msm_t m, const uint64_t s[4]);
int trh_ipa_msm_add_to_u_scalar(trh_ipa_msm_t m, const uint64_t s[4]);
int trh_ipa_msm_add_to_g_scalars_dev(trh_ipa_msm_t m, const void* scalars_dev, void* stream);          /* MSM::add_to_g_scalars, 2^k device scalars */
/* Guard::use_challenges for `count` (>= 1) guards in one pass over the 2^k g scalars:
 *     g[i] = alpha g[i] + sum_p weights[p] neg_c[p] prod_{j : bit (k - 1 - j) of i set} u[p][j]
 * u: count x k challenges (round order), neg_c: count scalars (-c), weights: count scalars or NULL (all one), alpha: NULL = one.
 * count = 1 without weights / alpha is Guard::use_challenges (compute_s(u, neg_c) added to g); weights_p = prod_{q > p} r_q with
 * alpha = prod_q r_q is BatchVerifier::finalize's chain of scale(r_q) / add_msm over the guards' MSMs, for their g parts.         */
int trh_ipa_msm_use_challenges(trh_ipa_msm_t m, size_t count, const uint64_t* u, const uint64_t* neg_c, const uint64_t* weights,
                               const uint64_t alpha[4], void* stream);
int trh_ipa_msm_scale(trh_ipa_msm_t m, const uint64_t factor[4], void* stream);   /* MSM::scale: g, w, u and every appended scalar */
int trh_ipa_msm_add_msm(trh_ipa_msm_t dst, trh_ipa_msm_t src, void* stream);       /* MSM::add_msm; same curve, context and base set */
/* MSM::eval: one full-range MSM over g_w_u (trh_msm_dev) when the g part exists, the appended terms (and w / u where that MSM does not
 * carry them) through the small MSM, the points added on the host.  is_identity: what eval returns; out_xyz: the point itself. */
int trh_ipa_msm_eval(trh_ipa_msm_t m, void* stream, int* is_identity, uint64_t out_xyz[12]);
const void* trh_ipa_msm_g_scalars_dev(trh_ipa_msm_t m);   /* the 2^k g scalars in device memory, NULL while there are none (tests, shims) */

/* ---- grand-product building blocks of the permutation / lookup arguments ----------------------
 * (plonk/permutation/prover.rs, plonk/lookup/prover.rs: batch_invert of the denominators, then the
 * running product z[0] = 1, z[i] = z[i-1] * numerator[i-1] / denominator[i-1])                    */
/* ff::BatchInvert: a[i] <- a[i]^-1 in place, zeros stay zero */
int trh_field_batch_invert_dev(int field, void* a_dev, size_t n, void* stream);
/* the division the product columns need, in the same pass: a[i] <- num[i] * a[i]^-1 (a zero denominator stays zero) */
int trh_field_batch_invert_mul_dev(int field, void* a_dev, const void* num_dev, size_t n, void* stream);
/* the products the running product is taken over, for every product column of a proof in ONE launch:
 *     out[r][i] = prod_{t in row r} (x_t[i] + c_t * y_t[i] + g_t)      (y_t NULL: x_t[i] + g_t),   i < n
 * row r owns terms[row_start[r] .. row_start[r + 1]) (row_start has rows + 1 entries, row_start[0] = 0).  Permutation chunk
 * (plonk/permutation/prover.rs Argument::commit): numerator terms (v_j, omega^i column, beta * delta^(col j), gamma), denominator
 * terms (v_j, sigma_j, beta, gamma); lookup product (plonk/lookup/prover.rs commit_product): numerator (A, -, -, beta)(S, -, -, gamma),
 * denominator (A', -, -, beta)(S', -, -, gamma).  c / g: Montgomery words; columns: n elements in device memory.              */
typedef struct trh_product_term {
    const void* x;
    const void* y;
    uint64_t c[4];
    uint64_t g[4];
} trh_product_term_t;
int trh_product_terms_dev(int field, const trh_product_term_t* terms, const uint32_t* row_start, uint32_t rows, size_t n, void* out_dev, void* stream);
/* out[i] = prod_{j < i} a[j], out[0] = 1 (exclusive scan; out must not alias a) */
int trh_field_prefix_product_dev(int field, const void* a_dev, void* out_dev, size_t n, void* stream);
/* the same for `rows` independent vectors of n elements stored back to back (all product columns of a proof at once) */
int trh_field_prefix_product_rows_dev(int field, const void* a_dev, void* out_dev, size_t n, size_t rows, void* stream);
/* chains the product columns of consecutive permutation sets (plonk/permutation/prover.rs Argument::commit starts set s from
 * z_(s-1)[u], u = the number of usable rows) after trh_field_prefix_product_rows_dev has made every row start from one: with z_in the
 * rows on entry, row r >= 1 becomes z_in[r][i] * c_r, c_r = prod_{t < r} z_in[t][link]; row 0 stays.  In place, canonical Montgomery
 * words in and out, bit-exact.  rows <= 1 succeeds and does nothing.  Asynchronous on args->stream (the stream travels in the struct,
 * as in trh_quotient_args_t), ordered behind the context's previous call; the rows - 1 carries are formed in the context's scratch by
 * a one-workgroup launch, then one pass multiplies: no host read, no synchronisation.
 * TRH_EINVAL: an unknown field id, n no power of two, link >= n, a null or misaligned z.                                          */
typedef struct trh_product_chain_args {
    void*  z;        /* rows x n stored elements back to back, in place: the output of trh_field_prefix_product_rows_dev */
    size_t n, rows;  /* n = 2^k elements per row */
    size_t link;     /* the row index u whose value starts the next set, link < n */
    void*  stream;
} trh_product_chain_args_t;
int trh_product_chain_dev(int field_id, const trh_product_chain_args_t* args);
/* out[i] = sum_{j < i} a[j], out[0] = 0 */
int trh_field_prefix_sum_dev(int field, const void* a_dev, void* out_dev, size_t n, void* stream);

/* ---- multiopen building blocks (poly/multiopen/prover.rs: the x1 / x4 linear combinations of the queried polynomials
 *      and the division of (q(X) - r(X)) by the (X - point) factors) ------------------------------------------------- */
/* out[i] = sum_b coeffs[b] * polys[b][i]; polys: batch x n back to back in device memory, coeffs: batch x 4 u64 on the host */
int trh_poly_lincomb_dev(int field, const void* polys_dev, size_t n, size_t batch, const uint64_t* coeffs_host, void* out_dev, void* stream);
/* arithmetic::kate_division(a, z): quotient of a(X) (n coefficients) by (X - z), n - 1 coefficients, remainder a(z) dropped.
 * pz_dev / pzinv_dev: z^i and z^-i for i < n (trh_field_powers_dev; shared by every polynomial divided at this point, z != 0),
 * scratch_dev: 2 n elements.                                                                                          */
int trh_poly_kate_division_dev(int field, const void* a_dev, size_t n, const void* pz_dev, const void* pzinv_dev, void* scratch_dev, void* q_dev, void* stream);

/* ---- lookup argument: plonk/lookup/prover.rs `permute_expression_pair` ------------------------------------------
 * out_input = the first usable_rows input values sorted (field Ord = canonical integer order); out_table[row] = out_input[row]
 * where that row starts a run of equal values (one instance of the value leaves the table multiset), the remaining rows take
 * the left-over table values in ascending order starting from the LAST repeated row, exactly as the Rust code fills them.
 * Returns TRH_EINVAL when an input value does not occur in the table (halo2: Error::ConstraintSystemFailure).  The blinding
 * rows behind usable_rows are the caller's.  Synchronises the stream.                                                       */
int trh_lookup_permute_dev(int field, const void* input_dev, const void* table_dev, size_t usable_rows, void* out_input_dev,
                           void* out_table_dev, void* stream);
/* every lookup of a proof at once (the reference's circuit has 31): `batch` input columns and `batch` table columns, column l at
 * element offset l * row_stride (row_stride >= usable_rows: whole 2^k-row columns can be passed with usable_rows < 2^k; the rows behind
 * usable_rows are not touched in the outputs, which use the same stride).  One set of launches and one host synchronisation for
 * the whole batch; TRH_EINVAL names the first lookup with an input value that does not occur in its table.                        */
int trh_lookup_permute_batch_dev(int field, const void* inputs_dev, const void* tables_dev, size_t usable_rows, size_t row_stride, size_t batch,
                                 void* out_inputs_dev, void* out_tables_dev, void* stream);

/* ---- gate expressions over resident columns: the h(X) numerator of plonk::create_proof ---------
 * halo2's `Expression<F>` (Constant / Selector / Fixed / Advice / Instance query at a Rotation, Negated, Sum,
 * Product, Scaled) compiled by the caller to a straight-line program for a stack machine that every row of the
 * (extended) domain runs on its own: PUSH_* push a value, ADD / SUB / MUL replace the two top entries (next op top),
 * NEG / SQR / MUL_CONST / ADD_CONST rewrite the top, FOLD does acc = acc * const[a] + top and pops (the challenge-y
 * Horner over gates), STORE_TOP / STORE_ACC write output a.  Locals hold shared sub-expressions.
 * A column query reads column[(row + rotation * rot_step) mod 2^log_n]: on the extended coset Rotation(r) is
 * r * 2^(extended_k - k) rows.  Constants are Montgomery limbs.                                           */
enum {
    TRH_EXPR_PUSH_COLUMN = 0, /* a = column index, rotation */
    TRH_EXPR_PUSH_CONST = 1,  /* a = constant index */
    TRH_EXPR_PUSH_LOCAL = 2,  /* a = local index */
    TRH_EXPR_ADD = 3,
    TRH_EXPR_SUB = 4,         /* next - top */
    TRH_EXPR_MUL = 5,
    TRH_EXPR_NEG = 6,
    TRH_EXPR_SQR = 7,
    TRH_EXPR_MUL_CONST = 8,   /* a = constant index */
    TRH_EXPR_ADD_CONST = 9,
    TRH_EXPR_STORE_LOCAL = 10, /* local[a] = top (kept) */
    TRH_EXPR_FOLD = 11,       /* acc = acc * const[a] + top; pop */
    TRH_EXPR_STORE_TOP = 12,  /* output[a][row] = top; pop */
    TRH_EXPR_STORE_ACC = 13   /* output[a][row] = acc */
};
typedef struct {
    uint32_t op;
    uint32_t a;
    int32_t rotation;
} trh_expr_insn_t;
typedef struct trh_expr* trh_expr_t;
/* validates the program (stack discipline, index ranges), fixes the LDS slot of every spill / refill and uploads it */
int trh_expr_create(int field, const trh_expr_insn_t* insns, size_t n_insn, const uint64_t* consts /* n_consts x 4 */, size_t n_consts,
                    size_t n_columns, size_t n_outputs, size_t n_locals, trh_expr_t* out);
void trh_expr_destroy(trh_expr_t e);
uint32_t trh_expr_lds_slots(trh_expr_t e); /* stack entries below the two register ones + locals */
/* replace one constant: the per-proof challenges (y, beta, gamma, theta) of an otherwise fixed program */
int trh_expr_set_const(trh_expr_t e, uint32_t index, const uint64_t value[4]);
/* columns_dev / outputs_dev: host arrays of device pointers (2^log_n x 4 u64 each); synchronises the stream */
int trh_expr_eval_dev(trh_expr_t e, const void* const* columns_dev, void* const* outputs_dev, uint32_t log_n, uint32_t rot_step, void* stream);
/* the same over columns in the coset-block layout of trh_domain_coeff_to_extended_blocks: n_blocks x 2^block_log rows per column,
 * Rotation(r) reads row (q + r) mod 2^block_log of the same block */
int trh_expr_eval_blocks_dev(trh_expr_t e, const void* const* columns_dev, void* const* outputs_dev, uint32_t block_log, uint32_t n_blocks, void* stream);

/* ---- the permutation and lookup terms of h(X): plonk/permutation/prover.rs and plonk/lookup/prover.rs `Committed::construct` ----------
 * What create_proof folds into the quotient's numerator behind the custom gates, over resident extended columns, per row:
 *   l_active = 1 - (l_last + l_blind), last = Rotation(-(blinding_factors + 1)), X = the row's domain point, acc = acc * y + t for every t:
 *   permutation (n_sets = ceil(n_perm_columns / chunk_len) sets; nothing when n_perm_columns = 0)
 *     l0 (1 - z_0);  l_last (z_last^2 - z_last), z_last the last set's column;  l0 (z_s - z_(s-1)(last)) for s = 1 .. n_sets - 1;
 *     l_active (z_s(+1) prod_j (v_j + beta sigma_j + gamma) - z_s prod_j (v_j + beta delta^j X + gamma)) for s = 0 .. n_sets - 1,
 *     j over the set's columns, delta^j by the global column index
 *   every lookup, in order (A, S compressed input / table, A', S' permuted, z the product column)
 *     l0 (1 - z);  l_last (z^2 - z);  l_active (z(+1) (A' + beta)(S' + gamma) - z (A + beta)(S + gamma));  l0 (A' - S');
 *     l_active (A' - S')(A' - A'(-1))
 * The handle holds what depends on the shape only (the tables X is made from, delta^j, the staging of the pointer table).  A call takes
 * the columns in either layout of the extended domain: n_blocks = 0 is the flat one (2^extended_k rows, Rotation(r) = r * 2^(extended_k - k)
 * rows, cyclic), n_blocks >= 1 the coset blocks of trh_domain_coeff_to_extended_blocks (n_blocks x 2^k rows, Rotation(r) inside a block).
 * acc holds the fold so far -- the STORE_ACC output of the gates' program run with the same y, or zeros -- and receives the result
 * (canonical Montgomery words, bit-exact).  With no column and no lookup acc is left as it is.  Every pointer is device memory, 16-byte
 * aligned; the arrays themselves are host arrays.  The stream travels in the struct.  Like trh_expr_eval_dev the entry stages its pointer
 * table in the handle and returns with the stream SYNCHRONISED; calls on one handle are serialised.
 * TRH_EINVAL: chunk_len = 0, blinding_factors + 2 > 2^k (create); n_blocks above 2^(extended_k - k), a null array whose count is
 * non-zero, a null column, null acc / l0 / l_blind / l_last, acc equal to any input pointer (a rotated read would see rows already
 * folded).                                                                                                                       */
typedef struct trh_quotient* trh_quotient_t;
int trh_quotient_create(trh_domain_t d, uint32_t n_perm_columns, uint32_t chunk_len, uint32_t n_lookups, uint32_t blinding_factors, trh_quotient_t* out);
void trh_quotient_destroy(trh_quotient_t q);
typedef struct trh_quotient_args {
    const void* const* perm_values;  /* n_perm_columns extended columns, permutation column order */
    const void* const* perm_sigmas;  /* n_perm_columns */
    const void* const* perm_z;       /* ceil(n_perm_columns / chunk_len) */
    const void* const* lookups;      /* n_lookups x 5: A, S, A', S', z */
    const void *l0, *l_blind, *l_last;
    uint64_t beta[4], gamma[4], y[4]; /* Montgomery */
    void* acc;                       /* in / out: the fold so far (the gates' STORE_ACC output, or zeros) */
    uint32_t n_blocks;               /* 0: flat layout; else coset blocks, 1 .. 2^(extended_k - k) */
    void* stream;
} trh_quotient_args_t;
int trh_quotient_terms_dev(trh_quotient_t q, const trh_quotient_args_t* args);

/* ---- MockProver::verify on resident columns (halo2_proofs 0.2.0 dev.rs): "which gate, which row, which lookup" for a witness that is
 *      already in device memory.  The gate part and the lookup part are below; the permutation part is trh_perm_check_dev.  Columns are plain
 *      values: cell poisoning and CellNotAssigned (region bookkeeping of the Rust host) are not modelled.
 * Neither entry takes a stream: the verdict is returned in host memory, so they synchronise in any case.  Their work is ordered behind the
 * context's previous call, whatever stream that call used, and is complete on return.  Data written OUTSIDE the library on a non-blocking
 * stream is the caller's to synchronise before the call.
 * Results: n_bad = the number of bad rows, first_bad_row = the smallest of them, usable_rows when there is none.  The bitmap (device memory,
 * 8-byte aligned, may be NULL) holds one bit per row, bit r % 64 of u64 word r / 64, set for a bad row; every word is written, zeros
 * included, so the caller never clears it; bits of rows at or beyond usable_rows are 0.
 * trh_expr_check_dev runs a compiled program exactly as trh_expr_eval_dev does with rot_step = 1 -- a query reads
 * column[(row + rotation) mod 2^log_n], so a rotation at the last usable row reads the blinding rows, as upstream -- and tests every output
 * (STORE_TOP a / STORE_ACC a: one gate polynomial each) against zero on rows [0, usable_rows) instead of storing it: nothing the size of a
 * column is written.  n_bad / first_bad_row: n_outputs entries; bitmap: n_outputs x W words, output a from word a * W, W = max(1, 2^log_n / 64).
 * TRH_EINVAL: usable_rows of 0 or above 2^log_n, null arrays, and what trh_expr_eval_dev refuses.                                         */
int trh_expr_check_dev(trh_expr_t e, const void* const* columns_dev, uint32_t log_n, size_t usable_rows, uint64_t* n_bad /* n_outputs */,
                       uint64_t* first_bad_row /* n_outputs */, void* bad_bitmap_dev_or_null);
/* trh_lookup_check_dev: input row r < usable_rows is bad when the tuple (inputs[0][r], .., inputs[width - 1][r]) equals no tuple
 * (tables[0][t], ..) with t < usable_rows -- exact tuple membership as MockProver does it, not the theta compression of the prover.  width is
 * 1 .. 16; the arrays are host arrays of `width` device pointers, every column has at least usable_rows elements (16-byte aligned, canonical
 * stored words compared word by word, as in trh_perm_check_dev; typically the outputs of trh_expr_eval_dev over the lookup's input and table
 * expressions); rows at or beyond usable_rows are never read.  1 <= usable_rows <= 2^30.  One result pair; bitmap: ceil(usable_rows / 64) words.
 * The table's rows go into an open-addressing set in a block of the device pool (4 bytes x the power of two at or above 2 * usable_rows);
 * trh_stat("lookup_check_probes") reports the slots the last check on this context visited.  field_id is TRH_FP / TRH_FQ; any other value is
 * refused as everywhere else (tests/test_gpu_mock.py checks that for this entry).                                                       */
int trh_lookup_check_dev(int field_id, const void* const* inputs_dev, const void* const* tables_dev, uint32_t width, size_t usable_rows, uint64_t* n_bad,
                         uint64_t* first_bad_row, void* bad_bitmap_dev_or_null);

/* ---- best_fft over curve points: Params::new's g -> g_lagrange -----------------------------
 * halo2_proofs::arithmetic::best_fft::<C::Curve>(a, omega, log_n): a'[i] = sum_j [omega^(i j)] a[j].
 * points_dev: 2^log_n affine PODs in device memory, transformed in place (natural order in and out)
 * and normalised to affine; omega: scalar field element, Montgomery, primitive 2^log_n-th root;
 * scale_or_null: when non-NULL every output is multiplied by this scalar (Params::new uses n^-1).  */
int trh_point_fft_dev(int curve, void* points_dev, uint32_t log_n, const uint64_t omega[4],
                      const uint64_t* scale_or_null, void* stream);

/* ---- GroupEncoding / ff::Field::sqrt: the 32-byte compressed points of pasta_curves (`to_bytes` / `from_bytes`) and the field square
 *      root they need -- what `Params::read` / `Params::write` (halo2_proofs 0.2.0 poly/commitment.rs) and a transcript's read_point /
 *      write_point are made of.  Encoding: x canonical (not Montgomery), 32 bytes little endian, bit 7 of byte 31 = parity of canonical y;
 *      the identity is 32 zero bytes.  Invalid: x >= the modulus, x^3 + 5 not a square (x = 0 included).                              */
/* out[i] = sqrt(a[i]) (n x 4 u64 Montgomery in and out, 16-byte aligned), is_square[i] = 1 / 0.  The root returned is the one whose CANONICAL
 * value is even (sqrt(0) = 0); a non-square gives 0 and flag 0.  pasta_curves itself promises no particular root.  Every element costs the
 * same fixed instruction sequence (csrc/fieldsqrt.h).                                                                                  */
int trh_field_sqrt_dev(int field, const void* a_dev, void* out_dev, void* is_square_dev /* n x u8 */, size_t n, void* stream);
/* n x 64-byte affine PODs -> n x 32-byte encodings */
int trh_points_compress_dev(int curve, const void* xy_dev, void* bytes_dev, size_t n, void* stream);
/* n x 32-byte encodings (4-byte aligned) -> n x 64-byte affine PODs; an invalid encoding gives the all-zero POD and ok[i] = 0 (ok_dev: n x u8, may
 * be NULL).  Returns TRH_OK when the kernel ran; *first_bad = the smallest invalid index, n when every encoding was valid (synchronises the
 * stream to read it; NULL = no synchronisation, look at ok_dev)                                                                          */
int trh_points_decompress_dev(int curve, const void* bytes_dev, void* xy_dev, void* ok_dev_or_null, size_t n, void* stream, uint64_t* first_bad_or_null);
/* Params::read's inner loop: n encodings in host memory -> an OWNED resident set, exactly as trh_bases_create_* would have made from the decoded
 * points (same sharding under trh_init_multi, usable with trh_bases_precompute / reserve / every trh_msm*); 32 instead of 64 bytes per point
 * cross the link.  An invalid encoding: TRH_EINVAL, trh_last_error() names the first bad index, *out untouched, nothing leaked.             */
int trh_bases_create_compressed(int curve, const uint8_t* bytes_host, size_t n, trh_bases_t* out);
/* Params::write: bases [offset, offset + n) of a resident set as n x 32 bytes in host memory */
int trh_bases_download_compressed(trh_bases_t b, size_t offset, size_t n, uint8_t* bytes_host);
/* host-side, no device needed (like trh_point_sum): a transcript's write_point / read_point of single commitments */
int trh_point_to_bytes(int curve, const uint64_t xyz[12], uint8_t out[32]);    /* Jacobian in, any Z (Z = 0: the identity) */
int trh_point_from_bytes(int curve, const uint8_t in[32], uint64_t out_xy[8]); /* TRH_EINVAL on an invalid encoding (out_xy zeroed) */

/* ---- the prover's random scalars, drawn on the device from a ChaCha20 seed: `C::Scalar::random(&mut rng)` for whole vectors ----------
 * create_proof draws the vanishing argument's random polynomial (2^k scalars), the opening's s(X) (2^k) and the blinding rows at the end of
 * every advice / permuted / product column one scalar at a time on the host.  Here the host draws 32 bytes from its own rng ONCE, and the
 * stream they seed is expanded where the values are used.  Element i of the stream (seed, stream_id):
 *   ChaCha20 block number i (RFC 8439 section 2.3 block function, 20 rounds, the original layout: 64-bit block counter in state words 12 - 13,
 *   64-bit stream id in words 14 - 15, low words first), its 64 bytes read as eight little-endian u64 limbs[0 .. 8), then
 *   (limbs[0 .. 4) + 2^256 limbs[4 .. 8)) mod m as 4 x u64 Montgomery words, fully reduced.
 * That is -- as recalled, not pinned by the reference -- what rand_chacha's `ChaCha20Rng::from_seed(seed)` (set_stream(stream_id)) yields through
 * pasta_curves' `Fp::random` / `Fq::random`.  One element is exactly one block; positions are block numbers.
 * The handle is HOST memory, like the Rust rng object: it belongs to no context or device and may be used with any.  Host draws and device
 * fills share its one position (guarded by a lock of the handle's own), so they interleave like calls on one rng: a call advances the
 * position by the elements it produced (n, rows * count, or 1) and a call that fails leaves it where it was.  position + elements > 2^64
 * is TRH_EINVAL (rand_chacha would wrap and repeat the stream); after a draw that ended exactly on the last block the position is 2^64:
 * trh_rng_position then fails and trh_rng_seek is the way back.  n == 0 / count == 0 / rows == 0 succeed and do nothing.
 * The fill entries are asynchronous on `stream` and ordered behind the context's previous call, like the other *_dev entries; device
 * elements must be 16-byte aligned.  The seed appears in no error message and in no trace output.
 * Every entry takes the handle first and the field id second (TRH_FP / TRH_FQ; an unknown id is refused as everywhere else).               */
typedef struct trh_rng* trh_rng_t;
int trh_rng_create(const uint8_t seed[32], uint64_t stream_id, trh_rng_t* out);   /* no device needed */
void trh_rng_destroy(trh_rng_t r);                                                 /* wipes the key */
int trh_rng_seek(trh_rng_t r, uint64_t block);
int trh_rng_position(trh_rng_t r, uint64_t* block);
/* host-side, one block, no device needed: the blinds of commitments, and trh_ipa_create_proof's rng callback -- that callback runs with the
 * context locked, which is allowed because this entry starts no device work and takes only the handle's own lock */
int trh_rng_next_scalar(trh_rng_t r, int field, uint64_t out_mont[4]);
/* out[i] = element position + i, i < n (the random polynomial, s(X)) */
int trh_rng_fill_dev(trh_rng_t r, int field, void* out_dev, size_t n, void* stream);
/* `rows` columns of row_len elements stored back to back: cell (r, first + c), c < count, = element position + r * count + c (row-major over
 * the cells written); every other cell is left untouched -- the blinding rows of a batch of resident columns, without a staging buffer.
 * first + count > row_len is TRH_EINVAL.                                                                                                   */
int trh_rng_fill_rows_dev(trh_rng_t r, int field, void* cols_dev, size_t rows, size_t row_len, size_t first, size_t count, void* stream);

/* ---- permutation keygen: plonk/permutation/keygen.rs `Assembly` { copy, build_vk, build_pk } (halo2_proofs 0.2.0, reached from keygen_vk /
 *      keygen_pk) and the permutation part of MockProver::verify ---------------------------------------------------------------------------
 * The assembly records the circuit's copy constraints over n_columns equality-enabled columns of n = 2^k rows and keeps the permutation they
 * induce.  A cell is one u32, cell = column * n + row, so n_columns * n <= 2^32 (and n_columns >= 1, k <= 27).  trh_perm_copy is
 * `Assembly::copy`: the cycles of the two cells are merged, the smaller into the larger, and the mapping of the two cells is swapped; copying
 * a cell to itself or repeating a copy changes nothing; a cell outside the columns is TRH_EINVAL and changes nothing.  The ORDER of the
 * copies decides the mapping (and through it the sigma commitments of the verifying key), as upstream -- restated as recalled, csrc/permkeygen.h.
 * trh_perm_sigma_dev writes the sigma columns build_vk commits and build_pk transforms: for `count` columns from first_column,
 *     sigma[c][r] = delta^(m / n) * omega^(m % n),  m = mapping[c * n + r]
 * (omega: the 2^k-th root of unity of EvaluationDomain, delta = 5^(2^32), pasta_curves DELTA), count x n elements back to back in device
 * memory, asynchronous on `stream` except for the upload of the mapping: the handle keeps one device copy per context, made by the first
 * device call after a copy (that call synchronises `stream` once) and reused until the next copy.
 * trh_perm_check_dev counts the cells whose value differs from the value of the cell they map to -- columns_dev: n_columns device pointers
 * (host array), n elements each, canonical stored forms, compared word by word; *n_bad = 0 means the copy constraints hold;
 * *first_bad_cell = the smallest such cell, n_columns * n when there is none.  It synchronises the stream.
 * The handle is HOST memory, like trh_rng_t: create, copy, mapping and destroy need no device.  Every entry takes the handle first; the device
 * entries take the field id second (an unknown id is refused as everywhere else).                                                        */
typedef struct trh_perm_s* trh_perm_t;
int trh_perm_create(uint32_t n_columns, uint32_t k, trh_perm_t* out);   /* no device needed */
void trh_perm_destroy(trh_perm_t p);
int trh_perm_copy(trh_perm_t p, uint32_t left_column, uint32_t left_row, uint32_t right_column, uint32_t right_row);
/* quads: count x (left_column, left_row, right_column, right_row), applied in order; stops at the first refused one (trh_last_error() names
 * its index; the copies before it stay made) */
int trh_perm_copy_batch(trh_perm_t p, const uint32_t* quads, size_t count);
/* the mapping of `count` columns from first_column: out_cells[(c - first_column) * n + r] = the cell that cell (c, r) maps to */
int trh_perm_mapping(trh_perm_t p, uint32_t first_column, uint32_t count, uint32_t* out_cells);
int trh_perm_sigma_dev(trh_perm_t p, int field, uint32_t first_column, uint32_t count, void* out_dev, void* stream);
int trh_perm_check_dev(trh_perm_t p, int field, const void* const* columns_dev, uint64_t* n_bad, uint64_t* first_bad_cell, void* stream);

/* ---- hash_to_curve: `Params::new(k)` (halo2_proofs 0.2.0 poly/commitment.rs), 2^k + 2 calls of pasta_curves 0.4 `C::hash_to_curve(prefix)(msg)` --
 * RFC 9380's hash_to_curve over BLAKE2b-512: expand_message_xmd with DST = prefix || "-" || "pallas" / "vesta" || "_XMD:BLAKE2b_SSWU_RO_" to two
 * elements of the curve's BASE field, simplified SWU (Z = -13) onto the iso-curve y^2 = x^3 + A x + 1265, the 3-isogeny to y^2 = x^3 + 5, cofactor 1
 * (csrc/hashtocurve.h restates every step; that the Rust crates produce these very bytes is recalled, not pinned -- DESIGN.md section 4).
 * Params::new: g[i] = hash("Halo2-Parameters")(00 || le32(i)), w = hash(..)(01), u = hash(..)(02), then trh_point_fft_dev for g_lagrange.
 * `prefix` is a NUL-terminated string of 0 - 128 bytes (longer: TRH_EINVAL).  Field elements are 4 x u64 Montgomery, points 64-byte affine
 * PODs (the identity all zero), both 16-byte aligned on the device.  The *_dev entries are asynchronous on `stream` and ordered behind the
 * context's previous call like the others; n = 0 succeeds and writes nothing; curve_id is TRH_PALLAS / TRH_VESTA, any other value is refused as
 * everywhere else (tests/test_gpu_hashtocurve.py and tests/test_hashtocurve_host.py check that for these four).                              */
/* host side, no device needed (like trh_point_from_bytes): w, u, and any single point; msg may be NULL when msg_len = 0 */
int trh_hash_to_curve(int curve_id, const char* prefix, const uint8_t* msg, size_t msg_len, uint64_t out_xy[8]);
/* hash_to_field alone: the message of element i is tag || le32(first + i), i < n, first + n <= 2^32 (beyond: TRH_EINVAL);
 * u_dev: n x 2 elements, u0 then u1 of each message */
int trh_hash_to_field_indexed_dev(int curve_id, const char* prefix, uint8_t tag, uint32_t first, size_t n, void* u_dev, void* stream);
/* out[i] = iso_map(sum over j < per_point of swu(u[i * per_point + j])), per_point 1 (RFC 9380's map_to_curve, encode_to_curve's second half)
 * or 2 (hash_to_curve's); u_dev: n x per_point fully reduced elements; u1 = -u0 gives the identity.  Every element costs the same fixed
 * instruction sequence, u = 0 and u^2 = -1 / Z included.                                                                                   */
int trh_map_to_curve_dev(int curve_id, const void* u_dev, size_t n, int per_point, void* xy_dev, void* stream);
/* the two above back to back over scratch memory of the context: xy[i] = hash(prefix)(tag || le32(first + i)) -- g[first .. first + n) of
 * Params::new for tag 0 */
int trh_hash_to_curve_indexed_dev(int curve_id, const char* prefix, uint8_t tag, uint32_t first, size_t n, void* xy_dev, void* stream);

/* ---- the proof transcript: `Blake2bWrite` / `Blake2bRead` with `Challenge255` (halo2_proofs 0.2.0 src/transcript.rs) -- what turns the items
 *      create_proof writes into the `Vec<u8>` that `transcript.finalize()` returns and `BatchVerifier::add_proof` takes -----------------------
 * State: BLAKE2b, 64-byte digest, no key, personalisation "Halo2-Transcript".  common_point absorbs 01 || x || y (32 bytes each, little endian,
 * canonical, base field; the identity is refused), common_scalar 02 || s (32 bytes, scalar field); write_* do the same and append the 32-byte
 * compressed point (trh_point_to_bytes' encoding) / the 32 bytes of s to the proof; squeeze_challenge_scalar absorbs 00, finalises a COPY of the
 * state and reduces the 64 bytes, read as a little-endian integer, modulo the scalar field's order; read_point takes 32 bytes, decodes them
 * (trh_point_from_bytes' rules, and the identity is refused) and absorbs the point, read_scalar takes 32 bytes, refuses a value >= the modulus
 * and absorbs it.  That the Rust crate produces these very bytes is recalled, not pinned (csrc/transcript.h).
 * Points go in as 12-word Jacobian (any Z != 0) and come out as the 8-word affine POD; scalars are 4 Montgomery words, fully reduced.
 * ERRORS LATCH: after the first refused operation (TRH_EINVAL) every later one does nothing, returns that code again and leaves its output
 * zero; trh_tr_status / trh_tr_message give the first error's code and text -- the callbacks of trh_transcript_t return void, so inside
 * trh_ipa_create_proof that is the only way an error is seen: ask for the status when the opening has returned.
 * The handle is HOST memory, like trh_rng_t: every entry works without a device and before trh_init, starts no device work and takes only the
 * handle's own lock, so the callbacks may run with the context locked.  curve_id is TRH_PALLAS / TRH_VESTA, any other value is refused as
 * everywhere else.                                                                                                                         */
typedef struct trh_tr* trh_tr_t;
int trh_tr_create_writer(int curve_id, trh_tr_t* out);
int trh_tr_create_reader(int curve_id, const uint8_t* proof, size_t len, trh_tr_t* out);   /* the bytes are copied; len = 0 is an empty proof */
void trh_tr_destroy(trh_tr_t t);
int trh_tr_common_point(trh_tr_t t, const uint64_t xyz[12]);
int trh_tr_common_scalar(trh_tr_t t, const uint64_t s_mont[4]);
int trh_tr_write_point(trh_tr_t t, const uint64_t xyz[12]);                                /* a writer's */
int trh_tr_write_scalar(trh_tr_t t, const uint64_t s_mont[4]);                             /* a writer's */
int trh_tr_read_point(trh_tr_t t, uint64_t out_xy[8]);                                     /* a reader's */
int trh_tr_read_scalar(trh_tr_t t, uint64_t out_mont[4]);                                  /* a reader's */
int trh_tr_squeeze_challenge_scalar(trh_tr_t t, uint64_t out_mont[4]);
/* *out = the writer as trh_ipa_create_proof's transcript: ctx and three functions of the library, so that the opening's round loop never
 * leaves it; valid while the handle lives */
int trh_tr_callbacks(trh_tr_t t, trh_transcript_t* out);
int trh_tr_status(trh_tr_t t);                              /* TRH_OK, or the latched error's code (its text goes to trh_last_error() too) */
int trh_tr_message(trh_tr_t t, char* out, size_t cap);      /* the latched error's text, empty while there is none; truncated to cap - 1 */
int trh_tr_bytes_len(trh_tr_t t, size_t* len);              /* a writer: the bytes written so far; a reader: the length of its proof */
int trh_tr_bytes(trh_tr_t t, uint8_t* out, size_t cap);     /* copies them out; cap below the length is TRH_EINVAL */
int trh_tr_remaining(trh_tr_t t, size_t* len);              /* a reader: the bytes not yet taken */

/* ---- packed witness intake: columns from machine integers and flag bits, expanded on the device ------------------------------------------
 * A host that knows its trace as machine words (any TinyRAM host does, before it wraps them in `F::from(u64)`) hands over the words and
 * bitmaps; the device makes the columns: 1 .. 8 bytes or one bit per cell cross the link instead of 32 bytes.
 * The source is n_cols columns, column c starting src_stride ELEMENTS (u32 words for TRH_INT_BITS) behind column c - 1, each with live_rows
 * live rows; the destination is n_cols columns of n stored elements (4 x u64 canonical Montgomery words, fully reduced, bit-exact) back to
 * back.  Row r < live_rows of column c is
 *   TRH_INT_BITS               bit r & 31 of the u32 word src[c * src_stride + (r >> 5)]: R mod m for a set bit, zero for a clear one; bits of
 *                              the last word at positions >= live_rows are ignored
 *   TRH_INT_U8 .. TRH_INT_U64  the element's value
 *   TRH_INT_I32, TRH_INT_I64   the element's value, m - |v| for v < 0
 * and rows live_rows .. n - 1 are WRITTEN as zero (nothing is loaded for them).  The source needs the natural alignment of its elements and
 * nothing more (a column may start at an odd element offset); the last column need not extend beyond its live rows.
 * trh_columns_from_ints_dev:  src is device memory.  Asynchronous on args->stream (the stream travels in the struct, as in
 *   trh_quotient_args_t), ordered behind the context's previous call; no host read, no synchronisation.
 * trh_columns_from_ints_host: src is ANY host memory, pageable included.  The packed bytes go through the context's pinned upload ring into
 *   context scratch, whole columns at a time -- as many as fit 64 MiB, one if a single packed column is larger, which bounds the scratch by
 *   max(64 MiB, one packed column) -- and the same kernel runs; it returns when the source has been read.  Counted by trh_io_stats.
 * trh_even_odd_split_dev:     kinds TRH_INT_U8 .. TRH_INT_U64, device src: dst takes w & 0x5555.. and dst_odd (w & 0xAAAA..) >> 1 of every
 *   word w, the two halves of the reference's even-bits decomposition (even + 2 odd = w, both with bits at even positions only); the
 *   halves need not cross the link once their word is on the device.
 * trh_even_bits_table_dev:    dst[i] = sum_j bit_j(i) 4^j for i < 2^(word_bits / 2), zero from there to n: the even-bits lookup table.
 *   TRH_EINVAL for an odd word_bits, word_bits outside 2 .. 64, 2^(word_bits / 2) > n, a null or misaligned dst.
 * n_cols == 0 or n == 0 succeeds and does nothing.  TRH_EINVAL, with nothing written: an unknown field or kind, src_stride too small for
 * live_rows, live_rows > n, a null or misaligned dst, a misaligned src; for the split also a signed or TRH_INT_BITS kind and a null or
 * misaligned dst_odd.                                                                                                                    */
enum { TRH_INT_BITS = 0, TRH_INT_U8, TRH_INT_U16, TRH_INT_U32, TRH_INT_U64, TRH_INT_I32, TRH_INT_I64 };
typedef struct trh_ints_args {
    int kind;
    const void* src;      /* device memory for *_dev, any host memory (pageable allowed) for *_host */
    size_t src_stride;    /* elements between consecutive columns (u32 words for BITS); >= live_rows (BITS: >= ceil(live_rows / 32)) */
    size_t n_cols, live_rows;
    void*  dst;           /* device, n_cols x n x 4 u64, 16-byte aligned: canonical Montgomery words */
    void*  dst_odd;       /* trh_even_odd_split_dev only: the odd halves, same shape; dst takes the even halves */
    size_t n;             /* rows per destination column, >= live_rows; rows live_rows .. n - 1 are WRITTEN as zero */
    void*  stream;
} trh_ints_args_t;
typedef struct trh_even_bits_table_args {
    uint32_t word_bits;   /* even, 2 .. 64 */
    void*  dst;           /* device, n x 4 u64, 16-byte aligned */
    size_t n;             /* >= 2^(word_bits / 2) */
    void*  stream;
} trh_even_bits_table_args_t;
int trh_columns_from_ints_dev(int field_id, const trh_ints_args_t* args);
int trh_columns_from_ints_host(int field_id, const trh_ints_args_t* args);
int trh_even_odd_split_dev(int field_id, const trh_ints_args_t* args);
int trh_even_bits_table_dev(int field_id, const trh_even_bits_table_args_t* args);

/* ---- the memory-consistency table: access log to sorted, checked columns, on the device ---------------------------------------------------
 * The one table of the reference's circuit whose rows are no per-row function of the trace (its Mem chip over the trace's access log).  The
 * host hands over the log as it was executed -- four word arrays -- and the tape; the device groups the accesses by address (a stable radix
 * sort on the address alone, so that time order survives inside a run), opens every run with an Init row (the tape word that lives at the
 * address, or 0; tape word i lives at address i * word_bits / 8 and has a run whether it is accessed or not), carries the most recently
 * stored value down each run and writes 13 columns of n rows, back to back in dst (csrc/memtable.h has the rules in full):
 *   s_trace  address  time  init  store  load  value  addr_inc  time_inc  addr_inc_even  addr_inc_odd  time_inc_even  time_inc_odd
 * rows = #runs + m rows are live; rows `rows` .. n - 1 are WRITTEN as zero.  src_index (optional) receives the log index of every row,
 * 0xFFFFFFFF for Init rows and behind the table.
 * Refusals (TRH_EINVAL), all with NOTHING written to dst or src_index:
 *   a log record with an address, time or value >= 2^word_bits, a time of 0 or one that does not exceed the record before it:
 *     trh_last_error() names the FIRST such log index;
 *   rows > max_rows: args->rows reports the rows the table would need;
 *   an unknown field, word_bits odd or outside 2 .. 32, a tape (t > 0) with word_bits % 8 != 0 or an address >= 2^word_bits, max_rows > n,
 *     t + 2 m >= 2^31, a null array that is not empty, a dst that is not 16-byte aligned, a word array that is not 4-byte aligned.
 * A load whose claimed value differs from the value the table carries to its row is REPORTED, not refused (a prover may want to prove that
 * a trace is wrong): n_inconsistent counts them, first_inconsistent is the smallest log index among them (m when there is none); the
 * `value` column holds the carried value either way.  m == 0 && t == 0 succeeds with rows == 0 and zeroes dst.
 * The stream travels in the struct, as in trh_ints_args_t.  The entry knows `rows` before it writes and returns it, so it is NOT
 * asynchronous: it synchronises with the host exactly twice -- once on args->stream after the sort, to read the log's verdict and the row
 * count, and once when its scratch returns to the device pool (trh_free waits for the device as hipFree does), which is also when the count
 * of inconsistent loads has landed.  Scratch is one block of the pool of trh_malloc, sized by memtable::make_plan (about 21 bytes per
 * record and 24 per row); the entry allocates nothing else.
 * trh_stat: "memtable_rows", "memtable_sort_passes" (ceil(word_bits / 8); 0 for an empty call) and "memtable_tiles" (the smallest tile count
 * among the sort over the records, the scan over the records and the scan over the rows: above 1, every stage crossed a tile boundary)
 * describe the last call on this context that got as far as its row count.                                                                  */
typedef struct trh_mem_table_args {
    uint32_t word_bits;                       /* even, 2 .. 32 */
    const uint32_t *address, *time, *value;   /* device, m each, in execution order */
    const uint32_t *store_bits;               /* device, ceil(m / 32) words: bit i & 31 of word i >> 5 is set for a store, clear for a load */
    size_t m;
    const uint32_t *tape; size_t t;           /* device; may be null when t == 0 */
    void*  dst;                               /* device, 13 x n x 4 u64, 16-byte aligned, canonical Montgomery words */
    size_t n, max_rows;                       /* rows per column; the table's extent, max_rows <= n */
    uint32_t* src_index;                      /* optional device, n words */
    void*  stream;
    uint64_t rows, n_inconsistent, first_inconsistent;   /* out */
} trh_mem_table_args_t;
int trh_mem_table_dev(int field_id, trh_mem_table_args_t* args);

/* ---- the Exe table: trace steps to temp-var columns and selectors, on the device ---------------------------------------------------------
 * For every step of the trace the reference's ExeChip::assign_trace derives the four temporary variables a, b, c, d (the non-deterministic
 * advice included), their one-hot selector cells and the plain trace cells: a pure per-row function of the step and its successor.  The
 * host hands over the steps as machine words, m of them in execution order:
 *   pc, inst, a, value   u32[m]; inst packs the opcode in bits 0 - 4, ri in bits 8 - 11, rj in bits 12 - 15, "operand A is a register" in
 *                        bit 16; a is the immediate or the register's number; value is the word loaded or stored, 0 elsewhere
 *   regs                 u32[m x reg_count], step-major: the registers BEFORE the step
 *   flag_bits            ceil(m / 32) words: bit i & 31 of word i >> 5 is the flag before step i
 * and the device writes 28 + 9 reg_count columns of n rows, back to back in dst (csrc/exetable.h has the layout in full):
 *   s_trace pc flag reg* opcode immediate value tv_a tv_b tv_c tv_d | sa_* | sb_* | sc_* | sd_* | sa_non_det sb_non_det sc_non_det sd_non_det
 * the first 24 + 9 reg_count being ADVICE of tests/golden/make_exe_gates.py.  Rows m .. n - 1 are WRITTEN as zero; `immediate` is A when A
 * is an immediate and 0 when it is a register; the successor of step m - 1 is the zero row (index m of no input is read).
 * The per-opcode selection is DATA: selection[opcode] packs one source per temporary variable, TRH_EXE_ENTRY(a, b, c, d), or is
 * TRH_EXE_UNKNOWN.  Sources: UNSET (no selector, value 0), PC, PC_NEXT, PC_PLUS_ONE, REG_RI, REG_RJ, REG_NEXT_RI, A, VALUE, ZERO, ONE,
 * MAX_WORD (2^word_bits - 1) and TRH_EXE_NONDET + rule.  A source is legal for a variable when the variable's selector family has its
 * column (a: pc_next reg reg_next a v_addr; b: pc pc_next pc_plus_one reg reg_next a max_word; c: reg reg_next a zero; d: pc reg reg_next
 * a zero one); UNSET and NONDET are legal everywhere.  Source A with a register operand sets s?_reg{A}, with an immediate s?_a.
 * Non-deterministic rules, integers over RI = reg[ri], RJ = reg[rj] (contents before the step), A = the operand's VALUE, W = word_bits:
 *   REM      A == 0 ? 0 : RJ mod A                                QUOT     A == 0 ? 0 : RJ div A
 *   CMP_GT   RI > A ? 2^W - (RI - A) : A - RI                     CMP_GE   RI >= A ? 2^W - 1 - (RI - A) : A - RI - 1
 *   MUL_HI   (RJ A) >> W                                          MUL_LO   (RJ A) mod 2^W
 *   SMUL_LO  the low word of the product of A and RJ as signed words
 *   XOR      RI xor A                                             PC_PLUS_ONE  pc + 1 (an integer: 2^32 when pc = 2^32 - 1)
 *   SHL_HI   s = min(A, W): (RJ 2^s) >> W                         SHR_LO   s = min(A, W): 2^s RJ - 2^W (RJ >> s), negative values as m - |v|
 * s = min(A, W) is this library's choice where the reference's 2u64.pow(a) overflows.
 * The default table (exetable.DEFAULT_SELECTION in the Python package, trh::exe_default_selection in trh.hpp) restates the reference's
 * TempVarSelectorsRow::from (aux.rs:105-398) with two departures:
 *   a register operand's value is the register's CONTENT, which is what the reference's reg_gate demands of a cell under s?_reg{A}; its
 *     push_temp_var_vals writes the register's NUMBER there (aux.rs:410-417);
 *   CJmp's d is NONDET(PC_PLUS_ONE); the reference sets both sd_pc and sd_one (aux.rs:1070-1073), which under pc_gate and one_gate forces
 *     pc = 1.
 * With the default table every produced row satisfies the 90 gates of tests/golden/exe_tempvar_gates.json.
 * Refusals (TRH_EINVAL), all with NOTHING written to dst; for a step, trh_last_error() names the FIRST offending step index:
 *   a step with an opcode the table does not know, ri, rj or a register operand >= reg_count, a pc, a, register or value >= 2^word_bits;
 *   a last step whose opcode is not 0b11111 (Answer);  m == 0 or m >= n;
 *   an unknown field, word_bits outside 2 .. 32, reg_count outside 1 .. 16, a table entry with an illegal source, a null array, a dst
 *     that is not 16-byte aligned, a word array that is not 4-byte aligned.
 * The stream travels in the struct, as in trh_mem_table_args_t.  A validation kernel runs first and the host reads its verdict -- the one
 * synchronisation of the entry, on args->stream; the row kernel is queued behind it and the entry returns without waiting for it.
 * trh_stat "exetable_rows": the m of the last call on this context that passed validation.                                                 */
enum { TRH_EXE_UNSET = 0, TRH_EXE_PC, TRH_EXE_PC_NEXT, TRH_EXE_PC_PLUS_ONE, TRH_EXE_REG_RI, TRH_EXE_REG_RJ, TRH_EXE_REG_NEXT_RI, TRH_EXE_A, TRH_EXE_VALUE,
       TRH_EXE_ZERO, TRH_EXE_ONE, TRH_EXE_MAX_WORD, TRH_EXE_NONDET = 16 /* + rule */ };
enum { TRH_EXE_RULE_REM = 0, TRH_EXE_RULE_QUOT, TRH_EXE_RULE_CMP_GT, TRH_EXE_RULE_CMP_GE, TRH_EXE_RULE_MUL_HI, TRH_EXE_RULE_MUL_LO, TRH_EXE_RULE_SMUL_LO,
       TRH_EXE_RULE_XOR, TRH_EXE_RULE_SHL_HI, TRH_EXE_RULE_SHR_LO, TRH_EXE_RULE_PC_PLUS_ONE, TRH_EXE_RULES };
#define TRH_EXE_UNKNOWN 0xFFFFFFFFu
#define TRH_EXE_ENTRY(a, b, c, d) ((uint32_t)(a) | (uint32_t)(b) << 8 | (uint32_t)(c) << 16 | (uint32_t)(d) << 24)
typedef struct trh_exe_table_args {
    uint32_t word_bits;                        /* 2 .. 32 */
    uint32_t reg_count;                        /* 1 .. 16 */
    const uint32_t *pc, *inst, *a, *value;     /* device, m each, in execution order */
    const uint32_t *regs;                      /* device, m x reg_count, step-major */
    const uint32_t *flag_bits;                 /* device, ceil(m / 32) words */
    size_t m;
    uint32_t selection[32];                    /* by opcode: TRH_EXE_ENTRY(a, b, c, d) or TRH_EXE_UNKNOWN */
    void*  dst;                                /* device, (28 + 9 reg_count) x n x 4 u64, 16-byte aligned, canonical Montgomery words */
    size_t n;                                  /* rows per column, > m */
    void*  stream;
} trh_exe_table_args_t;
int trh_exe_table_dev(int field_id, trh_exe_table_args_t* args);

/* ---- the Exe chips: Out, the changed flags and the sub-chips' advice, on the device ---------------------------------------------------------
 * The rest of what ExeChip::assign_trace (exe.rs:849-1067) writes per row: the Out selectors, ChangedSelectors, and the intermediates of the
 * logic, ssum, sprod, shift and flag2 - flag4 chips.  They are functions of the row's a, b, c, d, of the SUCCESSOR's flag (flag', 0 behind
 * the last step) and of a second per-opcode table.  The step arrays, selection and their rules are those of trh_exe_table_args_t; the entry
 * derives a, b, c, d itself, reads no column of trh_exe_table_dev, and the two can run in either order.
 * chips[opcode] is DATA like selection[opcode]: TRH_CHIP_* bits, or TRH_EXE_UNKNOWN.  Bits 0 - 12 are the reference's Out in Out::new order
 * (and xor or sum prod ssum sprod mod shift flag1 flag2 flag3 flag4), bit 13 is b_flag (flag4 reads the top bit of b: a left shift), bits
 * 14 - 16 are ch_pc, ch_flag, ch_reg[ri].  The default table (exetable.DEFAULT_CHIPS, trh::exe_default_chips) restates out.rs:148-349 and
 * the `ch:` fields of aux.rs:109-396.
 * dst: 52 + reg_count columns of n rows, cells as in trh_exe_table_dev, rows m .. n - 1 WRITTEN as zero:
 *   out_and out_xor out_or out_sum out_prod out_ssum out_sprod out_mod out_shift out_flag1 out_flag2 out_flag3 out_flag4
 *   ch_reg[reg_count] ch_pc ch_flag
 *   a_even a_odd b_even b_odd c_even c_odd d_even d_odd          one decomposition per variable (the reference allocates a's twice: bind
 *                                                                the same column twice)
 *   es_word es_even es_odd os_word os_even os_odd                logic: a_even + b_even, a_odd + b_odd, and their halves
 *   sg_a_msb sg_a_sigma sg_a_check sg_a_check_even sg_a_check_odd, the same for sg_b_ and sg_c_
 *   r_word r_even r_odd | a_shift a_power | a_flag | lsb_b b_flag
 * A cell is computed on a row whose chips entry has one of the cell's enabling bits and is ZERO elsewhere (the reference fills with
 * 2^64 - 1):
 *   a halves   mod and or xor ssum sprod            even / odd bits of a         b halves   mod sum ssum sprod flag4 and xor or
 *   c halves   xor prod shift ssum sprod                                         d halves   prod sprod
 *   es_*, os_* and xor or
 *   sg_a_*     ssum sprod     msb = bit W - 1, sigma = |a as a signed word|, check = a_odd + (1 - 2 msb) 2^(W - 2), check's halves
 *   sg_b_*     sprod flag4                          sg_c_*     ssum sprod
 *   r_*        flag3: c == 0 ? 0 : c - a - 1        shift: a > W ? 0 : W - a
 *   a_shift, a_power   shift: a > W; 2^min(a, W) (0 for a negative a)
 *   a_flag     flag2: the inverse of c + flag' in the field, 0 when c + flag' = 0
 *   lsb_b, b_flag      flag4: b & 1; bit 13 of the entry
 * a .. d are the signed integers of trh_exe_table_dev's rules (SHR_LO can be negative, pc + 1 can be 2^W).  A _word cell carries the
 * integer, a negative one as m - |v|; halves, msb, sigma and check come from an input that is a word (0 <= v < 2^W), otherwise all cells of
 * that group are zero.  VM semantics are not checked.
 * Two departures from the reference:
 *   saturated shifts  assign_shift writes a_power = 0 at A == W and overflows 2u64.pow above; with its own c, d the gate
 *     a_power b - d - 2^W c then fails at A == W.  Here a_power = 2^min(a, W), which with SHL_HI / SHR_LO's s = min(A, W) satisfies the gate
 *     for every A; the pow lookup table that goes with it carries (W, 2^W) where pow.rs:58-62 has (W, 0);
 *   a_flag  the reference inverts on every row and draws a random value when c + flag' = 0; here flag2 rows only, and 0 there.
 * Refusals (TRH_EINVAL, nothing written to dst): everything trh_exe_table_dev refuses, in its words; word_bits odd (the signed check puts
 * the sign at an odd bit, the even-bits table has 2^(W/2) rows); a chips entry, named by its opcode, with a bit above 16, with flag3 and
 * shift together (they share r_*), with bit 13 and no flag4, or known where selection's is unknown or the other way round.
 * One synchronisation, as in trh_exe_table_dev: the verdict on the steps; the row kernel and the inversion of the a_flag column (one field
 * inversion per strip of rows, Montgomery's trick) are queued behind it.  trh_stat "exechips_rows": the m of the last call that passed
 * validation; "exechips_flag2_rows": the flag2 rows its inversion kernel visited.
 * Measured on an MI355X at k = 18, reg_count = 8, word_bits = 32 (profiles/exechips_probe.txt): the entry 0.347 ms, 4.31 times a fill of
 * its 503 MB; the row kernel alone 1.35 times the fill; the inversion 0.186 ms of the entry -- alone 87, 28 and 27 times the fill of its
 * column at strips of 1, 4 and 8 rows per lane, the latency of one field inversion from a strip of 4 on.                                */
enum { TRH_CHIP_AND = 1 << 0, TRH_CHIP_XOR = 1 << 1, TRH_CHIP_OR = 1 << 2, TRH_CHIP_SUM = 1 << 3, TRH_CHIP_PROD = 1 << 4, TRH_CHIP_SSUM = 1 << 5,
       TRH_CHIP_SPROD = 1 << 6, TRH_CHIP_MOD = 1 << 7, TRH_CHIP_SHIFT = 1 << 8, TRH_CHIP_FLAG1 = 1 << 9, TRH_CHIP_FLAG2 = 1 << 10, TRH_CHIP_FLAG3 = 1 << 11,
       TRH_CHIP_FLAG4 = 1 << 12, TRH_CHIP_B_FLAG = 1 << 13, TRH_CHIP_CH_PC = 1 << 14, TRH_CHIP_CH_FLAG = 1 << 15, TRH_CHIP_CH_REG = 1 << 16 };
typedef struct trh_exe_chips_args {
    uint32_t word_bits;                        /* even, 2 .. 32 */
    uint32_t reg_count;                        /* 1 .. 16 */
    const uint32_t *pc, *inst, *a, *value;     /* device, m each, in execution order */
    const uint32_t *regs;                      /* device, m x reg_count, step-major */
    const uint32_t *flag_bits;                 /* device, ceil(m / 32) words */
    size_t m;
    uint32_t selection[32];                    /* by opcode: TRH_EXE_ENTRY(a, b, c, d) or TRH_EXE_UNKNOWN */
    uint32_t chips[32];                        /* by opcode: TRH_CHIP_* bits or TRH_EXE_UNKNOWN */
    void*  dst;                                /* device, (52 + reg_count) x n x 4 u64, 16-byte aligned, canonical Montgomery words */
    size_t n;                                  /* rows per column, > m */
    void*  stream;
} trh_exe_chips_args_t;
int trh_exe_chips_dev(int field_id, trh_exe_chips_args_t* args);

/* ---- element-wise field / group ops on device memory (parity tests of the device arithmetic;
 *      op: 0 add, 1 sub, 2 mul, 3 sqr, 4 neg, 5 inv, 6 to_mont, 7 from_mont) ------------------ */
int trh_field_op_dev(int field, int op, const void* a_dev, const void* b_dev, void* out_dev, size_t n, void* stream);
/* op: 0 out = p + q (both Jacobian 12 x u64), 1 out = p + q (q affine 8 x u64), 2 out = 2p; 3 / 4: p + q / 2p through the quad-lane
 * arithmetic of the small MSMs' bucket reduction (csrc/curve_q4.h); out Jacobian normalised */
int trh_point_op_dev(int curve, int op, const void* p_dev, const void* q_dev, void* out_dev, size_t n, void* stream);

/* ---- plain device memory helpers so that non-HIP hosts (Rust, ctypes) can stage buffers ----
 * trh_free keeps freed blocks for reuse by trh_malloc (per device, by rounded size; it returns when the device has drained, as
 * hipFree does): at most `pool_mb` MiB (trh_set_option / TRH_POOL_MB, default 4096; 0 switches the pool off), evicting the device's largest idle
 * blocks first.  The idle blocks are invisible to any other allocator in the process (torch's caching allocator, say): libtrh
 * returns them when one of its own allocations fails, and trh_pool_trim() returns them on request.  Freeing a block twice is
 * reported (TRH_EINVAL) while it still waits in the pool. */
int trh_malloc(void** dev, size_t bytes);
int trh_free(void* dev);
int trh_pool_trim(void);
size_t trh_pool_idle_bytes(void);
int trh_memcpy_h2d(void* dev, const void* host, size_t bytes);
int trh_memcpy_d2h(void* host, const void* dev, size_t bytes);
int trh_stream_synchronize(void* stream);
/* counters of the calling thread's context, by name.  "msm_lean_retries": MSMs of callers that vouched for uniformly random scalars (the
 * opening's rounds) whose whole-bin LDS sort met a bin that did not fit and that were therefore run a second time with the chunked passes;
 * "msm_lean_sorts": the MSMs enqueued that way so far, without the chunked passes behind the LDS sort (cumulative; a retry is not one), and
 * "msm_quad_combines": the launches of the combine's quad form, which only such callers get (cumulative; for tests, like the one before);
 * "msm_bin_sorted_windows": of the last MSM's last chunk of items, the (item, window) bucket sets whose level-1 bins all fit the LDS
 * bin sort (0 when that MSM did not use it; synchronises the device, for tests);
 * "msm_small_launches": MSMs that ran as ONE launch (up to 8448 pairs, batches of up to four); "ipa_generator_collapses": openings that
 * collapsed their generators from the fixed-base table (option ipa_fold);
 * "msm_chunks": the launch sets every pipeline MSM on this context ran as so far (cumulative): a batch goes through one set of launches
 * `chunk` items at a time -- at most 64, fewer where option msm_chunk_gb cuts it -- so a batch adds ceil(batch / chunk), a one-launch MSM none;
 * "msm_unit_chunks": of those, the chunks over a fixed-base table whose columns were still unanimously flag-like after their entries were
 * emitted and which therefore took the unit path (cumulative);
 * "msm_host_ranges": the ranges the last MSM with host scalars (trh_best_multiexp_*, trh_msm) on this context was cut into -- host bases: one up
 * to 2^21 pairs, equal ranges of about 2^20 above; resident bases: one up to 3 * 2^21 pairs, then 2^21, 2^22 and the rest;
 * "msm_range_tiles": the tiles of the last MSM enqueue on this context that ran as range tiles of at most 2^25 pairs (0 when it did not);
 * "ntt_tableless_passes": of the last transform, the passes after the first that had no inter-pass twiddle table and computed their twiddles
 * per element (1 from 2^26 elements, where the last pass's table would exceed 1.125 GiB; 0 below);
 * "lookup_check_probes": the slots of the set visited by the two kernels (insert, probe) of the last trh_lookup_check_dev on this context;
 * "memtable_rows", "memtable_sort_passes", "memtable_tiles": the last trh_mem_table_dev on this context (described with that entry);
 * "exetable_rows": the steps of the last trh_exe_table_dev on this context that passed validation;
 * "exechips_rows": the same of trh_exe_chips_dev; "exechips_flag2_rows": the rows with the flag2 bit that the inversion kernel of the last
 * trh_exe_chips_dev on this context visited (synchronises the device, for tests). */
int trh_stat(const char* name, uint64_t* value);
/* GPU-side timing without HIP headers: events recorded on a stream between the steps (a hipEvent_t each), read afterwards.
 * trh_event_elapsed_ms waits for `end` and returns the device time between the two records. */
int trh_event_create(void** out_event);
int trh_event_record(void* event, void* stream);
int trh_event_elapsed_ms(void* start, void* end, float* ms);
void trh_event_destroy(void* event);

/* ---- timing of the last MSM / NTT on this context (HIP events on the launch stream) -------- */
typedef struct trh_timing {
    float total_ms;        /* first kernel start -> last kernel end */
    float digits_ms;       /* MSM: scalar recode + histogram */
    float sort_ms;         /* MSM: bucket offsets + scatter */
    float accumulate_ms;   /* MSM: bucket accumulation (the dominant kernel) */
    float reduce_ms;       /* MSM: bucket reduction + window sums */
    int window_bits;
    int windows;
    float accumulate_kernel_ms; /* msm_accumulate_seg_kernel alone (accumulate_ms also covers the per-bucket combine) */
} trh_timing_t;
int trh_set_timing(int enabled);
int trh_last_timing(trh_timing_t* out);

#ifdef __cplusplus
}
#endif
#endif /* TRH_H */
