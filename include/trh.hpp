// trh.hpp -- C++17 host side over the C ABI of libtrh.so (include/trh.h), header-only.
//
// The reference is compiled Rust and the build image has no Rust toolchain, so the host layer a maintainer would
// write in the halo2_proofs fork is mirrored here in C++ with the reference's names, argument
// meaning and failure behaviour (the Rust functions panic on a violated precondition; these throw trh::Error):
//
//   trh::best_multiexp / trh::best_fft      halo2_proofs::arithmetic::{best_multiexp, best_fft}
//   trh::Params                             poly::commitment::Params  { commit, commit_lagrange } (+ device batch forms)
//   trh::EvaluationDomain                   poly::EvaluationDomain    { lagrange_to_coeff, coeff_to_extended,
//                                                                      extended_to_coeff, divide_by_vanishing_poly }
//   trh::Expression + compile_gates         plonk::Expression<F> and the y-folded evaluation of the gate polynomials
//   trh::ipa_create_proof                   poly::commitment::create_proof (IPA opening)
//   trh::IpaMsm                             poly::commitment::msm::MSM + Guard::use_challenges (the verifier's accumulator)
//   trh::Rng                                `C::Scalar::random(rng)` for whole vectors: a ChaCha20 seed expanded on the device
//   trh::PermutationAssembly                plonk::permutation::keygen::Assembly { copy, build_vk, build_pk } (+ the copy-constraint check)
//   trh::Blake2bWrite / trh::Blake2bRead    transcript::{Blake2bWrite, Blake2bRead} with Challenge255: the proof as bytes (host only)
//
// Reference call sites of all of these: /root/reference/src/test_utils.rs:21-49, 89-104 (through keygen_* and
// create_proof of the halo2_proofs crate pinned at /root/reference/Cargo.lock:619-621).
// examples/replay.cpp is the native driver built on this header; tests/test_gpu_native.py runs it.
#ifndef TRH_HPP
#define TRH_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "trh.h"

namespace trh {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
inline void check(int rc, const char* what) {
    if (rc != TRH_OK) throw Error(std::string(what) + ": libtrh error " + std::to_string(rc) + ": " + trh_last_error());
}
inline void require(bool cond, const char* what) {  // the reference's assert! / assert_eq!
    if (!cond) throw Error(std::string("assertion failed: ") + what);
}

using Limbs = std::array<uint64_t, 4>;  // pasta_curves::Fp / Fq in memory: Montgomery form, little-endian limbs
struct Affine { Limbs x, y; };           // all-zero = identity (the Rust shim repacks pasta's flagged Affine)
struct Point { Limbs x, y, z; };         // pasta's Point layout, normalised to Z = 1 by libtrh
enum class Curve : int { Pallas = TRH_PALLAS, Vesta = TRH_VESTA };
enum class Field : int { Fp = TRH_FP, Fq = TRH_FQ };
inline Field scalar_field(Curve c) { return c == Curve::Pallas ? Field::Fq : Field::Fp; }
inline Field base_field(Curve c) { return c == Curve::Pallas ? Field::Fp : Field::Fq; }

// ---- a little host field arithmetic (constants of expressions, checks in the example driver) ---------------
namespace host {
using u128 = unsigned __int128;
inline const Limbs& modulus(Field f) {
    static const Limbs P{0x992d30ed00000001ull, 0x224698fc094cf91bull, 0, 0x4000000000000000ull};
    static const Limbs Q{0x8c46eb2100000001ull, 0x224698fc0994a8ddull, 0, 0x4000000000000000ull};
    return f == Field::Fp ? P : Q;
}
inline bool geq(const Limbs& a, const Limbs& b) {
    for (int i = 3; i >= 0; --i) if (a[i] != b[i]) return a[i] > b[i];
    return true;
}
inline Limbs sub_raw(const Limbs& a, const Limbs& b) {
    Limbs r; u128 br = 0;
    for (int i = 0; i < 4; ++i) { u128 d = (u128)a[i] - b[i] - br; r[i] = (uint64_t)d; br = (d >> 64) & 1; }
    return r;
}
inline Limbs add(Field f, const Limbs& a, const Limbs& b) {
    Limbs r; u128 c = 0;
    for (int i = 0; i < 4; ++i) { c += (u128)a[i] + b[i]; r[i] = (uint64_t)c; c >>= 64; }
    return geq(r, modulus(f)) ? sub_raw(r, modulus(f)) : r;  // a + b < 2m < 2^256
}
inline Limbs sub(Field f, const Limbs& a, const Limbs& b) {
    if (geq(a, b)) return sub_raw(a, b);
    Limbs t = sub_raw(modulus(f), b); return add(f, a, t);
}
inline Limbs neg(Field f, const Limbs& a) { return sub(f, Limbs{0, 0, 0, 0}, a); }
inline uint64_t neg_inv64(Field f) { return f == Field::Fp ? 0x992d30ecffffffffull : 0x8c46eb20ffffffffull; }  // -m^-1 mod 2^64 (m = 1 mod 2^32)
// Montgomery product a b / 2^256 mod m (CIOS)
inline Limbs mul(Field f, const Limbs& a, const Limbs& b) {
    const Limbs& m = modulus(f);
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        u128 c = 0;
        for (int j = 0; j < 4; ++j) { c += (u128)t[j] + (u128)a[i] * b[j]; t[j] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
        const uint64_t q = t[0] * neg_inv64(f);
        c = (u128)t[0] + (u128)q * m[0]; c >>= 64;
        for (int j = 1; j < 4; ++j) { c += (u128)t[j] + (u128)q * m[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
        c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64); t[5] = 0;
    }
    Limbs r{t[0], t[1], t[2], t[3]};
    return (t[4] || geq(r, m)) ? sub_raw(r, m) : r;
}
inline Limbs one(Field f) {  // R mod m = 2^256 - m * floor(2^256 / m) = 2^256 - 3m for these moduli (m just above 2^254)
    const Limbs& m = modulus(f);
    Limbs z{0, 0, 0, 0}, r = sub_raw(z, m); r = sub_raw(r, m); r = sub_raw(r, m);
    return r;
}
// a^(m - 2) (Fermat); inv(0) = 0
inline Limbs inv(Field f, const Limbs& a) {
    Limbs e = modulus(f);
    e[0] -= 2;  // the low limbs of both moduli are far above 2: no borrow
    Limbs r = one(f);
    for (int i = 255; i >= 0; --i) {
        r = mul(f, r, r);
        if ((e[i / 64] >> (i % 64)) & 1) r = mul(f, r, a);
    }
    return r;
}
inline Limbs from_u64(Field f, uint64_t v) {  // v * R: double-and-add on the Montgomery one
    Limbs acc{0, 0, 0, 0}, base = one(f);
    for (int i = 0; i < 64; ++i) { if ((v >> i) & 1) acc = add(f, acc, base); base = add(f, base, base); }
    return acc;
}
}  // namespace host

// ---- halo2_proofs::arithmetic -------------------------------------------------------------------------------
inline Point best_multiexp(Curve c, const std::vector<Limbs>& coeffs, const std::vector<Affine>& bases) {
    require(coeffs.size() == bases.size(), "coeffs.len() == bases.len()");
    Point out;
    const auto fn = c == Curve::Pallas ? trh_best_multiexp_pallas : trh_best_multiexp_vesta;
    check(fn((const uint64_t*)coeffs.data(), (const uint64_t*)bases.data(), coeffs.size(), (uint64_t*)&out), "best_multiexp");
    return out;
}
inline void best_fft(Field f, std::vector<Limbs>& a, const Limbs& omega, uint32_t log_n) {
    require(a.size() == (size_t)1 << log_n, "a.len() == 1 << log_n");
    const auto fn = f == Field::Fp ? trh_best_fft_fp : trh_best_fft_fq;
    check(fn((uint64_t*)a.data(), omega.data(), log_n), "best_fft");
}

// the same over a batch of host slices with one omega (pipelined over PCIe)
inline void best_fft_batch(Field f, std::vector<std::vector<Limbs>*>& columns, const Limbs& omega, uint32_t log_n) {
    std::vector<uint64_t*> ptrs;
    for (auto* c : columns) { require(c->size() == (size_t)1 << log_n, "a.len() == 1 << log_n"); ptrs.push_back((uint64_t*)c->data()); }
    check((f == Field::Fp ? trh_best_fft_batch_fp : trh_best_fft_batch_fq)(ptrs.data(), ptrs.size(), omega.data(), log_n), "best_fft_batch");
}

// ---- device memory -------------------------------------------------------------------------------------------
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t bytes) : bytes_(bytes) { check(trh_malloc(&p_, bytes ? bytes : 16), "trh_malloc"); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }
    ~DeviceBuffer() { if (p_) (void)trh_free(p_); }
    void* data() const { return p_; }
    void* at(size_t byte_offset) const { return (char*)p_ + byte_offset; }
    size_t size() const { return bytes_; }
    void upload(const void* host, size_t bytes, size_t offset = 0) { require(offset + bytes <= bytes_, "upload range"); check(trh_memcpy_h2d(at(offset), host, bytes), "h2d"); }
    void download(void* host, size_t bytes, size_t offset = 0) const { require(offset + bytes <= bytes_, "download range"); check(trh_memcpy_d2h(host, at(offset), bytes), "d2h"); }
private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// ---- poly::commitment::Params ---------------------------------------------------------------------------------
class Bases {
public:
    Bases() = default;
    Bases(Curve c, const std::vector<Affine>& xy) {
        check((c == Curve::Pallas ? trh_bases_create_pallas : trh_bases_create_vesta)((const uint64_t*)xy.data(), xy.size(), &h_), "bases_create");
    }
    // n x 32-byte compressed points (pasta `to_bytes`) in host memory, decoded on the device; Error names the first invalid encoding
    static Bases from_compressed(Curve c, const uint8_t* bytes, size_t n) { Bases b; check(trh_bases_create_compressed((int)c, bytes, n, &b.h_), "bases_create_compressed"); return b; }
    static Bases generate(Curve c, uint64_t s0, uint64_t d, size_t n) { Bases b; check(trh_bases_generate((int)c, s0, d, 0, n, &b.h_), "bases_generate"); return b; }
    Bases(const Bases&) = delete;
    Bases& operator=(const Bases&) = delete;
    Bases(Bases&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Bases& operator=(Bases&& o) noexcept { std::swap(h_, o.h_); return *this; }
    ~Bases() { if (h_) trh_bases_destroy(h_); }
    trh_bases_t handle() const { return h_; }
    size_t len() const { return trh_bases_len(h_); }
    int precompute(int window_bits = 0) { check(trh_bases_precompute(h_, window_bits), "bases_precompute"); return trh_bases_precomputed_window_bits(h_); }
    // setup-time: the calling context's MSM scratch for batches of `batch` MSMs over the first n bases (the first batch then allocates nothing)
    void reserve(size_t n, size_t batch) const { check(trh_bases_reserve(h_, n, batch), "bases_reserve"); }
    std::vector<Affine> download() const { std::vector<Affine> v(len()); check(trh_bases_download(h_, 0, v.size(), (uint64_t*)v.data()), "bases_download"); return v; }
    std::vector<Affine> download(size_t offset, size_t n) const { std::vector<Affine> v(n); check(trh_bases_download(h_, offset, n, (uint64_t*)v.data()), "bases_download"); return v; }
    std::vector<uint8_t> download_compressed(size_t offset, size_t n) const {
        std::vector<uint8_t> v(32 * n); check(trh_bases_download_compressed(h_, offset, n, v.data()), "bases_download_compressed"); return v;
    }
    Point msm(const std::vector<Limbs>& scalars, size_t offset = 0) const {
        Point out; check(trh_msm(h_, offset, (const uint64_t*)scalars.data(), scalars.size(), 1, (uint64_t*)&out), "msm"); return out;
    }
private:
    trh_bases_t h_ = nullptr;
};

class Params {
public:
    // g, g_lagrange: n = 2^k points each; w, u as in commitment::Params.  Both base sets are kept resident with w appended.
    Params(Curve c, uint32_t k, std::vector<Affine> g, std::vector<Affine> g_lagrange, const Affine& w, const Affine& u, bool fixed_base_tables = true)
        : curve(c), k(k), n((size_t)1 << k), w(w), u(u) {
        require(g.size() == n && g_lagrange.size() == n, "g.len() == g_lagrange.len() == 1 << k");
        g.push_back(w); g_lagrange.push_back(w);
        g_ = Bases(c, g); g_lagrange_ = Bases(c, g_lagrange);
        if (fixed_base_tables) precompute();
    }
    // synthetic resident generators (the example driver / benchmarks): (s0 + i d) G
    Params(Curve c, uint32_t k, uint64_t s0, uint64_t d, bool fixed_base_tables = true) : curve(c), k(k), n((size_t)1 << k) {
        g_ = Bases::generate(c, s0, d, n + 1); g_lagrange_ = Bases::generate(c, s0 + 77, d + 2, n + 1);
        const auto gh = g_.download(); w = gh[n]; u = Bases::generate(c, 4242, 1, 1).download()[0];
        if (fixed_base_tables) precompute();
    }
    // Params::read / Params::write (halo2_proofs 0.2.0 poly/commitment.rs): k as u32 little endian, then g[0 .. n), g_lagrange[0 .. n), w, u as
    // 32-byte compressed points.  read sends the encodings to the device as they are and decodes them there (no host square roots, 32 bytes per
    // point over the link); an invalid encoding or a short file throws Error.
    static Params read(Curve c, const std::vector<uint8_t>& file, bool fixed_base_tables = true) {
        require(file.size() >= 4, "Params::read: the file holds k");
        const uint32_t k = (uint32_t)file[0] | (uint32_t)file[1] << 8 | (uint32_t)file[2] << 16 | (uint32_t)file[3] << 24;
        require(k <= 30, "Params::read: k <= 30");
        Params p;
        p.curve = c; p.k = k; p.n = (size_t)1 << k;
        const size_t n = p.n;
        require(file.size() >= 4 + 32 * (2 * n + 2), "Params::read: the file holds 2 n + 2 points");
        const uint8_t *g = file.data() + 4, *gl = g + 32 * n, *w = gl + 32 * n, *u = w + 32;
        std::vector<uint8_t> set(g, g + 32 * n);   // g || w
        set.insert(set.end(), w, w + 32);
        p.g_ = Bases::from_compressed(c, set.data(), n + 1);
        std::copy(gl, gl + 32 * n, set.begin());     // g_lagrange || w
        p.g_lagrange_ = Bases::from_compressed(c, set.data(), n + 1);
        p.w = p.g_.download(n, 1)[0];
        check(trh_point_from_bytes((int)c, u, (uint64_t*)&p.u), "Params::read: u");
        if (fixed_base_tables) {
            for (Bases* b : {&p.g_, &p.g_lagrange_}) { try { b->precompute(0); } catch (const Error&) { /* outside the table range: per-window path */ } }
            try {
                std::copy(g, g + 32 * n, set.begin());   // g || w || u
                set.insert(set.end(), u, u + 32);
                Bases b = Bases::from_compressed(c, set.data(), n + 2);
                b.precompute(0);
                p.ipa_ = std::move(b);
            } catch (const Error&) { /* the opening uses g || w and the per-window path */ }
        }
        return p;
    }
    // Params::new(k): g[i] = hash_to_curve("Halo2-Parameters")(00 || le32(i)) on the device, g_lagrange = n^-1 * best_fft(g, omega^-1) by the
    // point FFT, w and u (messages 01 and 02) from the host entry; then as the first constructor
    static Params create(Curve c, uint32_t k, bool fixed_base_tables = true) {
        require(k <= 24, "Params::create: k <= 24 (the point FFT's range)");
        static const char prefix[] = "Halo2-Parameters";
        const size_t n = (size_t)1 << k;
        std::vector<Affine> g(n), gl(n);
        {
            DeviceBuffer pts(n * sizeof(Affine));
            check(trh_hash_to_curve_indexed_dev((int)c, prefix, 0, 0, n, pts.data(), nullptr), "hash_to_curve_indexed_dev");
            pts.download(g.data(), n * sizeof(Affine));
            trh_domain_t d = nullptr;
            check(trh_domain_create((int)scalar_field(c), 2, k, &d), "domain_create");
            Limbs omega_inv, n_inv;
            const int rc = trh_domain_constant(d, 1, omega_inv.data()) | trh_domain_constant(d, 4, n_inv.data());
            trh_domain_destroy(d);
            check(rc, "domain_constant");
            check(trh_point_fft_dev((int)c, pts.data(), k, omega_inv.data(), n_inv.data(), nullptr), "point_fft_dev");
            pts.download(gl.data(), n * sizeof(Affine));
        }
        Affine w, u;
        const uint8_t m1 = 1, m2 = 2;
        check(trh_hash_to_curve((int)c, prefix, &m1, 1, (uint64_t*)&w), "hash_to_curve");
        check(trh_hash_to_curve((int)c, prefix, &m2, 1, (uint64_t*)&u), "hash_to_curve");
        return Params(c, k, std::move(g), std::move(gl), w, u, fixed_base_tables);
    }
    std::vector<uint8_t> write() const {
        std::vector<uint8_t> out{(uint8_t)k, (uint8_t)(k >> 8), (uint8_t)(k >> 16), (uint8_t)(k >> 24)};
        for (const Bases* b : {&g_, &g_lagrange_}) { const auto e = b->download_compressed(0, n); out.insert(out.end(), e.begin(), e.end()); }
        const auto we = g_.download_compressed(n, 1);
        out.insert(out.end(), we.begin(), we.end());
        const bool u_identity = u.x == Limbs{0, 0, 0, 0} && u.y == Limbs{0, 0, 0, 0};
        const Point up{u.x, u.y, u_identity ? Limbs{0, 0, 0, 0} : host::one(base_field(curve))};
        uint8_t ue[32];
        check(trh_point_to_bytes((int)curve, (const uint64_t*)&up, ue), "point_to_bytes");
        out.insert(out.end(), ue, ue + 32);
        return out;
    }
    void precompute() {
        for (Bases* b : {&g_, &g_lagrange_}) { try { b->precompute(0); } catch (const Error&) { /* outside the table range: per-window path */ } }
        // the opening's base set g || w || u with its own table: every MSM of trh_ipa_create_proof then runs in fixed-base mode
        try {
            std::vector<Affine> gwu = g_.download();
            gwu.push_back(u);
            Bases b(curve, gwu);
            b.precompute(0);
            ipa_ = std::move(b);
        } catch (const Error&) { /* the opening uses g || w and the per-window path */ }
    }
    Point commit(const std::vector<Limbs>& poly, const Limbs& blind) const { return commit_host(g_, poly, blind); }
    Point commit_lagrange(const std::vector<Limbs>& poly, const Limbs& blind) const { return commit_host(g_lagrange_, poly, blind); }
    // `batch` polynomials of n coefficients back to back in device memory
    std::vector<Point> commit_batch(const DeviceBuffer& polys, size_t batch, const std::vector<Limbs>& blinds, void* stream = nullptr) const { return commit_dev(g_, polys, batch, blinds, stream); }
    std::vector<Point> commit_lagrange_batch(const DeviceBuffer& polys, size_t batch, const std::vector<Limbs>& blinds, void* stream = nullptr) const { return commit_dev(g_lagrange_, polys, batch, blinds, stream); }
    // the same for polynomials in HOST memory, one vector per column (trh_commit_batch_host: chunked uploads under the MSMs)
    std::vector<Point> commit_batch_host(const std::vector<const std::vector<Limbs>*>& polys, const std::vector<Limbs>& blinds) const { return commit_hosts(g_, polys, blinds); }
    std::vector<Point> commit_lagrange_batch_host(const std::vector<const std::vector<Limbs>*>& polys, const std::vector<Limbs>& blinds) const { return commit_hosts(g_lagrange_, polys, blinds); }
    const Bases& g() const { return g_; }
    const Bases& g_lagrange() const { return g_lagrange_; }
    const Bases& ipa_bases() const { return ipa_.handle() ? ipa_ : g_; }  // g || w || u with tables when precompute() built it
    // setup-time sizing of the calling context's scratch for commit batches of `batch` columns and for the opening's round MSMs
    void reserve(size_t batch) const {
        g_.reserve(n + 1, batch);
        g_lagrange_.reserve(n + 1, batch);
        if (ipa_.handle()) ipa_.reserve(n + 2, 2);
    }

    Curve curve;
    uint32_t k;
    size_t n;
    Affine w{}, u{};
private:
    Params() : curve(Curve::Pallas), k(0), n(1) {}  // filled by read()
    Point commit_host(const Bases& b, const std::vector<Limbs>& poly, const Limbs& blind) const {
        require(poly.size() == n, "poly.len() == params.n");
        std::vector<Limbs> sc(poly); sc.push_back(blind);
        return b.msm(sc);
    }
    std::vector<Point> commit_hosts(const Bases& b, const std::vector<const std::vector<Limbs>*>& polys, const std::vector<Limbs>& blinds) const {
        require(blinds.size() == polys.size(), "one blind per polynomial");
        std::vector<const uint64_t*> ptrs;
        for (const auto* p : polys) { require(p->size() == n, "poly.len() == params.n"); ptrs.push_back((const uint64_t*)p->data()); }
        std::vector<Point> out(polys.size());
        check(trh_commit_batch_host(b.handle(), ptrs.data(), n, ptrs.size(), (const uint64_t*)blinds.data(), (uint64_t*)out.data()), "commit_batch_host");
        return out;
    }
    std::vector<Point> commit_dev(const Bases& b, const DeviceBuffer& polys, size_t batch, const std::vector<Limbs>& blinds, void* stream) const {
        require(blinds.size() == batch && polys.size() >= batch * n * 32, "batch x n coefficients and one blind per polynomial");
        std::vector<Point> out(batch);
        check(trh_commit_batch_dev(b.handle(), polys.data(), n, batch, (const uint64_t*)blinds.data(), stream, (uint64_t*)out.data()), "commit_batch");
        return out;
    }
    Bases g_, g_lagrange_, ipa_;
};

// ---- poly::EvaluationDomain -----------------------------------------------------------------------------------
class EvaluationDomain {
public:
    EvaluationDomain(Field f, uint32_t j, uint32_t k) : field(f), k(k), n((size_t)1 << k) { check(trh_domain_create((int)f, j, k, &d_), "EvaluationDomain::new"); extended_k = trh_domain_extended_k(d_); }
    EvaluationDomain(const EvaluationDomain&) = delete;
    EvaluationDomain& operator=(const EvaluationDomain&) = delete;
    ~EvaluationDomain() { if (d_) trh_domain_destroy(d_); }
    size_t extended_len() const { return (size_t)1 << extended_k; }
    // setup-time: tables and scratch of the per-column transforms for batches of `batch` polynomials on the calling context
    void reserve(size_t batch) const { check(trh_domain_reserve(d_, batch), "domain_reserve"); }
    Limbs constant(int which) const { Limbs v; check(trh_domain_constant(d_, which, v.data()), "domain_constant"); return v; }
    Limbs get_omega() const { return constant(0); }
    Limbs get_extended_omega() const { return constant(2); }
    // batch x 2^k (or 2^extended_k) elements, back to back in device memory
    void lagrange_to_coeff(void* a_dev, size_t batch, void* stream = nullptr) const { check(trh_domain_lagrange_to_coeff(d_, a_dev, batch, stream), "lagrange_to_coeff"); }
    void coeff_to_extended(const void* coeff_dev, void* ext_dev, size_t batch, void* stream = nullptr) const { check(trh_domain_coeff_to_extended(d_, coeff_dev, ext_dev, batch, stream), "coeff_to_extended"); }
    void extended_to_coeff(void* a_dev, size_t batch, void* stream = nullptr) const { check(trh_domain_extended_to_coeff(d_, a_dev, batch, stream), "extended_to_coeff"); }
    void divide_by_vanishing_poly(void* a_dev, size_t batch, void* stream = nullptr) const { check(trh_domain_divide_by_vanishing_poly(d_, a_dev, batch, stream), "divide_by_vanishing_poly"); }

    // the extended domain as coset blocks (trh.h): n_blocks x 2^k values per polynomial, block r entry q = coeff_to_extended's entry
    // q * 2^(extended_k - k) + r; the quotient needs quotient_blocks() = j - 1 of them
    uint32_t quotient_blocks() const { return trh_domain_quotient_blocks(d_); }
    void coeff_to_extended_blocks(const void* coeff_dev, void* ext_dev, size_t batch, uint32_t n_blocks, void* stream = nullptr) const {
        check(trh_domain_coeff_to_extended_blocks(d_, coeff_dev, ext_dev, batch, n_blocks, stream), "coeff_to_extended_blocks");
    }
    void blocks_to_quotient(void* num_blocks_dev, void* h_coeff_dev, bool divide_by_vanishing = true, void* stream = nullptr) const {
        check(trh_domain_blocks_to_quotient(d_, num_blocks_dev, h_coeff_dev, divide_by_vanishing ? 1 : 0, stream), "blocks_to_quotient");
    }
    // host polynomials, one vector per column (pipelined over PCIe): lagrange_to_coeff in place; coeff_to_extended 2^k -> 2^extended_k;
    // extended_to_coeff in place on one polynomial, optionally preceded by divide_by_vanishing_poly (the caller truncates)
    void lagrange_to_coeff_host(std::vector<std::vector<Limbs>*>& cols) const {
        std::vector<uint64_t*> ptrs;
        for (auto* c : cols) { require(c->size() == n, "a.len() == 1 << k"); ptrs.push_back((uint64_t*)c->data()); }
        check(trh_domain_lagrange_to_coeff_host(d_, ptrs.data(), ptrs.size()), "lagrange_to_coeff_host");
    }
    void coeff_to_extended_host(const std::vector<const std::vector<Limbs>*>& coeff, std::vector<std::vector<Limbs>*>& ext) const {
        require(coeff.size() == ext.size(), "one output per input");
        std::vector<const uint64_t*> in;
        std::vector<uint64_t*> out;
        for (const auto* c : coeff) { require(c->size() == n, "a.len() == 1 << k"); in.push_back((const uint64_t*)c->data()); }
        for (auto* e : ext) { require(e->size() == extended_len(), "ext.len() == 1 << extended_k"); out.push_back((uint64_t*)e->data()); }
        check(trh_domain_coeff_to_extended_host(d_, in.data(), out.data(), in.size()), "coeff_to_extended_host");
    }
    void extended_to_coeff_host(std::vector<Limbs>& a, bool divide_by_vanishing_first = false) const {
        require(a.size() == extended_len(), "a.len() == 1 << extended_k");
        check(trh_domain_extended_to_coeff_host(d_, (uint64_t*)a.data(), divide_by_vanishing_first ? 1 : 0), "extended_to_coeff_host");
    }

    trh_domain_t handle() const { return d_; }

    Field field;
    uint32_t k, extended_k = 0;
    size_t n;
private:
    trh_domain_t d_ = nullptr;
};

// ---- plonk::Expression<F> --------------------------------------------------------------------------------------
struct Expression;
using Expr = std::shared_ptr<const Expression>;
struct Expression {
    enum Kind { Constant, Selector, Fixed, Advice, Instance, Negated, Sum, Product, Scaled } kind;
    Limbs value{};      // Constant, Scaled
    uint32_t column = 0;
    int32_t rotation = 0;
    Expr a, b;
    int degree() const {
        switch (kind) {
            case Constant: return 0;
            case Selector: case Fixed: case Advice: case Instance: return 1;
            case Negated: case Scaled: return a->degree();
            case Sum: return std::max(a->degree(), b->degree());
            default: return a->degree() + b->degree();
        }
    }
};
inline Expr constant(const Limbs& v) { auto e = std::make_shared<Expression>(); e->kind = Expression::Constant; e->value = v; return e; }
inline Expr query(Expression::Kind k, uint32_t column, int32_t rotation = 0) { auto e = std::make_shared<Expression>(); e->kind = k; e->column = column; e->rotation = rotation; return e; }
inline Expr advice(uint32_t c, int32_t r = 0) { return query(Expression::Advice, c, r); }
inline Expr fixed(uint32_t c, int32_t r = 0) { return query(Expression::Fixed, c, r); }
inline Expr instance(uint32_t c, int32_t r = 0) { return query(Expression::Instance, c, r); }
inline Expr selector(uint32_t c) { return query(Expression::Selector, c, 0); }
inline Expr node(Expression::Kind k, Expr a, Expr b = nullptr) { auto e = std::make_shared<Expression>(); e->kind = k; e->a = std::move(a); e->b = std::move(b); return e; }
inline Expr operator-(const Expr& a) { return node(Expression::Negated, a); }
inline Expr operator+(const Expr& a, const Expr& b) { return node(Expression::Sum, a, b); }
inline Expr operator-(const Expr& a, const Expr& b) { return node(Expression::Sum, a, -b); }  // halo2: a - b == a + (-b)
inline Expr operator*(const Expr& a, const Expr& b) { return node(Expression::Product, a, b); }
inline Expr scaled(const Expr& a, const Limbs& v) { auto e = std::make_shared<Expression>(); e->kind = Expression::Scaled; e->a = a; e->value = v; return e; }

struct Program {
    Field field;
    std::vector<trh_expr_insn_t> insns;
    std::vector<Limbs> consts;                                  // index 0: the folding challenge y
    std::vector<std::pair<Expression::Kind, uint32_t>> columns;  // resident column of every slot, in slot order
    int max_degree = 0;
};

namespace detail {
inline int need(const Expr& e) {  // Sethi-Ullman number: stack entries the sub-expression needs
    switch (e->kind) {
        case Expression::Negated: case Expression::Scaled: return need(e->a);
        case Expression::Sum: case Expression::Product: { const int x = need(e->a), y = need(e->b); return x != y ? std::max(x, y) : x + 1; }
        default: return 1;
    }
}
struct Lowering {
    Program& p;
    uint32_t constant(const Limbs& v) {
        for (size_t i = 1; i < p.consts.size(); ++i) if (p.consts[i] == v) return (uint32_t)i;
        p.consts.push_back(v); return (uint32_t)p.consts.size() - 1;
    }
    uint32_t column(Expression::Kind k, uint32_t c) {
        for (size_t i = 0; i < p.columns.size(); ++i) if (p.columns[i].first == k && p.columns[i].second == c) return (uint32_t)i;
        p.columns.emplace_back(k, c); return (uint32_t)p.columns.size() - 1;
    }
    void op(uint32_t o, uint32_t a = 0, int32_t r = 0) { p.insns.push_back(trh_expr_insn_t{o, a, r}); }
    void emit(const Expr& e) {
        switch (e->kind) {
            case Expression::Constant: op(TRH_EXPR_PUSH_CONST, constant(e->value)); break;
            case Expression::Selector: case Expression::Fixed: case Expression::Advice: case Expression::Instance:
                op(TRH_EXPR_PUSH_COLUMN, column(e->kind, e->column), e->rotation); break;
            case Expression::Negated: emit(e->a); op(TRH_EXPR_NEG); break;
            case Expression::Scaled: emit(e->a); op(TRH_EXPR_MUL_CONST, constant(e->value)); break;
            case Expression::Sum:
                if (e->b->kind == Expression::Negated) {  // a + (-b): one SUB
                    const Expr &x = e->a, &y = e->b->a;
                    if (need(y) > need(x)) { emit(y); emit(x); op(TRH_EXPR_SUB); op(TRH_EXPR_NEG); }
                    else { emit(x); emit(y); op(TRH_EXPR_SUB); }
                } else {
                    const bool swap = need(e->b) > need(e->a);
                    emit(swap ? e->b : e->a); emit(swap ? e->a : e->b); op(TRH_EXPR_ADD);
                }
                break;
            case Expression::Product:
                if (e->a == e->b) { emit(e->a); op(TRH_EXPR_SQR); }
                else { const bool swap = need(e->b) > need(e->a); emit(swap ? e->b : e->a); emit(swap ? e->a : e->b); op(TRH_EXPR_MUL); }
                break;
        }
    }
};
}  // namespace detail

// gate polynomials folded into one output with the challenge y: h = h * y + gate (the order create_proof uses)
inline Program compile_gates(Field f, const std::vector<Expr>& gates, const Limbs& y) {
    Program p; p.field = f; p.consts.push_back(y);
    detail::Lowering lo{p};
    for (const Expr& g : gates) { p.max_degree = std::max(p.max_degree, g->degree()); lo.emit(g); lo.op(TRH_EXPR_FOLD, 0); }
    lo.op(TRH_EXPR_STORE_ACC, 0);
    return p;
}

// one output column per expression (numerator / denominator of a grand-product argument)
inline Program compile_outputs(Field f, const std::vector<Expr>& exprs) {
    Program p; p.field = f;
    p.consts.push_back(Limbs{0, 0, 0, 0});  // slot 0 is reserved for a challenge in compile_gates; unused here
    detail::Lowering lo{p};
    uint32_t i = 0;
    for (const Expr& e : exprs) { p.max_degree = std::max(p.max_degree, e->degree()); lo.emit(e); lo.op(TRH_EXPR_STORE_TOP, i++); }
    return p;
}

class GateEvaluator {
public:
    explicit GateEvaluator(Program p, size_t n_outputs = 1) : program(std::move(p)), n_outputs(n_outputs) {
        trh::check(trh_expr_create((int)program.field, program.insns.data(), program.insns.size(), (const uint64_t*)program.consts.data(), program.consts.size(),
                              program.columns.size(), n_outputs, 0, &e_), "expr_create");
    }
    GateEvaluator(const GateEvaluator&) = delete;
    GateEvaluator& operator=(const GateEvaluator&) = delete;
    ~GateEvaluator() { if (e_) trh_expr_destroy(e_); }
    void set_challenge(const Limbs& y) { trh::check(trh_expr_set_const(e_, 0, y.data()), "expr_set_const"); }
    // columns[i]: device pointer of program.columns[i] (2^log_n elements); out_dev: 2^log_n elements
    void eval(const std::vector<const void*>& columns, void* out_dev, uint32_t log_n, uint32_t rot_step, void* stream = nullptr) const {
        require(columns.size() == program.columns.size(), "one device column per program column");
        void* outs[1] = {out_dev};
        trh::check(trh_expr_eval_dev(e_, columns.data(), outs, log_n, rot_step, stream), "expr_eval");
    }
    // columns in the coset-block layout: n_blocks x 2^block_log rows each, Rotation(r) stays inside its block
    void eval_blocks(const std::vector<const void*>& columns, void* out_dev, uint32_t block_log, uint32_t n_blocks, void* stream = nullptr) const {
        require(columns.size() == program.columns.size(), "one device column per program column");
        void* outs[1] = {out_dev};
        trh::check(trh_expr_eval_blocks_dev(e_, columns.data(), outs, block_log, n_blocks, stream), "expr_eval_blocks");
    }
    void eval_outputs(const std::vector<const void*>& columns, const std::vector<void*>& outs, uint32_t log_n, uint32_t rot_step, void* stream = nullptr) const {
        require(columns.size() == program.columns.size() && outs.size() == n_outputs, "one device pointer per program column / output");
        trh::check(trh_expr_eval_dev(e_, columns.data(), outs.data(), log_n, rot_step, stream), "expr_eval");
    }
    // the gate part of MockProver::verify: every output (one gate polynomial each) tested against zero on rows [0, usable_rows), nothing stored.
    // n_bad[a] rows fail output a, the smallest is first_bad_row[a] (usable_rows when none); bitmap_dev (optional): n_outputs x max(1, 2^log_n / 64)
    // u64 words, one bit per row.  No stream: the verdict comes back to the host, ordered behind the context's previous call (trh.h)
    struct Check { std::vector<uint64_t> n_bad, first_bad_row; };
    Check check(const std::vector<const void*>& columns, uint32_t log_n, size_t usable_rows, void* bitmap_dev = nullptr) const {
        require(columns.size() == program.columns.size(), "one device column per program column");
        Check c{std::vector<uint64_t>(n_outputs), std::vector<uint64_t>(n_outputs)};
        trh::check(trh_expr_check_dev(e_, columns.data(), log_n, usable_rows, c.n_bad.data(), c.first_bad_row.data(), bitmap_dev), "expr_check");
        return c;
    }
    Program program;
    size_t n_outputs;
private:
    trh_expr_t e_ = nullptr;
};

// ---- the permutation and lookup terms of h(X) (trh_quotient_*): what plonk::create_proof folds into the quotient's numerator behind the custom
// gates, over resident extended columns in either layout (n_blocks = 0: flat, 2^extended_k rows; else coset blocks of 2^k rows).  acc_dev
// holds the fold so far -- GateEvaluator's output for the same y, or zeros -- and receives the result.  Returns with the stream synchronised.
class QuotientTerms {
public:
    struct Columns {
        std::vector<const void*> values, sigmas;  // n_perm_columns each, permutation column order
        std::vector<const void*> zs;              // ceil(n_perm_columns / chunk_len) product columns
        std::vector<const void*> lookups;         // n_lookups x 5: A, S, A', S', z
        const void *l0 = nullptr, *l_blind = nullptr, *l_last = nullptr;
    };
    QuotientTerms(const EvaluationDomain& d, uint32_t n_perm_columns, uint32_t chunk_len, uint32_t n_lookups, uint32_t blinding_factors)
        : n_perm_columns(n_perm_columns), chunk_len(chunk_len), n_lookups(n_lookups) {
        check(trh_quotient_create(d.handle(), n_perm_columns, chunk_len, n_lookups, blinding_factors, &q_), "quotient_create");
    }
    QuotientTerms(const QuotientTerms&) = delete;
    QuotientTerms& operator=(const QuotientTerms&) = delete;
    ~QuotientTerms() { if (q_) trh_quotient_destroy(q_); }
    size_t n_sets() const { return ((size_t)n_perm_columns + chunk_len - 1) / chunk_len; }
    void eval(void* acc_dev, const Columns& c, const Limbs& beta, const Limbs& gamma, const Limbs& y, uint32_t n_blocks = 0, void* stream = nullptr) const {
        require(c.values.size() == n_perm_columns && c.sigmas.size() == n_perm_columns && c.zs.size() == n_sets() && c.lookups.size() == 5 * (size_t)n_lookups,
                "one device column per permutation column, set and lookup column");
        trh_quotient_args_t a{};
        a.perm_values = c.values.data(); a.perm_sigmas = c.sigmas.data(); a.perm_z = c.zs.data(); a.lookups = c.lookups.data();
        a.l0 = c.l0; a.l_blind = c.l_blind; a.l_last = c.l_last;
        for (int i = 0; i < 4; ++i) { a.beta[i] = beta[i]; a.gamma[i] = gamma[i]; a.y[i] = y[i]; }
        a.acc = acc_dev; a.n_blocks = n_blocks; a.stream = stream;
        check(trh_quotient_terms_dev(q_, &a), "quotient_terms");
    }
    uint32_t n_perm_columns, chunk_len, n_lookups;
private:
    trh_quotient_t q_ = nullptr;
};

// ---- the prover's random scalars from a ChaCha20 seed (trh_rng_*): `C::Scalar::random(&mut rng)` for whole vectors ------------------
// The host draws 32 bytes from create_proof's rng once; element i of the stream they seed is ChaCha20 block i through from_u512 (trh.h).
// fill / fill_rows expand it in device memory, next_scalar on the host; all three share the one position.  Host memory: usable with any context.
class Rng {
public:
    explicit Rng(const std::array<uint8_t, 32>& seed, uint64_t stream_id = 0) { check(trh_rng_create(seed.data(), stream_id, &r_), "rng_create"); }
    Rng(const Rng&) = delete;
    Rng& operator=(const Rng&) = delete;
    Rng(Rng&& o) noexcept : r_(o.r_) { o.r_ = nullptr; }
    Rng& operator=(Rng&& o) noexcept { std::swap(r_, o.r_); return *this; }
    ~Rng() { if (r_) trh_rng_destroy(r_); }
    trh_rng_t handle() const { return r_; }
    void seek(uint64_t block) { check(trh_rng_seek(r_, block), "rng_seek"); }
    uint64_t position() const { uint64_t b = 0; check(trh_rng_position(r_, &b), "rng_position"); return b; }
    Limbs next_scalar(Field f) { Limbs v; check(trh_rng_next_scalar(r_, (int)f, v.data()), "rng_next_scalar"); return v; }
    // out_dev: n elements (the random polynomial, s(X))
    void fill(Field f, void* out_dev, size_t n, void* stream = nullptr) { check(trh_rng_fill_dev(r_, (int)f, out_dev, n, stream), "rng_fill"); }
    // cells [first, first + count) of `rows` columns of row_len elements stored back to back (blinding rows); the other cells are untouched
    void fill_rows(Field f, void* cols_dev, size_t rows, size_t row_len, size_t first, size_t count, void* stream = nullptr) {
        check(trh_rng_fill_rows_dev(r_, (int)f, cols_dev, rows, row_len, first, count, stream), "rng_fill_rows");
    }
private:
    trh_rng_t r_ = nullptr;
};

// An Rng as the `trh_rng_scalar_fn` / rng_ctx pair of ipa_create_proof: pass RngScalarFn::call and the object's address.  The callback runs
// with the context locked; trh_rng_next_scalar is host-only and takes only the handle's own lock, so that is allowed (trh.h).  A C callback
// cannot fail: a refused draw (the end of the stream) writes zero and sets `failed`, which the caller checks after the opening.
struct RngScalarFn {
    Rng& rng;
    Field field;
    bool failed = false;
    static void call(void* self, uint64_t out_mont[4]) {
        RngScalarFn* s = (RngScalarFn*)self;
        if (trh_rng_next_scalar(s->rng.handle(), (int)s->field, out_mont) != TRH_OK) { s->failed = true; for (int i = 0; i < 4; ++i) out_mont[i] = 0; }
    }
};

// ---- packed witness intake (trh_columns_from_ints_*, trh_even_odd_split_dev, trh_even_bits_table_dev): `F::from(u64)` for whole columns --
// A host that keeps its trace as machine words hands over words and bitmaps; the device expands them into columns of n stored elements,
// zero behind the live rows.  IntKind names the source's element type; Bits is a bitmap of u32 words, bit r & 31 of word r >> 5 for row r.
enum class IntKind : int { Bits = TRH_INT_BITS, U8 = TRH_INT_U8, U16 = TRH_INT_U16, U32 = TRH_INT_U32, U64 = TRH_INT_U64, I32 = TRH_INT_I32, I64 = TRH_INT_I64 };
template <class T> constexpr IntKind int_kind_of() {
    static_assert(std::is_integral<T>::value && (sizeof(T) == 1 ? std::is_unsigned<T>::value : sizeof(T) == 2 ? std::is_unsigned<T>::value : sizeof(T) == 4 || sizeof(T) == 8),
                  "u8, u16, u32, u64, i32 or i64");
    return sizeof(T) == 1 ? IntKind::U8 : sizeof(T) == 2 ? IntKind::U16 : sizeof(T) == 4 ? (std::is_signed<T>::value ? IntKind::I32 : IntKind::U32)
                                                                                           : (std::is_signed<T>::value ? IntKind::I64 : IntKind::U64);
}
// src: n_cols columns of live_rows elements, src_stride elements apart; dst_dev: n_cols x n elements.  src_on_host: any host memory
// (staged through the context's pinned ring), else device memory
inline void columns_from_ints(Field f, IntKind kind, const void* src, bool src_on_host, size_t src_stride, size_t n_cols, size_t live_rows, void* dst_dev, size_t n,
                              void* stream = nullptr) {
    trh_ints_args_t a{(int)kind, src, src_stride, n_cols, live_rows, dst_dev, nullptr, n, stream};
    check(src_on_host ? trh_columns_from_ints_host((int)f, &a) : trh_columns_from_ints_dev((int)f, &a), "columns_from_ints");
}
// one column from a host vector of machine integers
template <class T> inline void columns_from_ints(Field f, const std::vector<T>& values, void* dst_dev, size_t n, void* stream = nullptr) {
    columns_from_ints(f, int_kind_of<T>(), values.data(), true, values.size(), 1, values.size(), dst_dev, n, stream);
}
// the even-bits decomposition of resident words (unsigned kinds): even_dev takes w & 0x5555.., odd_dev (w & 0xAAAA..) >> 1
inline void even_odd_split(Field f, IntKind kind, const void* src_dev, size_t src_stride, size_t n_cols, size_t live_rows, void* even_dev, void* odd_dev, size_t n,
                           void* stream = nullptr) {
    trh_ints_args_t a{(int)kind, src_dev, src_stride, n_cols, live_rows, even_dev, odd_dev, n, stream};
    check(trh_even_odd_split_dev((int)f, &a), "even_odd_split");
}
// the even-bits lookup table of word_bits-bit words: 2^(word_bits / 2) rows, zero from there to n
inline void even_bits_table(Field f, uint32_t word_bits, void* dst_dev, size_t n, void* stream = nullptr) {
    trh_even_bits_table_args_t a{word_bits, dst_dev, n, stream};
    check(trh_even_bits_table_dev((int)f, &a), "even_bits_table");
}

// ---- the memory-consistency table (trh_mem_table_dev): an access log in execution order -> the 13 sorted, checked columns -----------------
// address / time / value: m resident words each; store_bits: ceil(m / 32) resident bitmap words; tape: t resident words (null for none);
// dst_dev: 13 x n elements.  Throws (check) on a refused log or one that needs more than max_rows rows.  Synchronises with the host.
struct MemTableResult { uint64_t rows, n_inconsistent, first_inconsistent; };
inline MemTableResult mem_table(Field f, uint32_t word_bits, const uint32_t* address_dev, const uint32_t* time_dev, const uint32_t* value_dev, const uint32_t* store_bits_dev,
                                size_t m, const uint32_t* tape_dev, size_t t, void* dst_dev, size_t n, size_t max_rows, uint32_t* src_index_dev = nullptr,
                                void* stream = nullptr) {
    trh_mem_table_args_t a{word_bits, address_dev, time_dev, value_dev, store_bits_dev, m, tape_dev, t, dst_dev, n, max_rows, src_index_dev, stream, 0, 0, 0};
    check(trh_mem_table_dev((int)f, &a), "mem_table");
    return MemTableResult{a.rows, a.n_inconsistent, a.first_inconsistent};
}

// ---- the Exe table (trh_exe_table_dev): the steps of a trace -> trace cells, temporary variables and their one-hot selectors ---------------
// ExeSelection: one TRH_EXE_ENTRY(a, b, c, d) per opcode, TRH_EXE_UNKNOWN for an opcode the table does not know.  exe_default_selection()
// restates the reference's TempVarSelectorsRow::from with the two departures trh.h documents (a register operand's content; CJmp's d).
typedef std::array<uint32_t, 32> ExeSelection;
inline uint32_t exe_encode(uint32_t opcode, uint32_t ri, uint32_t rj, bool a_is_reg) { return (opcode & 31u) | (ri & 15u) << 8 | (rj & 15u) << 12 | (a_is_reg ? 1u << 16 : 0u); }
inline ExeSelection exe_default_selection() {
    ExeSelection t;
    t.fill(TRH_EXE_UNKNOWN);
    const auto nd = [](int rule) { return TRH_EXE_NONDET + rule; };
    const uint32_t logic = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RJ, TRH_EXE_REG_NEXT_RI, TRH_EXE_UNSET);
    t[0] = t[1] = t[2] = logic;                                                                                   // and, or, xor
    t[3] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_MAX_WORD, TRH_EXE_REG_NEXT_RI, TRH_EXE_UNSET);                        // not
    t[4] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RJ, TRH_EXE_REG_NEXT_RI, TRH_EXE_ZERO);                           // add
    t[5] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_NEXT_RI, TRH_EXE_REG_RJ, TRH_EXE_ZERO);                           // sub
    t[6] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RJ, nd(TRH_EXE_RULE_MUL_HI), TRH_EXE_REG_NEXT_RI);                // mull
    t[7] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RJ, TRH_EXE_REG_NEXT_RI, nd(TRH_EXE_RULE_MUL_LO));                // umulh
    t[8] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RJ, TRH_EXE_REG_NEXT_RI, nd(TRH_EXE_RULE_SMUL_LO));               // smulh
    t[9] = TRH_EXE_ENTRY(nd(TRH_EXE_RULE_REM), TRH_EXE_REG_NEXT_RI, TRH_EXE_A, TRH_EXE_REG_RJ);                   // udiv
    t[10] = TRH_EXE_ENTRY(TRH_EXE_REG_NEXT_RI, nd(TRH_EXE_RULE_QUOT), TRH_EXE_A, TRH_EXE_REG_RJ);                 // umod
    t[11] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RJ, nd(TRH_EXE_RULE_SHL_HI), TRH_EXE_REG_NEXT_RI);               // shl
    t[12] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RJ, TRH_EXE_REG_NEXT_RI, nd(TRH_EXE_RULE_SHR_LO));               // shr
    t[13] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_RI, nd(TRH_EXE_RULE_XOR), TRH_EXE_UNSET);                        // cmpe
    t[14] = t[16] = TRH_EXE_ENTRY(TRH_EXE_REG_RI, nd(TRH_EXE_RULE_CMP_GT), TRH_EXE_A, TRH_EXE_ZERO);              // cmpa, cmpg
    t[15] = t[17] = TRH_EXE_ENTRY(TRH_EXE_REG_RI, nd(TRH_EXE_RULE_CMP_GE), TRH_EXE_A, TRH_EXE_ONE);               // cmpae, cmpge
    t[18] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_REG_NEXT_RI, TRH_EXE_ZERO, TRH_EXE_UNSET);                           // mov
    t[19] = TRH_EXE_ENTRY(TRH_EXE_REG_NEXT_RI, TRH_EXE_A, TRH_EXE_ZERO, TRH_EXE_REG_RI);                          // cmov
    t[20] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_PC_NEXT, TRH_EXE_ZERO, TRH_EXE_UNSET);                               // jmp
    t[21] = TRH_EXE_ENTRY(TRH_EXE_PC_NEXT, TRH_EXE_A, TRH_EXE_ZERO, nd(TRH_EXE_RULE_PC_PLUS_ONE));                // cjmp
    t[22] = TRH_EXE_ENTRY(TRH_EXE_PC_NEXT, TRH_EXE_PC_PLUS_ONE, TRH_EXE_ZERO, TRH_EXE_A);                         // cnjmp
    t[28] = TRH_EXE_ENTRY(TRH_EXE_VALUE, TRH_EXE_REG_NEXT_RI, TRH_EXE_ZERO, TRH_EXE_ZERO);                        // store.w
    t[29] = TRH_EXE_ENTRY(TRH_EXE_VALUE, TRH_EXE_REG_RI, TRH_EXE_ZERO, TRH_EXE_ZERO);                             // load.w
    t[31] = TRH_EXE_ENTRY(TRH_EXE_A, TRH_EXE_PC, TRH_EXE_ZERO, TRH_EXE_ZERO);                                     // answer
    return t;
}
inline size_t exe_columns(uint32_t reg_count) { return 28 + 9 * (size_t)reg_count; }
// pc / inst / a / value: m resident words each; regs: m x reg_count resident words, step-major; flag_bits: ceil(m / 32) resident bitmap
// words; dst_dev: exe_columns(reg_count) x n elements.  Throws (check) on refused steps or a bad table; synchronises with the host once.
inline void exe_table(Field f, uint32_t word_bits, uint32_t reg_count, const uint32_t* pc_dev, const uint32_t* inst_dev, const uint32_t* a_dev, const uint32_t* value_dev,
                      const uint32_t* regs_dev, const uint32_t* flag_bits_dev, size_t m, void* dst_dev, size_t n, const ExeSelection& selection = exe_default_selection(),
                      void* stream = nullptr) {
    trh_exe_table_args_t a{};
    a.word_bits = word_bits; a.reg_count = reg_count;
    a.pc = pc_dev; a.inst = inst_dev; a.a = a_dev; a.value = value_dev; a.regs = regs_dev; a.flag_bits = flag_bits_dev; a.m = m;
    for (size_t o = 0; o < selection.size(); ++o) a.selection[o] = selection[o];
    a.dst = dst_dev; a.n = n; a.stream = stream;
    check(trh_exe_table_dev((int)f, &a), "exe_table");
}

// ---- the Exe chips (trh_exe_chips_dev): the same steps -> Out, the changed flags and the sub-chips' advice ----------------------------------
// ExeChips: TRH_CHIP_* bits per opcode, TRH_EXE_UNKNOWN for an opcode the table does not know (exactly those the selection does not know).
// exe_default_chips() restates the reference's OutPut::OUT (out.rs:148-349) and the `ch:` fields of TempVarSelectorsRow::from.
typedef std::array<uint32_t, 32> ExeChips;
inline ExeChips exe_default_chips() {
    ExeChips t;
    t.fill(TRH_EXE_UNKNOWN);
    const uint32_t f12 = TRH_CHIP_FLAG1 | TRH_CHIP_FLAG2, reg = TRH_CHIP_CH_REG, flag = TRH_CHIP_CH_FLAG, pc = TRH_CHIP_CH_PC;
    t[0] = TRH_CHIP_AND | f12 | reg | flag;                                     // and
    t[1] = TRH_CHIP_OR | f12 | reg | flag;                                      // or
    t[2] = t[3] = TRH_CHIP_XOR | f12 | reg | flag;                              // xor, not
    t[4] = t[5] = TRH_CHIP_SUM | reg | flag;                                    // add, sub
    t[6] = t[7] = TRH_CHIP_PROD | f12 | reg | flag;                             // mull, umulh
    t[8] = TRH_CHIP_SPROD | f12 | reg | flag;                                   // smulh
    t[9] = t[10] = TRH_CHIP_MOD | f12 | TRH_CHIP_FLAG3 | reg | flag;            // udiv, umod
    t[11] = TRH_CHIP_SHIFT | TRH_CHIP_FLAG4 | TRH_CHIP_B_FLAG | reg | flag;     // shl: flag4 reads b's top bit
    t[12] = TRH_CHIP_SHIFT | TRH_CHIP_FLAG4 | reg | flag;                       // shr
    t[13] = TRH_CHIP_XOR | f12 | flag;                                          // cmpe
    t[14] = t[15] = TRH_CHIP_SUM | flag;                                        // cmpa, cmpae
    t[16] = t[17] = TRH_CHIP_SSUM | flag;                                       // cmpg, cmpge
    t[18] = TRH_CHIP_XOR | reg;                                                 // mov
    t[19] = TRH_CHIP_MOD | reg;                                                 // cmov
    t[20] = TRH_CHIP_XOR | pc;                                                  // jmp
    t[21] = t[22] = TRH_CHIP_MOD | pc;                                          // cjmp, cnjmp
    t[28] = TRH_CHIP_XOR;                                                       // store.w
    t[29] = reg;                                                                // load.w
    t[31] = 0;                                                                  // answer
    return t;
}
inline size_t exe_chip_columns(uint32_t reg_count) { return 52 + (size_t)reg_count; }
// the step arrays as in exe_table; dst_dev: exe_chip_columns(reg_count) x n elements; word_bits even.  Throws (check) on refused steps or a
// bad table; synchronises with the host once.
inline void exe_chips(Field f, uint32_t word_bits, uint32_t reg_count, const uint32_t* pc_dev, const uint32_t* inst_dev, const uint32_t* a_dev, const uint32_t* value_dev,
                      const uint32_t* regs_dev, const uint32_t* flag_bits_dev, size_t m, void* dst_dev, size_t n, const ExeSelection& selection = exe_default_selection(),
                      const ExeChips& chips = exe_default_chips(), void* stream = nullptr) {
    trh_exe_chips_args_t a{};
    a.word_bits = word_bits; a.reg_count = reg_count;
    a.pc = pc_dev; a.inst = inst_dev; a.a = a_dev; a.value = value_dev; a.regs = regs_dev; a.flag_bits = flag_bits_dev; a.m = m;
    for (size_t o = 0; o < selection.size(); ++o) { a.selection[o] = selection[o]; a.chips[o] = chips[o]; }
    a.dst = dst_dev; a.n = n; a.stream = stream;
    check(trh_exe_chips_dev((int)f, &a), "exe_chips");
}

// ---- plonk::permutation::keygen::Assembly (trh_perm_*): the copy constraints of the equality-enabled columns, the sigma columns they
// induce -- made on the device -- and what keygen_vk / keygen_pk derive from them ---------------------------------------------------------
// copy() merges cycles exactly as upstream does (the order of the copies decides the mapping).  Host memory, like Rng: copies and mapping()
// need no device; the device copy of the mapping is made by the first device call after a copy.
class PermutationAssembly {
public:
    PermutationAssembly(Field f, uint32_t k, uint32_t n_columns) : field(f), k(k), n((size_t)1 << (k & 31)), n_columns(n_columns) { check(trh_perm_create(n_columns, k, &p_), "permutation::Assembly::new"); }
    PermutationAssembly(const PermutationAssembly&) = delete;
    PermutationAssembly& operator=(const PermutationAssembly&) = delete;
    PermutationAssembly(PermutationAssembly&& o) noexcept : field(o.field), k(o.k), n(o.n), n_columns(o.n_columns), p_(o.p_) { o.p_ = nullptr; }
    PermutationAssembly& operator=(PermutationAssembly&& o) noexcept { std::swap(field, o.field); std::swap(k, o.k); std::swap(n, o.n); std::swap(n_columns, o.n_columns); std::swap(p_, o.p_); return *this; }
    ~PermutationAssembly() { if (p_) trh_perm_destroy(p_); }
    trh_perm_t handle() const { return p_; }
    void copy(uint32_t left_column, uint32_t left_row, uint32_t right_column, uint32_t right_row) { check(trh_perm_copy(p_, left_column, left_row, right_column, right_row), "permutation::Assembly::copy"); }
    // (left_column, left_row, right_column, right_row) per copy, in order
    void copy_many(const std::vector<std::array<uint32_t, 4>>& quads) { check(trh_perm_copy_batch(p_, (const uint32_t*)quads.data(), quads.size()), "permutation::Assembly::copy"); }
    // the cell (column * n + row) every cell of `count` columns from `first` maps to
    std::vector<uint32_t> mapping(uint32_t first, uint32_t count) const { std::vector<uint32_t> m((size_t)count * n); check(trh_perm_mapping(p_, first, count, m.data()), "perm_mapping"); return m; }
    std::vector<uint32_t> mapping() const { return mapping(0, n_columns); }
    // the sigma columns first .. first + count - 1 in Lagrange form, count x n elements back to back
    DeviceBuffer sigma_columns(uint32_t first, uint32_t count, void* stream = nullptr) const {
        DeviceBuffer out((size_t)count * n * 32);
        check(trh_perm_sigma_dev(p_, (int)field, first, count, out.data(), stream), "perm_sigma");
        return out;
    }
    DeviceBuffer sigma_columns(void* stream = nullptr) const { return sigma_columns(0, n_columns, stream); }
    // the permutation part of MockProver::verify over n_columns device columns of n canonical elements: the number of cells whose value
    // differs from the value of the cell they map to, and the smallest of them (n_columns * n when there is none)
    struct Check { uint64_t n_bad, first_bad_cell; };
    Check check_columns(const std::vector<const void*>& columns, void* stream = nullptr) const {
        require(columns.size() == n_columns, "one device pointer per column");
        Check c{0, 0};
        check(trh_perm_check_dev(p_, (int)field, columns.data(), &c.n_bad, &c.first_bad_cell, stream), "perm_check");
        return c;
    }
    // Assembly::build_vk: params.commit_lagrange(sigma_j, Blind::default()) for every column (the default blind is one)
    std::vector<Point> build_vk(const Params& params, void* stream = nullptr) const {
        require(params.k == k && scalar_field(params.curve) == field, "params.k == k, over the curve whose scalars the columns hold");
        const DeviceBuffer sigma = sigma_columns(stream);
        return params.commit_lagrange_batch(sigma, n_columns, std::vector<Limbs>(n_columns, host::one(field)), stream);
    }
    // Assembly::build_pk: the sigma columns, lagrange_to_coeff of them, coeff_to_extended of those
    struct ProvingKey { DeviceBuffer permutations, polys, cosets; };
    ProvingKey build_pk(const EvaluationDomain& domain, void* stream = nullptr) const {
        require(domain.k == k && domain.field == field, "domain.k == k, same field");
        ProvingKey pk;
        pk.permutations = sigma_columns(stream);
        pk.polys = sigma_columns(stream);
        domain.lagrange_to_coeff(pk.polys.data(), n_columns, stream);
        pk.cosets = DeviceBuffer((size_t)n_columns * domain.extended_len() * 32);
        domain.coeff_to_extended(pk.polys.data(), pk.cosets.data(), n_columns, stream);
        return pk;
    }
    Field field;
    uint32_t k;
    size_t n;
    uint32_t n_columns;
private:
    trh_perm_t p_ = nullptr;
};

// ---- transcript::{Blake2bWrite, Blake2bRead} with Challenge255 (trh_tr_*): the proof as bytes ---------------------------------------------
// Host memory, like Rng: usable without a device.  Points go in as normalised Jacobian and come out affine, scalars are Montgomery limbs.
// The handle latches its first error (trh.h); here every call that meets one throws trh::Error, and throw_if_failed() does after an
// opening that ran through callbacks(), where the C callbacks had no way to report it.
namespace detail {
class TranscriptHandle {
public:
    TranscriptHandle(const TranscriptHandle&) = delete;
    TranscriptHandle& operator=(const TranscriptHandle&) = delete;
    TranscriptHandle(TranscriptHandle&& o) noexcept : curve(o.curve), t_(o.t_) { o.t_ = nullptr; }
    TranscriptHandle& operator=(TranscriptHandle&& o) noexcept { std::swap(curve, o.curve); std::swap(t_, o.t_); return *this; }
    ~TranscriptHandle() { if (t_) trh_tr_destroy(t_); }
    trh_tr_t handle() const { return t_; }
    void common_point(const Point& p) { check(trh_tr_common_point(t_, (const uint64_t*)&p), "transcript common_point"); }
    void common_scalar(const Limbs& s) { check(trh_tr_common_scalar(t_, s.data()), "transcript common_scalar"); }
    Limbs squeeze_challenge_scalar() { Limbs c; check(trh_tr_squeeze_challenge_scalar(t_, c.data()), "transcript squeeze_challenge_scalar"); return c; }
    void throw_if_failed() const { check(trh_tr_status(t_), "transcript"); }
    Curve curve;
protected:
    explicit TranscriptHandle(Curve c) : curve(c) {}
    trh_tr_t t_ = nullptr;
};
}  // namespace detail

class Blake2bWrite : public detail::TranscriptHandle {
public:
    explicit Blake2bWrite(Curve c) : TranscriptHandle(c) { check(trh_tr_create_writer((int)c, &t_), "Blake2bWrite::init"); }
    void write_point(const Point& p) { check(trh_tr_write_point(t_, (const uint64_t*)&p), "transcript write_point"); }
    void write_scalar(const Limbs& s) { check(trh_tr_write_scalar(t_, s.data()), "transcript write_scalar"); }
    // the transcript argument of ipa_create_proof: the library's own functions over this writer; call throw_if_failed() when it has returned
    trh_transcript_t callbacks() const { trh_transcript_t cb; check(trh_tr_callbacks(t_, &cb), "transcript callbacks"); return cb; }
    // Blake2bWrite::finalize: the proof so far
    std::vector<uint8_t> bytes() const {
        size_t len = 0;
        check(trh_tr_bytes_len(t_, &len), "transcript bytes");
        std::vector<uint8_t> out(len);
        check(trh_tr_bytes(t_, out.data(), out.size()), "transcript bytes");
        return out;
    }
};

class Blake2bRead : public detail::TranscriptHandle {
public:
    Blake2bRead(Curve c, const uint8_t* proof, size_t len) : TranscriptHandle(c) { check(trh_tr_create_reader((int)c, proof, len, &t_), "Blake2bRead::init"); }
    Blake2bRead(Curve c, const std::vector<uint8_t>& proof) : Blake2bRead(c, proof.data(), proof.size()) {}
    Affine read_point() { Affine p; check(trh_tr_read_point(t_, (uint64_t*)&p), "transcript read_point"); return p; }
    Limbs read_scalar() { Limbs s; check(trh_tr_read_scalar(t_, s.data()), "transcript read_scalar"); return s; }
    size_t remaining() const { size_t len = 0; check(trh_tr_remaining(t_, &len), "transcript remaining"); return len; }
    bool finished() const { return remaining() == 0; }  // the proof has no byte left over
};

// ---- poly::commitment::create_proof (IPA opening) -------------------------------------------------------------------
// transcript / rng are the caller's (BLAKE2b transcript and OsRng in the reference): plain C callbacks as in trh.h; a Blake2bWrite's
// callbacks() keeps the transcript inside the library
inline std::pair<Limbs, Limbs> ipa_create_proof(const Params& params, const DeviceBuffer& p_poly, const Limbs& p_blind, const Limbs& x3, const DeviceBuffer& s_poly,
                                                const Limbs& s_blind, const trh_transcript_t& transcript, trh_rng_scalar_fn rng, void* rng_ctx, void* stream = nullptr) {
    require(p_poly.size() >= params.n * 32 && s_poly.size() >= params.n * 32, "px.len() == params.n");
    Limbs c, f;
    check(trh_ipa_create_proof(params.ipa_bases().handle(), (const uint64_t*)&params.u, params.k, p_poly.data(), p_blind.data(), x3.data(), s_poly.data(), s_blind.data(), &transcript, rng,
                               rng_ctx, stream, c.data(), f.data()), "ipa create_proof");
    return {c, f};
}

// ---- poly::commitment::msm::MSM (the verifier's accumulator) over the opening's base set -------------------------------------
// g scalars resident (absent until first set, as halo2's Option), w / u / appended terms on the host; eval() is MSM::eval
class IpaMsm {
public:
    explicit IpaMsm(const Params& params, void* stream = nullptr) : k_(params.k), stream_(stream) {
        check(trh_ipa_msm_create(params.ipa_bases().handle(), params.k, (const uint64_t*)&params.u, &m_), "Params::empty_msm");
    }
    IpaMsm(const IpaMsm&) = delete;
    IpaMsm& operator=(const IpaMsm&) = delete;
    IpaMsm(IpaMsm&& o) noexcept : m_(o.m_), k_(o.k_), stream_(o.stream_) { o.m_ = nullptr; }
    IpaMsm& operator=(IpaMsm&& o) noexcept { std::swap(m_, o.m_); std::swap(k_, o.k_); std::swap(stream_, o.stream_); return *this; }
    ~IpaMsm() { if (m_) trh_ipa_msm_destroy(m_); }
    trh_ipa_msm_t handle() const { return m_; }
    void append_term(const Limbs& scalar, const Affine& point) { check(trh_ipa_msm_append_term(m_, scalar.data(), (const uint64_t*)&point), "MSM::append_term"); }
    void add_constant_term(const Limbs& c) { check(trh_ipa_msm_add_constant_term(m_, c.data()), "MSM::add_constant_term"); }
    void add_to_w_scalar(const Limbs& s) { check(trh_ipa_msm_add_to_w_scalar(m_, s.data()), "MSM::add_to_w_scalar"); }
    void add_to_u_scalar(const Limbs& s) { check(trh_ipa_msm_add_to_u_scalar(m_, s.data()), "MSM::add_to_u_scalar"); }
    void add_to_g_scalars(const DeviceBuffer& scalars) {
        require(scalars.size() >= ((size_t)32 << k_), "scalars.len() == params.n");
        check(trh_ipa_msm_add_to_g_scalars_dev(m_, scalars.data(), stream_), "MSM::add_to_g_scalars");
    }
    // Guard::use_challenges for every guard at once: challenges[p] holds guard p's k round challenges; empty weights = all one
    void use_challenges(const std::vector<std::vector<Limbs>>& challenges, const std::vector<Limbs>& neg_c, const std::vector<Limbs>& weights = {},
                        const Limbs* alpha = nullptr) {
        require(challenges.size() == neg_c.size() && (weights.empty() || weights.size() == neg_c.size()), "one neg_c (and weight) per guard");
        std::vector<Limbs> u;
        for (const auto& row : challenges) { require(row.size() == k_, "u.len() == k"); u.insert(u.end(), row.begin(), row.end()); }
        check(trh_ipa_msm_use_challenges(m_, neg_c.size(), (const uint64_t*)u.data(), (const uint64_t*)neg_c.data(),
                                         weights.empty() ? nullptr : (const uint64_t*)weights.data(), alpha ? alpha->data() : nullptr, stream_), "Guard::use_challenges");
    }
    void scale(const Limbs& factor) { check(trh_ipa_msm_scale(m_, factor.data(), stream_), "MSM::scale"); }
    void add_msm(const IpaMsm& other) { check(trh_ipa_msm_add_msm(m_, other.m_, stream_), "MSM::add_msm"); }
    bool eval(Point* point = nullptr) const {
        int ident = 0;
        Point p;
        check(trh_ipa_msm_eval(m_, stream_, &ident, (uint64_t*)&p), "MSM::eval");
        if (point) *point = p;
        return ident != 0;
    }
private:
    trh_ipa_msm_t m_ = nullptr;
    uint32_t k_;
    void* stream_;
};

// ---- the remaining polynomial steps of create_proof on resident data -------------------------------------------------
// arithmetic::eval_polynomial for `batch` coefficient forms (n each, back to back) at one point
inline std::vector<Limbs> eval_polynomials(Field f, const void* polys_dev, size_t n, size_t batch, const Limbs& point, void* stream = nullptr) {
    std::vector<Limbs> out(batch);
    check(trh_poly_eval_batch_dev((int)f, polys_dev, n, batch, point.data(), stream, (uint64_t*)out.data()), "eval_polynomial");
    return out;
}
// poly/multiopen/prover.rs: sum_b coeffs[b] * polys[b]
inline void lincomb(Field f, const void* polys_dev, size_t n, const std::vector<Limbs>& coeffs, void* out_dev, void* stream = nullptr) {
    check(trh_poly_lincomb_dev((int)f, polys_dev, n, coeffs.size(), (const uint64_t*)coeffs.data(), out_dev, stream), "lincomb");
}
// plonk/lookup/prover.rs permute_expression_pair over the first usable_rows rows; throws where the Rust code returns
// Error::ConstraintSystemFailure (an input value that is not in the table)
inline void lookup_permute(Field f, const void* input_dev, const void* table_dev, size_t usable_rows, void* permuted_input_dev, void* permuted_table_dev, void* stream = nullptr) {
    check(trh_lookup_permute_dev((int)f, input_dev, table_dev, usable_rows, permuted_input_dev, permuted_table_dev, stream), "permute_expression_pair");
}

// all lookups of a proof at once: column l of inputs / tables / outputs at element offset l * row_stride
inline void lookup_permute_batch(Field f, const void* inputs_dev, const void* tables_dev, size_t usable_rows, size_t row_stride, size_t batch, void* permuted_inputs_dev,
                                 void* permuted_tables_dev, void* stream = nullptr) {
    check(trh_lookup_permute_batch_dev((int)f, inputs_dev, tables_dev, usable_rows, row_stride, batch, permuted_inputs_dev, permuted_tables_dev, stream), "permute_expression_pair (batch)");
}

// the lookup part of MockProver::verify: the input rows below usable_rows whose tuple (one element per input column) equals no table row's
// tuple -- exact membership, not the theta compression.  bitmap_dev (optional): ceil(usable_rows / 64) u64 words, one bit per row.  No stream (trh.h)
struct LookupCheck { uint64_t n_bad, first_bad_row; };
inline LookupCheck lookup_check(Field f, const std::vector<const void*>& inputs, const std::vector<const void*>& tables, size_t usable_rows, void* bitmap_dev = nullptr) {
    require(inputs.size() == tables.size(), "as many input columns as table columns");
    LookupCheck c{0, 0};
    check(trh_lookup_check_dev((int)f, inputs.data(), tables.data(), (uint32_t)inputs.size(), usable_rows, &c.n_bad, &c.first_bad_row, bitmap_dev), "lookup_check");
    return c;
}

// z[0] = z0, z[i + 1] = z[i] * num(row i) / den(row i): the product columns of the permutation argument
// (plonk/permutation/prover.rs) and of the lookup argument (plonk/lookup/prover.rs commit_product)
class GrandProduct {
public:
    GrandProduct(Field f, uint32_t k, const Expr& num, const Expr& den) : field(f), k(k), n((size_t)1 << k), ev_(compile_outputs(f, {num, den}), 2), num_(n * 32), den_(n * 32), ratio_(n * 32) {}
    const std::vector<std::pair<Expression::Kind, uint32_t>>& columns() const { return ev_.program.columns; }
    // columns[i]: device pointer of columns()[i]; z_dev: 2^k elements
    void compute(const std::vector<const void*>& cols, void* z_dev, uint32_t rot_step = 1, void* stream = nullptr) {
        ev_.eval_outputs(cols, {num_.data(), den_.data()}, k, rot_step, stream);
        check(trh_field_batch_invert_dev((int)field, den_.data(), n, stream), "batch_invert");
        check(trh_field_op_dev((int)field, 2 /* mul */, num_.data(), den_.data(), ratio_.data(), n, stream), "ratio");
        check(trh_field_prefix_product_dev((int)field, ratio_.data(), z_dev, n, stream), "prefix_product");
    }
    Field field;
    uint32_t k;
    size_t n;
private:
    GateEvaluator ev_;
    DeviceBuffer num_, den_, ratio_;
};

// Every product column of a proof at once, fixed-function (trh_product_terms_dev): a row is the list of the factors
// (x[i] + c y[i] + g) of one numerator or denominator product.  permutation chunk: numerator {v_j, omega^i column, beta delta^col_j, gamma},
// denominator {v_j, sigma_j, beta, gamma}; lookup: numerator {A, -, -, beta}{S, -, -, gamma}, denominator {A', -, -, beta}{S', -, -, gamma}
inline trh_product_term_t product_term(const void* x, const void* y, const Limbs& c, const Limbs& g) {
    trh_product_term_t t{};
    t.x = x; t.y = y;
    for (int i = 0; i < 4; ++i) { t.c[i] = c[i]; t.g[i] = g[i]; }
    return t;
}
// z_dev: rows x 2^k elements, z[r][0] = 1, z[r][i + 1] = z[r][i] * num_r(i) / den_r(i) (a zero denominator gives a zero ratio, as
// ff::BatchInvert followed by the multiplication does)
inline void grand_products(Field f, uint32_t k, const std::vector<std::vector<trh_product_term_t>>& num_rows, const std::vector<std::vector<trh_product_term_t>>& den_rows,
                           void* z_dev, void* stream = nullptr) {
    if (num_rows.size() != den_rows.size()) throw Error("grand_products: numerator / denominator row counts differ");
    const size_t rows = num_rows.size(), n = (size_t)1 << k;
    if (!rows) return;
    std::vector<trh_product_term_t> flat;
    std::vector<uint32_t> start{0};
    for (const auto* part : {&num_rows, &den_rows})
        for (const auto& row : *part) { flat.insert(flat.end(), row.begin(), row.end()); start.push_back((uint32_t)flat.size()); }
    DeviceBuffer nd(2 * rows * n * 32);
    check(trh_product_terms_dev((int)f, flat.data(), start.data(), (uint32_t)(2 * rows), n, nd.data(), stream), "product_terms");
    char* den = (char*)nd.data() + rows * n * 32;
    check(trh_field_batch_invert_mul_dev((int)f, den, nd.data(), rows * n, stream), "batch_invert_mul");
    check(trh_field_prefix_product_rows_dev((int)f, den, z_dev, n, rows, stream), "prefix_product_rows");
    check(trh_stream_synchronize(stream), "grand_products sync");  // nd is released on return
}

// Argument::commit's link between consecutive permutation sets, in place on the rows x n output of grand_products (trh_product_chain_dev)
inline void chain_products(Field f, void* z_dev, size_t n, size_t rows, size_t link, void* stream = nullptr) {
    trh_product_chain_args_t a{};
    a.z = z_dev; a.n = n; a.rows = rows; a.link = link; a.stream = stream;
    check(trh_product_chain_dev((int)f, &a), "product_chain");
}

// arithmetic::kate_division by (X - z) for polynomials of n coefficients.  The powers of z and 1 / z are built once, on the stream
// the divisions will run on (the constructor takes it: tables built on another stream could still be in flight when divide() reads
// them); z = 0 (z_inv ignored) divides by X: the quotient is the coefficient list shifted down by one.
class KateDivider {
public:
    KateDivider(Field f, size_t n, const Limbs& z, const Limbs& z_inv, void* stream = nullptr)
        : field(f), n(n), zero_(z == Limbs{0, 0, 0, 0}), stream_(stream), pz_(zero_ ? 32 : n * 32), pzinv_(zero_ ? 32 : n * 32), scratch_(zero_ ? 32 : 2 * n * 32) {
        if (zero_) return;
        check(trh_field_powers_dev((int)f, pz_.data(), n, z.data(), stream), "powers");
        check(trh_field_powers_dev((int)f, pzinv_.data(), n, z_inv.data(), stream), "powers");
    }
    // a_dev: len coefficients (default: n; a shorter polynomial uses the prefixes of the power tables -- the multiopen sets divide by the
    // same point at lengths n, n - 1, ...), q_dev: len - 1 coefficients; runs on the constructor's stream
    void divide(const void* a_dev, void* q_dev, size_t len = 0) {
        if (len == 0) len = n;
        require(len <= n, "kate_division: polynomial longer than the divider's tables");
        if (zero_) {  // a(X) / X, remainder a_0 dropped: host-ordered device-to-device copy through the ABI's helpers
            std::vector<Limbs> tmp(len);
            check(trh_stream_synchronize(stream_), "sync");
            check(trh_memcpy_d2h(tmp.data(), a_dev, len * 32), "d2h");
            check(trh_memcpy_h2d(q_dev, tmp.data() + 1, (len - 1) * 32), "h2d");
            return;
        }
        check(trh_poly_kate_division_dev((int)field, a_dev, len, pz_.data(), pzinv_.data(), scratch_.data(), q_dev, stream_), "kate_division");
    }
    Field field;
    size_t n;
private:
    bool zero_;
    void* stream_;
    DeviceBuffer pz_, pzinv_, scratch_;
};

inline void init(int device = 0) { check(trh_init(device), "trh_init"); }

// An independent libtrh context on one device (own scratch, own lock, own stream): one per host thread that should overlap with others, one
// per GPU of a node.  bind() makes it the calling thread's context until unbind(); objects created while it is bound (Bases, Params,
// EvaluationDomain, DeviceBuffer) live on its device.
class Context {
public:
    explicit Context(int device = 0) { check(trh_ctx_create(device, &c_), "trh_ctx_create"); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ~Context() { if (c_) trh_ctx_destroy(c_); }
    void bind() const { check(trh_ctx_set_current(c_), "trh_ctx_set_current"); }
    static void unbind() { check(trh_ctx_set_current(nullptr), "trh_ctx_set_current"); }
    void* stream() const { return trh_ctx_stream(c_); }
    int device() const { return trh_ctx_device(c_); }
private:
    trh_ctx_t c_ = nullptr;
};

}  // namespace trh
#endif  // TRH_HPP
