// The proof transcript: Blake2bWrite / Blake2bRead with Challenge255 of halo2_proofs 0.2.0 (src/transcript.rs), host only.
//
// THE FORMAT -- recalled, not pinned: the crate's source is not vendored by the reference (DESIGN.md section 4 lists every point).
//   state                       BLAKE2b, 64-byte digest, no key, personalisation the 16 bytes "Halo2-Transcript" (blake2b.h)
//   common_point(P)             absorb 01 || x || y, each coordinate 32 bytes little endian, canonical (out of Montgomery form), base field;
//                               the identity is an error ("cannot write points at infinity to the transcript")
//   common_scalar(s)            absorb 02 || s, 32 bytes little endian canonical, scalar field
//   write_point / write_scalar  common_*, then the proof grows by the 32-byte compressed point (fieldsqrt.h point_encode) / the 32 bytes of s
//   squeeze_challenge_scalar    absorb 00, finalise a COPY of the state into 64 bytes, read them as a little-endian 512-bit integer and reduce it
//                               modulo the scalar field's order (from_bytes_wide; chacha.h fe_from_u512); the running state goes on
//   read_point                  take 32 bytes, decode them (point_decode), then common_point; fewer than 32 bytes left, an invalid encoding and
//                               the identity are errors
//   read_scalar                 take 32 bytes, a value >= the modulus is an error, then common_scalar
//
// ERRORS LATCH.  The three callbacks of trh_transcript_t return void, so a transcript inside trh_ipa_create_proof cannot fail where it stands:
// the first error is kept with its code and message, and every later operation does nothing and leaves its outputs zero.
//
// A handle is host memory and belongs to no context; its operations start no device work and take nothing but the handle's own lock, so they
// may run with a context locked -- as the callbacks of trh_ipa_create_proof do (the rule trh.h states for trh_rng_next_scalar).
//
// Plain C++, no HIP: tests/native/transcript_test.cpp compiles it with g++ under address + undefined sanitizers.  A translation unit that
// defines TRH_TRANSCRIPT_ABI before including this header also gets the definitions of the trh_tr_* entries of include/trh.h: csrc/capi.hip
// for the library, the stand-alone test for itself (it brings its own set_error).
#pragma once
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/trh.h"
#include "blake2b.h"
#include "chacha.h"
#include "curve.h"
#include "dispatch.h"
#include "fieldsqrt.h"

namespace trh {

void set_error(const char* fmt, ...);  // the calling thread's trh_last_error() (capi.hip; ctx.h declares it too)

static const uint8_t TRANSCRIPT_PERSON[16] = {'H', 'a', 'l', 'o', '2', '-', 'T', 'r', 'a', 'n', 's', 'c', 'r', 'i', 'p', 't'};
constexpr uint8_t TRANSCRIPT_PREFIX_CHALLENGE = 0, TRANSCRIPT_PREFIX_POINT = 1, TRANSCRIPT_PREFIX_SCALAR = 2;

// the eight little-endian words of a 256-bit value against the modulus of F: true when the value is below it
template <class F> inline bool words_below_modulus(const u32 (&w)[8]) {
    for (int i = 7; i >= 0; --i)
        if (w[i] != F::MOD[i]) return w[i] < F::MOD[i];
    return false;
}

struct Transcript {
    std::mutex mu;
    const int curve;
    const bool reader;
    Blake2b state{TRANSCRIPT_PERSON};
    std::vector<uint8_t> bytes;  // a writer: the proof so far; a reader: the proof
    size_t at = 0;               // a reader: the bytes taken
    int status = TRH_OK;         // the first error, kept
    char message[160] = "";

    Transcript(int curve, bool reader) : curve(curve), reader(reader) {}

    int fail(const char* what) {
        if (status == TRH_OK) {
            status = TRH_EINVAL;
            snprintf(message, sizeof(message), "transcript: %s", what);
        }
        return status;
    }

    // ---- absorbing: the affine point / the scalar in register form (Montgomery) -------------------------------------------------------
    template <class B> int absorb_point(const Affine<B>& p) {
        if (aff_is_identity(p)) return fail("cannot write points at infinity to the transcript");
        uint8_t buf[65];
        u32 w[8];
        buf[0] = TRANSCRIPT_PREFIX_POINT;
        fe_store(fe_from_mont(p.x), w);
        memcpy(buf + 1, w, 32);
        fe_store(fe_from_mont(p.y), w);
        memcpy(buf + 33, w, 32);
        state.update(buf, sizeof(buf));
        return TRH_OK;
    }
    template <class S> void absorb_scalar_canonical(const u32 (&w)[8]) {
        uint8_t buf[33];
        buf[0] = TRANSCRIPT_PREFIX_SCALAR;
        memcpy(buf + 1, w, 32);
        state.update(buf, sizeof(buf));
    }
    template <class B> static Affine<B> affine_of(const uint64_t xyz[12]) {
        JacobianMem j;
        memcpy(&j, xyz, 96);
        return xyzz_to_affine(xyzz_from_jacobian(jac_load<B>(j)));
    }

    // ---- the operations; the caller holds mu ------------------------------------------------------------------------------------------
    template <class Cv> int common_point(const uint64_t xyz[12]) {
        if (status != TRH_OK) return status;
        return absorb_point(affine_of<typename Cv::Base>(xyz));
    }
    template <class Cv> int common_scalar(const uint64_t s_mont[4]) {
        if (status != TRH_OK) return status;
        u32 w[8];
        memcpy(w, s_mont, 32);
        fe_store(fe_from_mont(fe_load<typename Cv::Scalar>(w)), w);
        absorb_scalar_canonical<typename Cv::Scalar>(w);
        return TRH_OK;
    }
    template <class Cv> int write_point(const uint64_t xyz[12]) {
        if (status != TRH_OK) return status;
        if (reader) return fail("write_point on a reader");
        const Affine<typename Cv::Base> p = affine_of<typename Cv::Base>(xyz);
        if (absorb_point(p) != TRH_OK) return status;
        u32 e[8];
        point_encode(p.x, p.y, e);
        const uint8_t* b = (const uint8_t*)e;
        bytes.insert(bytes.end(), b, b + 32);
        return TRH_OK;
    }
    template <class Cv> int write_scalar(const uint64_t s_mont[4]) {
        if (status != TRH_OK) return status;
        if (reader) return fail("write_scalar on a reader");
        u32 w[8];
        memcpy(w, s_mont, 32);
        fe_store(fe_from_mont(fe_load<typename Cv::Scalar>(w)), w);
        absorb_scalar_canonical<typename Cv::Scalar>(w);
        const uint8_t* b = (const uint8_t*)w;
        bytes.insert(bytes.end(), b, b + 32);
        return TRH_OK;
    }
    template <class Cv> int squeeze_challenge_scalar(uint64_t out_mont[4]) {
        memset(out_mont, 0, 32);
        if (status != TRH_OK) return status;
        const uint8_t prefix = TRANSCRIPT_PREFIX_CHALLENGE;
        state.update(&prefix, 1);
        Blake2b copy = state;  // finish() ends the state it runs on; the sponge itself goes on
        uint8_t digest[BLAKE2B_OUT];
        copy.finish(digest);
        u32 w[16], r[8];
        memcpy(w, digest, 64);  // little endian: word j of the integer is bytes 4 j .. 4 j + 3
        fe_store(fe_from_u512<typename Cv::Scalar>(w), r);
        memcpy(out_mont, r, 32);
        return TRH_OK;
    }
    template <class Cv> int read_point(uint64_t out_xy[8]) {
        memset(out_xy, 0, 64);
        if (status != TRH_OK) return status;
        if (!reader) return fail("read_point on a writer");
        if (bytes.size() - at < 32) return fail("read_point: fewer than 32 bytes of the proof are left");
        u32 e[8];
        memcpy(e, bytes.data() + at, 32);
        Affine<typename Cv::Base> p;
        if (!point_decode(e, p.x, p.y, sqrt_table_host<typename Cv::Base>())) return fail("read_point: not the encoding of a point");
        if (absorb_point(p) != TRH_OK) return status;
        at += 32;
        AffineMem m;
        aff_store(p, m);
        memcpy(out_xy, &m, 64);
        return TRH_OK;
    }
    template <class Cv> int read_scalar(uint64_t out_mont[4]) {
        memset(out_mont, 0, 32);
        if (status != TRH_OK) return status;
        if (!reader) return fail("read_scalar on a writer");
        if (bytes.size() - at < 32) return fail("read_scalar: fewer than 32 bytes of the proof are left");
        u32 w[8], r[8];
        memcpy(w, bytes.data() + at, 32);
        if (!words_below_modulus<typename Cv::Scalar>(w)) return fail("read_scalar: the value is not below the modulus");
        at += 32;
        absorb_scalar_canonical<typename Cv::Scalar>(w);
        fe_store(fe_to_mont(fe_load<typename Cv::Scalar>(w)), r);
        memcpy(out_mont, r, 32);
        return TRH_OK;
    }
};

}  // namespace trh

#ifdef TRH_TRANSCRIPT_ABI
// ---- the trh_tr_* entries of include/trh.h ---------------------------------------------------------------------------------------------
struct trh_tr : trh::Transcript {
    using trh::Transcript::Transcript;
};

namespace trh {
namespace {

// runs op under the handle's lock; a refusal goes to trh_last_error() with the handle's own message
template <class Op> int tr_run(trh_tr_t t, const char* who, bool pointers_ok, Op&& op) {
    if (!t || !pointers_ok) { set_error("%s: null pointer", who); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(t->mu);
    const int rc = with_curve(t->curve, [&](auto cv) { return op(cv); });
    if (rc != TRH_OK) set_error("%s", t->message);
    return rc;
}
int tr_create(int curve_id, bool reader, const uint8_t* proof, size_t len, trh_tr_t* out, const char* who) {
    if (curve_id != TRH_PALLAS && curve_id != TRH_VESTA) { set_error("unknown curve id %d", curve_id); return TRH_EINVAL; }
    if (!out || (len && !proof)) { set_error("%s: null pointer", who); return TRH_EINVAL; }
    trh_tr* t = new (std::nothrow) trh_tr(curve_id, reader);
    if (!t) { set_error("%s: out of memory", who); return TRH_ENOMEM; }
    try {
        if (len) t->bytes.assign(proof, proof + len);
    } catch (const std::bad_alloc&) {
        delete t;
        set_error("%s: out of memory", who);
        return TRH_ENOMEM;
    }
    *out = t;
    return TRH_OK;
}
// the three callbacks of trh_transcript_t over a handle: plain C functions, nothing to report where they stand (the handle keeps the error)
void tr_cb_write_point(void* ctx, const uint64_t xyz[12]) { trh_tr_write_point((trh_tr_t)ctx, xyz); }
void tr_cb_write_scalar(void* ctx, const uint64_t s_mont[4]) { trh_tr_write_scalar((trh_tr_t)ctx, s_mont); }
void tr_cb_squeeze(void* ctx, uint64_t out_mont[4]) { trh_tr_squeeze_challenge_scalar((trh_tr_t)ctx, out_mont); }

}  // namespace
}  // namespace trh

extern "C" {

int trh_tr_create_writer(int curve_id, trh_tr_t* out) { return trh::tr_create(curve_id, false, nullptr, 0, out, "tr_create_writer"); }
int trh_tr_create_reader(int curve_id, const uint8_t* proof, size_t len, trh_tr_t* out) { return trh::tr_create(curve_id, true, proof, len, out, "tr_create_reader"); }
void trh_tr_destroy(trh_tr_t t) { delete t; }

int trh_tr_common_point(trh_tr_t t, const uint64_t xyz[12]) {
    return trh::tr_run(t, "tr_common_point", xyz != nullptr, [&](auto cv) { return t->template common_point<decltype(cv)>(xyz); });
}
int trh_tr_common_scalar(trh_tr_t t, const uint64_t s_mont[4]) {
    return trh::tr_run(t, "tr_common_scalar", s_mont != nullptr, [&](auto cv) { return t->template common_scalar<decltype(cv)>(s_mont); });
}
int trh_tr_write_point(trh_tr_t t, const uint64_t xyz[12]) {
    return trh::tr_run(t, "tr_write_point", xyz != nullptr, [&](auto cv) { return t->template write_point<decltype(cv)>(xyz); });
}
int trh_tr_write_scalar(trh_tr_t t, const uint64_t s_mont[4]) {
    return trh::tr_run(t, "tr_write_scalar", s_mont != nullptr, [&](auto cv) { return t->template write_scalar<decltype(cv)>(s_mont); });
}
int trh_tr_read_point(trh_tr_t t, uint64_t out_xy[8]) {
    return trh::tr_run(t, "tr_read_point", out_xy != nullptr, [&](auto cv) { return t->template read_point<decltype(cv)>(out_xy); });
}
int trh_tr_read_scalar(trh_tr_t t, uint64_t out_mont[4]) {
    return trh::tr_run(t, "tr_read_scalar", out_mont != nullptr, [&](auto cv) { return t->template read_scalar<decltype(cv)>(out_mont); });
}
int trh_tr_squeeze_challenge_scalar(trh_tr_t t, uint64_t out_mont[4]) {
    return trh::tr_run(t, "tr_squeeze_challenge_scalar", out_mont != nullptr, [&](auto cv) { return t->template squeeze_challenge_scalar<decltype(cv)>(out_mont); });
}

int trh_tr_callbacks(trh_tr_t t, trh_transcript_t* out) {
    if (!t || !out) { trh::set_error("tr_callbacks: null pointer"); return TRH_EINVAL; }
    if (t->reader) { trh::set_error("tr_callbacks: the handle is a reader"); return TRH_EINVAL; }
    out->ctx = t;
    out->write_point = trh::tr_cb_write_point;
    out->write_scalar = trh::tr_cb_write_scalar;
    out->squeeze_challenge_scalar = trh::tr_cb_squeeze;
    return TRH_OK;
}

int trh_tr_status(trh_tr_t t) {
    if (!t) { trh::set_error("tr_status: null handle"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(t->mu);
    if (t->status != TRH_OK) trh::set_error("%s", t->message);
    return t->status;
}
int trh_tr_message(trh_tr_t t, char* out, size_t cap) {
    if (!t || !out || !cap) { trh::set_error("tr_message: null pointer"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(t->mu);
    snprintf(out, cap, "%s", t->message);
    return TRH_OK;
}

int trh_tr_bytes_len(trh_tr_t t, size_t* len) {
    if (!t || !len) { trh::set_error("tr_bytes_len: null pointer"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(t->mu);
    *len = t->bytes.size();
    return TRH_OK;
}
int trh_tr_bytes(trh_tr_t t, uint8_t* out, size_t cap) {
    if (!t) { trh::set_error("tr_bytes: null handle"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(t->mu);
    if (t->bytes.size() > cap || (!out && !t->bytes.empty())) { trh::set_error("tr_bytes: %zu bytes do not fit a buffer of %zu", t->bytes.size(), out ? cap : (size_t)0); return TRH_EINVAL; }
    if (!t->bytes.empty()) memcpy(out, t->bytes.data(), t->bytes.size());
    return TRH_OK;
}
int trh_tr_remaining(trh_tr_t t, size_t* len) {
    if (!t || !len) { trh::set_error("tr_remaining: null pointer"); return TRH_EINVAL; }
    if (!t->reader) { trh::set_error("tr_remaining: the handle is a writer"); return TRH_EINVAL; }
    std::lock_guard<std::mutex> lk(t->mu);
    *len = t->bytes.size() - t->at;
    return TRH_OK;
}

}  // extern "C"
#endif  // TRH_TRANSCRIPT_ABI
