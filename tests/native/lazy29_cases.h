// Case runner of the signed 29-bit lazy domain (csrc/field.h "Fy", csrc/curve.h "XYZZz"), shared by the host and the device: one
// function template per operation under test, each from raw operand limbs to raw result limbs, so that the SAME records go through
// the inline-assembly branch of field.h on the device (lazy29_dev_test.hip) and through its plain C++ branch on the host
// (lazy29_vec_test.cpp under UBSan, and the host pass of the device driver).  tests/lazy29_gen.py writes the records and holds the
// big-integer reference of every operation.
//
// Case file: flat little-endian records of LZ_IN_WORDS 32-bit words: op, field (0 Fp, 1 Fq), then eight operand slots of nine
// words (an Fy as its signed limbs; an operation that takes memory words reads the first eight words of a slot).  Records of one
// (op, field) are contiguous.  Result file: per record LZ_OUT_WORDS words: five result slots of nine words and one flag word
// (the bool of an operation that returns one).  Unused slots are zero.
#pragma once
#include "../../tiny-ram-halo2_amd/csrc/curve.h"

namespace lz {
using namespace trh;

constexpr int LZ_IN_SLOTS = 8, LZ_OUT_SLOTS = 5;
constexpr int LZ_IN_WORDS = 2 + LZ_IN_SLOTS * NLIMBS, LZ_OUT_WORDS = LZ_OUT_SLOTS * NLIMBS + 1;

enum Op : int {
    OP_FROM_FE = 0, OP_TO_FE, OP_LOAD_STORE, OP_STORE_LOAD,
    OP_MUL, OP_MUL_NONNEG, OP_SQR, OP_MUL2, OP_MUL_SUB, OP_SQR_SUB_SUB2,
    OP_ADD, OP_SUB, OP_SUB_SUB2, OP_NORM, OP_BALANCE,
    OP_MUL_ADD_LAZY, OP_MUL_SUB_LAZY, OP_MUL_NEG_LAZY, OP_MUL_BAL_WIDE,
    OP_MAYBE_ZERO, OP_IS_ZERO,
    OP_PT_FROM_CANONICAL, OP_PT_TO_CANONICAL, OP_DBL_AFFINE, OP_DBL, OP_MADD, OP_MADD_MAIN, OP_PT_ADD,
    OP_COUNT
};

struct In { i32 s[LZ_IN_SLOTS][NLIMBS]; };
struct Out { i32 r[LZ_OUT_SLOTS][NLIMBS]; u32 flag; };

template <class F> TRH_HD Fy<F> get(const In& in, int k) {
    Fy<F> a;
#pragma unroll
    for (int i = 0; i < NLIMBS; ++i) a.l[i] = in.s[k][i];
    return a;
}
template <class F> TRH_HD void put(Out& o, int k, const Fy<F>& a) {
#pragma unroll
    for (int i = 0; i < NLIMBS; ++i) o.r[k][i] = a.l[i];
}
template <class F> TRH_HD Fe<F> get_fe(const In& in, int k) { return fe_load<F>((const u32*)in.s[k]); }
template <class F> TRH_HD void put_fe(Out& o, int k, const Fe<F>& a) { fe_store(a, (u32*)o.r[k]); }
template <class F> TRH_HD XYZZz<F> get_pt(const In& in, int k) {
    XYZZz<F> p; p.x = get<F>(in, k); p.y = get<F>(in, k + 1); p.zz = get<F>(in, k + 2); p.zzz = get<F>(in, k + 3); return p;
}
template <class F> TRH_HD AffineZ<F> get_aff(const In& in, int k) {
    AffineZ<F> p; p.x = get<F>(in, k); p.y = get<F>(in, k + 1); return p;
}
template <class F> TRH_HD void put_pt(Out& o, const XYZZz<F>& p) { put(o, 0, p.x); put(o, 1, p.y); put(o, 2, p.zz); put(o, 3, p.zzz); }

// ---- one function per operation ----
template <class F> TRH_HD void case_from_fe(const In& in, Out& o) { put(o, 0, fy_from_fe(get_fe<F>(in, 0))); }
template <class F> TRH_HD void case_to_fe(const In& in, Out& o) { put_fe(o, 0, fy_to_fe(get<F>(in, 0))); }
template <class F> TRH_HD void case_load_store(const In& in, Out& o) {  // words -> limbs (slot 0) -> words (slot 1)
    const u32* w = (const u32*)in.s[0];
    const Fy<F> a = fy_load<F>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
    put(o, 0, a);
    fy_store(a, (u32*)o.r[1]);
}
template <class F> TRH_HD void case_store_load(const In& in, Out& o) {  // limbs -> words (slot 0) -> limbs (slot 1)
    u32* w = (u32*)o.r[0];
    fy_store(get<F>(in, 0), w);
    put(o, 1, fy_load<F>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]));
}
template <class F> TRH_HD void case_mul(const In& in, Out& o) { put(o, 0, fy_mul(get<F>(in, 0), get<F>(in, 1))); }
template <class F> TRH_HD void case_mul_nonneg(const In& in, Out& o) { put(o, 0, fy_mul_nonneg(get<F>(in, 0), get<F>(in, 1))); }
template <class F> TRH_HD void case_sqr(const In& in, Out& o) { put(o, 0, fy_sqr(get<F>(in, 0))); }
template <class F> TRH_HD void case_mul2(const In& in, Out& o) { put(o, 0, fy_mul2(get<F>(in, 0), get<F>(in, 1), get<F>(in, 2), get<F>(in, 3))); }
template <class F> TRH_HD void case_mul_sub(const In& in, Out& o) { put(o, 0, fy_mul_sub(get<F>(in, 0), get<F>(in, 1), get<F>(in, 2))); }
template <class F> TRH_HD void case_sqr_sub_sub2(const In& in, Out& o) { put(o, 0, fy_sqr_sub_sub2(get<F>(in, 0), get<F>(in, 1), get<F>(in, 2))); }
template <class F> TRH_HD void case_add(const In& in, Out& o) { put(o, 0, fy_add(get<F>(in, 0), get<F>(in, 1))); }
template <class F> TRH_HD void case_sub(const In& in, Out& o) { put(o, 0, fy_sub(get<F>(in, 0), get<F>(in, 1))); }
template <class F> TRH_HD void case_sub_sub2(const In& in, Out& o) { put(o, 0, fy_sub_sub2(get<F>(in, 0), get<F>(in, 1), get<F>(in, 2))); }
template <class F> TRH_HD void case_norm(const In& in, Out& o) { put(o, 0, fy_norm(get<F>(in, 0))); }
template <class F> TRH_HD void case_balance(const In& in, Out& o) { put(o, 0, fy_balance(get<F>(in, 0))); }
template <class F> TRH_HD void case_mul_add_lazy(const In& in, Out& o) { put(o, 0, fy_mul(fy_add_lazy(get<F>(in, 0), get<F>(in, 1)), get<F>(in, 2))); }
template <class F> TRH_HD void case_mul_sub_lazy(const In& in, Out& o) { put(o, 0, fy_mul(fy_sub_lazy(get<F>(in, 0), get<F>(in, 1)), get<F>(in, 2))); }
template <class F> TRH_HD void case_mul_neg_lazy(const In& in, Out& o) { put(o, 0, fy_mul(fy_neg_lazy(get<F>(in, 0)), get<F>(in, 1))); }
template <class F> TRH_HD void case_mul_bal_wide(const In& in, Out& o) { put(o, 0, fy_mul(get<F>(in, 0), get<F>(in, 1))); }  // wide multiplicand, balanced twiddle
template <class F> TRH_HD void case_maybe_zero(const In& in, Out& o) { o.flag = fy_maybe_zero_mod(get<F>(in, 0)) ? 1u : 0u; }
template <class F> TRH_HD void case_is_zero(const In& in, Out& o) { o.flag = fy_is_zero_mod(get<F>(in, 0)) ? 1u : 0u; }
template <class F> TRH_HD void case_pt_from_canonical(const In& in, Out& o) {
    XYZZ<F> p; p.x = get_fe<F>(in, 0); p.y = get_fe<F>(in, 1); p.zz = get_fe<F>(in, 2); p.zzz = get_fe<F>(in, 3);
    const XYZZz<F> z = xyzzz_from_canonical(p);
    put_pt(o, z);
    o.flag = xyzzz_is_identity(z) ? 1u : 0u;
}
template <class F> TRH_HD void case_pt_to_canonical(const In& in, Out& o) {
    const XYZZ<F> c = xyzzz_to_canonical(get_pt<F>(in, 0));
    put_fe(o, 0, c.x); put_fe(o, 1, c.y); put_fe(o, 2, c.zz); put_fe(o, 3, c.zzz);
    o.flag = xyzz_is_identity(c) ? 1u : 0u;
}
template <class F> TRH_HD void case_dbl_affine(const In& in, Out& o) { put_pt(o, xyzzz_dbl_affine(get_aff<F>(in, 0))); }
template <class F> TRH_HD void case_dbl(const In& in, Out& o) { put_pt(o, xyzzz_dbl(get_pt<F>(in, 0))); }
template <class F> TRH_HD void case_madd(const In& in, Out& o) {
    XYZZz<F> acc = get_pt<F>(in, 0);
    xyzzz_madd(acc, get_aff<F>(in, 4));
    put_pt(o, acc);
}
template <class F> TRH_HD void case_madd_main(const In& in, Out& o) {  // acc (slots 0 .. 3), R (slot 4), "same x" (flag)
    XYZZz<F> acc = get_pt<F>(in, 0);
    Fy<F> R;
    o.flag = xyzzz_madd_main(acc, get_aff<F>(in, 4), R) ? 1u : 0u;
    put_pt(o, acc);
    put(o, 4, R);
}
template <class F> TRH_HD void case_pt_add(const In& in, Out& o) { put_pt(o, xyzzz_add(get_pt<F>(in, 0), get_pt<F>(in, 4))); }

template <int OP, class F> TRH_HD void run_case(const In& in, Out& o) {
#pragma unroll
    for (int k = 0; k < LZ_OUT_SLOTS; ++k)
#pragma unroll
        for (int i = 0; i < NLIMBS; ++i) o.r[k][i] = 0;
    o.flag = 0;
    if constexpr (OP == OP_FROM_FE) case_from_fe<F>(in, o);
    else if constexpr (OP == OP_TO_FE) case_to_fe<F>(in, o);
    else if constexpr (OP == OP_LOAD_STORE) case_load_store<F>(in, o);
    else if constexpr (OP == OP_STORE_LOAD) case_store_load<F>(in, o);
    else if constexpr (OP == OP_MUL) case_mul<F>(in, o);
    else if constexpr (OP == OP_MUL_NONNEG) case_mul_nonneg<F>(in, o);
    else if constexpr (OP == OP_SQR) case_sqr<F>(in, o);
    else if constexpr (OP == OP_MUL2) case_mul2<F>(in, o);
    else if constexpr (OP == OP_MUL_SUB) case_mul_sub<F>(in, o);
    else if constexpr (OP == OP_SQR_SUB_SUB2) case_sqr_sub_sub2<F>(in, o);
    else if constexpr (OP == OP_ADD) case_add<F>(in, o);
    else if constexpr (OP == OP_SUB) case_sub<F>(in, o);
    else if constexpr (OP == OP_SUB_SUB2) case_sub_sub2<F>(in, o);
    else if constexpr (OP == OP_NORM) case_norm<F>(in, o);
    else if constexpr (OP == OP_BALANCE) case_balance<F>(in, o);
    else if constexpr (OP == OP_MUL_ADD_LAZY) case_mul_add_lazy<F>(in, o);
    else if constexpr (OP == OP_MUL_SUB_LAZY) case_mul_sub_lazy<F>(in, o);
    else if constexpr (OP == OP_MUL_NEG_LAZY) case_mul_neg_lazy<F>(in, o);
    else if constexpr (OP == OP_MUL_BAL_WIDE) case_mul_bal_wide<F>(in, o);
    else if constexpr (OP == OP_MAYBE_ZERO) case_maybe_zero<F>(in, o);
    else if constexpr (OP == OP_IS_ZERO) case_is_zero<F>(in, o);
    else if constexpr (OP == OP_PT_FROM_CANONICAL) case_pt_from_canonical<F>(in, o);
    else if constexpr (OP == OP_PT_TO_CANONICAL) case_pt_to_canonical<F>(in, o);
    else if constexpr (OP == OP_DBL_AFFINE) case_dbl_affine<F>(in, o);
    else if constexpr (OP == OP_DBL) case_dbl<F>(in, o);
    else if constexpr (OP == OP_MADD) case_madd<F>(in, o);
    else if constexpr (OP == OP_MADD_MAIN) case_madd_main<F>(in, o);
    else if constexpr (OP == OP_PT_ADD) case_pt_add<F>(in, o);
}

// ---- host side of both drivers: the records of a file, its runs of one (op, field), the host pass ----
struct Rec { u32 op, field; In in; };
static_assert(sizeof(Rec) == LZ_IN_WORDS * 4 && sizeof(Out) == LZ_OUT_WORDS * 4, "record layout");

}  // namespace lz

#include <cstdio>
#include <vector>
namespace lz {

inline bool read_cases(const char* path, std::vector<Rec>& recs) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return false; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    bool ok = bytes >= 0 && bytes % (long)sizeof(Rec) == 0;
    if (ok) {
        recs.resize((size_t)bytes / sizeof(Rec));
        ok = recs.empty() || std::fread(recs.data(), sizeof(Rec), recs.size(), f) == recs.size();
    }
    std::fclose(f);
    for (size_t i = 0; ok && i < recs.size(); ++i) ok = recs[i].op < (u32)OP_COUNT && recs[i].field < 2u;
    if (!ok) std::fprintf(stderr, "%s: not a case file\n", path);
    return ok;
}
inline bool write_results(const char* path, const std::vector<Out>& a, const std::vector<Out>* b = nullptr) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", path); return false; }
    bool ok = a.empty() || std::fwrite(a.data(), sizeof(Out), a.size(), f) == a.size();
    if (b) ok = ok && (b->empty() || std::fwrite(b->data(), sizeof(Out), b->size(), f) == b->size());
    return std::fclose(f) == 0 && ok;
}
// end of the run of records that share recs[i]'s (op, field)
inline size_t run_end(const std::vector<Rec>& recs, size_t i) {
    size_t j = i;
    while (j < recs.size() && recs[j].op == recs[i].op && recs[j].field == recs[i].field) ++j;
    return j;
}
template <int OP> inline void host_one(const Rec& r, Out& o) {
    if (r.field == 0) run_case<OP, FpParams>(r.in, o); else run_case<OP, FqParams>(r.in, o);
}
template <int OP = 0> inline void host_case(const Rec& r, Out& o) {
    if constexpr (OP < OP_COUNT) {
        if ((int)r.op == OP) host_one<OP>(r, o); else host_case<OP + 1>(r, o);
    }
}

}  // namespace lz
