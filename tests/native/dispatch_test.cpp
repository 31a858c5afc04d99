// Host driver of csrc/dispatch.h: with_field / with_curve hand the lambda the tag of the id, pair a curve's scalar and base field the
// right way round, and pass the lambda's value through.  Built by g++ with -fsanitize=undefined -fno-sanitize-recover
// (tests/test_encoding_host.py).  No GPU, no HIP.  Prints "dispatch: ok" and returns 0, or names the first failure and returns 1.
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../tiny-ram-halo2_amd/csrc/dispatch.h"

using namespace trh;

// the moduli as the oracle writes them (pasta.py P and Q, little-endian 32-bit words): p of Pallas' base field, q of Vesta's
static const u32 P_WORDS[8] = {0x00000001u, 0x992d30edu, 0x094cf91bu, 0x224698fcu, 0u, 0u, 0u, 0x40000000u};
static const u32 Q_WORDS[8] = {0x00000001u, 0x8c46eb21u, 0x0994a8ddu, 0x224698fcu, 0u, 0u, 0u, 0x40000000u};

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { std::fprintf(stderr, "dispatch: FAILED %s\n", what); ++failures; }
}
template <class F> static bool modulus_is(const u32 (&w)[8]) { return std::memcmp(F::MOD, w, 32) == 0; }

int main() {
    expect(std::memcmp(P_WORDS, Q_WORDS, 32) != 0, "the two moduli differ");
    // with_field: the tag's modulus is the field's
    expect(with_field(TRH_FP, [](auto f) { return modulus_is<decltype(f)>(P_WORDS); }), "TRH_FP -> Fp");
    expect(with_field(TRH_FQ, [](auto f) { return modulus_is<decltype(f)>(Q_WORDS); }), "TRH_FQ -> Fq");
    expect(with_field(TRH_FP, [](auto f) { return decltype(f)::ID; }) == TRH_FP && with_field(TRH_FQ, [](auto f) { return decltype(f)::ID; }) == TRH_FQ, "tag ID = field id");
    // with_curve: Pallas has scalars in Fq and coordinates in Fp, Vesta the other way round
    expect(with_curve(TRH_PALLAS, [](auto cv) { return modulus_is<typename decltype(cv)::Scalar>(Q_WORDS) && modulus_is<typename decltype(cv)::Base>(P_WORDS); }), "Pallas -> (scalar Fq, base Fp)");
    expect(with_curve(TRH_VESTA, [](auto cv) { return modulus_is<typename decltype(cv)::Scalar>(P_WORDS) && modulus_is<typename decltype(cv)::Base>(Q_WORDS); }), "Vesta -> (scalar Fp, base Fq)");
    static_assert(std::is_same<PallasTag::Scalar, VestaTag::Base>::value && std::is_same<PallasTag::Base, VestaTag::Scalar>::value, "the cycle");
    // an id that passed check_field / check_curve and is not the first one takes the second instantiation, as the if / else chains did
    expect(with_field(5, [](auto f) { return decltype(f)::ID; }) == TRH_FQ, "other field id -> second tag");
    expect(with_curve(5, [](auto cv) { return decltype(cv)::Base::ID; }) == TRH_FQ, "other curve id -> second tag");
    // the lambda's value comes back, whatever its type; captures are seen; a void lambda compiles
    int calls = 0;
    expect(with_field(TRH_FQ, [&](auto f) { ++calls; return 40 + decltype(f)::ID; }) == 41, "int passed through");
    expect(with_curve(TRH_PALLAS, [&](auto cv) { ++calls; return 0.5 + decltype(cv)::Scalar::ID; }) == 1.5, "double passed through");
    with_curve(TRH_VESTA, [&](auto) { ++calls; });
    expect(calls == 3, "the lambda ran once per call");
    if (failures) return 1;
    std::printf("dispatch: ok\n");
    return 0;
}
