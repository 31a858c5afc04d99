// From a runtime field / curve id of the C ABI to the template instantiation: with_field(field, fn) and with_curve(curve, fn) call the
// generic lambda fn with a tag -- FpParams{} / FqParams{}, PallasTag{} / VestaTag{} -- and return what it returns, so that the arguments
// of a launch are written once for both instantiations and the (scalar field, base field) pairing of a curve is written here only.
//     return with_field(field, [&](auto f) { return powers_t<decltype(f)>(out_dev, n, x_mont, s); });
//     with_curve(curve, [&](auto cv) { hipLaunchKernelGGL((k<typename decltype(cv)::Base>), ...); });
// The id has been validated by then (check_field / check_curve, ctx.h): any other value than TRH_FP / TRH_PALLAS takes the second tag.
// Plain C++, no HIP: tests/native/dispatch_test.cpp compiles it for the host alone.
#pragma once
#include "../../include/trh.h"
#include "field.h"

namespace trh {

struct PallasTag { using Scalar = FqParams; using Base = FpParams; };
struct VestaTag { using Scalar = FpParams; using Base = FqParams; };

template <class Fn>
inline auto with_field(int field, Fn&& fn) {
    if (field == TRH_FP) return fn(FpParams{});
    return fn(FqParams{});
}
template <class Fn>
inline auto with_curve(int curve, Fn&& fn) {
    if (curve == TRH_PALLAS) return fn(PallasTag{});
    return fn(VestaTag{});
}

}  // namespace trh
