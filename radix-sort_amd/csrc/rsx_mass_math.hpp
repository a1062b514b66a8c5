// rsx_mass_math.hpp — the mass of a weight and the target rule of rsx_segmented_weighted_select, pure: a weight is quantised once to a 32-bit
// fixed-point mass, every sum of masses is a 64-bit integer add, and a target is a mass in [1, total].  No HIP type in here, so that plain
// g++ compiles it too (host/harness/wselect_selftest.cpp runs it on a case file); under hipcc every function is __host__ __device__.
// Included by rsx_wselect.hpp, and by rsx_wbins.hpp: rsx_segmented_weighted_histogram sums the same masses per bin, and has a signed form of
// them (signed_mass_of_bits below; host/harness/whist_selftest.cpp runs it).
//
//   mass(w) = 0 unless w > 0 (NaN, negatives and both zeros weigh nothing), else min(floor(w * 2^(31 - weight_exp)), 2^31)
//
// i.e. ldexp(w, 31 - weight_exp) and a truncating conversion that saturates.  Scaling a binary float by a power of two is exact, so no
// rounding enters; the functions below take the same value from the bits of w (significand shifted by the exponent), which is that
// product without a floating-point unit in between: no denormal mode, no overflow to infinity and no conversion of an out-of-range
// value can change it, on the host or on the device.  wselect_selftest compares them with the ldexp form.
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RSX_MASS_HD __host__ __device__ __forceinline__
#else
#define RSX_MASS_HD inline
#endif

namespace rsx_mass {

constexpr uint32_t kWeightUint32 = 0, kWeightFloat32 = 1, kWeightFloat64 = 2;      // RSX_WEIGHT_*
constexpr uint32_t kMassOne = 1u << 31;                                             // the mass of a weight of 2^weight_exp or more
constexpr int32_t kMaxWeightExp = 2048;                                             // |weight_exp| beyond every float64 exponent is refused

// floor(sig * 2^sh) saturated at 2^31, for a significand sig > 0 below 2^53
RSX_MASS_HD uint32_t scaled(uint64_t sig, int sh)
{
    if (sh >= 0) {
        if (sh > 31 || sig >= (1ull << (31 - sh))) return kMassOne;
        return static_cast<uint32_t>(sig << sh);
    }
    if (sh <= -64) return 0u;
    const uint64_t v = sig >> (-sh);
    return v >= kMassOne ? kMassOne : static_cast<uint32_t>(v);
}

// the mass of a float32 weight given by its bits
RSX_MASS_HD uint32_t mass_f32_bits(uint32_t b, int32_t weight_exp)
{
    const uint32_t e = (b >> 23) & 0xFFu, m = b & 0x7FFFFFu;
    if ((b >> 31) || (e == 0u && m == 0u)) return 0u;          // negative sign (-0, -NaN included), +0
    if (e == 0xFFu) return m ? 0u : kMassOne;                    // NaN, +inf
    const uint64_t sig = e ? (m | 0x800000u) : m;                // w = sig * 2^(max(e, 1) - 150)
    return scaled(sig, static_cast<int>(e ? e : 1u) - 150 + 31 - weight_exp);
}

// the mass of a float64 weight given by its bits
RSX_MASS_HD uint32_t mass_f64_bits(uint64_t b, int32_t weight_exp)
{
    const uint32_t e = static_cast<uint32_t>(b >> 52) & 0x7FFu;
    const uint64_t m = b & 0xFFFFFFFFFFFFFull;
    if ((b >> 63) || (e == 0u && m == 0u)) return 0u;
    if (e == 0x7FFu) return m ? 0u : kMassOne;
    const uint64_t sig = e ? (m | (1ull << 52)) : m;             // w = sig * 2^(max(e, 1) - 1075)
    return scaled(sig, static_cast<int>(e ? e : 1u) - 1075 + 31 - weight_exp);
}

// The mass of the weight whose bits are `bits` (the low 32 for the 4-byte kinds).  RSX_WEIGHT_UINT32: the stored word.
RSX_MASS_HD uint32_t mass_of_bits(uint64_t bits, uint32_t kind, int32_t weight_exp)
{
    if (kind == kWeightUint32) return static_cast<uint32_t>(bits);
    if (kind == kWeightFloat32) return mass_f32_bits(static_cast<uint32_t>(bits), weight_exp);
    return mass_f64_bits(bits, weight_exp);
}

// The SIGNED mass of a float weight (rsx_segmented_weighted_histogram with RSX_WHIST_SIGNED; float kinds only): the mass of |w| — the
// sign bit cleared, then the rule above — as `magnitude`, and whether it is added negated.  NaN of either sign and both zeros weigh
// nothing (and are not negative); -inf weighs -2^31.  The sum a signed mass enters is a two's-complement int64: add
// signed_addend(magnitude, negative) as a uint64, modulo 2^64.
struct SignedMass {
    uint32_t magnitude;
    bool negative;
};

RSX_MASS_HD SignedMass signed_mass_of_bits(uint64_t bits, uint32_t kind, int32_t weight_exp)
{
    const bool f32 = kind == kWeightFloat32;
    const uint64_t sign = f32 ? (1ull << 31) : (1ull << 63);
    const uint64_t low = f32 ? (bits & 0xFFFFFFFFull) : bits;
    const uint32_t mag = f32 ? mass_f32_bits(static_cast<uint32_t>(low & ~sign), weight_exp) : mass_f64_bits(low & ~sign, weight_exp);
    return SignedMass{mag, mag != 0u && (low & sign) != 0};
}

RSX_MASS_HD uint64_t signed_addend(uint32_t magnitude, bool negative)
{
    const uint64_t m = magnitude;
    return negative ? 0ull - m : m;
}

// The target of one slot as a mass in [1, total]; 0: the slot has no answer.
//   absolute form: `bits` is the uint64 target T itself; 0 and T > total have no answer.
//   fraction form: `bits` are those of the double f; T = clamp(ceil((double)total * f), 1, total): one IEEE multiply of the round-to-nearest
//   conversion of total, then ceil.  NaN and total == 0 have no answer; f <= 0 gives 1 (the first element with mass), f >= 1 gives total.
RSX_MASS_HD uint64_t target_of(uint64_t bits, bool fraction, uint64_t total)
{
    if (!fraction) return bits >= 1 && bits <= total ? bits : 0ull;
    double f;
    memcpy(&f, &bits, sizeof f);
    if (f != f || total == 0) return 0ull;
    const double td = static_cast<double>(total);
    const double x = td * f;                         // |x| may be infinite; it is compared before it is converted
    if (!(x > 1.0)) return 1ull;
    if (x >= td) return total;                       // td may lie above total by rounding: everything at or above it is the whole mass
    const uint64_t t = static_cast<uint64_t>(x);     // 1 < x < td <= 2^63: in range
    return static_cast<double>(t) < x ? t + 1 : t;   // ceil (t + 1 <= total: x lies below td, and no double lies between total and td)
}

}  // namespace rsx_mass
