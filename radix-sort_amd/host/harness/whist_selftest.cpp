// whist_selftest.cpp — CPU-only run of csrc/rsx_mass_math.hpp as rsx_segmented_weighted_histogram uses it: the mass of a weight, unsigned
// (mass_of_bits, rsx_segmented_weighted_select's rule) and signed (signed_mass_of_bits + signed_addend): the functions the kernel calls,
// compiled by plain g++, on a small case file.  No library, no HIP.
// (Also the program to build with -fsanitize=address,undefined: bin/whist_selftest_san.)
//
//   whist_selftest CASE_FILE
//
// Case file, one case per line, whitespace-separated decimals:
//   KIND WEIGHT_EXP SIGNED BITS     the weight with these bits (KIND 0 uint32, 1 float32, 2 float64; SIGNED 0 or 1; BITS unsigned)
// Output: one line per case, the 64-bit word the kernel adds for that weight as a signed decimal (the two's-complement reading: a
// uint32 mass and an unsigned float mass are never negative).
// Every float mass is also computed as the contract words it — ldexp(|w| or w, 31 - weight_exp), a truncating conversion, saturated at
// 2^31, negated for a negative weight in the signed form — and the two must agree.
// Exit code: 0; 1 for a malformed file (SIGNED with KIND 0 included); 2 if the header's mass differs from the ldexp form.
#include "rsx_mass_math.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

namespace {

int64_t mass_by_ldexp(double w, int32_t weight_exp, bool is_signed)
{
    const bool negative = is_signed && std::signbit(w);
    const double a = is_signed ? std::fabs(w) : w;
    if (!(a > 0.0)) return 0;
    const double s = std::ldexp(a, 31 - weight_exp);         // exact, or infinite, or below 1
    const int64_t m = s >= 2147483648.0 ? int64_t{1} << 31 : static_cast<int64_t>(s);
    return negative ? -m : m;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::cerr << "usage: whist_selftest CASE_FILE\n";
        return 1;
    }
    std::ifstream in(argv[1]);
    if (!in) return 1;
    uint32_t kind;
    while (in >> kind) {
        int32_t wexp;
        uint32_t is_signed;
        uint64_t bits;
        if (!(in >> wexp >> is_signed >> bits)) return 1;
        if (kind > rsx_mass::kWeightFloat64 || is_signed > 1 || wexp > rsx_mass::kMaxWeightExp || wexp < -rsx_mass::kMaxWeightExp) return 1;
        if (kind == rsx_mass::kWeightUint32 && (is_signed || wexp != 0)) return 1;
        if (kind != rsx_mass::kWeightFloat64 && bits > 0xFFFFFFFFull) return 1;
        uint64_t word;
        if (is_signed) {
            const rsx_mass::SignedMass sm = rsx_mass::signed_mass_of_bits(bits, kind, wexp);
            word = rsx_mass::signed_addend(sm.magnitude, sm.negative);
        } else {
            word = rsx_mass::mass_of_bits(bits, kind, wexp);
        }
        int64_t value;
        std::memcpy(&value, &word, sizeof value);
        if (kind == rsx_mass::kWeightFloat32) {
            const uint32_t b32 = static_cast<uint32_t>(bits);
            float w;
            std::memcpy(&w, &b32, sizeof w);
            if (value != mass_by_ldexp(static_cast<double>(w), wexp, is_signed != 0)) return 2;
        } else if (kind == rsx_mass::kWeightFloat64) {
            double w;
            std::memcpy(&w, &bits, sizeof w);
            if (value != mass_by_ldexp(w, wexp, is_signed != 0)) return 2;
        }
        std::cout << value << "\n";
    }
    if (!in.eof()) return 1;
    std::cout.flush();
    return 0;
}
