// rsx_bin_math.hpp — the bin arithmetic of rsx_segmented_histogram, pure: the order map, the even forms and the bisection of the edges on
// a plain array.  No HIP type in here, so that plain g++ compiles it too (host/harness/bins_selftest.cpp runs it on a case file, which
// makes the device's arithmetic checkable without a GPU); under hipcc every function is __host__ __device__.  Included by rsx_bins.hpp.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSX_HD __host__ __device__ __forceinline__
#define RSX_UNROLL _Pragma("unroll")
#else
#define RSX_HD inline
#define RSX_UNROLL
#endif

namespace rsx_bins {

constexpr uint32_t kNoBin = 0xFFFFFFFFu;      // the key falls into no bin: dropped

// The forms of the call: which arithmetic turns a key into a bin.
constexpr int kFormEvenInt = 0, kFormEvenFloat = 1, kFormEdges = 2;

// float for 4-byte keys, double for 8-byte keys
template <typename Key> struct FloatOf;
template <> struct FloatOf<uint32_t> { using type = float; };
template <> struct FloatOf<uint64_t> { using type = double; };

RSX_HD uint32_t sign_fill(uint32_t x) { return static_cast<uint32_t>(static_cast<int32_t>(x) >> 31); }
RSX_HD uint64_t sign_fill(uint64_t x) { return static_cast<uint64_t>(static_cast<int64_t>(x) >> 63); }

// rsx::codec_encode: the engine's order as the unsigned order of the mapped key, (A, M) from order_consts
template <typename Key>
RSX_HD Key order_map(Key x, Key a, Key m)
{
    return (x ^ (sign_fill(x) & m)) ^ a;
}

// (x - lo) and (. * scale), each rounded once to nearest: no contraction, no reassociation
#if defined(__HIP_DEVICE_COMPILE__)
RSX_HD float sub_rn(float a, float b) { return __fsub_rn(a, b); }
RSX_HD float mul_rn(float a, float b) { return __fmul_rn(a, b); }
RSX_HD double sub_rn(double a, double b) { return __dsub_rn(a, b); }
RSX_HD double mul_rn(double a, double b) { return __dmul_rn(a, b); }
#else
RSX_HD float sub_rn(float a, float b) { volatile float r = a - b; return r; }
RSX_HD float mul_rn(float a, float b) { volatile float r = a * b; return r; }
RSX_HD double sub_rn(double a, double b) { volatile double r = a - b; return r; }
RSX_HD double mul_rn(double a, double b) { volatile double r = a * b; return r; }
#endif

// What the even forms need, by value in the kernel arguments.  Integer keys: lo = the low bound under the ASCENDING map (lo ^ flip), flip =
// the sign bit of signed keys.  Float keys: lo, hi and scale = Key(B) / (hi - lo) as bit patterns.  descending: bin b becomes B - 1 - b.
template <typename Key>
struct EvenArgs {
    Key lo, hi, scale, flip;
    uint32_t shift, descending;
};

// The even form's arguments from the caller's bit patterns (host side, once per call); false: refused, *what says why.
template <typename Key>
inline bool make_even_args(bool is_float, bool is_signed, bool descending, uint64_t lo_bits, uint64_t hi_bits, uint32_t width_shift, uint64_t nbins,
                           EvenArgs<Key>* ev, const char** what)
{
    using F = typename FloatOf<Key>::type;
    *ev = EvenArgs<Key>{};
    ev->descending = descending ? 1u : 0u;
    if (is_float) {
        const Key lob = static_cast<Key>(lo_bits), hib = static_cast<Key>(hi_bits);
        const F lo = __builtin_bit_cast(F, lob), hi = __builtin_bit_cast(F, hib);
        if (width_shift != 0) {
            *what = "width_shift belongs to the integer key kinds (float keys: lo_bits and hi_bits)";
            return false;
        }
        if (!(lo - lo == 0) || !(hi - hi == 0) || !(lo < hi)) {
            *what = "lo_bits and hi_bits must be finite keys with lo < hi";
            return false;
        }
        volatile F width = hi - lo;                     // (each step rounded once, in the key's own precision)
        volatile F scale = static_cast<F>(nbins) / width;
        const F sc = scale;
        if (!(sc - sc == 0) || !(sc > 0)) {
            *what = "num_bins / (hi - lo) must be a finite positive number in the key's precision";
            return false;
        }
        ev->lo = lob;
        ev->hi = hib;
        ev->scale = __builtin_bit_cast(Key, sc);
        return true;
    }
    if (hi_bits != 0) {
        *what = "hi_bits belongs to the float key kinds (integer keys: lo_bits and width_shift)";
        return false;
    }
    if (width_shift >= 8u * sizeof(Key)) {
        *what = "width_shift must be below the key's width in bits";
        return false;
    }
    ev->flip = is_signed ? static_cast<Key>(Key{1} << (sizeof(Key) * 8 - 1)) : Key{0};
    ev->lo = static_cast<Key>(lo_bits) ^ ev->flip;
    ev->shift = width_shift;
    return true;
}

// Even form, integer keys: bin (k - lo) >> shift on the ascending-mapped words, kNoBin before lo or from bin B on.
template <typename Key>
RSX_HD uint32_t even_int_bin(Key k, const EvenArgs<Key>& p, uint32_t nbins)
{
    const Key u = k ^ p.flip;
    if (u < p.lo) return kNoBin;
    const Key d = static_cast<Key>(u - p.lo) >> p.shift;
    if (d >= static_cast<Key>(nbins)) return kNoBin;
    const uint32_t b = static_cast<uint32_t>(d);
    return p.descending ? nbins - 1u - b : b;
}

// Even form, float keys: min(B - 1, floor((x - lo) * scale)) for lo <= x <= hi by IEEE comparison (-0.0 is 0.0, a NaN is dropped).
template <typename Key>
RSX_HD uint32_t even_float_bin(Key k, const EvenArgs<Key>& p, uint32_t nbins)
{
    using F = typename FloatOf<Key>::type;
    const F x = __builtin_bit_cast(F, k), lo = __builtin_bit_cast(F, p.lo), hi = __builtin_bit_cast(F, p.hi);
    if (!(lo <= x && x <= hi)) return kNoBin;
    const F t = mul_rn(sub_rn(x, lo), __builtin_bit_cast(F, p.scale));       // >= 0 (or -0.0)
    const uint32_t b = t >= static_cast<F>(nbins - 1u) ? nbins - 1u : static_cast<uint32_t>(t);
    return p.descending ? nbins - 1u - b : b;
}

// N bisections in lockstep (rsx::search_bisect's arithmetic under RSX_SEARCH_RIGHT): at(i) = mapped edge i; (base[r], len[r]) in,
// base[r] = #{ i : at(i) <= q[r] } out on sorted edges.  Every index formed lies in [base, base + len) as given.
template <int N, typename Key, typename At>
RSX_HD void bisect_right(At&& at, const Key (&q)[N], uint32_t (&base)[N], uint32_t (&len)[N])
{
    uint32_t any = 0;
    RSX_UNROLL
    for (int r = 0; r < N; ++r) {
        any |= len[r];
    }
    while (any != 0) {
        Key k[N];
        RSX_UNROLL
        for (int r = 0; r < N; ++r) {
            k[r] = len[r] != 0 ? at(base[r] + (len[r] >> 1)) : Key{0};
        }
        any = 0;
        RSX_UNROLL
        for (int r = 0; r < N; ++r) {
            const uint32_t half = len[r] >> 1;
            const bool before = len[r] != 0 && k[r] <= q[r];
            base[r] = before ? base[r] + half + 1 : base[r];
            len[r] = before ? len[r] - half - 1 : half;
            any |= len[r];
        }
    }
}

// Edges form: j = the position of the mapped key q among the nbins + 1 mapped edges -> bin j - 1 for 1 <= j <= B; the last bin is closed
// on both sides (j == B + 1 and q is edge B itself: the map is a bijection, so equal mapped words are equal bits); kNoBin otherwise.
template <typename Key>
RSX_HD uint32_t edges_bin_of(uint32_t j, Key q, Key last_edge, uint32_t nbins)
{
    if (j >= 1u && j <= nbins) return j - 1u;
    return j == nbins + 1u && q == last_edge ? nbins - 1u : kNoBin;
}

}  // namespace rsx_bins
