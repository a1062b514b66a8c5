// bins_selftest.cpp — CPU-only run of csrc/rsx_bin_math.hpp, the bin arithmetic of rsx_segmented_histogram: the functions the kernels call,
// compiled by plain g++, on a small case file.  No library, no HIP.  (Also the program to build with -fsanitize=address,undefined.)
//
//   bins_selftest CASE_FILE        reads the case, writes one line per key: its bin, 4294967295 for a dropped key
//
// Case file, whitespace-separated unsigned decimals:
//   key_bytes (4 | 8)  key_kind (0 unsigned | 1 signed | 2 float)  descending (0 | 1)  form (0 even | 2 edges)
//   num_bins  lo_bits  hi_bits  width_shift  num_edges (num_bins + 1 in the edges form, else 0)  num_keys
//   then the edges and the keys as bit patterns.
// Exit code: 0; 2 for a case the even form's argument check refuses (its reason on stderr); 1 for a malformed file.
#include "rsx_bin_math.hpp"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <vector>

template <typename Key>
static int run(std::istream& in, int kind, bool descending, int form, uint64_t nbins, uint64_t lo_bits, uint64_t hi_bits, uint32_t shift, uint64_t nedges,
               uint64_t nkeys)
{
    constexpr Key sign = static_cast<Key>(Key{1} << (sizeof(Key) * 8 - 1));
    // the engine's order constants (order_consts of the C ABI)
    Key a, m;
    if (kind == 2) {
        m = static_cast<Key>(~sign);
        a = descending ? static_cast<Key>(~sign) : sign;
    } else {
        m = 0;
        const Key flip = kind == 1 ? sign : Key{0};
        a = descending ? static_cast<Key>(~flip) : flip;
    }
    std::vector<Key> edges(nedges), keys(nkeys);
    for (Key& x : edges) {
        uint64_t v;
        if (!(in >> v)) return 1;
        x = rsx_bins::order_map(static_cast<Key>(v), a, m);
    }
    for (Key& x : keys) {
        uint64_t v;
        if (!(in >> v)) return 1;
        x = static_cast<Key>(v);
    }
    const uint32_t B = static_cast<uint32_t>(nbins);
    if (form == rsx_bins::kFormEdges) {
        if (nedges != nbins + 1) return 1;
        for (const Key k : keys) {
            const Key q[1] = {rsx_bins::order_map(k, a, m)};
            uint32_t base[1] = {0}, len[1] = {B + 1u};
            rsx_bins::bisect_right<1>([&](uint32_t i) { return edges[i]; }, q, base, len);
            std::cout << rsx_bins::edges_bin_of(base[0], q[0], edges[B], B) << "\n";
        }
        return 0;
    }
    rsx_bins::EvenArgs<Key> ev;
    const char* what = nullptr;
    if (!rsx_bins::make_even_args<Key>(kind == 2, kind == 1, descending, lo_bits, hi_bits, shift, nbins, &ev, &what)) {
        std::cerr << "refused: " << what << "\n";
        return 2;
    }
    for (const Key k : keys) {
        std::cout << (kind == 2 ? rsx_bins::even_float_bin(k, ev, B) : rsx_bins::even_int_bin(k, ev, B)) << "\n";
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::cerr << "usage: bins_selftest CASE_FILE\n";
        return 1;
    }
    std::ifstream in(argv[1]);
    uint64_t key_bytes, kind, descending, form, nbins, lo_bits, hi_bits, shift, nedges, nkeys;
    if (!(in >> key_bytes >> kind >> descending >> form >> nbins >> lo_bits >> hi_bits >> shift >> nedges >> nkeys)) return 1;
    if ((key_bytes != 4 && key_bytes != 8) || kind > 2 || (form != 0 && form != 2) || nbins == 0 || nbins > (1ull << 31) || nedges > (1u << 20) ||
        nkeys > (1u << 24))
        return 1;
    const int rc = key_bytes == 4 ? run<uint32_t>(in, static_cast<int>(kind), descending != 0, static_cast<int>(form), nbins, lo_bits, hi_bits,
                                                  static_cast<uint32_t>(shift), nedges, nkeys)
                                  : run<uint64_t>(in, static_cast<int>(kind), descending != 0, static_cast<int>(form), nbins, lo_bits, hi_bits,
                                                  static_cast<uint32_t>(shift), nedges, nkeys);
    std::cout.flush();
    return rc;
}
