// expand_selftest.cpp — CPU-only run of csrc/rsx_expand_math.hpp, the owner rule and the tile-range arithmetic of rsx_segmented_expand: the
// functions the kernels call, compiled by plain g++, on a small case file.  No library, no HIP.  (Also the program to build with
// -fsanitize=address,undefined: bin/expand_selftest_san.)
//
//   expand_selftest CASE_FILE
//
// Case file, whitespace-separated unsigned decimals:
//   num_segments  n  out_addr  elem_bytes (4 | 8)
//   then the num_segments + 1 offsets (valid: non-decreasing, off[S] <= n).
// Output:
//   one line "o OWNER RANK" per position of [off[0], off[S]), in order (owner_plus_one - 1 and the position minus that segment's offset);
//   one line "t T SPLIT_LO SPLIT_HI A B HEAD NVEC TAIL" per tile of the absolute grid of 4096 positions over [0, n): the starts inside
//   the tile are the segments [SPLIT_LO, SPLIT_HI), [A, B) is the tile's part of [off[0], off[S]), and an output whose element 0 lies at
//   byte address out_addr stores it as HEAD single elements, NVEC 16-byte stores and TAIL single elements.
// Exit code: 0; 1 for a malformed file or offsets that are not valid.
#include "rsx_expand_math.hpp"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::cerr << "usage: expand_selftest CASE_FILE\n";
        return 1;
    }
    std::ifstream in(argv[1]);
    uint64_t nseg, n, addr, eb;
    if (!(in >> nseg >> n >> addr >> eb)) return 1;
    if (nseg > (1u << 22) || n > (1u << 24) || (eb != 4 && eb != 8) || addr % eb != 0) return 1;
    std::vector<uint64_t> off(nseg + 1);
    for (uint64_t& x : off) {
        if (!(in >> x)) return 1;
    }
    for (uint64_t s = 0; s < nseg; ++s) {
        if (off[s + 1] < off[s]) return 1;
    }
    if (off[nseg] > n) return 1;
    const uint64_t lo = off[0], hi = off[nseg];
    for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t own = rsx_expand::owner_plus_one(off.data(), nseg, i) - 1;
        if (own >= nseg) return 1;
        std::cout << "o " << own << " " << i - off[own] << "\n";
    }
    const uint64_t ntiles = (n + rsx_expand::kTileSlots - 1) >> rsx_expand::kTileShift;
    for (uint64_t t = 0; t < ntiles; ++t) {
        const rsx_expand::Range r = rsx_expand::tile_range(t, lo, hi);
        const rsx_expand::Stores st = rsx_expand::tile_stores(addr, static_cast<uint32_t>(eb), r.a, r.b);
        std::cout << "t " << t << " " << rsx_expand::tile_split(off.data(), nseg, t) << " " << rsx_expand::tile_split(off.data(), nseg, t + 1) << " " << r.a << " "
                  << r.b << " " << st.head << " " << st.nvec << " " << st.tail << "\n";
    }
    std::cout.flush();
    return 0;
}
