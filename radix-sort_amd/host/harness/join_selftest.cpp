// join_selftest.cpp — CPU-only run of csrc/rsx_join_math.hpp, the rules of rsx_segmented_join that are no kernel: the rows an A element
// emits for its number of partners and the kind of join, the two-level row offset and its split at the boundaries of the 4096-row output
// grid, and the store arithmetic of every output tile: the functions the kernels call, compiled by plain g++, on a small case file.  No
// library, no HIP.  (Also the program to build with -fsanitize=address,undefined: bin/join_selftest_san.)
//
//   join_selftest CASE_FILE
//
// Case file, whitespace-separated unsigned decimals:
//   op (0 .. 3)  na  out_capacity  out_addr  elem_bytes (4 | 8)
//   then na partner counts c_j (each at most 2^31), one per A position.
// The program lays the table out as join_count_kernel does (tiles of 4096 positions, the padding behind na counting 0, pre the exclusive
// prefix inside a tile, tbase the exclusive prefix of the tile totals with the total at its end) and prints:
//   one line "e E_0 E_1 ..." of the na effective counts, one line "f F_0 ..." of first_partner(j, c_j, op) (lb stands in as j);
//   one line "r R_0 ... R_na" of row_offset at every position and at na;
//   one line "p TOTAL";
//   one line "t U SPLIT_LO SPLIT_HI A B HEAD NVEC TAIL" per tile of the output grid up to the first that writes no row (that one included):
//   the A positions whose rows start inside tile U are [SPLIT_LO, SPLIT_HI), [A, B) are the rows it writes, and an output whose element 0
//   lies at byte address out_addr stores them as HEAD single elements, NVEC 16-byte stores and TAIL single elements.
// Exit code: 0; 1 for a malformed file.
#include "rsx_join_math.hpp"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <vector>

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::cerr << "usage: join_selftest CASE_FILE\n";
        return 1;
    }
    std::ifstream in(argv[1]);
    uint64_t op, na, cap, addr, eb;
    if (!(in >> op >> na >> cap >> addr >> eb)) return 1;
    if (op > rsx_join::kAnti || na > (1u << 22) || (eb != 4 && eb != 8) || addr % eb != 0) return 1;
    std::vector<uint64_t> c(na);
    for (uint64_t& x : c) {
        if (!(in >> x) || x > (1ull << 31)) return 1;
    }
    const uint64_t ntiles = (na + rsx_join::kTileSlots - 1) >> rsx_join::kTileShift;
    std::vector<uint64_t> pre(ntiles << rsx_join::kTileShift, 0), tbase(ntiles + 1, 0);
    std::cout << "e";
    for (uint64_t t = 0; t < ntiles; ++t) {
        uint64_t sum = 0;
        for (uint64_t k = 0; k < rsx_join::kTileSlots; ++k) {
            const uint64_t j = (t << rsx_join::kTileShift) + k;
            pre[j] = sum;
            if (j < na) {
                const uint64_t e = rsx_join::effective_count(c[j], static_cast<uint32_t>(op));
                std::cout << " " << e;
                sum += e;
            }
        }
        tbase[t + 1] = tbase[t] + sum;
    }
    std::cout << "\nf";
    for (uint64_t j = 0; j < na; ++j) {
        std::cout << " " << rsx_join::first_partner(static_cast<uint32_t>(j), c[j], static_cast<uint32_t>(op));
    }
    std::cout << "\nr";
    for (uint64_t j = 0; j <= na; ++j) {
        std::cout << " " << rsx_join::row_offset(tbase.data(), pre.data(), ntiles, j);
    }
    const uint64_t total = tbase[ntiles];
    std::cout << "\np " << total << "\n";
    for (uint64_t u = 0;; ++u) {
        const rsx_expand::Range r = rsx_join::tile_rows(u, total, cap);
        const rsx_expand::Stores st = rsx_expand::tile_stores(addr, static_cast<uint32_t>(eb), r.a, r.b);
        std::cout << "t " << u << " " << rsx_join::split(tbase.data(), pre.data(), ntiles, u << rsx_join::kTileShift) << " "
                  << rsx_join::split(tbase.data(), pre.data(), ntiles, (u + 1) << rsx_join::kTileShift) << " " << r.a << " " << r.b << " " << st.head << " " << st.nvec
                  << " " << st.tail << "\n";
        if (r.a >= r.b) break;
    }
    std::cout.flush();
    return 0;
}
