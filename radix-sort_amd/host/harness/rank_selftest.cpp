// rank_selftest.cpp — CPU-only run of csrc/rsx_rank_math.hpp as rsx_segmented_rank uses it: the per-tile edges of a sorted segment, the
// three carries joined over its tiles, and the rank and tie count of every sorted position under the five methods: the functions the
// kernels call, compiled by plain g++, on a small case file.  No library, no HIP.
// (Also the program to build with -fsanitize=address,undefined: bin/rank_selftest_san.)
//
//   rank_selftest CASE_FILE
//
// Case file, one case per line, whitespace-separated unsigned decimals after the tag:
//   S TILE A M  V_0 C_0 ... V_(M-1) C_(M-1)
// a sorted segment that starts A keys into a tile of TILE keys (A < TILE) and holds C_0 keys of value V_0, then C_1 of V_1, ...: adjacent
// equal values are one run.  The tiles are the grid of TILE keys clipped at the segment's ends, as the kernels see it.
// Output per case: "S L T" (keys, tiles), then six lines: the ranks under ordinal, min, max, dense, average (min + max) and the tie counts,
// in sorted order.  Every value is also found by a plain scan over the whole segment without tiles, and the two must agree.
// Exit code: 0; 1 for a malformed file (an unknown tag, TILE == 0, A >= TILE, a zero count, more than 2^22 keys, a missing number); 2 if
// the header's answer differs from the plain scan's.
#include "rsx_rank_math.hpp"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace {

constexpr uint64_t kMaxKeys = 1ull << 22;

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::cerr << "usage: rank_selftest CASE_FILE\n";
        return 1;
    }
    std::ifstream in(argv[1]);
    if (!in) return 1;
    std::string tag;
    while (in >> tag) {
        if (tag != "S") return 1;
        uint64_t tile, a, m;
        if (!(in >> tile >> a >> m)) return 1;
        if (tile == 0 || tile > kMaxKeys || a >= tile || m > kMaxKeys) return 1;
        std::vector<uint64_t> keys;
        for (uint64_t i = 0; i < m; ++i) {
            uint64_t v, c;
            if (!(in >> v >> c)) return 1;
            if (c == 0 || keys.size() + c > kMaxKeys) return 1;
            keys.insert(keys.end(), c, v);
        }
        const uint32_t L = static_cast<uint32_t>(keys.size());
        const uint32_t T = L ? static_cast<uint32_t>((a + L + tile - 1) / tile) : 0;
        auto head = [&](uint32_t q) { return q == 0 || keys[q] != keys[q - 1]; };
        // tile t covers the sorted positions [lo(t), lo(t + 1))
        auto lo = [&](uint32_t t) -> uint32_t {
            if (t == 0) return 0;
            const uint64_t x = static_cast<uint64_t>(t) * tile - a;
            return x < L ? static_cast<uint32_t>(x) : L;
        };
        std::vector<rsx_rank::Edge> edges(T);
        for (uint32_t t = 0; t < T; ++t) {
            rsx_rank::Edge e{0, rsx_rank::kNone, rsx_rank::kNone};
            for (uint32_t q = lo(t); q < lo(t + 1); ++q) {
                if (!head(q)) continue;
                e.heads = rsx_rank::carry_dense(e.heads, 1);
                e.first = rsx_rank::carry_next(q, e.first);
                e.last = rsx_rank::carry_start(e.last, q);
            }
            edges[t] = e;
        }
        std::vector<rsx_rank::Carry> carry(T);
        rsx_rank::join([&](uint32_t t) { return edges[t]; }, T, L, carry.data());
        std::vector<uint32_t> out[rsx_rank::kMethods + 1];
        for (auto& o : out) o.resize(L);
        for (uint32_t t = 0; t < T; ++t) {
            // inside the tile: the same three folds, element by element
            uint32_t start = carry[t].start, dense = carry[t].dense;
            std::vector<uint32_t> ends(lo(t + 1) - lo(t));
            uint32_t next = carry[t].next;
            for (uint32_t q = lo(t + 1); q-- > lo(t);) {
                ends[q - lo(t)] = next;
                next = rsx_rank::carry_next(next, head(q) ? q : rsx_rank::kNone);
            }
            for (uint32_t q = lo(t); q < lo(t + 1); ++q) {
                if (head(q)) {
                    start = rsx_rank::carry_start(start, q);
                    dense = rsx_rank::carry_dense(dense, 1);
                }
                if (start == rsx_rank::kNone) return 2;          // (position 0 is a head)
                for (uint32_t method = 0; method < rsx_rank::kMethods; ++method) {
                    out[method][q] = rsx_rank::rank_of(method, start, ends[q - lo(t)], dense - 1, q);
                }
                out[rsx_rank::kMethods][q] = rsx_rank::ties_of(start, ends[q - lo(t)]);
            }
        }
        // the plain scan
        for (uint32_t q = 0, distinct = 0; q < L;) {
            uint32_t r = q;
            while (r < L && keys[r] == keys[q]) ++r;
            for (uint32_t i = q; i < r; ++i) {
                const uint32_t want[rsx_rank::kMethods + 1] = {i, q, r - 1, distinct, q + r - 1, r - q};
                for (uint32_t method = 0; method <= rsx_rank::kMethods; ++method) {
                    if (out[method][i] != want[method]) return 2;
                }
            }
            q = r;
            ++distinct;
        }
        std::cout << "S " << L << " " << T << "\n";
        for (const auto& o : out) {
            for (uint32_t q = 0; q < L; ++q) {
                std::cout << (q ? " " : "") << o[q];
            }
            std::cout << "\n";
        }
    }
    if (!in.eof()) return 1;
    std::cout.flush();
    return 0;
}
