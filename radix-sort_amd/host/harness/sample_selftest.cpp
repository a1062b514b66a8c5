// sample_selftest.cpp — CPU-only run of csrc/rsx_sample_math.hpp as rsx_segmented_sample uses it: the chunked walk over a segment's per-tile
// masses to (the tile that holds a target, the mass before it) and the crossing inside a piece: the functions the kernel calls, compiled
// by plain g++, on a small case file.  No library, no HIP.
// (Also the program to build with -fsanitize=address,undefined: bin/sample_selftest_san.)
//
//   sample_selftest CASE_FILE
//
// Case file, one case per line, whitespace-separated: a tag, then unsigned decimals:
//   W TA TB T M...          the walk of a segment over the tiles TA .. TB with the piece masses M (TB - TA + 1 of them) for the target T
//   L COUNT BEFORE T M...   the crossing in a piece of COUNT masses M that begins at running mass BEFORE
// Output: one line per case: "W tile before" (tile 4294967295: no tile holds T) or "L index P" (index COUNT: none crosses).
// Every answer is also found by a plain linear scan without chunks, and the two must agree.
// Exit code: 0; 1 for a malformed file (an unknown tag, TB < TA, more than 2^22 masses, a mass above 2^44, a missing number); 2 if the
// header's answer differs from the linear scan's.
#include "rsx_sample_math.hpp"

#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace {

constexpr uint64_t kMaxMasses = 1ull << 22, kMaxMass = 1ull << 44;      // (a tile's piece weighs 2^12 * 2^32 at most)

bool read_masses(std::istream& in, uint64_t count, std::vector<uint64_t>& m)
{
    m.resize(count);
    for (uint64_t i = 0; i < count; ++i) {
        if (!(in >> m[i]) || m[i] > kMaxMass) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::cerr << "usage: sample_selftest CASE_FILE\n";
        return 1;
    }
    std::ifstream in(argv[1]);
    if (!in) return 1;
    std::string tag;
    std::vector<uint64_t> m;
    while (in >> tag) {
        if (tag == "W") {
            uint64_t ta, tb, T;
            if (!(in >> ta >> tb >> T)) return 1;
            if (tb < ta || tb >= rsx_sample::kNoTile || tb - ta + 1 > kMaxMasses) return 1;
            if (!read_masses(in, tb - ta + 1, m)) return 1;
            const uint32_t a = static_cast<uint32_t>(ta), b = static_cast<uint32_t>(tb);
            const rsx_sample::Found f = rsx_sample::walk([&](uint32_t t) { return m[t - a]; }, a, b, T);
            uint32_t tile = rsx_sample::kNoTile;
            uint64_t before = 0;
            for (uint64_t i = 0; i < m.size(); ++i) {
                if (T > before && T <= before + m[i]) {
                    tile = a + static_cast<uint32_t>(i);
                    break;
                }
                before += m[i];
            }
            if (f.tile != tile || f.before != before) return 2;
            std::cout << "W " << f.tile << " " << f.before << "\n";
        } else if (tag == "L") {
            uint64_t count, before, T;
            if (!(in >> count >> before >> T)) return 1;
            if (count > kMaxMasses || before > (1ull << 62)) return 1;
            if (!read_masses(in, count, m)) return 1;
            uint64_t p = 0;
            const uint64_t i = rsx_sample::locate([&](uint64_t j) { return m[j]; }, count, before, T, &p);
            uint64_t want = count, run = before;
            for (uint64_t j = 0; j < count; ++j) {
                run += m[j];
                if (m[j] != 0 && run >= T && run - m[j] < T) {
                    want = j;
                    break;
                }
            }
            if (i != want || p != run) return 2;
            std::cout << "L " << i << " " << p << "\n";
        } else {
            return 1;
        }
    }
    if (!in.eof()) return 1;
    std::cout.flush();
    return 0;
}
