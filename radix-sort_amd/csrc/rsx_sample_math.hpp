// rsx_sample_math.hpp — the arithmetic of rsx_segmented_sample that needs no HIP type, pure: where a segment's pieces lie on the 4096-element
// tile grid, the chunked walk over the per-tile masses of a segment to (the tile that holds a target, the mass before that tile), and the
// crossing rule inside a piece.  Plain g++ compiles it too (host/harness/sample_selftest.cpp runs it on case files); under hipcc every
// function is __host__ __device__.  Included by rsx_sample.hpp.  The mass of a weight and the target rule: rsx_mass_math.hpp, unchanged.
//
//   P_i = m_0 + ... + m_i in index order, 64-bit integer sums; the answer to a target T in [1, total] is the smallest i with P_i >= T,
//   i.e. the one i with P_(i-1) < T <= P_i: crosses(P_(i-1), m_i, T).  An element of mass 0 never crosses.  The same rule picks the tile
//   (m = the mass of the segment's piece in that tile) and the chunk of tiles (m = the chunk's sum): a target that equals the prefix at
//   the end of a tile, or of a chunk, is answered inside it, and a tile or chunk whose piece weighs nothing is never the answer.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RSX_SAMPLE_HD __host__ __device__ __forceinline__
#else
#define RSX_SAMPLE_HD inline
#endif

namespace rsx_sample {

constexpr int kTileShift = 12;                                   // the family's global tile grid: 4096 elements
constexpr uint32_t kTileKeys = 1u << kTileShift;
constexpr uint32_t kWalkLane = 4;                                // consecutive tiles per lane and step of the walk
constexpr uint32_t kWalkTiles = 256;                             // tiles per chunk of the walk: 64 lanes x kWalkLane
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

// before < T <= before + m, without overflow (before + m <= total < 2^63)
RSX_SAMPLE_HD bool crosses(uint64_t before, uint64_t m, uint64_t T)
{
    return before < T && T - before <= m;
}

// The tiles a non-empty segment [b, e) touches: first .. last.
RSX_SAMPLE_HD uint32_t first_tile(uint64_t b) { return static_cast<uint32_t>(b >> kTileShift); }
RSX_SAMPLE_HD uint32_t last_tile(uint64_t e) { return static_cast<uint32_t>((e - 1) >> kTileShift); }

// The piece of segment [b, e) in tile t: [max(tile start, b), min(tile end, e)).
struct Piece {
    uint64_t start, end;
};

RSX_SAMPLE_HD Piece piece_of(uint64_t b, uint64_t e, uint32_t t)
{
    const uint64_t ts = static_cast<uint64_t>(t) << kTileShift, te = ts + kTileKeys;
    return Piece{b > ts ? b : ts, e < te ? e : te};
}

// The mass of the piece in tile t of a segment that covers the tiles ta < tb (more than one): the pass stores per tile
//   lead[t] = the mass of the elements of tile t that belong to the segment of the tile's FIRST element (the whole tile if it ends later),
//   tail[t] = the mass of the elements of tile t that belong to the segment of the tile's LAST element,
// each under its own segment's bound.  The first tile of a segment holds its tail, every later one its lead.
RSX_SAMPLE_HD uint64_t piece_mass(const uint64_t* lead, const uint64_t* tail, uint32_t ta, uint32_t t)
{
    return t == ta ? tail[t] : lead[t];
}

struct Found {
    uint32_t tile;          // kNoTile: T is 0 or beyond the sum
    uint64_t before;        // the mass of the segment before that tile
};

// The walk, sequential form: chunks of kWalkTiles tiles from ta on; the chunk whose sum crosses T, then the tile in it.  mass(t) is the
// piece mass of tile t.  The kernel takes the same steps with a wave: a lane sums kWalkLane consecutive tiles, the lanes are scanned,
// and crosses() picks the chunk, the lane and the tile.
template <typename Mass>
RSX_SAMPLE_HD Found walk(Mass mass, uint32_t ta, uint32_t tb, uint64_t T)
{
    uint64_t before = 0;
    for (uint64_t c = ta; c <= tb; c += kWalkTiles) {
        const uint64_t c_end = c + kWalkTiles - 1 < tb ? c + kWalkTiles - 1 : tb;
        uint64_t sum = 0;
        for (uint64_t t = c; t <= c_end; ++t) {
            sum += mass(static_cast<uint32_t>(t));
        }
        if (!crosses(before, sum, T)) {
            before += sum;
            continue;
        }
        for (uint64_t t = c; t <= c_end; ++t) {
            const uint64_t m = mass(static_cast<uint32_t>(t));
            if (crosses(before, m, T)) return Found{static_cast<uint32_t>(t), before};
            before += m;
        }
    }
    return Found{kNoTile, before};
}

// The crossing inside a piece of `count` masses that begins at mass `before`: the index of the element that answers T and P of that
// element; count if none crosses.
template <typename Mass>
RSX_SAMPLE_HD uint64_t locate(Mass mass, uint64_t count, uint64_t before, uint64_t T, uint64_t* p_out)
{
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t m = mass(i);
        if (crosses(before, m, T)) {
            *p_out = before + m;
            return i;
        }
        before += m;
    }
    *p_out = before;
    return count;
}

}  // namespace rsx_sample
