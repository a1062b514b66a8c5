// rsx_args.hpp — the pure part of the C ABI's argument checks: address arithmetic on the caller's buffers.  No HIP type and no engine in
// here, so that plain g++ compiles it (host/harness/args_selftest.cpp runs it on made-up addresses).  Included by rsx_capi.hip; the
// segmented family reaches it through check_buffers (capi_family.inc).
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace rsx_args {

// One device range of the caller's (or of the engine's).  A null pointer or zero bytes is "not given": it overlaps nothing.
struct Buf {
    const void* p;
    uint64_t bytes;
};

inline bool overlaps(const void* a, uint64_t abytes, const void* b, uint64_t bbytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}

inline bool overlaps(const Buf& a, const Buf& b)
{
    return overlaps(a.p, a.bytes, b.p, b.bytes);
}

// (a null pointer is aligned to everything: whether a pointer is required is the caller's own check)
inline bool aligned(const void* p, uint64_t size)
{
    return reinterpret_cast<uintptr_t>(p) % size == 0;
}

inline bool aligned16(const void* p)
{
    return aligned(p, 16);
}

// Which rule a call's buffers break, in the order the rules are tested.
enum class Clash { None, Engine, Outputs, OutputInput };

// The rules every call of the segmented family shares: nothing of the caller's lies in one of the engine's four buffers, no two outputs
// overlap, no output overlaps an input.  (Inputs may overlap each other: the calls that mind say so themselves.)
inline Clash clash(const Buf (&engine)[4], std::initializer_list<Buf> outs, std::initializer_list<Buf> ins)
{
    for (const std::initializer_list<Buf>& mine : {outs, ins}) {
        for (const Buf& b : mine) {
            for (const Buf& own : engine) {
                if (overlaps(b, own)) return Clash::Engine;
            }
        }
    }
    for (const Buf* a = outs.begin(); a != outs.end(); ++a) {
        for (const Buf* b = a + 1; b != outs.end(); ++b) {
            if (overlaps(*a, *b)) return Clash::Outputs;
        }
        for (const Buf& b : ins) {
            if (overlaps(*a, b)) return Clash::OutputInput;
        }
    }
    return Clash::None;
}

}  // namespace rsx_args
