// args_selftest.cpp — CPU-only checks of csrc/rsx_args.hpp, the address arithmetic behind the C ABI's buffer rules.  The addresses are
// made-up integers: nothing is dereferenced.  Exit code = number of failed checks.
#include "rsx_args.hpp"

#include <iostream>

using rsx_args::aligned;
using rsx_args::aligned16;
using rsx_args::Buf;
using rsx_args::clash;
using rsx_args::Clash;
using rsx_args::overlaps;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checked;                                                                 \
        if (!(cond)) {                                                               \
            ++g_failed;                                                              \
            std::cerr << "CHECK failed: " #cond " (" << __FILE__ << ":" << __LINE__ << ")\n"; \
        }                                                                            \
    } while (0)

static const void* at(std::uintptr_t address)
{
    return reinterpret_cast<const void*>(address);
}

int main()
{
    // ranges: [0x1000, 0x1100) against its neighbours
    const Buf a{at(0x1000), 0x100};
    CHECK(!overlaps(a, Buf{at(0x1100), 0x100}) && !overlaps(Buf{at(0x1100), 0x100}, a));       // adjacent above
    CHECK(!overlaps(a, Buf{at(0x0F00), 0x100}) && !overlaps(Buf{at(0x0F00), 0x100}, a));       // adjacent below
    CHECK(overlaps(a, Buf{at(0x10FF), 0x100}) && overlaps(Buf{at(0x10FF), 0x100}, a));         // one byte at the upper end
    CHECK(overlaps(a, Buf{at(0x0F01), 0x100}) && overlaps(Buf{at(0x0F01), 0x100}, a));         // one byte at the lower end
    CHECK(overlaps(a, Buf{at(0x1040), 0x10}) && overlaps(Buf{at(0x1040), 0x10}, a));           // containment
    CHECK(overlaps(a, a) && overlaps(a, Buf{at(0x1000), 1}) && overlaps(a, Buf{at(0x10FF), 1}));
    CHECK(!overlaps(a, Buf{nullptr, 0x100}) && !overlaps(Buf{nullptr, 0x100}, a) && !overlaps(Buf{nullptr, 8}, Buf{nullptr, 8}));       // null
    CHECK(!overlaps(a, Buf{at(0x1040), 0}) && !overlaps(Buf{at(0x1040), 0}, a));               // zero bytes
    CHECK(overlaps(at(0x1000), 0x100, at(0x10FF), 1) && !overlaps(at(0x1000), 0x100, at(0x1100), 1));      // the four-argument form

    // the rules: engine buffers at 0x10000, 0x20000, 0x30000, 0x40000 (keys[0], perm[0], keys[1], perm[1])
    const Buf engine[4] = {{at(0x10000), 0x4000}, {at(0x20000), 0x2000}, {at(0x30000), 0x4000}, {at(0x40000), 0x2000}};
    const Buf o1{at(0x50000), 0x1000}, o2{at(0x51000), 0x1000}, o3{at(0x52000), 0x1000};       // adjacent outputs
    const Buf i1{at(0x60000), 0x1000}, i2{at(0x61000), 0x1000};
    CHECK(clash(engine, {o1, o2, o3}, {i1, i2}) == Clash::None);
    CHECK(clash(engine, {}, {}) == Clash::None && clash(engine, {}, {i1, i2}) == Clash::None && clash(engine, {o1}, {}) == Clash::None);
    CHECK(clash(engine, {}, {i1, i1}) == Clash::None);                                         // zero outputs: inputs may overlap each other
    CHECK(clash(engine, {}, {Buf{at(0x41FFF), 1}}) == Clash::Engine);                          // ... but not the engine
    for (const Buf& own : engine) {
        CHECK(clash(engine, {o1, own}, {i1}) == Clash::Engine);                                // an output equal to an engine buffer
        CHECK(clash(engine, {o1}, {i1, own}) == Clash::Engine);
        const std::uintptr_t end = reinterpret_cast<std::uintptr_t>(own.p) + own.bytes;
        CHECK(clash(engine, {Buf{at(end - 1), 0x10}}, {}) == Clash::Engine && clash(engine, {Buf{at(end), 0x10}}, {}) == Clash::None);
        CHECK(clash(engine, {o1}, {Buf{at(end - 0x100), 0x10}}) == Clash::Engine);             // an input inside it
        CHECK(clash(engine, {Buf{own.p, 0}}, {Buf{nullptr, own.bytes}}) == Clash::None);       // zero bytes, null
    }
    CHECK(clash(engine, {o1, o2, Buf{at(0x50FFF), 0x1000}}, {i1}) == Clash::Outputs);          // the last output on the first
    CHECK(clash(engine, {o1, o1}, {}) == Clash::Outputs && clash(engine, {o1, o2, o2}, {i1, i2}) == Clash::Outputs);
    CHECK(clash(engine, {o1, o2, Buf{at(0x5FFFF), 0x2}}, {i1, i2}) == Clash::OutputInput);     // the last output against the first input
    CHECK(clash(engine, {o1, o2, o3}, {i1, Buf{at(0x50800), 0x10}}) == Clash::OutputInput);    // the first output against the last input
    CHECK(clash(engine, {o1, o2, i2}, {i1, i2}) == Clash::OutputInput);                        // an output equal to an input
    CHECK(clash(engine, {o1, Buf{nullptr, 0x1000}, Buf{o1.p, 0}}, {Buf{nullptr, 0x1000}, Buf{o1.p, 0}}) == Clash::None);       // absent buffers
    // precedence: the engine rule first, then the pairs in order (an output's later outputs, then the inputs, before the next output)
    CHECK(clash(engine, {o1, o1}, {engine[3]}) == Clash::Engine);
    CHECK(clash(engine, {o1, o2, o2}, {o1}) == Clash::OutputInput && clash(engine, {o1, o1}, {o1}) == Clash::Outputs);

    // alignment to 4, 8, 16 and to the key size of both key widths; null is aligned to everything
    for (std::uintptr_t p = 0x7000; p < 0x7020; ++p) {
        for (std::uint64_t size : {4u, 8u, 16u}) CHECK(aligned(at(p), size) == (p % size == 0));
        CHECK(aligned16(at(p)) == (p % 16 == 0));
    }
    for (std::uint64_t key_bytes : {sizeof(std::uint32_t), sizeof(std::uint64_t)}) {
        CHECK(aligned(at(0x7000 + key_bytes), key_bytes) && !aligned(at(0x7000 + key_bytes / 2), key_bytes) && !aligned(at(0x7001), key_bytes));
        CHECK(aligned(nullptr, key_bytes));
    }
    CHECK(aligned(at(0x7004), 4) && !aligned(at(0x7004), 8) && aligned(at(0x7008), 8) && !aligned(at(0x7008), 16) && aligned16(nullptr));

    std::cout << "args_selftest: " << (g_checked - g_failed) << "/" << g_checked << " checks passed" << std::endl;
    return g_failed;
}
