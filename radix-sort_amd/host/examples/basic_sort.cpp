// basic_sort.cpp — the smallest complete program on the public API; plays the role of the
// reference's examples/basic_sort/basic_sort.cpp:23-139 (2^20 random uint32 keys, compare with
// std::sort, print the per-step timings, non-zero exit code on mismatch).
//
//   basic_sort [num_elements] [--int64 | --float32 | --float64] [--descending] [--argsort] [--pinned] [--ranks R [--gpus G] [--peer-stores]]
//
// The call sequence is the API contract: caller-owned vectors -> HostSpans -> initialize ->
// (padGPUData) -> uploadData -> calculate -> downloadData -> getRuntimes -> release.
// --ranks R: the same sequence on RadixSortMultiGPU<T> — the array sharded over R ranks (rank r on device r % G; several ranks on one GPU
// talk through the loopback communicator, one rank per GPU through RCCL).
// --float32 / --float64: keys are random bit patterns (NaNs of both signs, ±inf, ±0 and denormals among them), sorted in IEEE 754
// totalOrder.  --descending: stable descending order.  The result is checked bit for bit against std::stable_sort (and, with
// --argsort, the permutation against the stable argsort); the sharded engine takes integer keys in ascending order only.
#include "Common/ComputeState.h"
#include "Dataset.h"
#include "HostData.h"
#include "Parameters.h"
#include "RadixSortGPU.h"
#include "RadixSortMultiGPU.h"

#include <algorithm>
#include <cstdint>
#include <random>
#include <type_traits>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <numeric>
#include <string>

namespace {

struct Choices {
    std::uint32_t count = 1U << 20U;
    bool wide = false;       // int64 keys instead of uint32
    int float_bytes = 0;     // 4 / 8: float / double keys
    bool descending = false;
    bool argsort = false;    // carry h_Permut through the sort
    bool pinned = false;
    int ranks = 0;           // > 0: RadixSortMultiGPU over this many ranks
    int gpus = 1;
    bool peer_stores = false;
};

Choices parse(int argc, char** argv)
{
    Choices c;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--int64") c.wide = true;
        else if (a == "--float32") c.float_bytes = 4;
        else if (a == "--float64") c.float_bytes = 8;
        else if (a == "--descending") c.descending = true;
        else if (a == "--argsort") c.argsort = true;
        else if (a == "--pinned") c.pinned = true;
        else if (a == "--peer-stores") c.peer_stores = true;
        else if ((a == "--ranks" || a == "--gpus") && i + 1 < argc) (a == "--ranks" ? c.ranks : c.gpus) = std::atoi(argv[++i]);
        else c.count = static_cast<std::uint32_t>(std::strtoul(a.c_str(), nullptr, 0));
    }
    return c;
}

// The unsigned word whose order is the sort order of a key: IEEE 754 totalOrder for floats, two's complement for signed
// integers, inverted for descending order (include/radixsort_hip.h, key kinds).
template <typename Key>
using Bits = std::conditional_t<sizeof(Key) == 4, std::uint32_t, std::uint64_t>;

template <typename Key>
Bits<Key> order_bits(Key key, bool descending)
{
    Bits<Key> x;
    std::memcpy(&x, &key, sizeof x);
    constexpr Bits<Key> sign = Bits<Key>{1} << (sizeof(Key) * 8 - 1);
    if constexpr (std::is_floating_point_v<Key>) x ^= (x & sign) ? static_cast<Bits<Key>>(~Bits<Key>{0}) : sign;
    else if constexpr (std::is_signed_v<Key>) x ^= sign;
    return descending ? static_cast<Bits<Key>>(~x) : x;
}

template <typename Key>
bool same_bits(Key a, Key b)
{
    return std::memcmp(&a, &b, sizeof(Key)) == 0;
}

template <typename Key>
bool run(ComputeState& gpu, const Choices& opt)
{
    RadixSortGPU<Key> sorter;
    sorter.setDescending(opt.descending);
    sorter.enablePermutation(opt.argsort);
    sorter.enablePinnedTransfers(opt.pinned);

    // the engine sorts Resize(count) elements: whatever the host buffer holds past `count`
    // (zeros here) is part of the sorted range, exactly as in the reference
    const std::uint32_t rounded = sorter.Resize(opt.count);
    HostData<Key> host;
    host.m_hKeys.assign(rounded, Key{0});
    host.m_hResultFromGPU.assign(rounded, Key{0});
    host.m_hHistograms.assign(AlgorithmParameters<Key>::_HISTOSIZE, 0U);
    host.m_hGlobsum.assign(AlgorithmParameters<Key>::_NUM_HISTOSPLIT, 0U);
    host.h_Permut.resize(rounded);
    std::iota(host.h_Permut.begin(), host.h_Permut.end(), 0U);
    if constexpr (std::is_floating_point_v<Key>) {
        std::mt19937_64 rng(20261016);
        for (std::uint32_t i = 0; i < opt.count; ++i) {
            const Bits<Key> x = static_cast<Bits<Key>>(rng());
            std::memcpy(&host.m_hKeys[i], &x, sizeof x);
        }
    } else {
        const RandomDistributed<Key> input(opt.count);
        std::copy(input.dataset.begin(), input.dataset.end(), host.m_hKeys.begin());
    }

    const auto fail = [&](const char* step, OperationStatus s) {
        std::cerr << step << " failed: " << to_string(s) << " (" << rsx_last_error() << ")\n";
        return false;
    };
    auto& queue = gpu.m_CLCommandQueue;
    OperationStatus s = sorter.initialize(gpu.device(), gpu.m_CLContext, opt.count, MakeHostSpans(host));
    if (s != OperationStatus::OK) return fail("initialize", s);
    if (rounded != opt.count) sorter.padGPUData(queue, sizeof(Key) * opt.count);   // overwritten by the upload, as in the reference
    if ((s = sorter.uploadData(queue)) != OperationStatus::OK) return fail("uploadData", s);
    if ((s = sorter.calculate(queue)) != OperationStatus::OK) return fail("calculate", s);
    if ((s = sorter.downloadData(queue)) != OperationStatus::OK) return fail("downloadData", s);

    // the stable argsort (unique): keys bit for bit, and with --argsort the permutation itself
    std::vector<std::uint32_t> order(rounded);
    std::iota(order.begin(), order.end(), 0U);
    std::stable_sort(order.begin(), order.end(), [&](std::uint32_t a, std::uint32_t b) {
        return order_bits(host.m_hKeys[a], opt.descending) < order_bits(host.m_hKeys[b], opt.descending);
    });
    bool ok = true;
    for (std::uint32_t i = 0; i < rounded && ok; ++i) {
        ok = same_bits(host.m_hKeys[order[i]], host.m_hResultFromGPU[i]) && (!opt.argsort || host.h_Permut[i] == order[i]);
    }

    const RuntimesGPU t = sorter.getRuntimes();
    std::cout << "per-launch averages [ms]: histogram " << t.timeHisto.avg << "  scan " << t.timeScan.avg << "  paste " << t.timePaste.avg
              << "  reorder " << t.timeReorder.avg << "  (sum " << t.timeTotal.avg << ")\n";
    sorter.release();
    return ok;
}

// The sharded engine behind the same five calls.
template <typename Key>
bool runSharded(const Choices& opt)
{
    RadixSortMultiGPU<Key> sorter;
    const std::uint64_t rounded = sorter.Resize(opt.count);
    HostData<Key> host;
    host.m_hKeys.assign(rounded, Key{0});
    host.m_hResultFromGPU.assign(rounded, Key{0});
    host.h_Permut.resize(rounded);
    std::iota(host.h_Permut.begin(), host.h_Permut.end(), 0U);
    {
        const RandomDistributed<Key> input(opt.count);
        std::copy(input.dataset.begin(), input.dataset.end(), host.m_hKeys.begin());
    }
    ShardedSortOptions so;
    so.devices.clear();
    for (int r = 0; r < opt.ranks; ++r) so.devices.push_back(r % std::max(opt.gpus, 1));
    so.withPermutation = opt.argsort;
    so.exchange = opt.peer_stores ? ShardedSortOptions::Exchange::PeerStores : ShardedSortOptions::Exchange::AllToAll;
    const auto fail = [&](const char* step, OperationStatus s) {
        std::cerr << step << " failed: " << to_string(s) << " (" << sorter.lastError() << ")\n";
        return false;
    };
    OperationStatus s = sorter.initialize(so, opt.count, MakeHostSpans(host));
    if (s != OperationStatus::OK) return fail("initialize", s);
    if ((s = sorter.uploadData()) != OperationStatus::OK) return fail("uploadData", s);
    if ((s = sorter.calculate()) != OperationStatus::OK) return fail("calculate", s);
    if ((s = sorter.downloadData()) != OperationStatus::OK) return fail("downloadData", s);
    std::vector<Key> expect(host.m_hKeys);
    std::sort(expect.begin(), expect.end());
    bool ok = expect == host.m_hResultFromGPU;
    for (std::uint64_t i = 0; opt.argsort && i < rounded && ok; ++i) {
        const std::uint32_t from = host.h_Permut[i];
        ok = from < rounded && host.m_hKeys[from] == host.m_hResultFromGPU[i] &&
             (i == 0 || host.m_hResultFromGPU[i - 1] != host.m_hResultFromGPU[i] || host.h_Permut[i - 1] < from);
    }
    std::cout << sorter.world() << " ranks, path " << sorter.lastPath() << ", communicator: " << sorter.communicator() << "; keys per rank:";
    for (const std::uint64_t load : sorter.rankLoads()) std::cout << ' ' << load;
    std::cout << "\nstep (wall clock of calculate()): " << sorter.getRuntimes().timeTotal.avg << " ms\n";
    sorter.release();
    return ok;
}

}  // namespace

int main(int argc, char** argv)
{
    const Choices opt = parse(argc, argv);
    ComputeState gpu;
    if (!gpu.init()) return 1;
    if (opt.ranks > 0 && (opt.float_bytes || opt.descending)) {
        std::cerr << "the sharded sort (--ranks) takes integer keys in ascending order\n";
        return 2;
    }
    const char* type = opt.float_bytes == 4 ? " float" : opt.float_bytes == 8 ? " double" : opt.wide ? " int64_t" : " uint32_t";
    std::cout << "Sorting " << opt.count << type << " values on the GPU" << (opt.descending ? " in descending order" : "")
              << (opt.argsort ? " (with permutation)" : "") << "...\n";
    bool ok;
    if (opt.ranks > 0) ok = opt.wide ? runSharded<std::int64_t>(opt) : runSharded<std::uint32_t>(opt);
    else if (opt.float_bytes == 4) ok = run<float>(gpu, opt);
    else if (opt.float_bytes == 8) ok = run<double>(gpu, opt);
    else ok = opt.wide ? run<std::int64_t>(gpu, opt) : run<std::uint32_t>(gpu, opt);
    std::cout << "Result: " << (ok ? "PASSED" : "FAILED") << "\n";
    return ok ? 0 : 1;
}
