// event_scan.h -- the three-launch exclusive scan of the event-stream files (csrc/event_tables.hip, csrc/event_stats.hip).
//
// A scan is three launches on the caller's stream: per-tile sums (2048 values a workgroup), one workgroup over the sums,
// the tiles again with their offsets.  The kernel boundary is the only ordering between workgroups: no workgroup waits
// for another, no look-back.  Sums are uint32 and wrap: a scan of +-1 values reads them as two's complement.
//
// Everything here has internal linkage (an unnamed namespace): each translation unit instantiates the templates on its
// own functors and carries its own copy of the one kernel that is no template.
#pragma once
#include "common.h"

namespace enerf {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRounds = 8;
constexpr uint32_t kScanTile = kThreads * kRounds;     // values per workgroup of a scan

// exclusive scan of v over the workgroup's 256 threads (all of them must call); total = the workgroup's sum
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const uint32_t incl = wave_incl_scan_add_u32(v, 0);
    const int wave = threadIdx.x >> 6;
    if (lane_id() == kWave - 1) lds[wave] = incl;
    __syncthreads();
    uint32_t below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const uint32_t s = lds[w];
        below += w < wave ? s : 0u;
        all += s;
    }
    __syncthreads();
    total = all;
    return below + incl - v;
}

// F: uint32_t load(uint32_t i) const; void store(uint32_t i, uint32_t exclusive, uint32_t value) const.
// n_dev != nullptr: the length is min(*n_dev, n) (a count the host has not read)
template <class F>
__global__ void __launch_bounds__(kThreads) k_scan_sums(F f, uint32_t n, const uint32_t* __restrict__ n_dev,
                                                        uint32_t* __restrict__ sums) {
    __shared__ uint32_t lds[kWaves];
    if (n_dev) n = *n_dev < n ? *n_dev : n;
    const uint32_t base = blockIdx.x * kScanTile;
    uint32_t s = 0;
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        if (i < n) s += f.load(i);
    }
    uint32_t total;
    block_excl_scan(s, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[nb] -> their exclusive scan in place, *total = their sum
__global__ void __launch_bounds__(kThreads) k_scan_top(uint32_t* __restrict__ sums, uint32_t nb,
                                                       uint32_t* __restrict__ total_out) {
    __shared__ uint32_t lds[kWaves];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? sums[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(v, lds, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

template <class F>
__global__ void __launch_bounds__(kThreads) k_scan_apply(F f, uint32_t n, const uint32_t* __restrict__ n_dev,
                                                         const uint32_t* __restrict__ sums) {
    __shared__ uint32_t lds[kWaves];
    if (n_dev) n = *n_dev < n ? *n_dev : n;
    const uint32_t base = blockIdx.x * kScanTile;
    if (base >= n) return;                              // (uniform over the workgroup)
    uint32_t carry = sums[blockIdx.x];
    for (int r = 0; r < kRounds; ++r) {
        const uint32_t i = base + r * kThreads + threadIdx.x;
        const uint32_t v = i < n ? f.load(i) : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan(v, lds, total);
        if (i < n) f.store(i, carry + ex, v);
        carry += total;
    }
}

// `sums`: div_up(n, kScanTile) words at least; *total = the sum of all n values
template <class F>
int scan(const F& f, uint32_t n, const uint32_t* n_dev, uint32_t* sums, uint32_t* total, hipStream_t s, const char* what) {
    const uint32_t nb = div_up(n, kScanTile);
    k_scan_sums<F><<<nb, kThreads, 0, s>>>(f, n, n_dev, sums);
    ENERF_LAUNCH_CHECK(what);
    k_scan_top<<<1, kThreads, 0, s>>>(sums, nb, total);
    ENERF_LAUNCH_CHECK(what);
    k_scan_apply<F><<<nb, kThreads, 0, s>>>(f, n, n_dev, sums);
    ENERF_LAUNCH_CHECK(what);
    return 0;
}

}  // namespace
}  // namespace enerf
