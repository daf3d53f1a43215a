// scan.hip — the exclusive scan of a table of counters into out[count + 1] (out[count] = the grand total), for gfx950:
// bucket counts -> bucket starts of the broad phase's grid, per-(cluster, colour) counts -> segment starts and active
// flags -> ranks of the cluster solver (cluster.hip). One launch up to 32768 counters (k_scan_small), else three.
#include <cassert>

#include "kernels.hpp"

namespace phys {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanChunk = kScanThreads * kScanItems;

// `block_used` (bucket grid only): per block, how many of its counters are non-zero = buckets in use; k_scan_block_sums
// adds them up. Bodies per bucket in use is how CROWDED the grid is, which decides the pair kernel of later updates
// (launch_broadphase). (Counted here, where every counter is read anyway: one atomic per workgroup of k_cell_assign -
// 3906 of them at 1M bodies - cost that kernel 36 us.)
__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const uint32_t* __restrict__ in, uint32_t count,
                                                              uint32_t* __restrict__ block_sums,
                                                              uint32_t* __restrict__ block_used = nullptr) {
    __shared__ uint32_t wsum[kScanThreads / 64], wused[kScanThreads / 64];
    const uint32_t base = blockIdx.x * kScanChunk + threadIdx.x * kScanItems;
    uint32_t s = 0, u = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const uint32_t v = (base + k < count) ? in[base + k] : 0u;
        s += v;
        u += v != 0u ? 1u : 0u;
    }
    // (block_put / block_get of wave.hpp, written out: the two butterflies interleaved, and the kernel - part of every
    // update of a world above 32768 bodies - keeps the instructions it had)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s += (uint32_t)__shfl_xor((int)s, off, 64); u += (uint32_t)__shfl_xor((int)u, off, 64); }
    if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = s; wused[threadIdx.x >> 6] = u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0, tu = 0;
        for (int k = 0; k < kScanThreads / 64; ++k) { t += wsum[k]; tu += wused[k]; }
        block_sums[blockIdx.x] = t;
        if (block_used) block_used[blockIdx.x] = tu;
    }
}

// one block: exclusive scan of the block sums in place (loops with a carry for long inputs)
__global__ __launch_bounds__(1024) void k_scan_block_sums(uint32_t* __restrict__ sums, uint32_t count,
                                                          const uint32_t* __restrict__ block_used = nullptr,
                                                          StepCounters* __restrict__ ctr = nullptr) {
    __shared__ uint32_t wused[16];
    if (block_used) {  // buckets in use, summed over the blocks of k_scan_reduce (no atomics on the way)
        uint32_t u = 0;
        for (uint32_t k = threadIdx.x; k < count; k += 1024) u += block_used[k];
        const uint32_t t = block_sum<1024>(u, wused);
        if (threadIdx.x == 0) ctr->n_used_buckets = t;
    }
    (void)block_scan_in_place<1024>(sums, count);
}

__global__ __launch_bounds__(kScanThreads) void k_scan_final(const uint32_t* __restrict__ in, uint32_t count,
                                                             const uint32_t* __restrict__ block_sums,
                                                             uint32_t* __restrict__ out /*count + 1*/) {
    __shared__ uint32_t wtot[kScanThreads / 64];
    const uint32_t base = blockIdx.x * kScanChunk + threadIdx.x * kScanItems;
    uint32_t v[kScanItems];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) { v[k] = (base + k < count) ? in[base + k] : 0u; s += v[k]; }
    const uint32_t inc = wave_inclusive_scan(s);
    if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t off = block_sums[blockIdx.x];
    for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) off += wtot[k];
    uint32_t run = off + inc - s;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < count) out[base + k] = run;
        run += v[k];
        if (base + k + 1 == count) out[count] = run;  // grand total in the extra slot
    }
}

// small tables (<= 32768 counters): the whole exclusive scan in ONE workgroup, one launch instead of three
// (measured at 64 items per thread, for the cluster solver's 672 x 64 segment table: 25.6 us - one workgroup's lanes read
// 256-byte runs each, every line is touched by eight load instructions - against 3 x 4.8 us for the three launches)
constexpr int kScanSmallThreads = 1024;
constexpr int kScanSmallItems = 32;
// ZERO_IN: the counters are left zeroed for their next use (a per-step histogram then needs no memset launch of its own)
template <bool ZERO_IN>
__global__ __launch_bounds__(kScanSmallThreads) void k_scan_small(uint32_t* __restrict__ in, uint32_t count /* multiple of 4 */,
                                                                  uint32_t* __restrict__ out /*count + 1*/) {
    __shared__ uint32_t wtot[kScanSmallThreads / 64];
    const uint32_t base = threadIdx.x * kScanSmallItems;
    uint4 v[kScanSmallItems / 4];
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanSmallItems / 4; ++k) {
        v[k] = make_uint4(0u, 0u, 0u, 0u);
        if (base + 4 * k < count) {
            v[k] = *reinterpret_cast<const uint4*>(in + base + 4 * k);
            if (ZERO_IN) *reinterpret_cast<uint4*>(in + base + 4 * k) = make_uint4(0u, 0u, 0u, 0u);
        }
        sum += v[k].x + v[k].y + v[k].z + v[k].w;
    }
    const uint32_t inc = wave_inclusive_scan(sum);
    if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t run = inc - sum;
    for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) run += wtot[k];
#pragma unroll
    for (int k = 0; k < kScanSmallItems / 4; ++k) {
        if (base + 4 * k < count) {
            uint4 o;
            o.x = run; o.y = o.x + v[k].x; o.z = o.y + v[k].y; o.w = o.z + v[k].z;
            *reinterpret_cast<uint4*>(out + base + 4 * k) = o;
            run = o.w + v[k].w;
        }
    }
    if (threadIdx.x == kScanSmallThreads - 1) {
        uint32_t total = 0;
        for (int k = 0; k < kScanSmallThreads / 64; ++k) total += wtot[k];
        out[count] = total;  // grand total in the extra slot
    }
}

// ---- host side -------------------------------------------------------------------------------------
bool scan_is_one_launch(uint32_t count) { return count <= (uint32_t)(kScanSmallThreads * kScanSmallItems); }
size_t scan_scratch_words(uint32_t count) { return (count + kScanChunk - 1) / kScanChunk; }

// count: a multiple of 4 (k_scan_small reads uint4; every caller's table is a power of two or rounded up). zero_in: only
// honoured by the one-launch scan (scan_is_one_launch(count)); the caller zeroes the counters itself otherwise.
// block_used / ctr: only honoured by the three-launch scan (the grids large enough for the pair kernel's choice to
// matter). prof_stage >= 0: every launch is a profiler scope of that stage (scopes do not nest: the caller has none open).
void launch_exclusive_scan(phys_world* w, uint32_t* in, uint32_t count, uint32_t* out, bool zero_in, uint32_t* scratch,
                           uint32_t* block_used, StepCounters* ctr, int prof_stage) {
    hipStream_t s = w->stream;
    assert(count % 4 == 0);
    auto launch = [&](auto&& enqueue) {
        if (prof_stage >= 0) { PHYS_PROF(w, (uint32_t)prof_stage); enqueue(); } else enqueue();
    };
    if (scan_is_one_launch(count)) {
        launch([&] {
            if (zero_in) hipLaunchKernelGGL(k_scan_small<true>, dim3(1), dim3(kScanSmallThreads), 0, s, in, count, out);
            else hipLaunchKernelGGL(k_scan_small<false>, dim3(1), dim3(kScanSmallThreads), 0, s, in, count, out);
        });
        return;
    }
    const uint32_t nblk = (uint32_t)scan_scratch_words(count);
    launch([&] { hipLaunchKernelGGL(k_scan_reduce, dim3(nblk), dim3(kScanThreads), 0, s, in, count, scratch, block_used); });
    launch([&] { hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(1024), 0, s, scratch, nblk, (const uint32_t*)block_used, ctr); });
    launch([&] { hipLaunchKernelGGL(k_scan_final, dim3(nblk), dim3(kScanThreads), 0, s, in, count, scratch, out); });
}

}  // namespace phys
