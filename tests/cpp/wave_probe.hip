// wave_probe.hip — test-only probes of physics_amd/csrc/wave.hpp and scan.hip (tests/test_gpu_wave_primitives.py,
// tests/test_wave_ref_cpu.py). Built as tests/cpp/libwave_probe.so by the `wave_probe` rule of
// physics_amd/csrc/Makefile, with that Makefile's HIPFLAGS, and linked against libphysics_hip.so: the scan entry points
// run the product's own code object, the header-only primitives are instantiated here. No kernel of this file is part
// of libphysics_hip.so.
//
// Every kernel is a thin wrapper: it calls ONE primitive and stores what every lane got; whatever is compared, summed or
// sorted is the test's business (tests/wave_ref.py). Every entry point takes host pointers, allocates, copies, launches,
// synchronises and frees for itself (as phys_block_spmv does) and leaves the caller's current device as it found it.
// They return 0, a negative number for arguments they refuse (a kernel is never launched on sizes that do not fit its
// buffers), or the hipError_t of the call that failed.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../physics_amd/csrc/kernels.hpp"
#include "../../include/spec/force_field.h"
#include "../../include/spec/volume.h"

using namespace phys;

namespace {

constexpr int32_t kBadArg = -1;

#define WP_TRY(expr)                                  \
    do {                                              \
        const hipError_t _e = (expr);                 \
        if (_e != hipSuccess) {                       \
            (void)hipGetLastError();                  \
            return (int32_t)_e;                       \
        }                                             \
    } while (0)

// the caller's current device, put back on every way out
struct DeviceKeeper {
    int prev = -1;
    DeviceKeeper() { if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; } }
    ~DeviceKeeper() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// a device copy of `bytes` of host memory (at least 16 bytes are allocated, so that an empty array still has an address)
struct Mirror {
    DevBuf<uint8_t> d;
    void* host = nullptr;
    size_t bytes = 0;
    hipError_t up(void* h, size_t n, hipStream_t s) {
        host = h; bytes = n;
        hipError_t e = d.resize(n > 16 ? n : 16);
        if (e == hipSuccess && n) e = hipMemcpyAsync(d.p, h, n, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e;
    }
    hipError_t down(hipStream_t s) {
        hipError_t e = bytes ? hipMemcpyAsync(host, d.p, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e;
    }
    template <class T> T* as() { return reinterpret_cast<T*>(d.p); }
};

// ---- kernels ------------------------------------------------------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_probe_block_scan(uint32_t* __restrict__ p, uint32_t count, uint32_t* __restrict__ totals) {
    totals[threadIdx.x] = block_scan_in_place<THREADS>(p, count);
}

enum WaveOp { kWaveScan = 0, kWaveSum = 1, kWaveMaxU32 = 2, kWaveMaxInt = 3, kWaveMaxFloat = 4, kWaveOps = 5 };
template <int OP>
__global__ __launch_bounds__(1024) void k_probe_wave(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t v = in[i];
    if (OP == kWaveScan) out[i] = wave_inclusive_scan(v);
    if (OP == kWaveSum) out[i] = wave_sum(v);
    if (OP == kWaveMaxU32) out[i] = wave_max<uint32_t>(v);
    if (OP == kWaveMaxInt) out[i] = (uint32_t)wave_max<int>((int)v);
    if (OP == kWaveMaxFloat) out[i] = __float_as_uint(wave_max<float>(__uint_as_float(v)));
}

__global__ __launch_bounds__(1024) void k_probe_lane_rank(const unsigned long long* __restrict__ masks, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    out[i] = lane_rank(masks[i >> 6]);
}

enum BlockOp { kBlockSum = 0, kBlockPutGetSum = 1, kBlockPutGetMaxU32 = 2, kBlockPutGetMaxFloat = 3, kBlockOps = 4 };
template <int THREADS, int OP>
__global__ __launch_bounds__(THREADS) void k_probe_block_reduce(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_wave[THREADS / 64];
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    const uint32_t v = in[i];
    if (OP == kBlockSum) {
        out[i] = block_sum<THREADS>(v, s_wave);
    } else if (OP == kBlockPutGetSum) {
        block_put(v, s_wave, op_sum{});
        __syncthreads();
        out[i] = block_get<THREADS>(s_wave, op_sum{});
    } else if (OP == kBlockPutGetMaxU32) {
        block_put(v, s_wave, op_max{});
        __syncthreads();
        out[i] = block_get<THREADS>(s_wave, op_max{});
    } else {
        float* s_f = reinterpret_cast<float*>(s_wave);
        block_put(__uint_as_float(v), s_f, op_max{});
        __syncthreads();
        out[i] = __float_as_uint(block_get<THREADS>(s_f, op_max{}));
    }
}

constexpr int kAppendThreads = 256;
__global__ __launch_bounds__(kAppendThreads) void k_probe_append(const uint32_t* __restrict__ flags, uint32_t* __restrict__ counter,
                                                                 uint32_t* __restrict__ base_out, uint32_t* __restrict__ slot_out) {
    const uint32_t i = blockIdx.x * kAppendThreads + threadIdx.x;
    const unsigned long long mask = __ballot(flags[i] != 0u);
    const uint32_t base = wave_append_base(mask, counter);
    base_out[i] = base;
    slot_out[i] = base + lane_rank(mask);  // as every site forms a hit lane's slot
}

// the wave counts of events.hip (kEventThreads / 64) and trigger.hip (its kTgThreads / 64, local to that file)
constexpr int kReserveWaves = kEventThreads / 64;
static_assert(kReserveWaves == 4, "k_trigger_eval reserves with four waves as well");
template <bool BY_COUNT>
__global__ __launch_bounds__(kReserveWaves * 64) void k_probe_reserve(const uint32_t* __restrict__ counts, uint32_t trips,
                                                                      unsigned long long* __restrict__ cursor,
                                                                      unsigned long long* __restrict__ slots) {
    __shared__ SlotAppend<kReserveWaves> sh;
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const size_t i = ((size_t)blockIdx.x * trips + trip) * (kReserveWaves * 64) + threadIdx.x;
        const uint32_t c = counts[i];
        slots[i] = BY_COUNT ? slots_reserve_count<kReserveWaves>(c, trip, sh, cursor) : slots_reserve_flag<kReserveWaves>(c != 0u, trip, sh, cursor);
    }
}

// records per tile and threads of k_trigger_eval and k_field_apply (their kTgTile / kFfTile, local to those files)
constexpr uint32_t kTile = 32;
constexpr int kTileThreads = 256;
constexpr uint32_t kTileReadShift = 67;  // a thread reads back a vector that a thread of ANOTHER wave staged
template <uint32_t VEC>
__global__ __launch_bounds__(kTileThreads) void k_probe_tile_stage(const vol_f4* __restrict__ rec, uint32_t T, uint32_t first,
                                                                   vol_f4 fill, vol_f4* __restrict__ lds_out, vol_f4* __restrict__ read_out) {
    static_assert(kTile * VEC <= (uint32_t)kTileThreads && kTile * VEC > 2 * kTileReadShift, "one vector per thread; the shift leaves the wave");
    __shared__ vol_f4 tile[kTile * VEC];
    if (threadIdx.x < kTile * VEC) tile[threadIdx.x] = fill;  // what the first tile must leave behind its own records
    uint32_t k = 0;
    for (uint32_t t0 = first; t0 < T; t0 += kTile, ++k) {
        const uint32_t tn = min(kTile, T - t0);
        tile_stage<VEC>(tile, rec, t0, tn);
        // the whole tile, staged or left over ...
        if (threadIdx.x < kTile * VEC) {
            const uint32_t j = (threadIdx.x + kTileReadShift) % (kTile * VEC);
            lds_out[(size_t)k * kTile * VEC + j] = tile[j];
        }
        // ... and a staged vector for every thread of the workgroup
        read_out[(size_t)k * kTileThreads + threadIdx.x] = tile[(threadIdx.x + kTileReadShift) % (tn * VEC)];
    }
}

template <class F>
int32_t run_on_device0(F&& body) {
    DeviceKeeper keep;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return (int32_t)hipErrorNoDevice; }
    WP_TRY(hipSetDevice(0));
    return body();
}

}  // namespace

extern "C" {

// ---- scan.hip, host side (no device needed) -------------------------------------------------------------------------------
int32_t wave_probe_scan_is_one_launch(uint32_t count) { return scan_is_one_launch(count) ? 1 : 0; }
uint64_t wave_probe_scan_scratch_words(uint32_t count) { return (uint64_t)scan_scratch_words(count); }
void wave_probe_counters_layout(uint32_t* bytes, uint32_t* n_used_buckets_offset) {
    *bytes = (uint32_t)sizeof(StepCounters);
    *n_used_buckets_offset = (uint32_t)offsetof(StepCounters, n_used_buckets);
}

// launch_exclusive_scan on the world's stream. Every array is the caller's whole buffer - padding and guard words included -
// copied up before and back after. used_words == 0: no block_used and no counters (ctr_bytes must be 0 as well).
int32_t wave_probe_exclusive_scan(phys_world* w, uint32_t* in, uint64_t in_words, uint32_t count, uint32_t* out, uint64_t out_words,
                                  int32_t zero_in, uint32_t* scratch, uint64_t scratch_words, uint32_t* block_used, uint64_t used_words,
                                  void* ctr, uint64_t ctr_bytes) {
    if (!w || !in || !out || !scratch) return kBadArg;
    if (count == 0 || count % 4 != 0 || in_words < count || out_words < (uint64_t)count + 1) return kBadArg;
    if (scratch_words < scan_scratch_words(count)) return kBadArg;
    if ((used_words != 0) != (ctr_bytes != 0)) return kBadArg;  // k_scan_block_sums writes the sum of block_used through ctr
    if (used_words && (used_words < scan_scratch_words(count) || !block_used || !ctr || ctr_bytes != sizeof(StepCounters))) return kBadArg;
    DeviceKeeper keep;
    WP_TRY(hipSetDevice(w->device));
    hipStream_t s = w->stream;
    Mirror d_in, d_out, d_scratch, d_used, d_ctr;
    WP_TRY(d_in.up(in, in_words * 4, s));
    WP_TRY(d_out.up(out, out_words * 4, s));
    WP_TRY(d_scratch.up(scratch, scratch_words * 4, s));
    WP_TRY(d_used.up(block_used, used_words * 4, s));
    WP_TRY(d_ctr.up(ctr, ctr_bytes, s));
    launch_exclusive_scan(w, d_in.as<uint32_t>(), count, d_out.as<uint32_t>(), zero_in != 0, d_scratch.as<uint32_t>(),
                          used_words ? d_used.as<uint32_t>() : nullptr, used_words ? d_ctr.as<StepCounters>() : nullptr);
    WP_TRY(hipGetLastError());
    WP_TRY(hipStreamSynchronize(s));
    WP_TRY(d_in.down(s));
    WP_TRY(d_out.down(s));
    WP_TRY(d_scratch.down(s));
    WP_TRY(d_used.down(s));
    WP_TRY(d_ctr.down(s));
    return 0;
}

// ---- wave.hpp -------------------------------------------------------------------------------------------------------------
// block_scan_in_place<threads> (256 or 1024) of p[0 .. count) in ONE workgroup; p has p_words >= count words (guard
// included); totals[threads]: what each lane was returned
int32_t wave_probe_block_scan(int32_t threads, uint32_t* p, uint64_t p_words, uint32_t count, uint32_t* totals) {
    if ((threads != 256 && threads != 1024) || !p || !totals || p_words < count) return kBadArg;
    return run_on_device0([&]() -> int32_t {
        Mirror d_p, d_tot;
        WP_TRY(d_p.up(p, p_words * 4, nullptr));
        WP_TRY(d_tot.up(totals, (size_t)threads * 4, nullptr));
        if (threads == 256) hipLaunchKernelGGL(k_probe_block_scan<256>, dim3(1), dim3(256), 0, nullptr, d_p.as<uint32_t>(), count, d_tot.as<uint32_t>());
        else hipLaunchKernelGGL(k_probe_block_scan<1024>, dim3(1), dim3(1024), 0, nullptr, d_p.as<uint32_t>(), count, d_tot.as<uint32_t>());
        WP_TRY(hipGetLastError());
        WP_TRY(d_p.down(nullptr));
        WP_TRY(d_tot.down(nullptr));
        return 0;
    });
}

// one 32-bit word per thread in, one out (int and float by their bits); op: WaveOp; threads: 64, 256 or 1024 per workgroup
int32_t wave_probe_wave_op(int32_t op, int32_t threads, uint32_t blocks, uint32_t* in, uint32_t* out) {
    if (op < 0 || op >= kWaveOps || (threads != 64 && threads != 256 && threads != 1024) || blocks == 0 || blocks > 64 || !in || !out) return kBadArg;
    return run_on_device0([&]() -> int32_t {
        const size_t n = (size_t)blocks * threads;
        Mirror d_in, d_out;
        WP_TRY(d_in.up(in, n * 4, nullptr));
        WP_TRY(d_out.up(out, n * 4, nullptr));
        const dim3 g(blocks), b(threads);
        switch (op) {
        case kWaveScan: hipLaunchKernelGGL(k_probe_wave<kWaveScan>, g, b, 0, nullptr, d_in.as<uint32_t>(), d_out.as<uint32_t>()); break;
        case kWaveSum: hipLaunchKernelGGL(k_probe_wave<kWaveSum>, g, b, 0, nullptr, d_in.as<uint32_t>(), d_out.as<uint32_t>()); break;
        case kWaveMaxU32: hipLaunchKernelGGL(k_probe_wave<kWaveMaxU32>, g, b, 0, nullptr, d_in.as<uint32_t>(), d_out.as<uint32_t>()); break;
        case kWaveMaxInt: hipLaunchKernelGGL(k_probe_wave<kWaveMaxInt>, g, b, 0, nullptr, d_in.as<uint32_t>(), d_out.as<uint32_t>()); break;
        default: hipLaunchKernelGGL(k_probe_wave<kWaveMaxFloat>, g, b, 0, nullptr, d_in.as<uint32_t>(), d_out.as<uint32_t>()); break;
        }
        WP_TRY(hipGetLastError());
        WP_TRY(d_out.down(nullptr));
        return 0;
    });
}

// lane_rank of masks[wave] (one 64-bit ballot per wave of the launch, workgroup-major) in every lane
int32_t wave_probe_lane_rank(int32_t threads, uint32_t blocks, uint64_t* masks, uint32_t* out) {
    if ((threads != 64 && threads != 256 && threads != 1024) || blocks == 0 || blocks > 64 || !masks || !out) return kBadArg;
    return run_on_device0([&]() -> int32_t {
        const size_t n = (size_t)blocks * threads;
        Mirror d_m, d_out;
        WP_TRY(d_m.up(masks, n / 64 * 8, nullptr));
        WP_TRY(d_out.up(out, n * 4, nullptr));
        hipLaunchKernelGGL(k_probe_lane_rank, dim3(blocks), dim3(threads), 0, nullptr, d_m.as<unsigned long long>(), d_out.as<uint32_t>());
        WP_TRY(hipGetLastError());
        WP_TRY(d_out.down(nullptr));
        return 0;
    });
}

// op: BlockOp; threads: 256 or 1024; one word per thread in, the workgroup's result as every thread got it out
int32_t wave_probe_block_reduce(int32_t op, int32_t threads, uint32_t blocks, uint32_t* in, uint32_t* out) {
    if (op < 0 || op >= kBlockOps || (threads != 256 && threads != 1024) || blocks == 0 || blocks > 64 || !in || !out) return kBadArg;
    return run_on_device0([&]() -> int32_t {
        const size_t n = (size_t)blocks * threads;
        Mirror d_in, d_out;
        WP_TRY(d_in.up(in, n * 4, nullptr));
        WP_TRY(d_out.up(out, n * 4, nullptr));
        const dim3 g(blocks), b(threads);
        uint32_t* i = d_in.as<uint32_t>();
        uint32_t* o = d_out.as<uint32_t>();
#define WP_BLOCK_CASE(OP)                                                                                      \
    case OP:                                                                                                   \
        if (threads == 256) hipLaunchKernelGGL((k_probe_block_reduce<256, OP>), g, b, 0, nullptr, i, o);       \
        else hipLaunchKernelGGL((k_probe_block_reduce<1024, OP>), g, b, 0, nullptr, i, o);                     \
        break;
        switch (op) {
            WP_BLOCK_CASE(kBlockSum)
            WP_BLOCK_CASE(kBlockPutGetSum)
            WP_BLOCK_CASE(kBlockPutGetMaxU32)
            WP_BLOCK_CASE(kBlockPutGetMaxFloat)
        }
#undef WP_BLOCK_CASE
        WP_TRY(hipGetLastError());
        WP_TRY(d_out.down(nullptr));
        return 0;
    });
}

// wave_append_base in `blocks` workgroups of 256: flags[i] != 0 is lane i's vote (every wave needs one yes); *counter in and
// out; base_out: what wave_append_base returned to the lane, slot_out: that + lane_rank(ballot)
int32_t wave_probe_append(uint32_t blocks, uint32_t* flags, uint32_t* counter, uint32_t* base_out, uint32_t* slot_out) {
    if (blocks == 0 || blocks > 64 || !flags || !counter || !base_out || !slot_out) return kBadArg;
    const size_t n = (size_t)blocks * kAppendThreads;
    for (size_t wv = 0; wv < n / 64; ++wv) {  // the header's precondition: no wave calls it with an empty ballot
        bool any = false;
        for (size_t l = 0; l < 64; ++l) any = any || flags[64 * wv + l] != 0u;
        if (!any) return kBadArg;
    }
    return run_on_device0([&]() -> int32_t {
        Mirror d_f, d_c, d_b, d_s;
        WP_TRY(d_f.up(flags, n * 4, nullptr));
        WP_TRY(d_c.up(counter, 4, nullptr));
        WP_TRY(d_b.up(base_out, n * 4, nullptr));
        WP_TRY(d_s.up(slot_out, n * 4, nullptr));
        hipLaunchKernelGGL(k_probe_append, dim3(blocks), dim3(kAppendThreads), 0, nullptr, d_f.as<uint32_t>(), d_c.as<uint32_t>(),
                           d_b.as<uint32_t>(), d_s.as<uint32_t>());
        WP_TRY(hipGetLastError());
        WP_TRY(d_c.down(nullptr));
        WP_TRY(d_b.down(nullptr));
        WP_TRY(d_s.down(nullptr));
        return 0;
    });
}

// `blocks` workgroups of 256 make `trips` reservations each. counts[(block * trips + trip) * 256 + thread]: the lane's items
// (by_count: slots_reserve_count; else slots_reserve_flag with emit = count != 0). *cursor in and out; slots: the first slot
// each lane was given, in the layout of counts.
int32_t wave_probe_reserve(int32_t by_count, uint32_t blocks, uint32_t trips, uint32_t* counts, uint64_t* cursor, uint64_t* slots) {
    if (blocks == 0 || blocks > 64 || trips == 0 || trips > 64 || !counts || !cursor || !slots) return kBadArg;
    return run_on_device0([&]() -> int32_t {
        const size_t n = (size_t)blocks * trips * (kReserveWaves * 64);
        Mirror d_n, d_c, d_s;
        WP_TRY(d_n.up(counts, n * 4, nullptr));
        WP_TRY(d_c.up(cursor, 8, nullptr));
        WP_TRY(d_s.up(slots, n * 8, nullptr));
        const dim3 g(blocks), b(kReserveWaves * 64);
        if (by_count) hipLaunchKernelGGL(k_probe_reserve<true>, g, b, 0, nullptr, d_n.as<uint32_t>(), trips, d_c.as<unsigned long long>(), d_s.as<unsigned long long>());
        else hipLaunchKernelGGL(k_probe_reserve<false>, g, b, 0, nullptr, d_n.as<uint32_t>(), trips, d_c.as<unsigned long long>(), d_s.as<unsigned long long>());
        WP_TRY(hipGetLastError());
        WP_TRY(d_c.down(nullptr));
        WP_TRY(d_s.down(nullptr));
        return 0;
    });
}

// tile_stage<vec> (VOL_REC_VEC or FF_REC_VEC) in one workgroup of 256 over the tiles of 32 records [first, n_rec), as
// k_trigger_eval and k_field_apply walk them. rec: n_rec records of vec x 4 floats. The LDS tile starts out filled with
// fill[4]. Per tile k: lds_out[k][32 * vec][4] is the whole LDS tile behind the staging, read_out[k][256][4] what thread x
// read at vector (x + 67) % (tn * vec) of it. n_tiles: the caller's count of tiles, which sizes both.
int32_t wave_probe_tile_stage(int32_t vec, float* rec, uint32_t n_rec, uint32_t first, uint32_t n_tiles, float* fill, float* lds_out,
                              float* read_out) {
    if ((vec != VOL_REC_VEC && vec != FF_REC_VEC) || !rec || !fill || !lds_out || !read_out) return kBadArg;
    if (first >= n_rec || n_rec > (1u << 20) || n_tiles != (n_rec - first + kTile - 1) / kTile) return kBadArg;
    return run_on_device0([&]() -> int32_t {
        Mirror d_rec, d_lds, d_read;
        WP_TRY(d_rec.up(rec, (size_t)n_rec * vec * 16, nullptr));
        WP_TRY(d_lds.up(lds_out, (size_t)n_tiles * kTile * vec * 16, nullptr));
        WP_TRY(d_read.up(read_out, (size_t)n_tiles * kTileThreads * 16, nullptr));
        vol_f4 f;
        std::memcpy(&f, fill, sizeof(f));
        if (vec == VOL_REC_VEC)
            hipLaunchKernelGGL(k_probe_tile_stage<VOL_REC_VEC>, dim3(1), dim3(kTileThreads), 0, nullptr, d_rec.as<const vol_f4>(), n_rec, first, f,
                               d_lds.as<vol_f4>(), d_read.as<vol_f4>());
        else
            hipLaunchKernelGGL(k_probe_tile_stage<FF_REC_VEC>, dim3(1), dim3(kTileThreads), 0, nullptr, d_rec.as<const vol_f4>(), n_rec, first, f,
                               d_lds.as<vol_f4>(), d_read.as<vol_f4>());
        WP_TRY(hipGetLastError());
        WP_TRY(d_lds.down(nullptr));
        WP_TRY(d_read.down(nullptr));
        return 0;
    });
}

}  // extern "C"
