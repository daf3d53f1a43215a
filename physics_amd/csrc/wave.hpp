// wave.hpp — the wave (64 lanes) and workgroup idioms every kernel file shares: reductions, scans, ballot ranks,
// appends behind one atomic. Device functions only, no state; the one parameter is the workgroup size, a template
// argument. DESIGN.md section 18.
#pragma once
#include <hip/hip_runtime.h>

namespace phys {

// ---- one wave ---------------------------------------------------------------------------------------------------------
// butterfly over the 64 lanes: every lane ends with op folded over all lanes' values (op commutative and associative)
template <class T, class Op>  // T: 32 bits (uint32_t, int, float)
__device__ __forceinline__ T wave_reduce(T v, Op op) {
    static_assert(sizeof(T) == 4, "one dword per lane");
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __builtin_bit_cast(T, __shfl_xor(__builtin_bit_cast(int, v), off, 64)));
    return v;
}
struct op_sum { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
// `b > a ? b : a`: a NaN in operand b is ignored, a NaN in operand a is KEPT. In wave_reduce a is the lane's own value: a
// lane that holds a NaN ends with NaN, and the values that would have reached another lane through it are lost to that
// lane - a lane without NaN ends with the maximum over SOME of the wave's non-NaN lanes, its own among them, not
// necessarily all of them (block_get then drops a wave whose lane 0 held a NaN). So these are maxima of values that are
// never NaN: a caller folds NaN away per thread first (constraints.hip block_amax: `e > m ? e : m` from 0).
struct op_max { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; } };
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_reduce(v, op_sum{}); }
template <class T>  // uint32_t, int, float
__device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, op_max{}); }

// inclusive prefix sum over the wave: lane 63 holds the wave's total
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// set bits of a ballot below this lane: the lane's place among the lanes that voted yes
__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
    const int lane = threadIdx.x & 63;
    return (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// Append behind ONE atomic per wave (same-address atomics serialise chip-wide): lane 0 adds popc(mask) to *counter and
// the old value comes back to every lane; the lane's slot is that base + lane_rank(mask). Every lane of the wave calls
// it together, with a non-zero mask.
__device__ __forceinline__ uint32_t wave_append_base(unsigned long long mask, uint32_t* counter) {
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == 0u) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    return (uint32_t)__shfl((int)base, 0, 64);
}

// ---- one workgroup of THREADS lanes, through one LDS word per wave ------------------------------------------------------
// A reduction is two halves around the caller's barrier: block_put (every lane; lane 0 of each wave leaves its wave's
// result in s_wave) and, behind a __syncthreads(), block_get (whoever wants the result: every lane, or thread 0 alone).
// A site that has something of its own to do in front of that barrier puts it between the two.
template <class T, class Op>
__device__ __forceinline__ void block_put(T v, T* s_wave, Op op) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = v;
}
// (the fold starts from T(0): sums, and maxima of values that are never negative)
template <int THREADS, class T, class Op>
__device__ __forceinline__ T block_get(const T* s_wave, Op op) {
    T t = T(0);
    for (int k = 0; k < THREADS / 64; ++k) t = op(t, s_wave[k]);
    return t;
}
// the sum over the workgroup, to every lane (one barrier; s_wave is free again behind the caller's next one)
template <int THREADS>
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s_wave) {
    block_put(v, s_wave, op_sum{});
    __syncthreads();
    return block_get<THREADS>(s_wave, op_sum{});
}

// One workgroup's exclusive scan of p[0 .. count) in place, THREADS words per trip with a carry; returns the grand
// total to every lane. One barrier per trip: the wave totals alternate between two sets (see SlotAppend), and every
// lane keeps the carry itself.
template <int THREADS>
__device__ __forceinline__ uint32_t block_scan_in_place(uint32_t* __restrict__ p, uint32_t count) {
    __shared__ uint32_t s_tot[2][THREADS / 64];
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t carry = 0, set = 0;
    for (uint32_t base = 0; base < count; base += THREADS, set ^= 1u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < count ? p[i] : 0u;
        const uint32_t inc = wave_inclusive_scan(v);
        if ((threadIdx.x & 63u) == 63u) s_tot[set][wave] = inc;
        __syncthreads();
        uint32_t before = carry;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)(THREADS / 64); ++k) {
            const uint32_t t = s_tot[set][k];
            if (k < wave) before += t;
            carry += t;
        }
        if (i < count) p[i] = before + inc - v;
    }
    return carry;
}

// ---- a tile of records through LDS ---------------------------------------------------------------------------------------
// Records [t0, t0 + tn) of VEC 16-byte vectors each (V: the vector type) from `rec` into `tile`, one vector per thread - the
// caller asserts that a whole tile is no more than that -, a barrier in front (the previous tile has been read by everybody)
// and one behind. Every thread of the workgroup calls it.
template <uint32_t VEC, class V>
__device__ __forceinline__ void tile_stage(V* tile, const V* __restrict__ rec, uint32_t t0, uint32_t tn) {
    __syncthreads();
    if (threadIdx.x < tn * VEC) tile[threadIdx.x] = rec[VEC * (size_t)t0 + threadIdx.x];
    __syncthreads();
}

// ---- slots of an append-only buffer, reserved once per workgroup and trip ------------------------------------------------
// LDS of one reservation; the per-wave totals alternate between two sets, so that a wave which runs ahead into the
// next trip does not overwrite totals a slower wave still adds up
template <int WAVES>
struct SlotAppend {
    uint32_t wave_total[2][WAVES];
    unsigned long long base;
};

// The first slot of this lane's items: `excl` of them belong to lower lanes of its wave, `wave_total` (wave-uniform) to
// the wave. ONE global atomic per workgroup; the cursor keeps counting past any capacity, which the caller checks per
// slot. Every thread of the workgroup calls it, once per trip.
template <int WAVES>
__device__ __forceinline__ unsigned long long slots_reserve(uint32_t excl, uint32_t wave_total, uint32_t trip, SlotAppend<WAVES>& sh,
                                                            unsigned long long* cursor) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, set = trip & 1u;
    if (lane == 0) sh.wave_total[set][wave] = wave_total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < WAVES; ++k) t += sh.wave_total[set][k];
        sh.base = t ? atomicAdd(cursor, (unsigned long long)t) : 0ull;
    }
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t k = 0; k < wave; ++k) off += sh.wave_total[set][k];
    return sh.base + off + excl;
}
// one item or none per lane (the slot is meaningful where emit is true)
template <int WAVES>
__device__ __forceinline__ unsigned long long slots_reserve_flag(bool emit, uint32_t trip, SlotAppend<WAVES>& sh, unsigned long long* cursor) {
    const unsigned long long mask = __ballot(emit);
    return slots_reserve(lane_rank(mask), (uint32_t)__popcll(mask), trip, sh, cursor);
}
// `count` items per lane, in consecutive slots
template <int WAVES>
__device__ __forceinline__ unsigned long long slots_reserve_count(uint32_t count, uint32_t trip, SlotAppend<WAVES>& sh, unsigned long long* cursor) {
    const uint32_t incl = wave_inclusive_scan(count);
    return slots_reserve(incl - count, (uint32_t)__shfl((int)incl, 63, 64), trip, sh, cursor);
}

}  // namespace phys
