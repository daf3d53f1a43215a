// coloring.hip — the deterministic manifold colouring that orders the solver, and the colour-major sort of the rows,
// for gfx950. No reference counterpart; the colouring rule is that of include/spec/contact_solve.h.
//
// colouring: synchronous Jones-Plassmann rounds on the line graph over the NEW manifolds, one launch per round
//   (k_color_round, three rotating per-body priority buffers) + k_color_finish, or everything including the
//   colour-major sort in one workgroup for small scenes (k_color_small). max / or are order-independent, so the
//   colours are a pure function of (previous colouring, manifold SET). Round 0's priorities and the list of the
//   uncoloured manifolds come from k_narrowphase (narrowphase.hip).
#include "kernels.hpp"

namespace phys {

// ---- colouring --------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t stored_manifolds(const StepCounters* ctr, uint64_t max_manifolds) {
    const uint32_t m = ctr->n_manifolds;
    return (uint64_t)m < max_manifolds ? m : (uint32_t)max_manifolds;
}

constexpr int kColorStage = 8192;  // losers of one workgroup and round staged in LDS (k_color_round)

// Ordering between the waves of ONE workgroup that talk through global memory (single-workgroup colouring
// kernels): every wave's stores and atomics have been performed at the L2 once its vmcnt has drained, and the
// readers load past the L1 (sc1 atomic loads), so draining + the workgroup barrier is all it takes. An
// agent-scope __threadfence() here would write back and invalidate caches of the whole XCD from all 16 waves
// (microseconds per round) for data that never leaves this CU's path to its L2.
__device__ __forceinline__ void drain_stores_for_workgroup() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// One synchronous Jones-Plassmann round in ONE launch. Three per-body priority buffers rotate:
//   top      (read)   maxima over the manifolds uncoloured at the start of this round - complete;
//   top_next (atomic) losers of this round = exactly the manifolds uncoloured at the start of the next
//                     round publish their priority there (it was cleared one round ago);
//   top_clr  (store)  the buffer read one round ago, cleared at the losers' bodies for the round after next.
// Round 0's `top` is filled by k_narrowphase at emission time.
// body of one round for the manifolds m = first, first + stride, ...; returns this lane's wins
// AGG: `next_list` is a list in global memory shared by all workgroups of the launch. Same-address atomics serialise
// chip-wide (~88 per microsecond), so the losers of a workgroup are staged in LDS (`stage`, one LDS atomic per wave and
// trip) and the caller appends them with ONE global atomic; only what does not fit the stage goes out directly.
template <bool BYPASS_L1, bool AGG = false>
__device__ __forceinline__ uint32_t color_round_lanes(uint32_t first, uint32_t stride, uint32_t M,
                                                      const uint32_t* list /* null: every manifold; else M ids */,
                                                      uint32_t* next_list /* non-null: `list` holds uncoloured ids only, and
                                                                             the losers of this round are appended here */,
                                                      uint32_t* next_count,
                                                      const uint32_t* __restrict__ man_a, const uint32_t* __restrict__ man_b,
                                                      uint32_t* __restrict__ man_color, const uint64_t* __restrict__ man_prio,
                                                      const unsigned long long* top, unsigned long long* top_next,
                                                      unsigned long long* top_clr, unsigned long long* used,
                                                      StepCounters* __restrict__ ctr, uint32_t* stage = nullptr,
                                                      uint32_t* stage_n = nullptr, uint32_t stage_cap = 0) {
    uint32_t wins = 0;
    for (uint32_t i = first; i < M; i += stride) {
        // (single-launch loops: a global list was written by other waves of this workgroup one round ago)
        const uint32_t m = list ? (BYPASS_L1 ? __hip_atomic_load(&list[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : list[i]) : i;
        if (!next_list && man_color[m] != kUncolored) continue;
        const unsigned long long p = man_prio[m];
        const uint32_t a = man_a[m], b = man_b[m];
        const bool gb = PHYS_IS_STATIC_PARTNER(b);  // the ground or a static collider: no colour state of its own
        bool lose = false;
        // BYPASS_L1 (single-launch finish loop): words other waves changed with atomics inside this launch
        // must come from L2, not from a line this CU cached rounds ago
        const unsigned long long ta = BYPASS_L1 ? __hip_atomic_load(&top[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : top[a];
        unsigned long long tb = p;
        if (!gb) tb = BYPASS_L1 ? __hip_atomic_load(&top[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : top[b];
        if (ta == p && tb == p) {
            unsigned long long mask = BYPASS_L1 ? __hip_atomic_load(&used[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : used[a];
            unsigned long long mb = 0ull;
            if (!gb) { mb = BYPASS_L1 ? __hip_atomic_load(&used[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : used[b]; }
            const unsigned long long ma = mask;
            mask |= mb;
            uint32_t c = 0;
            while (c < (uint32_t)(PHYS_MAX_COLORS - 1) && ((mask >> c) & 1ull)) ++c;
            if (((mask >> c) & 1ull)) flag_overflow(ctr, kOvfColors);  // more than PHYS_MAX_COLORS at one body
            // the winner is the only manifold touching a or b that colours this round
            if (BYPASS_L1) {
                __hip_atomic_store(&used[a], ma | (1ull << c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (!gb) __hip_atomic_store(&used[b], mb | (1ull << c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                used[a] = ma | (1ull << c);
                if (!gb) used[b] = mb | (1ull << c);
            }
            man_color[m] = c;
            ++wins;
        } else {
            lose = true;
            if (next_list && !AGG) next_list[atomicAdd(next_count, 1u)] = m;
            atomicMax(&top_next[a], p);
            if (BYPASS_L1) __hip_atomic_store(&top_clr[a], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else top_clr[a] = 0ull;
            if (!gb) {
                atomicMax(&top_next[b], p);
                if (BYPASS_L1) __hip_atomic_store(&top_clr[b], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else top_clr[b] = 0ull;
            }
        }
        if (AGG) {
            const unsigned long long losers = __ballot(lose);
            if (losers) {
                const int lane = (int)(threadIdx.x & 63u), leader = __ffsll((long long)losers) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(stage_n, (uint32_t)__popcll(losers));  // LDS
                base = (uint32_t)__shfl((int)base, leader, 64);
                if (lose) {
                    const uint32_t at = base + (uint32_t)__popcll(losers & ((1ull << lane) - 1ull));
                    if (at < stage_cap) stage[at] = m;
                    else next_list[atomicAdd(next_count, 1u)] = m;  // the stage is full (a launch far smaller than its list)
                }
            }
        }
    }
    return wins;
}

// One synchronous Jones-Plassmann round in ONE launch. Three per-body priority buffers rotate:
//   top      (read)   maxima over the manifolds uncoloured at the start of this round - complete;
//   top_next (atomic) losers of this round = exactly the manifolds uncoloured at the start of the next
//                     round publish their priority there (it was cleared one round ago);
//   top_clr  (store)  the buffer read one round ago, cleared at the losers' bodies for the round after next.
// Round 0's `top` is filled by k_narrowphase at emission time.
// The round runs over the LIST of the manifolds that were uncoloured at its start (round 0: written by the narrow
// phase; round r + 1: the losers of round r) - a steady pile has a few per cent of new manifolds per update, and
// scanning the colours of all of them in every round was 7.4 us per launch on C5, twenty times per step.
__global__ __launch_bounds__(kColorThreads) void k_color_round(uint32_t round, uint64_t max_manifolds,
                                                              const uint32_t* __restrict__ man_a,
                                                              const uint32_t* __restrict__ man_b,
                                                              uint32_t* __restrict__ man_color,
                                                              const uint64_t* __restrict__ man_prio,
                                                              const unsigned long long* __restrict__ top,
                                                              unsigned long long* __restrict__ top_next,
                                                              unsigned long long* __restrict__ top_clr,
                                                              unsigned long long* __restrict__ used,
                                                              const uint32_t* __restrict__ list, uint32_t* __restrict__ next_list,
                                                              StepCounters* __restrict__ ctr) {
    // block-uniform early exit (every thread must act on the SAME read: a barrier follows)
    __shared__ uint32_t s_count;
    __shared__ uint32_t s_wins[kColorThreads / 64];
    if (threadIdx.x == 0) {
        const uint32_t c = ctr->unc_count[round % 3u];
        s_count = (uint64_t)c < max_manifolds ? c : (uint32_t)max_manifolds;
        // the counter read one round ago is appended to one round from now
        if (blockIdx.x == 0) ctr->unc_count[(round + 2u) % 3u] = 0u;
    }
    __syncthreads();
    const uint32_t count = s_count;
    if (blockIdx.x * blockDim.x >= count) return;
    __shared__ uint32_t s_stage[kColorStage];
    __shared__ uint32_t s_stage_n, s_stage_base;
    if (threadIdx.x == 0) s_stage_n = 0;
    __syncthreads();
    uint32_t* next_count = &ctr->unc_count[(round + 1u) % 3u];
    uint32_t wins = color_round_lanes<false, true>(blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, count, list, next_list,
                                                   next_count, man_a, man_b, man_color, man_prio, top, top_next, top_clr, used, ctr,
                                                   s_stage, &s_stage_n, (uint32_t)kColorStage);
    __syncthreads();
    const uint32_t staged = s_stage_n < (uint32_t)kColorStage ? s_stage_n : (uint32_t)kColorStage;
    if (threadIdx.x == 0 && staged) s_stage_base = atomicAdd(next_count, staged);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < staged; i += kColorThreads) next_list[s_stage_base + i] = s_stage[i];
    // ONE global atomic per workgroup (same-address atomics serialise chip-wide at ~88 per microsecond)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wins += (uint32_t)__shfl_xor((int)wins, off, 64);
    if ((threadIdx.x & 63) == 0) s_wins[threadIdx.x >> 6] = wins;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int k = 0; k < kColorThreads / 64; ++k) t += s_wins[k];
        if (t) {
            atomicSub(&ctr->n_uncolored, t);
            // rounds used = index of the last round that coloured something + 1 (every round with an
            // uncoloured manifold colours at least the one of highest priority)
            if (round + 1 > ctr->color_rounds) atomicMax(&ctr->color_rounds, round + 1);
        }
    }
}

// Runs the rounds that are still needed after the launched ones, inside ONE workgroup (barrier between rounds), over
// the same shrinking lists, so the host never has to ask the device whether the colouring is complete. Normally
// nothing or a handful of manifolds is left.
__global__ __launch_bounds__(kColorThreads) void k_color_finish(uint32_t round, uint64_t max_manifolds,
                                                               const uint32_t* __restrict__ man_a,
                                                               const uint32_t* __restrict__ man_b,
                                                               uint32_t* __restrict__ man_color,
                                                               const uint64_t* __restrict__ man_prio,
                                                               unsigned long long* __restrict__ state /*4n*/, uint64_t n,
                                                               uint32_t* __restrict__ lists /* 2 x max_manifolds */,
                                                               StepCounters* __restrict__ ctr) {
    __shared__ uint32_t s_left;
    __shared__ uint32_t s_cnt[2];
    __shared__ uint32_t s_wins[kColorThreads / 64];
    if (threadIdx.x == 0) {
        s_left = ctr->n_uncolored;
        const uint32_t c = ctr->unc_count[round % 3u];  // what round `round` would have read
        s_cnt[round & 1u] = (uint64_t)c < max_manifolds ? c : (uint32_t)max_manifolds;
    }
    __syncthreads();
    const uint32_t left0 = s_left;
    uint32_t left = left0;
    unsigned long long* used = state;
    while (left != 0) {
        unsigned long long* top = state + (1 + round % 3) * n;
        unsigned long long* top_next = state + (1 + (round + 1) % 3) * n;
        unsigned long long* top_clr = state + (1 + (round + 2) % 3) * n;
        const uint32_t cur = round & 1u, nxt = cur ^ 1u;
        if (threadIdx.x == 0) s_cnt[nxt] = 0;
        __syncthreads();
        uint32_t wins = color_round_lanes<true>(threadIdx.x, kColorThreads, s_cnt[cur], lists + cur * max_manifolds, lists + nxt * max_manifolds,
                                                &s_cnt[nxt], man_a, man_b, man_color, man_prio, top, top_next, top_clr, used, ctr);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) wins += (uint32_t)__shfl_xor((int)wins, off, 64);
        if ((threadIdx.x & 63) == 0) s_wins[threadIdx.x >> 6] = wins;
        drain_stores_for_workgroup();  // this round's stores and atomics are performed before anyone starts the next
        __syncthreads();
        uint32_t t = 0;
        for (int k = 0; k < kColorThreads / 64; ++k) t += s_wins[k];
        left -= t;
        ++round;
        __syncthreads();
        if (t == 0) break;  // cannot happen (the highest priority always wins); never spin
    }
    if (threadIdx.x == 0 && left != left0) {
        ctr->n_uncolored = left;
        ctr->color_rounds = round;
    }
}

// ---- colour-major renumbering: counting sort of the manifolds by colour ---------------------------
// hist (per-workgroup colour histogram) -> offsets (one workgroup scans colour-major) -> place.
// No global atomics; the order inside a colour is (workgroup, arrival), which nothing depends on.

__global__ __launch_bounds__(1024) void k_color_hist(uint64_t max_manifolds, const uint32_t* __restrict__ man_color,
                                                     uint32_t* __restrict__ block_hist /*[colour][nb]*/, uint32_t nb,
                                                     const StepCounters* __restrict__ ctr) {
    __shared__ uint32_t h[PHYS_MAX_COLORS];
    if (threadIdx.x < PHYS_MAX_COLORS) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t M = stored_manifolds(ctr, max_manifolds);
    for (uint32_t base = blockIdx.x * kSortChunk; base < M; base += gridDim.x * kSortChunk) {
#pragma unroll
        for (int k = 0; k < kSortChunk / 1024; ++k) {
            const uint32_t m = base + k * 1024 + threadIdx.x;
            if (m < M) {
                const uint32_t c = man_color[m];
                if (c < (uint32_t)PHYS_MAX_COLORS) atomicAdd(&h[c], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < PHYS_MAX_COLORS) block_hist[threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// one workgroup: exclusive scan of block_hist in colour-major order (in place) + per-colour totals
__global__ __launch_bounds__(1024) void k_color_offsets(uint32_t* __restrict__ block_hist, uint32_t nb, StepCounters* __restrict__ ctr) {
    // every WAVE owns a run of consecutive entries, read 64 at a time (coalesced, all loads in flight at once), scanned
    // with shuffles and a running carry; then one scan of the 16 wave totals (38 us for the 32 dependent block-wide passes
    // of the first version at 512 workgroups, 59 us with a run per THREAD - 32 dependent uncoalesced loads - 8 us so)
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t carry_s;
    const uint32_t kPerColor = nb;
    const uint32_t kTotal = PHYS_MAX_COLORS * kPerColor;   // <= 64 * 512
    const uint32_t per_wave = (kTotal + 15u) / 16u;        // nb is a power of two: a multiple of 4
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t w_begin = wave * per_wave < kTotal ? wave * per_wave : kTotal;
    const uint32_t w_end = w_begin + per_wave < kTotal ? w_begin + per_wave : kTotal;
    constexpr int kTrips = (PHYS_MAX_COLORS * kSortBlocksMax / 16 + 63) / 64;  // 32, eight at a time (registers)
    constexpr int kHalf = kTrips / 4;
    uint32_t v[kHalf];
    uint32_t run = 0;  // sum of this wave's entries in front of the current trip
    // pass 1: the wave's total; pass 2 (after the scan of the wave totals): the exclusive offsets, written in place
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t base = 0;
        if (pass == 1) {
            if (lane == 0) wtot[wave] = run;
            __syncthreads();
            for (uint32_t k = 0; k < wave; ++k) base += wtot[k];
            if (threadIdx.x == 1023) carry_s = base + run;
            run = 0;
        }
        for (int half = 0; half < 4; ++half) {
            const uint32_t h_begin = w_begin + (uint32_t)(half * kHalf) * 64u;
            if (h_begin >= w_end) break;  // wave-uniform
#pragma unroll
            for (int k = 0; k < kHalf; ++k) {
                const uint32_t i = h_begin + (uint32_t)k * 64u + lane;
                v[k] = i < w_end ? block_hist[i] : 0u;
            }
#pragma unroll
            for (int k = 0; k < kHalf; ++k) {
                uint32_t inc = v[k];
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
                    if (lane >= (uint32_t)off) inc += o;
                }
                const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
                const uint32_t i = h_begin + (uint32_t)k * 64u + lane;
                if (pass == 1 && i < w_end) {
                    const uint32_t excl = base + run + inc - v[k];
                    block_hist[i] = excl;
                    if (i % kPerColor == 0) ctr->color_start[i / kPerColor] = excl;
                }
                run += total;
            }
        }
    }
    uint32_t ncol = 0;
    __syncthreads();
    if (threadIdx.x == 0) ctr->color_start[PHYS_MAX_COLORS] = carry_s;
    __syncthreads();
    if (threadIdx.x < PHYS_MAX_COLORS) {
        const uint32_t cnt = ctr->color_start[threadIdx.x + 1] - ctr->color_start[threadIdx.x];
        ctr->color_count[threadIdx.x] = cnt;
        uint32_t cmax = cnt ? threadIdx.x + 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)cmax, off, 64);
            cmax = o > cmax ? o : cmax;
        }
        ncol = cmax;
        if (threadIdx.x == 0) ctr->n_colors = ncol;
    }
}

__global__ __launch_bounds__(1024) void k_color_place(uint64_t max_manifolds, const uint32_t* __restrict__ man_color,
                                                      const uint32_t* __restrict__ block_off /*scanned block_hist*/, uint32_t nb,
                                                      uint32_t* __restrict__ row_src, const StepCounters* __restrict__ ctr,
                                                      StepCounters* snap_out /* host-mapped, may be null */) {
    __shared__ uint32_t cursor[PHYS_MAX_COLORS];
    if (threadIdx.x < PHYS_MAX_COLORS) cursor[threadIdx.x] = block_off[threadIdx.x * nb + blockIdx.x];
    counters_snapshot(ctr, snap_out);
    __syncthreads();
    const uint32_t M = stored_manifolds(ctr, max_manifolds);
    for (uint32_t base = blockIdx.x * kSortChunk; base < M; base += gridDim.x * kSortChunk) {
#pragma unroll
        for (int k = 0; k < kSortChunk / 1024; ++k) {
            const uint32_t m = base + k * 1024 + threadIdx.x;
            if (m < M) {
                const uint32_t c = man_color[m];
                if (c < (uint32_t)PHYS_MAX_COLORS) row_src[atomicAdd(&cursor[c], 1u)] = m;
            }
        }
    }
}

// Small scenes (<= 40k manifolds): the WHOLE colouring stage in ONE launch of ONE workgroup - every
// Jones-Plassmann round (over a list of the uncoloured manifolds gathered into LDS: with persistent colouring
// only the new ones), the colour-major counting sort, and the snapshot of the counters into pinned host memory
// (the launch-size hints of later steps) - instead of ~3 round launches + finish + sort + a copy.
constexpr int kSmallList = 6144;  // ids per list; two lists: the uncoloured of this round / of the next
__global__ __launch_bounds__(kColorThreads) void k_color_small(uint64_t max_manifolds, const uint32_t* __restrict__ man_a,
                                                              const uint32_t* __restrict__ man_b, uint32_t* man_color,
                                                              const uint64_t* __restrict__ man_prio,
                                                              unsigned long long* __restrict__ state /*4n*/, uint64_t n,
                                                              uint32_t* __restrict__ row_src, StepCounters* ctr,
                                                              StepCounters* snap_out /* host-mapped, may be null */) {
    __shared__ uint32_t s_list[2][kSmallList];
    __shared__ uint32_t s_cnt[2];
    __shared__ uint32_t s_n, s_left;
    __shared__ uint32_t s_wins[kColorThreads / 64];
    __shared__ uint32_t h[PHYS_MAX_COLORS], cursor[PHYS_MAX_COLORS];
    const uint32_t M = stored_manifolds(ctr, max_manifolds);
    if (threadIdx.x == 0) { s_n = 0; s_left = ctr->n_uncolored; }
    if (threadIdx.x < PHYS_MAX_COLORS) h[threadIdx.x] = 0;
    // the colours of this thread's manifolds (m = k * 1024 + thread) stay in registers for all three passes
    // (gather the uncoloured, histogram, placement); a larger M than the launch expected takes the slow loops
    const bool in_regs = M <= (uint32_t)(kSmallTrips * kColorThreads);
    uint32_t col[kSmallTrips];
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < kSmallTrips; ++k) {
            const uint32_t m = k * kColorThreads + threadIdx.x;
            col[k] = m < M ? man_color[m] : 0xFFFFFFFEu;  // neither a colour nor kUncolored
        }
    }
    __syncthreads();
    uint32_t left = s_left;
    if (left != 0 && left <= M) {
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < kSmallTrips; ++k) {
                if (col[k] == kUncolored) {
                    const uint32_t at = atomicAdd(&s_n, 1u);
                    if (at < (uint32_t)kSmallList) s_list[0][at] = k * kColorThreads + threadIdx.x;
                }
            }
        } else {
            for (uint32_t m = threadIdx.x; m < M; m += kColorThreads) {
                if (man_color[m] == kUncolored) {
                    const uint32_t at = atomicAdd(&s_n, 1u);
                    if (at < (uint32_t)kSmallList) s_list[0][at] = m;
                }
            }
        }
        __syncthreads();
        // The rounds run over a LIST of the uncoloured manifolds that shrinks with every round (the losers of a round
        // are the list of the next one). A full re-colouring starts with more than a list holds: it scans all
        // manifolds until few enough are left.
        bool listed = s_n <= (uint32_t)kSmallList;
        uint32_t cur = 0;
        if (threadIdx.x == 0) s_cnt[0] = s_n;
        unsigned long long* used = state;
        uint32_t round = 0;
        while (left != 0) {
            unsigned long long* top = state + (1 + round % 3) * n;
            unsigned long long* top_next = state + (1 + (round + 1) % 3) * n;
            unsigned long long* top_clr = state + (1 + (round + 2) % 3) * n;
            const uint32_t nxt = cur ^ 1u;
            if (threadIdx.x == 0) s_cnt[nxt] = 0;
            __syncthreads();
            uint32_t wins = listed
                ? color_round_lanes<true>(threadIdx.x, kColorThreads, s_cnt[cur], s_list[cur], s_list[nxt], &s_cnt[nxt], man_a, man_b,
                                          man_color, man_prio, top, top_next, top_clr, used, ctr)
                : color_round_lanes<true>(threadIdx.x, kColorThreads, M, nullptr, nullptr, nullptr, man_a, man_b, man_color,
                                          man_prio, top, top_next, top_clr, used, ctr);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) wins += (uint32_t)__shfl_xor((int)wins, off, 64);
            if ((threadIdx.x & 63) == 0) s_wins[threadIdx.x >> 6] = wins;
            drain_stores_for_workgroup();  // this round's stores and atomics are performed before anyone starts the next
            __syncthreads();
            uint32_t t = 0;
            for (int k = 0; k < kColorThreads / 64; ++k) t += s_wins[k];
            left -= t;
            ++round;
            if (t == 0) break;  // cannot happen (the highest priority always wins); never spin
            if (listed) {
                cur = nxt;
            } else if (left != 0 && left <= (uint32_t)kSmallList) {
                // few enough are left: list them (each thread looks at the manifolds it has been handling itself)
                if (threadIdx.x == 0) s_cnt[0] = 0;
                __syncthreads();
                for (uint32_t m = threadIdx.x; m < M; m += kColorThreads)
                    if (__hip_atomic_load(&man_color[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kUncolored)
                        s_list[0][atomicAdd(&s_cnt[0], 1u)] = m;
                listed = true;
                cur = 0;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            ctr->n_uncolored = left;
            ctr->color_rounds = round;
        }
        if (in_regs) {  // colours other waves of this workgroup wrote: read past the L1
#pragma unroll
            for (int k = 0; k < kSmallTrips; ++k)
                if (col[k] == kUncolored)
                    col[k] = __hip_atomic_load(&man_color[k * kColorThreads + threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // colour-major counting sort
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < kSmallTrips; ++k) if (col[k] < (uint32_t)PHYS_MAX_COLORS) atomicAdd(&h[col[k]], 1u);
    } else {
        for (uint32_t m = threadIdx.x; m < M; m += kColorThreads) {
            const uint32_t c = __hip_atomic_load(&man_color[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c < (uint32_t)PHYS_MAX_COLORS) atomicAdd(&h[c], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < PHYS_MAX_COLORS) {  // one wave: exclusive scan of the 64 counts
        const uint32_t cnt = h[threadIdx.x];
        uint32_t inc = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
            if ((int)threadIdx.x >= off) inc += o;
        }
        const uint32_t start = inc - cnt;
        cursor[threadIdx.x] = start;
        ctr->color_start[threadIdx.x] = start;
        ctr->color_count[threadIdx.x] = cnt;
        if (threadIdx.x == 63) ctr->color_start[PHYS_MAX_COLORS] = inc;
        uint32_t cmax = cnt ? threadIdx.x + 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)cmax, off, 64);
            cmax = o > cmax ? o : cmax;
        }
        if (threadIdx.x == 0) ctr->n_colors = cmax;
    }
    drain_stores_for_workgroup();
    __syncthreads();
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < kSmallTrips; ++k)
            if (col[k] < (uint32_t)PHYS_MAX_COLORS) row_src[atomicAdd(&cursor[col[k]], 1u)] = k * kColorThreads + threadIdx.x;
    } else {
        for (uint32_t m = threadIdx.x; m < M; m += kColorThreads) {
            const uint32_t c = __hip_atomic_load(&man_color[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c < (uint32_t)PHYS_MAX_COLORS) row_src[atomicAdd(&cursor[c], 1u)] = m;
        }
    }
    if (snap_out) {  // the counters as they stand after the colouring stage
        const uint32_t words = (uint32_t)(sizeof(StepCounters) / 4);
        if (threadIdx.x < words)
            reinterpret_cast<uint32_t*>(snap_out)[threadIdx.x] =
                __hip_atomic_load(reinterpret_cast<uint32_t*>(ctr) + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static void launch_color_round(phys_world* w, uint32_t round, unsigned blocks) {
    unsigned long long* used = w->color_state.p;
    unsigned long long* T[3] = {w->color_state.p + w->n, w->color_state.p + 2 * w->n, w->color_state.p + 3 * w->n};
    PHYS_PROF(w, PHYS_STAGE_COLOR);
    hipLaunchKernelGGL(k_color_round, dim3(blocks), dim3(kColorThreads), 0, w->stream, round, w->max_manifolds,
                       w->man_a.p, w->man_b.p, w->man_color.p, w->man_prio.p, T[round % 3], T[(round + 1) % 3],
                       T[(round + 2) % 3], used, w->unc_list.p + (round & 1u) * w->max_manifolds,
                       w->unc_list.p + ((round + 1u) & 1u) * w->max_manifolds, w->counters.p);
}

// a pinned snapshot slot as the device sees it, for a kernel that writes the counters out itself; null: the copy path takes over
static StepCounters* snapshot_slot_for_kernel(phys_world* w) {
    StepCounters* slot = snapshot_acquire(w);
    StepCounters* d_slot = nullptr;
    if (slot && hipHostGetDevicePointer((void**)&d_slot, slot, 0) != hipSuccess) {
        d_slot = nullptr;
        (void)hipGetLastError();  // an answer handled here (the copy path takes over), not an error to leave behind
    }
    return d_slot;
}

// Colouring + colour-major renumbering, entirely device-driven: the plan's round launches (surplus launches exit at
// once), one finish launch that completes whatever is left, then histogram / offsets / place. No host check, except on the
// Probe path. A snapshot of the counters goes to pinned memory asynchronously; later steps use it only as a HINT for launch sizes.
void launch_coloring(phys_world* w, const ColorPlan& plan, bool cluster) {
    const uint64_t n = w->n;
    if (n == 0) return;
    hipStream_t s = w->stream;
    bool snapshot_done = false;
    if (plan.path == ColorPath::Small) {
        // one workgroup does the whole stage, snapshot of the counters included
        StepCounters* d_slot = snapshot_slot_for_kernel(w);
        { PHYS_PROF(w, PHYS_STAGE_COLOR);
          hipLaunchKernelGGL(k_color_small, dim3(1), dim3(kColorThreads), 0, s, w->max_manifolds, w->man_a.p, w->man_b.p,
                             w->man_color.p, w->man_prio.p, w->color_state.p, (uint64_t)n, w->row_src.p, w->counters.p, d_slot); }
        if (d_slot) { snapshot_commit(w, plan.full); snapshot_done = true; }
    } else {
        uint32_t rounds = plan.rounds;
        for (uint32_t r = 0; r < rounds; ++r) launch_color_round(w, r, plan.round_blocks);
        if (plan.path == ColorPath::Probe) {
            // first step after phys_set_bodies: nothing is known about the scene yet, so this one step asks the
            // device (a single-workgroup finish / tail over millions of manifolds would take seconds)
            for (int guard = 0; guard < 4096; ++guard) {
                for (uint32_t k = 0; k < 8; ++k) launch_color_round(w, rounds++, plan.round_blocks);
                (void)hipMemcpyAsync(w->h_counters, w->counters.p, sizeof(StepCounters), hipMemcpyDeviceToHost, s);
                (void)hipStreamSynchronize(s);
                if (w->prof.on) w->prof.collect(s);
                if (w->h_counters->n_uncolored == 0 || w->h_counters->overflow) break;
            }
        }
        { PHYS_PROF(w, PHYS_STAGE_COLOR);
          hipLaunchKernelGGL(k_color_finish, dim3(1), dim3(kColorThreads), 0, s, rounds, w->max_manifolds, w->man_a.p, w->man_b.p,
                             w->man_color.p, w->man_prio.p, w->color_state.p, (uint64_t)n, w->unc_list.p, w->counters.p); }
        // the snapshot of the counters (launch-size hints of later updates) is written by the last kernel of the sort itself,
        // into a host-mapped slot: the copy engine's turn between two kernels of the stream cost 4.4 us per update
        StepCounters* d_snap = plan.path == ColorPath::Known ? snapshot_slot_for_kernel(w) : nullptr;
        if (cluster) {
            launch_cluster_sort(w, plan, d_snap);  // rows by (owner cluster, colour); counts the colours too
        } else {
            const uint32_t nb = plan.sort_blocks;
            { PHYS_PROF(w, PHYS_STAGE_ROWS);
              hipLaunchKernelGGL(k_color_hist, dim3(nb), dim3(1024), 0, s, w->max_manifolds, w->man_color.p, w->color_block_hist.p, nb, w->counters.p); }
            { PHYS_PROF(w, PHYS_STAGE_ROWS);
              hipLaunchKernelGGL(k_color_offsets, dim3(1), dim3(1024), 0, s, w->color_block_hist.p, nb, w->counters.p); }
            // (n_colors and the per-colour counts are final here: k_color_place below may copy the counters out)
            { PHYS_PROF(w, PHYS_STAGE_ROWS);
              hipLaunchKernelGGL(k_color_place, dim3(nb), dim3(1024), 0, s, w->max_manifolds, w->man_color.p, w->color_block_hist.p, nb,
                                 w->row_src.p, w->counters.p, d_snap); }
        }
        if (d_snap) { snapshot_commit(w, plan.full); snapshot_done = true; }
    }
    // the new manifolds of this update go into the colour table in k_rows_build (launch_solver, which takes the plan's stamp
    // and `rebuild`): one launch less
    if (plan.rebuild) {  // start from an empty table: every manifold of this update is inserted
        PHYS_PROF(w, PHYS_STAGE_ROWS);
        (void)hipMemsetAsync(w->ctab.p, 0xFF, ((size_t)w->ctab_mask + 1) * 16, s);
    }
    w->ctab_valid = true;
    w->color_epoch++;
    if (plan.path == ColorPath::Probe) {
        // ... and adopts the exact counters as the first hint (the solver launches right after are planned from them)
        (void)hipMemcpyAsync(w->h_counters, w->counters.p, sizeof(StepCounters), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        if (!w->h_counters->overflow) hint_adopt(w->hint, *w->h_counters, plan.full, /*exact=*/true);
    } else if (!snapshot_done) {
        snapshot_counters_async(w, plan.full);
    }
}

}  // namespace phys
