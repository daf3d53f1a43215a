// broadphase.hip — AABB broad phase for gfx950. No reference counterpart; the
// result is specified as the SET of pairs (i < j) whose fattened AABBs overlap (include/spec/collide.h).
//
// Pipeline per step (all sizes live on the device; nothing returns to the host):
//   1. k_cell_assign   body -> cell of a uniform grid whose cell edge is the largest AABB extent of the
//                      step (x1.001), cell -> bucket by 3-D Morton interleave of the low cell bits
//                      (neighbouring cells = neighbouring buckets = neighbouring memory), count per bucket.
//   2. exclusive scan  bucket counts -> bucket starts (scan.hip: one launch up to 32768 buckets, else 3 small kernels).
//   3. k_scatter       bodies grouped by bucket: ids + a bucket-ordered COPY of the AABBs (24 B each), so
//                      the pair kernel streams candidates instead of gathering them.
//   4. k_find_pairs    one lane per body (bucket order), half shell of 14 cells; overlap test; hits are
//                      compacted with wavefront ballot + popcount into a per-wave LDS stage and flushed
//                      with one global atomic per flush (not per hit) and coalesced 8-byte stores.
// The emission order is arbitrary; nothing downstream depends on it (DESIGN.md "determinism").
// Algorithmic bytes: 24 N (each AABB read once) + 8 P (each pair written once).
#include <algorithm>
#include <vector>

#include <cstdlib>

#include "kernels.hpp"

namespace phys {

constexpr uint32_t kInvalid = 0xFFFFFFFFu;

// (bucket of a cell: kernels.hpp grid_bucket - brick-major, per-axis sizes)
__device__ __forceinline__ float grid_inv_cell(const StepCounters* ctr) {
    const float ext = __uint_as_float(ctr->max_extent_bits);
    const float cell = ext > 0.0f ? ext * 1.001f : 1.0f;
    return 1.0f / cell;
}

__global__ __launch_bounds__(256) void k_cell_assign(uint32_t n, const float* __restrict__ aabb,
                                                     const uint32_t* __restrict__ shape,
                                                     const StepCounters* __restrict__ ctr, GridShape axis_mask,
                                                     uint32_t* __restrict__ bucket_of, uint32_t* __restrict__ rank,
                                                     uint32_t* __restrict__ bucket_count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (shape[i] == PHYS_SPEC_SHAPE_NONE) { bucket_of[i] = kInvalid; return; }
    const float inv_cell = grid_inv_cell(ctr);
    const v3 lo = ld3(aabb, 2 * i), hi = ld3(aabb, 2 * i + 1);
    const int cx = grid_cell_coord(0.5f * (lo.x + hi.x), inv_cell);
    const int cy = grid_cell_coord(0.5f * (lo.y + hi.y), inv_cell);
    const int cz = grid_cell_coord(0.5f * (lo.z + hi.z), inv_cell);
    const uint32_t bk = grid_bucket(cx, cy, cz, axis_mask);
    bucket_of[i] = bk;
    rank[i] = atomicAdd(&bucket_count[bk], 1u);  // order inside a bucket is irrelevant downstream
}

// ---- group bodies by bucket -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scatter(uint32_t n, const float* __restrict__ aabb,
                                                 const uint32_t* __restrict__ bucket_of,
                                                 const uint32_t* __restrict__ rank,
                                                 const uint32_t* __restrict__ bucket_start,
                                                 uint32_t* __restrict__ sorted_ids, float* __restrict__ sorted_box) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t bk = bucket_of[i];
    if (bk == kInvalid) return;
    const uint32_t s = bucket_start[bk] + rank[i];
    sorted_ids[s] = i;
    st3(sorted_box, 2 * s, ld3(aabb, 2 * i));
    st3(sorted_box, 2 * s + 1, ld3(aabb, 2 * i + 1));
}

// ---- candidate pairs ------------------------------------------------------------------------------
constexpr int kStagePerWave = 512;  // pairs staged in LDS per wave before a flush (4 KiB)

struct PairStage {
    uint32_t* lds;    // this wave's LDS segment: kStagePerWave pairs (2 u32 each)
    uint32_t count;   // wave-uniform
};

__device__ __forceinline__ void stage_flush(PairStage& st, uint32_t* __restrict__ pairs, uint64_t max_pairs,
                                            StepCounters* __restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    if (st.count == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctr->n_pairs, st.count);
    base = (uint32_t)__shfl((int)base, 0, 64);
    if ((uint64_t)base + st.count > max_pairs) {
        if (lane == 0) flag_overflow(ctr, kOvfPairs);
    }
    for (uint32_t k = lane; k < st.count; k += 64) {
        const uint64_t dst = (uint64_t)base + k;
        if (dst < max_pairs) {
            const uint2 pr = reinterpret_cast<const uint2*>(st.lds)[k];
            reinterpret_cast<uint2*>(pairs)[dst] = pr;
        }
    }
    st.count = 0;
}

// every lane of the wave calls this together (hit may be false); compacts the hits into the LDS stage
template <int kStageCap = kStagePerWave>
__device__ __forceinline__ void stage_push(PairStage& st, bool hit, uint32_t a, uint32_t b,
                                           uint32_t* __restrict__ pairs, uint64_t max_pairs,
                                           StepCounters* __restrict__ ctr) {
    const unsigned long long mask = __ballot(hit);
    if (mask == 0ull) return;
    const uint32_t hits = (uint32_t)__popcll(mask);
    if (st.count + hits > (uint32_t)kStageCap) stage_flush(st, pairs, max_pairs, ctr);
    if (hit) reinterpret_cast<uint2*>(st.lds)[st.count + lane_rank(mask)] = make_uint2(a, b);
    st.count += hits;
}

// kLanesPerBody lanes share one body: each takes every kLanesPerBody-th cell of the half shell, so the
// dependent chain per lane (bucket range -> candidate ids/boxes) is a quarter as long and four times as
// many loads are in flight. The ranges of a lane's cells are fetched up front (independent loads).
template <int kLanesPerBody>
__global__ __launch_bounds__(kPairThreads) void k_find_pairs(const uint32_t* __restrict__ bucket_start,
                                                             uint32_t table_size, GridShape axis_mask,
                                                             const uint32_t* __restrict__ sorted_ids,
                                                             const float* __restrict__ sorted_box,
                                                             uint32_t* __restrict__ pairs, uint64_t max_pairs,
                                                             StepCounters* __restrict__ ctr) {
    constexpr int kCellsPerLane = (14 + kLanesPerBody - 1) / kLanesPerBody;
    __shared__ uint32_t stage[(kPairThreads / 64) * kStagePerWave * 2];
    PairStage st;
    st.lds = stage + (threadIdx.x >> 6) * kStagePerWave * 2;
    st.count = 0;
    const uint32_t n_active = bucket_start[table_size];
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t s = g / kLanesPerBody;
    const uint32_t sub = g % kLanesPerBody;
    const bool live = s < n_active;
    const float inv_cell = grid_inv_cell(ctr);
    uint32_t i = 0;
    aabb_t bi;
    bi.lo = v3_make(0, 0, 0); bi.hi = v3_make(0, 0, 0);
    int cx = 0, cy = 0, cz = 0;
    if (live) {
        i = sorted_ids[s];
        bi.lo = ld3(sorted_box, 2 * s);
        bi.hi = ld3(sorted_box, 2 * s + 1);
        cx = grid_cell_coord(0.5f * (bi.lo.x + bi.hi.x), inv_cell);
        cy = grid_cell_coord(0.5f * (bi.lo.y + bi.hi.y), inv_cell);
        cz = grid_cell_coord(0.5f * (bi.lo.z + bi.hi.z), inv_cell);
    }
    // half shell: own cell (c = 0) + the 13 cells with (dz, dy, dx) > (0, 0, 0) lexicographically
    uint32_t t0[kCellsPerLane], t1[kCellsPerLane];
#pragma unroll
    for (int k = 0; k < kCellsPerLane; ++k) {
        const int c = (int)sub + kLanesPerBody * k;
        int dx, dy, dz;
        if (c == 0) { dx = 0; dy = 0; dz = 0; }
        else if (c == 1) { dx = 1; dy = 0; dz = 0; }
        else if (c < 5) { dx = c - 3; dy = 1; dz = 0; }
        else { dx = (c - 5) % 3 - 1; dy = ((c - 5) / 3) % 3 - 1; dz = 1; }
        t0[k] = 0; t1[k] = 0;
        if (live && c < 14) {
            const uint32_t bk = grid_bucket(cx + dx, cy + dy, cz + dz, axis_mask);
            t0[k] = bucket_start[bk];
            t1[k] = bucket_start[bk + 1];
        }
    }
#pragma unroll
    for (int k = 0; k < kCellsPerLane; ++k) {
        const bool own_cell = (sub == 0 && k == 0);
        uint32_t t = t0[k];
        const uint32_t t_end = t1[k];
        while (__any(t < t_end)) {
            bool hit = false;
            uint32_t j = 0;
            if (t < t_end) {
                j = sorted_ids[t];
                aabb_t bj;
                bj.lo = ld3(sorted_box, 2 * t);
                bj.hi = ld3(sorted_box, 2 * t + 1);
                // own cell: each unordered pair once by id order. Other cells: a bucket can alias a far cell
                // (wrap-around); such a candidate fails the overlap test, and the 14 buckets are distinct.
                hit = aabb_overlap(bi, bj) && (!own_cell || i < j);
                ++t;
            }
            stage_push(st, hit, i < j ? i : j, i < j ? j : i, pairs, max_pairs, ctr);
        }
    }
    stage_flush(st, pairs, max_pairs, ctr);
}

// ---- candidate pairs, one workgroup per BRICK of the grid ------------------------------------------------------------
// k_find_pairs above walks, per body, 14 cells x (bucket range -> candidates) as dependent loads through the L2: 204 us
// for 1M bodies (C4), 2 % of the HBM rate, and 6.2x the compulsory traffic, because the lanes of a workgroup sit on
// eight XCDs' worth of unrelated cells and every L2 ends up fetching most of the boxes. Here a workgroup owns one brick
// of 4 x 4 x 4 cells - 64 consecutive buckets, so its bodies are ONE run of the bucket-sorted arrays - and first stages
// what its bodies can meet: the 6 x 6 x 5 cells of the brick and its half-shell halo (x, y from -1 to 4, z from 0 to 4):
//   1. 180 lanes fetch the bucket ranges of the region's cells (one round trip), a scan turns the counts into LDS offsets;
//   2. all lanes copy the region's {box, id} records into LDS (second round trip; 28 bytes each, every record of the
//      region exactly once per brick = 2.8 records staged per body);
//   3. four lanes per own body walk the body's 14 cells in LDS; hits go through the same ballot / popcount stage.
// The chain a body waits for is two global round trips per BRICK instead of 28 per body. A region with more records
// than the stage holds (a scene far denser than its grid) is walked in global memory as before - same code path, the
// cell table then holds positions in the sorted arrays instead of in LDS. Bricks are dealt so that the workgroups of one
// XCD (blockIdx % 8) cover one contiguous eighth of the table: a box is fetched into ONE L2, and again only by the
// neighbour XCDs along the eighth's two faces. Same pair SET as k_find_pairs (each pair found by the body whose cell
// comes first in the half-shell order; own-cell pairs by id order).
constexpr int kBrickLanesPerBody = 4;
// pairs staged per wave: 256 (2 KiB) where a body has many pairs (C5: 12 - at 128 the flushes, one same-address atomic
// each, made its search 0.244 ms instead of 0.069), 128 where it has few (C4: 1.3; a seventh workgroup per CU fits)

// WHAT THE PAIR SEARCH WAITS FOR IS THE PAIR COUNTER. Same-address atomics serialise chip-wide at ~88 per microsecond, and
// every flush of a stage is one: the one-lane-per-body kernel flushes once per wave (1M bodies: 15.6k flushes = 180 of
// its 204 us), a first version of this kernel with one brick per workgroup flushed 80k times (814 us). So the workgroups
// are PERSISTENT - a few per CU, each working through many bricks - and keep their hits in LDS across bricks; between two
// bricks, once half the stage is full, the four waves' hits go out behind ONE atomic (C4: ~2.5k atomics for 1.3M pairs).
// A wave whose own part fills up inside a brick (dense scenes) still flushes on its own.
template <int kBrickStagePerWave>
__device__ __forceinline__ void workgroup_flush(PairStage& st, uint32_t* s_cnt, uint32_t* s_base, uint32_t* __restrict__ pairs,
                                                uint64_t max_pairs, StepCounters* __restrict__ ctr, bool force) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) s_cnt[wave] = st.count;
    __syncthreads();
    const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const bool go = total != 0u && (force || total >= (uint32_t)(2 * kBrickStagePerWave));  // workgroup-uniform
    if (go && threadIdx.x == 0) {
        const uint32_t base = atomicAdd(&ctr->n_pairs, total);
        if ((uint64_t)base + total > max_pairs) flag_overflow(ctr, kOvfPairs);
        *s_base = base;
    }
    __syncthreads();
    if (go) {
        uint32_t off = *s_base;
        for (uint32_t k = 0; k < wave; ++k) off += s_cnt[k];
        for (uint32_t k = lane; k < st.count; k += 64) {
            const uint64_t dst = (uint64_t)off + k;
            if (dst < max_pairs) reinterpret_cast<uint2*>(pairs)[dst] = reinterpret_cast<const uint2*>(st.lds)[k];
        }
        st.count = 0;
    }
    __syncthreads();  // s_cnt / s_base are reused by the next flush
}

// `cap` records fit the dynamic LDS of this launch (sized by the host from the largest region of an EARLIER update:
// StepCounters::max_region; a brick with more than that walks global memory - slower, same pairs).
template <int kBrickStagePerWave>
__global__ __launch_bounds__(kPairThreads, 7) void k_find_pairs_brick(const uint32_t* __restrict__ bucket_start, uint32_t n_bricks,
                                                                   GridShape g, const uint32_t* __restrict__ sorted_ids,
                                                                   const float* __restrict__ sorted_box,
                                                                   uint32_t* __restrict__ pairs, uint64_t max_pairs,
                                                                   StepCounters* __restrict__ ctr, uint32_t cap) {
    __shared__ uint32_t stage[(kPairThreads / 64) * kBrickStagePerWave * 2];
    __shared__ uint32_t s_gstart[kRegCells];    // position of a region cell's first record in the sorted arrays
    __shared__ uint32_t s_off[kRegCells + 1];   // exclusive scan of the cells' record counts (position in s_rec)
    extern __shared__ float s_rec[];            // cap x {lo xyz, hi xyz, id}: odd stride, distinct banks for neighbouring records
    __shared__ uint32_t s_wsum[4], s_cnt[4], s_base;
    PairStage st;
    st.lds = stage + (threadIdx.x >> 6) * kBrickStagePerWave * 2;
    st.count = 0;
    const float inv_cell = grid_inv_cell(ctr);
    const uint32_t sub = threadIdx.x % kBrickLanesPerBody;
    // XCD-aware deal (a label, never relied on for correctness): workgroups with equal blockIdx % 8 share an L2 and take
    // ONE contiguous eighth of the table between them, brick by brick in turn (neighbouring bricks are in flight together
    // on one L2). (Measured and dropped: eighths of equal BODY count taken from the bucket scan - no faster on any scene.)
    uint32_t first = blockIdx.x, last = n_bricks, step = gridDim.x;
    if (gridDim.x >= 8u && n_bricks >= 8u) {
        const uint32_t label = blockIdx.x & 7u, per = n_bricks >> 3;  // n_bricks is a power of two
        step = (gridDim.x - label + 7u) >> 3;
        first = label * per + (blockIdx.x >> 3);
        last = (label + 1u) * per;
    }
    // The bucket ranges of a brick (its own run, and the 180 cells of its region, one per lane) are asked for ONE BRICK
    // AHEAD: what a brick then waits for is a single round trip - its records - instead of three in a row (ranges ->
    // records, and its own bodies behind the run's bounds), with only a few workgroups per CU to hide them.
    uint32_t nx_begin = 0, nx_end = 0, nx_c0 = 0, nx_cnt = 0;
    auto ask = [&](uint32_t brick) {
        nx_begin = bucket_start[brick * 64u];
        nx_end = bucket_start[brick * 64u + 64u];
        nx_c0 = 0; nx_cnt = 0;
        if (threadIdx.x < (uint32_t)kRegCells) {
            const uint32_t bx = brick & ((1u << g.sx) - 1u), by = (brick >> g.sx) & ((1u << g.sy) - 1u), bz = brick >> (g.sx + g.sy);
            const uint32_t r = threadIdx.x;
            const uint32_t rx = r % kRegX, ry = (r / kRegX) % kRegY, rz = r / (kRegX * kRegY);
            const uint32_t bk = grid_bucket_masked(((bx << 2) + rx - 1u) & g.mx, ((by << 2) + ry - 1u) & g.my, ((bz << 2) + rz) & g.mz, g);
            nx_c0 = bucket_start[bk];
            nx_cnt = bucket_start[bk + 1] - nx_c0;
        }
    };
    if (first < last) ask(first);
    uint32_t seen_max = 0;
    for (uint32_t brick = first; brick < last; brick += step) {
        const uint32_t own_begin = nx_begin, own_end = nx_end, my_c0 = nx_c0, my_cnt = nx_cnt;
        if (brick + step < last) ask(brick + step);
        if (own_begin == own_end) continue;  // workgroup-uniform: an empty brick
        constexpr uint32_t kBodiesPerTrip = kPairThreads / kBrickLanesPerBody;
        const uint32_t n_own = own_end - own_begin;
        // the first trip's own bodies: asked for now, needed behind the staging
        uint32_t i0 = 0;
        aabb_t b0;
        b0.lo = v3_make(0, 0, 0); b0.hi = v3_make(0, 0, 0);
        if (threadIdx.x / kBrickLanesPerBody < n_own) {
            const uint32_t sidx = own_begin + threadIdx.x / kBrickLanesPerBody;
            i0 = sorted_ids[sidx];
            b0.lo = ld3(sorted_box, 2 * sidx);
            b0.hi = ld3(sorted_box, 2 * sidx + 1);
        }
        // 1. bucket ranges of the region's cells (asked for one brick ago), scanned
        {
            const uint32_t cnt = my_cnt;
            if (threadIdx.x < (uint32_t)kRegCells) s_gstart[threadIdx.x] = my_c0;
            const uint32_t inc = wave_inclusive_scan(cnt);
            if ((threadIdx.x & 63u) == 63u) s_wsum[threadIdx.x >> 6] = inc;
            __syncthreads();
            uint32_t base = 0;
            for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) base += s_wsum[k];
            if (threadIdx.x < (uint32_t)kRegCells) s_off[threadIdx.x] = base + inc - cnt;
            if (threadIdx.x == (uint32_t)kRegCells - 1u) s_off[kRegCells] = base + inc;
            __syncthreads();
        }
        const uint32_t total = s_off[kRegCells];
        const bool staged = total <= cap;
        seen_max = total > seen_max ? total : seen_max;
        // 2. the region's records into LDS
        if (staged) {
            for (uint32_t q = threadIdx.x; q < total; q += kPairThreads) {
                uint32_t lo = 0, hi = kRegCells;  // the cell r with s_off[r] <= q < s_off[r + 1]
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_off[mid] <= q) lo = mid; else hi = mid;
                }
                const uint32_t t = s_gstart[lo] + (q - s_off[lo]);
                const v3 blo = ld3(sorted_box, 2 * t), bhi = ld3(sorted_box, 2 * t + 1);
                float* rec = s_rec + 7u * q;
                rec[0] = blo.x; rec[1] = blo.y; rec[2] = blo.z; rec[3] = bhi.x; rec[4] = bhi.y; rec[5] = bhi.z;
                rec[6] = __uint_as_float(sorted_ids[t]);
            }
            __syncthreads();
        }
        // 3. the brick's own bodies, four lanes each, against the 14 cells of their half shell.
        // (Measured and dropped, same pairs: (own body, candidate) tests enumerated per own CELL, sixteen cells per wave, both
        // sides from LDS - 2.6x slower, three dependent LDS trips per cell and nothing to overlap them; a lane walking its
        // four cells as one run, moving on the moment a cell is exhausted - fewer passes, 5-15 % slower: the cursor costs
        // more than the passes it saves.)
        for (uint32_t base = 0; base < n_own; base += kBodiesPerTrip) {
            const uint32_t jo = base + threadIdx.x / kBrickLanesPerBody;
            const bool live = jo < n_own;
            uint32_t i = i0;
            aabb_t bi = b0;
            if (base != 0u && live) {
                const uint32_t sidx = own_begin + jo;
                i = sorted_ids[sidx];
                bi.lo = ld3(sorted_box, 2 * sidx);
                bi.hi = ld3(sorted_box, 2 * sidx + 1);
            }
            // the brick's origin is a multiple of four cells on every axis: the low two bits are the place in the brick
            const uint32_t lx = (uint32_t)grid_cell_coord(0.5f * (bi.lo.x + bi.hi.x), inv_cell) & 3u;
            const uint32_t ly = (uint32_t)grid_cell_coord(0.5f * (bi.lo.y + bi.hi.y), inv_cell) & 3u;
            const uint32_t lz = (uint32_t)grid_cell_coord(0.5f * (bi.lo.z + bi.hi.z), inv_cell) & 3u;
#pragma unroll
            for (int k = 0; k < (14 + kBrickLanesPerBody - 1) / kBrickLanesPerBody; ++k) {
                const int c = (int)sub + kBrickLanesPerBody * k;
                int dx, dy, dz;  // half shell: own cell (c = 0) + the 13 cells with (dz, dy, dx) > (0, 0, 0) lexicographically
                if (c == 0) { dx = 0; dy = 0; dz = 0; }
                else if (c == 1) { dx = 1; dy = 0; dz = 0; }
                else if (c < 5) { dx = c - 3; dy = 1; dz = 0; }
                else { dx = (c - 5) % 3 - 1; dy = ((c - 5) / 3) % 3 - 1; dz = 1; }
                uint32_t t = 0, t_end = 0;
                if (live && c < 14) {
                    const uint32_t rid = ((lz + (uint32_t)dz) * kRegY + (ly + (uint32_t)(dy + 1))) * kRegX + (lx + (uint32_t)(dx + 1));
                    t = staged ? s_off[rid] : s_gstart[rid];
                    t_end = t + (s_off[rid + 1] - s_off[rid]);
                }
                const bool own_cell = c == 0;
                while (__any(t < t_end)) {
                    bool hit = false;
                    uint32_t j = 0;
                    if (t < t_end) {
                        aabb_t bj;
                        if (staged) {
                            const float* rec = s_rec + 7u * t;
                            bj.lo = v3_make(rec[0], rec[1], rec[2]);
                            bj.hi = v3_make(rec[3], rec[4], rec[5]);
                            j = __float_as_uint(rec[6]);
                        } else {
                            j = sorted_ids[t];
                            bj.lo = ld3(sorted_box, 2 * t);
                            bj.hi = ld3(sorted_box, 2 * t + 1);
                        }
                        // own cell: each unordered pair once by id order. Other cells: a bucket can alias a far cell
                        // (wrap-around); such a candidate fails the overlap test, and the 14 buckets are distinct.
                        hit = aabb_overlap(bi, bj) && (!own_cell || i < j);
                        ++t;
                    }
                    stage_push<kBrickStagePerWave>(st, hit, i < j ? i : j, i < j ? j : i, pairs, max_pairs, ctr);
                }
            }
        }
        // the region tables and records are rewritten by the next brick: everybody is done with them behind the flush's barriers
        workgroup_flush<kBrickStagePerWave>(st, s_cnt, &s_base, pairs, max_pairs, ctr, /*force=*/false);
    }
    workgroup_flush<kBrickStagePerWave>(st, s_cnt, &s_base, pairs, max_pairs, ctr, /*force=*/true);
    // the largest region met: what a later update sizes its stage by (only a raise is an atomic)
    if (threadIdx.x == 0 && seen_max > ctr->max_region) atomicMax(&ctr->max_region, seen_max);
}

// ---- slot grid (small scenes) ------------------------------------------------------------------------
// With a table of >= 2 buckets per body almost every bucket holds 0-2 bodies: instead of counting, scanning and
// scattering (three dependent launches) a body simply takes one of EIGHT slots of its bucket (id + box) and the
// pair kernel reads the neighbours' slots directly. A body that finds the eight slots taken goes to a short overflow list that every body also tests against, so the pair SET is the same as with the
// sorted grid whatever the occupancy; only the speed depends on it.
constexpr uint32_t kSlotsPerBucket = 8;

__global__ __launch_bounds__(256) void k_cell_insert(uint32_t n, const float* __restrict__ aabb,
                                                     const uint32_t* __restrict__ shape, StepCounters* __restrict__ ctr,
                                                     GridShape axis_mask, uint32_t* __restrict__ rank,
                                                     uint32_t* __restrict__ bucket_count, uint32_t* __restrict__ slot_ids,
                                                     float* __restrict__ slot_box, uint32_t* __restrict__ ovf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || shape[i] == PHYS_SPEC_SHAPE_NONE) return;
    const float inv_cell = grid_inv_cell(ctr);
    const v3 lo = ld3(aabb, 2 * i), hi = ld3(aabb, 2 * i + 1);
    const int cx = grid_cell_coord(0.5f * (lo.x + hi.x), inv_cell);
    const int cy = grid_cell_coord(0.5f * (lo.y + hi.y), inv_cell);
    const int cz = grid_cell_coord(0.5f * (lo.z + hi.z), inv_cell);
    const uint32_t bk = grid_bucket(cx, cy, cz, axis_mask);
    const uint32_t r = atomicAdd(&bucket_count[bk], 1u);  // which slot is irrelevant downstream
    rank[i] = r;
    if (r < kSlotsPerBucket) {
        // id AND box go into the slot: the pair kernel then needs no gather by id behind the slot record
        slot_ids[kSlotsPerBucket * bk + r] = i;
        st3(slot_box, 2 * (kSlotsPerBucket * bk + r), lo);
        st3(slot_box, 2 * (kSlotsPerBucket * bk + r) + 1, hi);
    } else {
        ovf[atomicAdd(&ctr->n_grid_ovf, 1u)] = i;
    }
}

template <int kLanesPerBody>
__global__ __launch_bounds__(kPairThreads) void k_find_pairs_slots(uint32_t n, const float* __restrict__ aabb,
                                                                   const uint32_t* __restrict__ shape,
                                                                   const uint32_t* __restrict__ rank,
                                                                   const uint32_t* __restrict__ bucket_count,
                                                                   const uint32_t* __restrict__ slot_ids,
                                                                   const float* __restrict__ slot_box,
                                                                   const uint32_t* __restrict__ ovf, GridShape axis_mask,
                                                                   uint32_t* __restrict__ pairs, uint64_t max_pairs,
                                                                   StepCounters* __restrict__ ctr) {
    constexpr int kCellsPerLane = (14 + kLanesPerBody - 1) / kLanesPerBody;
    __shared__ uint32_t stage[(kPairThreads / 64) * kStagePerWave * 2];
    PairStage st;
    st.lds = stage + (threadIdx.x >> 6) * kStagePerWave * 2;
    st.count = 0;
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = g / kLanesPerBody;
    const uint32_t sub = g % kLanesPerBody;
    const bool live = i < n && shape[i] != PHYS_SPEC_SHAPE_NONE;
    const float inv_cell = grid_inv_cell(ctr);
    aabb_t bi;
    bi.lo = v3_make(0, 0, 0); bi.hi = v3_make(0, 0, 0);
    int cx = 0, cy = 0, cz = 0;
    bool in_overflow = false;
    if (live) {
        bi.lo = ld3(aabb, 2 * i);
        bi.hi = ld3(aabb, 2 * i + 1);
        cx = grid_cell_coord(0.5f * (bi.lo.x + bi.hi.x), inv_cell);
        cy = grid_cell_coord(0.5f * (bi.lo.y + bi.hi.y), inv_cell);
        cz = grid_cell_coord(0.5f * (bi.lo.z + bi.hi.z), inv_cell);
        in_overflow = rank[i] >= kSlotsPerBucket;
    }
    // half shell: own cell (c = 0) + the 13 cells with (dz, dy, dx) > (0, 0, 0) lexicographically. A body of the
    // overflow list looks at nobody's slots: its pairs come from the others' (and its own) pass over that list.
    uint32_t cnt[kCellsPerLane], first[kCellsPerLane];
#pragma unroll
    for (int k = 0; k < kCellsPerLane; ++k) {
        const int c = (int)sub + kLanesPerBody * k;
        int dx, dy, dz;
        if (c == 0) { dx = 0; dy = 0; dz = 0; }
        else if (c == 1) { dx = 1; dy = 0; dz = 0; }
        else if (c < 5) { dx = c - 3; dy = 1; dz = 0; }
        else { dx = (c - 5) % 3 - 1; dy = ((c - 5) / 3) % 3 - 1; dz = 1; }
        cnt[k] = 0; first[k] = 0;
        if (live && !in_overflow && c < 14) {
            const uint32_t bk = grid_bucket(cx + dx, cy + dy, cz + dz, axis_mask);
            const uint32_t have = bucket_count[bk];
            first[k] = kSlotsPerBucket * bk;
            cnt[k] = have < kSlotsPerBucket ? have : kSlotsPerBucket;
        }
    }
#pragma unroll
    for (int k = 0; k < kCellsPerLane; ++k) {
        const bool own_cell = (sub == 0 && k == 0);
        for (uint32_t r = 0; __any(r < cnt[k]); ++r) {
            bool hit = false;
            uint32_t j = 0;
            if (r < cnt[k]) {
                const uint32_t slot = first[k] + r;
                j = slot_ids[slot];
                aabb_t bj;
                bj.lo = ld3(slot_box, 2 * slot);
                bj.hi = ld3(slot_box, 2 * slot + 1);
                // own cell: each unordered pair once by id order. Other cells: a bucket can alias a far cell
                // (wrap-around); such a candidate fails the overlap test, and the 14 buckets are distinct.
                hit = aabb_overlap(bi, bj) && (!own_cell || i < j);
            }
            stage_push(st, hit, i < j ? i : j, i < j ? j : i, pairs, max_pairs, ctr);
        }
    }
    // everybody against the overflow list: a slotted body takes every overflow body it overlaps, two overflow
    // bodies meet once (by id order)
    const uint32_t n_ovf = ctr->n_grid_ovf;
    for (uint32_t o = 0; o < n_ovf; ++o) {
        const uint32_t j = ovf[o];
        bool hit = false;
        if (live && sub == 0 && j != i && (!in_overflow || i < j)) {
            aabb_t bj;
            bj.lo = ld3(aabb, 2 * j);
            bj.hi = ld3(aabb, 2 * j + 1);
            hit = aabb_overlap(bi, bj);
        }
        stage_push(st, hit, i < j ? i : j, i < j ? j : i, pairs, max_pairs, ctr);
    }
    stage_flush(st, pairs, max_pairs, ctr);
}

// ---- host side -------------------------------------------------------------------------------------
int32_t collision_alloc(phys_world* w) {
    const uint64_t n = w->n;
    const CollisionSizes sz = collision_sizes(w->cfg, n, debug_switches());
    w->max_pairs = sz.max_pairs;
    w->max_manifolds = sz.max_manifolds;
    if (!sz.ok) {
        set_error("max_pairs / max_manifolds exceed u32 indexing");
        return PHYS_ERR_INVALID_ARG;
    }
    const uint32_t T = w->grid_table_size;  // grid_plan (phys_set_bodies), before this
    {
        // one allocation, zeroed by one memset per step: [bucket counts | colouring state | StepCounters]
        const size_t b_bytes = sz.bucket_bytes, c_bytes = sz.color_bytes;
        w->step_zero.free();  // a block of exactly this size
        PHYS_HIP_TRY(w->step_zero.resize(b_bytes + c_bytes + sz.counter_bytes));
        w->bucket_count.point_at(reinterpret_cast<uint32_t*>(w->step_zero.p), T);
        w->color_state.point_at(reinterpret_cast<unsigned long long*>(w->step_zero.p + b_bytes), c_bytes / 8);
        w->counters.point_at(reinterpret_cast<StepCounters*>(w->step_zero.p + b_bytes + c_bytes), 1);
        w->step_zero_reset_bytes = b_bytes + c_bytes + kCountersStepResetBytes;
        w->step_zero_full_bytes = b_bytes + c_bytes + kCountersExtentResetBytes;  // not the sticky word behind it
        PHYS_HIP_TRY(hipMemsetAsync(w->step_zero.p, 0, b_bytes + c_bytes + sz.counter_bytes, w->stream));  // sticky word too
    }
    PHYS_HIP_TRY(w->bucket_of.resize(n));
    PHYS_HIP_TRY(w->bucket_cursor.resize(n));  // rank of each body inside its bucket
    PHYS_HIP_TRY(w->bucket_start.resize((size_t)T + 1));
    PHYS_HIP_TRY(w->scan_block_sums.resize(2 * std::max<size_t>(scan_scratch_words(T) + 1, 64)));  // sums | buckets in use
    PHYS_HIP_TRY(w->sorted_ids.resize(n));
    PHYS_HIP_TRY(w->slot_ids.resize((size_t)kSlotsPerBucket * T));
    PHYS_HIP_TRY(w->slot_box.resize((size_t)6 * kSlotsPerBucket * T));
    PHYS_HIP_TRY(w->grid_ovf.resize(n));
    w->sorted_grid_valid = false;
    PHYS_HIP_TRY(w->sorted_box.resize(6 * n));
    PHYS_HIP_TRY(w->pairs.resize(2 * w->max_pairs));
    if (!(w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY)) {
        const uint64_t M = w->max_manifolds;
        PHYS_HIP_TRY(w->man_a.resize(M)); PHYS_HIP_TRY(w->man_b.resize(M));
        PHYS_HIP_TRY(w->man_color.resize(M));
        PHYS_HIP_TRY(w->man_geo.resize(kManifoldFloats * M));
        w->warm = sz.warm;
        if (w->warm) {
            PHYS_HIP_TRY(w->man_geo_prev.resize(kManifoldFloats * M));
            PHYS_HIP_TRY(w->man_imp.resize(kImpulseFloats * M));
            PHYS_HIP_TRY(w->man_imp_prev.resize(kImpulseFloats * M));
            PHYS_HIP_TRY(w->man_prev.resize(4));  // only its address is used: "warm starting is on" (the index itself is in man_geo)
        }
        PHYS_HIP_TRY(w->man_prio.resize(M));
        PHYS_HIP_TRY(w->row_src.resize(M));
        PHYS_HIP_TRY(w->unc_list.resize(2 * M));
        PHYS_HIP_TRY(w->ctab.resize(2 * sz.ctab_slots));
        w->ctab_mask = (uint32_t)(sz.ctab_slots - 1);
        w->ctab_valid = false;
        w->color_epoch = 0;
        PHYS_HIP_TRY(w->color_block_hist.resize((size_t)kMaxColors * 512));
        w->row_all.free();  // exactly kRowPlanes planes of M rows
        PHYS_HIP_TRY(w->row_all.resize(row_plane_floats(kRowPlanes, M)));
        w->flow_vel.free();  // null unless allocated below: per-colour launches only
        if (sz.flow_buffers) {
            PHYS_HIP_TRY(w->flow_vel.resize(kBodyGranuleBytes / sizeof(float) * n));
            // tags of an earlier scene must never look like tags of this one
            PHYS_HIP_TRY(hipMemsetAsync(w->flow_vel.p, 0, kBodyGranuleBytes * n, w->stream));
            PHYS_HIP_TRY(hipMemsetAsync(w->row_all.p + row_plane_floats(kRowPlaneAcc, M), 0, row_plane_floats(kRowAccPlanes, M) * sizeof(float), w->stream));
            // PHYS_DEBUG_FLOW_EPOCH=<n>: start the tag epoch near its wrap (test of the 16-bit epoch reset)
            w->flow_epoch = debug_switches().flow_epoch;
        }
    }
    return PHYS_OK;
}

void zero_step_state(phys_world* w, bool including_extent) {
    PHYS_PROF(w, PHYS_STAGE_MISC);
    (void)hipMemsetAsync(w->step_zero.p, 0, including_extent ? w->step_zero_full_bytes : w->step_zero_reset_bytes, w->stream);
}

// bucket_start / sorted_ids / sorted_box from the current AABBs; the bucket counts must be zero
void build_sorted_grid(phys_world* w) {
    const uint32_t n = (uint32_t)w->n;
    const uint32_t T = w->grid_table_size;
    const GridShape axis_mask = w->grid_shape;
    hipStream_t s = w->stream;
    const dim3 gb((n + 255) / 256), tb(256);
    w->sorted_grid_valid = true;
    { PHYS_PROF(w, PHYS_STAGE_GRID); hipLaunchKernelGGL(k_cell_assign, gb, tb, 0, s, n, w->aabb.p, w->shape.p, w->counters.p, axis_mask, w->bucket_of.p,
                       w->bucket_cursor.p, w->bucket_count.p); }
    // (the second half of the scratch: buckets in use per block of the three-launch scan, summed into n_used_buckets)
    launch_exclusive_scan(w, w->bucket_count.p, T, w->bucket_start.p, false, w->scan_block_sums.p,
                          w->scan_block_sums.p + w->scan_block_sums.n / 2, w->counters.p, PHYS_STAGE_GRID);
    { PHYS_PROF(w, PHYS_STAGE_GRID); hipLaunchKernelGGL(k_scatter, gb, tb, 0, s, n, w->aabb.p, w->bucket_of.p, w->bucket_cursor.p, w->bucket_start.p,
                       w->sorted_ids.p, w->sorted_box.p); }
}

void launch_broadphase(phys_world* w, const PairPlan& plan) {
    const uint32_t n = (uint32_t)w->n;
    if (n == 0) return;
    w->grid_valid = true;
    const uint32_t T = w->grid_table_size;
    const GridShape axis_mask = w->grid_shape;
    hipStream_t s = w->stream;
    const dim3 wgs(plan.wgs), tb(kPairThreads);
    if (plan.kernel == PairKernel::Slots) {
        // slot grid: two launches for the whole broad phase
        w->sorted_grid_valid = false;
        { PHYS_PROF(w, PHYS_STAGE_GRID); hipLaunchKernelGGL(k_cell_insert, dim3((n + 255) / 256), dim3(256), 0, s, n, w->aabb.p, w->shape.p, w->counters.p,
                           axis_mask, w->bucket_cursor.p, w->bucket_count.p, w->slot_ids.p, w->slot_box.p, w->grid_ovf.p); }
        PHYS_PROF(w, PHYS_STAGE_PAIRS);
        hipLaunchKernelGGL((k_find_pairs_slots<4>), wgs, tb, 0, s,
                           n, w->aabb.p, w->shape.p, w->bucket_cursor.p, w->bucket_count.p, w->slot_ids.p, w->slot_box.p, w->grid_ovf.p, axis_mask,
                           w->pairs.p, w->max_pairs, w->counters.p);
        return;
    }
    build_sorted_grid(w);
    if (plan.kernel == PairKernel::Brick128 || plan.kernel == PairKernel::Brick256) {
        static bool attr_set[64] = {};
        (void)allow_dynamic_lds(attr_set, w->device, {reinterpret_cast<const void*>(&k_find_pairs_brick<128>),
                                                      reinterpret_cast<const void*>(&k_find_pairs_brick<256>)}, 150 * 1024);
        const uint32_t n_bricks = T >> 6;
        PHYS_PROF(w, PHYS_STAGE_PAIRS);
        if (plan.kernel == PairKernel::Brick128)
            hipLaunchKernelGGL(k_find_pairs_brick<128>, wgs, tb, plan.lds, s, w->bucket_start.p, n_bricks, axis_mask,
                               w->sorted_ids.p, w->sorted_box.p, w->pairs.p, w->max_pairs, w->counters.p, plan.cap);
        else
            hipLaunchKernelGGL(k_find_pairs_brick<256>, wgs, tb, plan.lds, s, w->bucket_start.p, n_bricks, axis_mask,
                               w->sorted_ids.p, w->sorted_box.p, w->pairs.p, w->max_pairs, w->counters.p, plan.cap);
        return;
    }
    PHYS_PROF(w, PHYS_STAGE_PAIRS);
    if (plan.kernel == PairKernel::Lanes4)
        hipLaunchKernelGGL((k_find_pairs<4>), wgs, tb, 0, s,
                           w->bucket_start.p, T, axis_mask, w->sorted_ids.p, w->sorted_box.p, w->pairs.p, w->max_pairs, w->counters.p);
    else
        hipLaunchKernelGGL((k_find_pairs<1>), wgs, tb, 0, s,
                           w->bucket_start.p, T, axis_mask, w->sorted_ids.p, w->sorted_box.p, w->pairs.p, w->max_pairs, w->counters.p);
}

// phys_broadphase read-out: pairs sorted by (i, j). The sort is a host-side convenience of this
// read-out call; the per-step pipeline never sorts (nothing downstream depends on pair order).
int32_t sorted_pairs_to_host(phys_world* w, uint32_t* pairs_out, uint64_t cap, uint64_t* n_pairs) {
    PHYS_TRY(fetch_counters(w));
    if (w->h_counters->overflow & kOvfPairs) {
        set_error("pair capacity exceeded: raise phys_config.max_pairs");
        return PHYS_ERR_CAPACITY;
    }
    const uint64_t m = w->h_counters->n_pairs;
    *n_pairs = m;
    if (!pairs_out || m == 0) return PHYS_OK;
    std::vector<uint32_t> raw(2 * m);
    PHYS_HIP_TRY(hipMemcpy(raw.data(), w->pairs.p, 8 * m, hipMemcpyDeviceToHost));
    sort_pairs(raw.data(), m, pairs_out, cap);
    return PHYS_OK;
}

}  // namespace phys
