// static.hip — static colliders (phys_set_static_bodies) for gfx950: the grid of the immovable
// shapes, built once on the host when the set is given, and the per-update pass that pairs bodies with them.
//
// Grid: uniform cells of the median static extent over the SMALL statics, stored as CSR (cell -> ascending static ids);
//   a static goes into every cell its fattened AABB covers. A static that would cover more than kStLargeCells cells (a
//   floor slab, a long wall) goes to a short LARGE list instead, which every body tests. Cell coordinates come from
//   st_cell on both sides - the host build and the device query run the same float operations - and st_cell is
//   monotone, so a point common to a body's box and a static's box lies in a cell of both cell ranges: the pair is found.
//   A pair seen in several cells is kept only in the first cell of the two ranges' intersection (each component the
//   larger of the two low corners), so it is counted once.
// Per update (bodies' fattened AABBs of this update, k_step_velocity_aabb), one lane per body slot, ghosts included:
//   k_static_count   pairs of each body; wave sums (shuffles) and one total per workgroup
//   k_static_scan    one workgroup: exclusive scan of the workgroup totals, the grand total into the counters
//   k_static_fill    the workgroup's offset + the lane's exclusive prefix inside its workgroup (wave shuffle scan, then
//                    the wave totals); each lane writes its body's pairs with ascending static ids
//   So the list is ordered by (body, static) and its bits never depend on timing: no atomic decides a position.
#include <algorithm>
#include <vector>

#include "kernels.hpp"

namespace phys {

namespace {

constexpr int kStThreads = 256;
// (kStMaxDim, kStLargeCells and st_cell, which the host build and st_visit both run: setup.hpp)

struct StaticGrid {
    const float4* __restrict__ box;  // 2 per static: {lo, packed first cell} {hi, -}
    const uint32_t* __restrict__ cell_start;
    const uint32_t* __restrict__ cell_ids;
    const uint32_t* __restrict__ large;
    uint32_t n_large;
    float ox, oy, oz, inv;
    uint32_t dx, dy, dz;  // dx == 0: no small statics
};

__device__ __forceinline__ bool st_overlap(float4 blo, float4 bhi, v3 lo, v3 hi) {
    return blo.x <= hi.x && lo.x <= bhi.x && blo.y <= hi.y && lo.y <= bhi.y && blo.z <= hi.z && lo.z <= bhi.z;
}

// f(k) once for every static k whose fattened AABB overlaps [lo, hi] (an inverted box - a body without a shape - meets
// none): the large list, then the cells of the box, z-major
template <class F>
__device__ __forceinline__ void st_visit(const StaticGrid& g, v3 lo, v3 hi, F&& f) {
    for (uint32_t j = 0; j < g.n_large; ++j) {
        const uint32_t k = g.large[j];
        if (st_overlap(g.box[2 * (size_t)k], g.box[2 * (size_t)k + 1], lo, hi)) f(k);
    }
    if (g.dx == 0u) return;
    const uint32_t x0 = st_cell(lo.x, g.ox, g.inv, g.dx), x1 = st_cell(hi.x, g.ox, g.inv, g.dx);
    const uint32_t y0 = st_cell(lo.y, g.oy, g.inv, g.dy), y1 = st_cell(hi.y, g.oy, g.inv, g.dy);
    const uint32_t z0 = st_cell(lo.z, g.oz, g.inv, g.dz), z1 = st_cell(hi.z, g.oz, g.inv, g.dz);
    for (uint32_t z = z0; z <= z1; ++z)
        for (uint32_t y = y0; y <= y1; ++y)
            for (uint32_t x = x0; x <= x1; ++x) {
                const uint32_t c = (z * g.dy + y) * g.dx + x;
                const uint32_t e1 = g.cell_start[c + 1];
                for (uint32_t e = g.cell_start[c]; e < e1; ++e) {
                    const uint32_t k = g.cell_ids[e];
                    const float4 blo = g.box[2 * (size_t)k], bhi = g.box[2 * (size_t)k + 1];
                    if (!st_overlap(blo, bhi, lo, hi)) continue;
                    const uint32_t p = __float_as_uint(blo.w);
                    const uint32_t fx = max(x0, p & 1023u), fy = max(y0, (p >> 10) & 1023u), fz = max(z0, p >> 20);
                    if (fx == x && fy == y && fz == z) f(k);
                }
            }
}

__global__ __launch_bounds__(kStThreads) void k_static_count(uint32_t n, const float* __restrict__ aabb, StaticGrid g,
                                                             uint32_t* __restrict__ count, uint32_t* __restrict__ block_total) {
    __shared__ uint32_t s_wave[kStThreads / 64];
    const uint32_t i = blockIdx.x * kStThreads + threadIdx.x;
    uint32_t c = 0;
    if (i < n) {
        st_visit(g, ld3(aabb, 2 * i), ld3(aabb, 2 * i + 1), [&](uint32_t) { ++c; });
        count[i] = c;
    }
    const uint32_t t = block_sum<kStThreads>(c, s_wave);
    if (threadIdx.x == 0) block_total[blockIdx.x] = t;
}

// one workgroup of 1024: exclusive scan of the nb workgroup totals in place; the grand total goes into the counters (and
// the overflow bit 0 when the pairs do not fit)
__global__ __launch_bounds__(1024) void k_static_scan(uint32_t* __restrict__ block_total, uint32_t nb, uint64_t cap,
                                                      StepCounters* __restrict__ ctr) {
    const uint32_t total = block_scan_in_place<1024>(block_total, nb);
    if (threadIdx.x == 0) {
        ctr->n_static_pairs = total;
        if ((uint64_t)total > cap) flag_overflow(ctr, kOvfPairs);
    }
}

__global__ __launch_bounds__(kStThreads) void k_static_fill(uint32_t n, const float* __restrict__ aabb, StaticGrid g,
                                                            const uint32_t* __restrict__ count, const uint32_t* __restrict__ block_off,
                                                            uint64_t cap, uint32_t* __restrict__ pairs) {
    __shared__ uint32_t s_wave[kStThreads / 64];
    const uint32_t i = blockIdx.x * kStThreads + threadIdx.x;
    const uint32_t c = i < n ? count[i] : 0u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // the lane's exclusive prefix: inside the wave by a shuffle scan, across the waves from their totals
    const uint32_t inc = wave_inclusive_scan(c);
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t off = block_off[blockIdx.x] + inc - c;
    for (uint32_t k = 0; k < wave; ++k) off += s_wave[k];
    if (c == 0u) return;  // (no barrier follows)
    const v3 lo = ld3(aabb, 2 * i), hi = ld3(aabb, 2 * i + 1);
    // ascending static ids: the e-th pair takes the least id above the previous one (a body meets a few statics)
    uint32_t prev = 0u;
    for (uint32_t e = 0; e < c; ++e) {
        uint32_t next = 0xFFFFFFFFu;
        st_visit(g, lo, hi, [&](uint32_t k) { if ((e == 0u || k > prev) && k < next) next = k; });
        const uint64_t at = (uint64_t)off + e;
        if (at < cap) reinterpret_cast<uint2*>(pairs)[at] = make_uint2(i, next);
        prev = next;
    }
}

StaticGrid static_grid(const phys_world* w) {
    StaticGrid g;
    g.box = reinterpret_cast<const float4*>(w->st_box.p);
    g.cell_start = w->st_cell_start.p;
    g.cell_ids = w->st_cell_ids.p;
    g.large = w->st_large.p;
    g.n_large = w->st_n_large;
    g.ox = w->st_org[0]; g.oy = w->st_org[1]; g.oz = w->st_org[2];
    g.inv = w->st_inv_cell;
    g.dx = w->st_dim[0]; g.dy = w->st_dim[1]; g.dz = w->st_dim[2];
    return g;
}

}  // namespace

// Replaces the static set (arguments checked by the caller). The records and the grid are built on the host (setup.hpp
// build_static_set); here they are uploaded and committed.
int32_t static_set(phys_world* w, uint64_t n, const float* pos, const float* rot, const uint32_t* shape, const float* he) {
    hipStream_t s = w->stream;
    PHYS_HIP_TRY(hipStreamSynchronize(s));  // no update in flight reads the buffers replaced below
    // no statics until every buffer of the new set is in place: a failed allocation or copy below leaves a world without
    // statics, never a count that runs past the records (k_rc_trace, k_narrowphase)
    w->n_static = 0;
    w->static_capsules = false;
    w->st_n_large = 0;
    w->st_dim[0] = w->st_dim[1] = w->st_dim[2] = 0;
    w->static_pairs_sized = false;
    if (n == 0) return PHYS_OK;
    const StaticSet set = build_static_set(n, pos, rot, shape, he, w->cfg.contact_margin, w->cfg.friction);
    w->static_capsules = set.capsules;
    PHYS_HIP_TRY(w->st_geo.resize(set.geo.size()));
    PHYS_HIP_TRY(w->st_rc.resize(set.rc.size()));
    PHYS_HIP_TRY(w->st_box.resize(set.box.size()));
    PHYS_HIP_TRY(w->st_cell_start.resize(set.cell_start.size()));
    PHYS_HIP_TRY(w->st_cell_ids.resize(set.cell_ids.size()));
    PHYS_HIP_TRY(w->st_large.resize(set.large.size()));
    auto up = [&](auto& dst, const auto& src) { return hipMemcpyAsync(dst.p, src.data(), 4 * src.size(), hipMemcpyHostToDevice, s); };
    PHYS_HIP_TRY(w->st_filt.resize(set.filt.size()));
    PHYS_HIP_TRY(up(w->st_filt, set.filt));
    PHYS_HIP_TRY(w->st_mat.resize(set.mat.size()));
    PHYS_HIP_TRY(up(w->st_mat, set.mat));
    PHYS_HIP_TRY(up(w->st_geo, set.geo));
    PHYS_HIP_TRY(up(w->st_rc, set.rc));
    PHYS_HIP_TRY(up(w->st_box, set.box));
    PHYS_HIP_TRY(up(w->st_cell_start, set.cell_start));
    PHYS_HIP_TRY(up(w->st_cell_ids, set.cell_ids));
    PHYS_HIP_TRY(up(w->st_large, set.large));
    PHYS_HIP_TRY(hipStreamSynchronize(s));  // the staged set dies here
    w->st_n_large = set.n_large;
    for (int a = 0; a < 3; ++a) { w->st_org[a] = set.org[a]; w->st_dim[a] = set.dim[a]; }
    w->st_inv_cell = set.inv_cell;
    w->n_static = n;  // committed last
    return PHYS_OK;
}

// the (body, static) pairs of this update into st_pairs, their count into the counters (k_narrowphase reads both)
int32_t launch_static_pairs(phys_world* w) {
    const uint64_t n = w->n;
    if (w->n_static == 0 || n == 0) return PHYS_OK;
    hipStream_t s = w->stream;
    const uint32_t nb = (uint32_t)((n + kStThreads - 1) / kStThreads);
    if (w->st_count.n < n || w->st_block.n < (size_t)nb + 1) {
        PHYS_HIP_TRY(hipStreamSynchronize(s));  // the buffers replaced below may still be read by queued updates
        PHYS_HIP_TRY(w->st_count.resize(n));
        PHYS_HIP_TRY(w->st_block.resize((size_t)nb + 1));
    }
    // Capacity. The first update after phys_set_static_bodies / phys_set_bodies MEASURES its pair count (the count and
    // the scan, then one read-back and a wait) and sizes the buffer at 1.5 times that; later updates only grow it from the
    // counts they report back (counter snapshots, phys_sync). An update whose pairs outgrow it raises overflow bit 0 once
    // and the next ones have room. Never less than four pairs per body slot.
    const bool measure = !w->static_pairs_sized;
    const StaticGrid g = static_grid(w);
    PHYS_PROF(w, PHYS_STAGE_PAIRS);
    hipLaunchKernelGGL(k_static_count, dim3(nb), dim3(kStThreads), 0, s, (uint32_t)n, w->aabb.p, g, w->st_count.p, w->st_block.p);
    if (measure) {
        hipLaunchKernelGGL(k_static_scan, dim3(1), dim3(1024), 0, s, w->st_block.p, nb, ~0ull, w->counters.p);
        uint32_t total = 0;
        PHYS_HIP_TRY(hipMemcpyAsync(&total, &w->counters.p->n_static_pairs, sizeof(total), hipMemcpyDeviceToHost, s));
        PHYS_HIP_TRY(hipStreamSynchronize(s));
        if (total > w->static_pairs_seen) w->static_pairs_seen = total;
        w->static_pairs_sized = true;
    }
    uint64_t want = std::max<uint64_t>(w->max_static_pairs, std::max<uint64_t>(4 * n, 1024));
    if (w->static_pairs_seen + w->static_pairs_seen / 2 > want) want = w->static_pairs_seen + w->static_pairs_seen / 2;
    want = std::min<uint64_t>(want, 0xFFFFFFF0ull);
    if (w->st_pairs.n < 2 * want) {
        PHYS_HIP_TRY(hipStreamSynchronize(s));
        PHYS_HIP_TRY(w->st_pairs.resize(2 * want));
    }
    w->max_static_pairs = want;
    if (!measure)
        hipLaunchKernelGGL(k_static_scan, dim3(1), dim3(1024), 0, s, w->st_block.p, nb, w->max_static_pairs, w->counters.p);
    hipLaunchKernelGGL(k_static_fill, dim3(nb), dim3(kStThreads), 0, s, (uint32_t)n, w->aabb.p, g, w->st_count.p, w->st_block.p,
                       w->max_static_pairs, w->st_pairs.p);
    return PHYS_OK;
}

// the (body, static) pairs of the last update that k_narrowphase may read, and the static geometry
void static_narrow_args(const phys_world* w, uint64_t* cap, const uint32_t** pairs, const float** geo) {
    const bool on = w->n_static != 0 && w->st_pairs.p;
    *cap = on ? w->max_static_pairs : 0;
    *pairs = on ? w->st_pairs.p : nullptr;
    *geo = on ? w->st_geo.p : nullptr;
}

}  // namespace phys
