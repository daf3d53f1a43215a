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
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.hpp"

namespace phys {

namespace {

constexpr int kStThreads = 256;
constexpr uint32_t kStMaxDim = 1024;    // cells per axis: three 10-bit cell coordinates pack into one word
constexpr uint32_t kStLargeCells = 64;  // a static covering more cells than this is tested by every body instead

// cell of coordinate x along one axis, clamped to [0, dim - 1] (NaN: cell 0). Host and device run these operations
// alike (no contraction: -ffp-contract=off), and the result is monotone in x.
__host__ __device__ __forceinline__ uint32_t st_cell(float x, float org, float inv, uint32_t dim) {
    float t = floorf((x - org) * inv);
    if (!(t >= 0.0f)) t = 0.0f;
    const float top = (float)(dim - 1u);
    t = t > top ? top : t;
    return (uint32_t)t;
}

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

// Replaces the static set (arguments checked by the caller). Builds the records and the grid on the host.
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
    const float margin = w->cfg.contact_margin;
    std::vector<float> geo(16 * n, 0.0f), rc(12 * n, 0.0f), box(8 * n, 0.0f);
    std::vector<float> lo(3 * n), hi(3 * n), edge(n);
    for (uint64_t k = 0; k < n; ++k) {
        quat q;
        if (rot) { q.i = rot[4 * k]; q.j = rot[4 * k + 1]; q.k = rot[4 * k + 2]; q.w = rot[4 * k + 3]; }
        else { q.i = 0.0f; q.j = 0.0f; q.k = 0.0f; q.w = 1.0f; }
        const v3 c = v3_make(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
        const v3 h = v3_make(he[3 * k], he[3 * k + 1], he[3 * k + 2]);
        const uint32_t id = PHYS_STATIC_ID_BIT | (uint32_t)k;
        const float g[16] = {c.x, c.y, c.z, 0.0f, q.i, q.j, q.k, q.w, h.x, h.y, h.z, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        std::memcpy(&geo[16 * k], g, sizeof(g));
        std::memcpy(&geo[16 * k + 3], &shape[k], 4);
        std::memcpy(&rc[12 * k], g, 48);
        std::memcpy(&rc[12 * k + 3], &shape[k], 4);
        std::memcpy(&rc[12 * k + 11], &id, 4);
        if (shape[k] == PHYS_SHAPE_CAPSULE) w->static_capsules = true;
        // fattened by the contact margin like the bodies' boxes (a capsule's from its segment and radius, collide.h): a pair
        // is a candidate wherever body-body pairs would be
        const aabb_t b = body_aabb(c, q, h, shape[k], margin);
        lo[3 * k] = b.lo.x; lo[3 * k + 1] = b.lo.y; lo[3 * k + 2] = b.lo.z;
        hi[3 * k] = b.hi.x; hi[3 * k + 1] = b.hi.y; hi[3 * k + 2] = b.hi.z;
        edge[k] = std::max(b.hi.x - b.lo.x, std::max(b.hi.y - b.lo.y, b.hi.z - b.lo.z));
    }
    // cell edge: the median extent (a few huge statics do not coarsen the grid; they go to the large list)
    std::vector<float> sorted_edge(edge);
    std::nth_element(sorted_edge.begin(), sorted_edge.begin() + n / 2, sorted_edge.end());
    double cell = sorted_edge[n / 2];
    if (!(cell > 0.0) || !std::isfinite(cell)) cell = 1.0;
    auto covered = [&](uint64_t k, double cl) {  // cells of static k at edge cl (an upper bound: two partial cells per axis)
        double cells = 1.0;
        for (int a = 0; a < 3; ++a) cells *= std::floor((double)(hi[3 * k + a] - lo[3 * k + a]) / cl) + 2.0;
        return cells;
    };
    std::vector<uint8_t> is_large(n, 0);
    std::vector<uint32_t> large;
    double blo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, bhi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    uint64_t n_small = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (covered(k, cell) > (double)kStLargeCells) { is_large[k] = 1; large.push_back((uint32_t)k); continue; }
        ++n_small;
        for (int a = 0; a < 3; ++a) { blo[a] = std::min(blo[a], (double)lo[3 * k + a]); bhi[a] = std::max(bhi[a], (double)hi[3 * k + a]); }
    }
    std::vector<uint32_t> cell_start(2, 0), cell_ids;
    uint32_t dim[3] = {0, 0, 0};
    float org[3] = {0.0f, 0.0f, 0.0f}, inv = 0.0f;
    if (n_small) {
        // at most kStMaxDim cells per axis and a few cells per small static in all: far-flung statics coarsen the grid
        const double max_cells = std::max<double>(4096.0, 8.0 * (double)n_small);
        for (int guard = 0; guard < 200; ++guard) {
            double total = 1.0;
            bool fits = true;
            for (int a = 0; a < 3; ++a) {
                const double d = std::floor((bhi[a] - blo[a]) / cell) + 1.0;
                if (d > (double)kStMaxDim) fits = false;
                total *= d;
            }
            if (fits && total <= max_cells) break;
            cell *= 1.25;
        }
        inv = (float)(1.0 / cell);
        for (int a = 0; a < 3; ++a) {
            org[a] = (float)blo[a];
            // the span at the float cell edge, +1 for rounding; clamped by st_cell anyway
            dim[a] = (uint32_t)std::min<double>(kStMaxDim, std::floor((bhi[a] - blo[a]) * (double)inv) + 2.0);
        }
        const uint64_t cells = (uint64_t)dim[0] * dim[1] * dim[2];
        std::vector<uint32_t> cnt(cells + 1, 0), range(6 * n, 0);
        for (uint64_t k = 0; k < n; ++k) {
            if (is_large[k]) continue;
            uint32_t* r = &range[6 * k];
            for (int a = 0; a < 3; ++a) {
                r[a] = st_cell(lo[3 * k + a], org[a], inv, dim[a]);
                r[3 + a] = st_cell(hi[3 * k + a], org[a], inv, dim[a]);
            }
            const uint32_t p = r[0] | (r[1] << 10) | (r[2] << 20);
            std::memcpy(&box[8 * k + 3], &p, 4);
            for (uint32_t z = r[2]; z <= r[5]; ++z)
                for (uint32_t y = r[1]; y <= r[4]; ++y)
                    for (uint32_t x = r[0]; x <= r[3]; ++x) cnt[(z * dim[1] + y) * dim[0] + x]++;
        }
        cell_start.assign(cells + 1, 0);
        for (uint64_t c = 0; c < cells; ++c) cell_start[c + 1] = cell_start[c] + cnt[c];
        cell_ids.assign(cell_start[cells] ? cell_start[cells] : 1, 0);
        std::vector<uint32_t> cur(cell_start.begin(), cell_start.end() - 1);
        for (uint64_t k = 0; k < n; ++k) {  // ascending k: every cell's list is ascending
            if (is_large[k]) continue;
            const uint32_t* r = &range[6 * k];
            for (uint32_t z = r[2]; z <= r[5]; ++z)
                for (uint32_t y = r[1]; y <= r[4]; ++y)
                    for (uint32_t x = r[0]; x <= r[3]; ++x) cell_ids[cur[(z * dim[1] + y) * dim[0] + x]++] = (uint32_t)k;
        }
    }
    for (uint64_t k = 0; k < n; ++k) {
        box[8 * k] = lo[3 * k]; box[8 * k + 1] = lo[3 * k + 1]; box[8 * k + 2] = lo[3 * k + 2];
        box[8 * k + 4] = hi[3 * k]; box[8 * k + 5] = hi[3 * k + 1]; box[8 * k + 6] = hi[3 * k + 2];
    }
    if (cell_ids.empty()) cell_ids.assign(1, 0);
    if (large.empty()) large.assign(1, 0);  // (never read: st_n_large is 0)
    PHYS_HIP_TRY(w->st_geo.resize(16 * n));
    PHYS_HIP_TRY(w->st_rc.resize(12 * n));
    PHYS_HIP_TRY(w->st_box.resize(8 * n));
    PHYS_HIP_TRY(w->st_cell_start.resize(cell_start.size()));
    PHYS_HIP_TRY(w->st_cell_ids.resize(cell_ids.size()));
    PHYS_HIP_TRY(w->st_large.resize(large.size()));
    // every static starts with the default collision filter (phys_set_static_filters changes them)
    std::vector<uint32_t> filt(2 * n);
    for (uint64_t k = 0; k < n; ++k) { filt[2 * k] = kFilterDefaultWord; filt[2 * k + 1] = 0u; }
    PHYS_HIP_TRY(w->st_filt.resize(2 * n));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_filt.p, filt.data(), 4 * filt.size(), hipMemcpyHostToDevice, s));
    // ... and the default material {cfg.friction, 0} (phys_set_static_materials)
    std::vector<float> mat(2 * n, 0.0f);
    for (uint64_t k = 0; k < n; ++k) mat[2 * k] = w->cfg.friction;
    PHYS_HIP_TRY(w->st_mat.resize(2 * n));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_mat.p, mat.data(), 4 * mat.size(), hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_geo.p, geo.data(), 4 * geo.size(), hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_rc.p, rc.data(), 4 * rc.size(), hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_box.p, box.data(), 4 * box.size(), hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_cell_start.p, cell_start.data(), 4 * cell_start.size(), hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_cell_ids.p, cell_ids.data(), 4 * cell_ids.size(), hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipMemcpyAsync(w->st_large.p, large.data(), 4 * large.size(), hipMemcpyHostToDevice, s));
    PHYS_HIP_TRY(hipStreamSynchronize(s));  // staging vectors die here
    w->st_n_large = is_large.empty() ? 0u : (uint32_t)std::count(is_large.begin(), is_large.end(), (uint8_t)1);
    for (int a = 0; a < 3; ++a) { w->st_org[a] = org[a]; w->st_dim[a] = dim[a]; }
    w->st_inv_cell = inv;
    if (n_small == 0) w->st_dim[0] = w->st_dim[1] = w->st_dim[2] = 0;
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
