// query.hip — overlap queries against the current poses (phys_overlap): for each query shape, every target whose closed
// shape it intersects, as ascending ids in CSR form. Read-only like the ray casts: it walks the query grid that raycast.hip
// builds (launch_query_grid, not grown) and writes only qr_* buffers of its own.
//
//   launch_query_grid   the ray casts' grid over the exact AABBs
//   k_ov_query<false>   one query per lane: the cells its padded AABB covers (or every body, when it covers more cells than
//                       there are bodies), every static, the ground; counts the targets it intersects
//   (host)              exclusive scan of the counts into offsets_out (u64); PHYS_ERR_CAPACITY when the total exceeds cap
//   k_ov_query<true>    the same walk again, writing each query's ids into its segment (bucket order)
//   k_ov_order          one wave per query: its segment ascending (copied when already ascending; bitonic sort in LDS up
//                       to kOvSortLds ids; rank by counting through LDS tiles above that)
// A bucket can hold a body's records of other cells and, when two of its cells hash to one bucket, two records of the same
// body. A record counts only in the first cell the body shares with the query (componentwise larger low corner of the two
// cell ranges) and only if no earlier record of its bucket names the same body: every id appears once.
#include <vector>

#include "shape_overlap.hpp"

namespace phys {

namespace {

constexpr int kOvThreads = 256;
constexpr int kOvSortThreads = 64;       // one wave per query segment
constexpr uint32_t kOvSortLds = 2048;    // ids sorted in LDS (8 KB per wave)
constexpr unsigned kOvMaxSortBlocks = 1u << 16;

// (the exact test qr_overlap, QShape and aabb_touch: shape_overlap.hpp, shared with the trigger volumes)
// FILL = false: count[q] = the number of targets query q intersects. FILL = true: their ids into ids[offsets[q] ...]
// FILT: phys_overlap_filtered (one QueryFilters argument, the pack `filt`): a target whose category misses the query's mask
// is skipped before its exact test; without it the pack is empty and the kernel is the one it was before filters
template <bool FILL, bool FILT, typename... Filt>
__global__ __launch_bounds__(kOvThreads) void k_ov_query(uint32_t nq, const uint32_t* __restrict__ qtype, const float* __restrict__ qpos,
                                                        const float* __restrict__ qrot, const float* __restrict__ qhe,
                                                        const uint32_t* __restrict__ ignore_body, const RcHeader* __restrict__ hdr,
                                                        uint32_t bits, const uint32_t* __restrict__ start, const float4* __restrict__ rec,
                                                        uint32_t n_bodies, const float* __restrict__ pos, const float* __restrict__ rot,
                                                        const float* __restrict__ he, const uint32_t* __restrict__ shape, int ground,
                                                        float ground_y, const float4* __restrict__ st_rec, uint32_t n_static,
                                                        uint32_t* __restrict__ count, const unsigned long long* __restrict__ offsets,
                                                        uint32_t* __restrict__ ids, Filt... filt) {
    static_assert(sizeof...(Filt) == (FILT ? 1u : 0u), "one QueryFilters argument exactly in the filtered instance");
    const uint32_t q = blockIdx.x * kOvThreads + threadIdx.x;
    if (q >= nq) return;
    QueryFilters qf{};
    if constexpr (FILT) qf = filter_arg(filt...);
    const uint32_t qm = FILT ? (uint32_t)qf.query_mask[q] : 0xFFFFu;
    uint32_t cnt = 0;
    const unsigned long long base = FILL ? offsets[q] : 0ull;
    const uint32_t room = FILL ? (uint32_t)(offsets[q + 1] - base) : 0u;
    auto emit = [&](uint32_t id) {
        if (FILL && cnt < room) ids[base + cnt] = id;
        ++cnt;
    };
    const uint32_t type = qtype[q];
    const v3 c = ld3(qpos, q), h = ld3(qhe, q);
    const float4 q4 = qrot ? reinterpret_cast<const float4*>(qrot)[q] : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    const uint32_t ign = ignore_body && ignore_body[q] < n_bodies ? ignore_body[q] : 0xFFFFFFFFu;
    const float sum = ((c.x + c.y) + (c.z + h.x)) + ((h.y + h.z) + ((q4.x + q4.y) + (q4.z + q4.w)));
    aabb_t qa;
    // an invalid query (other shape, non-finite pose, negative extent) intersects nothing
    if (isfinite(sum) && h.x >= 0.0f && h.y >= 0.0f && h.z >= 0.0f && rc_aabb_of(c, q4, h, type, &qa)) {
        const QShape Q = qs_make(type, c, q4, h);
        const RcGrid g = rc_grid(hdr);
        if (g.valid && n_bodies) {
            aabb_t qp;  // padded like the bodies' cells
            qp.lo = v3_make(qa.lo.x - g.pad, qa.lo.y - g.pad, qa.lo.z - g.pad);
            qp.hi = v3_make(qa.hi.x + g.pad, qa.hi.y + g.pad, qa.hi.z + g.pad);
            const int x0 = rc_coord(qp.lo.x, g.lox, g.inv, g.nx), x1 = rc_coord(qp.hi.x, g.lox, g.inv, g.nx);
            const int y0 = rc_coord(qp.lo.y, g.loy, g.inv, g.ny), y1 = rc_coord(qp.hi.y, g.loy, g.inv, g.ny);
            const int z0 = rc_coord(qp.lo.z, g.loz, g.inv, g.nz), z1 = rc_coord(qp.hi.z, g.loz, g.inv, g.nz);
            const unsigned long long cells = (unsigned long long)(x1 - x0 + 1) * (unsigned long long)(y1 - y0 + 1) *
                                             (unsigned long long)(z1 - z0 + 1);
            if (cells > n_bodies) {
                // more cells than bodies: every owned body directly, in ascending order
                for (uint32_t i = 0; i < n_bodies; ++i) {
                    aabb_t b;
                    if (i == ign || (FILT && (qf.body[i].x & qm) == 0u) || !rc_aabb(pos, rot, he, shape, i, &b) || !aabb_touch(b, qp)) continue;
                    if (qr_overlap(Q, qs_make(shape[i], ld3(pos, i), reinterpret_cast<const float4*>(rot)[i], ld3(he, i)))) emit(i);
                }
            } else {
                for (int z = z0; z <= z1; ++z)
                    for (int y = y0; y <= y1; ++y)
                        for (int x = x0; x <= x1; ++x) {
                            const uint32_t bk = rc_bucket(x, y, z, bits);
                            const uint32_t b0 = start[bk], b1 = start[bk + 1];
                            for (uint32_t k = b0; k < b1; ++k) {
                                const float4 r0 = rec[3 * (size_t)k], r1 = rec[3 * (size_t)k + 1], r2 = rec[3 * (size_t)k + 2];
                                const uint32_t id = __float_as_uint(r2.w);
                                const v3 bc = v3_make(r0.x, r0.y, r0.z), bh = v3_make(r2.x, r2.y, r2.z);
                                aabb_t b;
                                if (id == ign || (FILT && (qf.body[id].x & qm) == 0u) || !rc_aabb_of(bc, r1, bh, __float_as_uint(r0.w), &b) ||
                                    !aabb_touch(b, qp))
                                    continue;
                                // only in the first cell the body shares with the query: the record may be another cell's
                                const RcCells bcl = rc_body_cells(g, b);
                                if (x > bcl.x1 || y > bcl.y1 || z > bcl.z1 || max(bcl.x0, x0) != x || max(bcl.y0, y0) != y ||
                                    max(bcl.z0, z0) != z)
                                    continue;
                                // two cells of the body hashed to this bucket: only its first record here counts
                                bool dup = false;
                                for (uint32_t k2 = b0; k2 < k && !dup; ++k2) dup = __float_as_uint(rec[3 * (size_t)k2 + 2].w) == id;
                                if (dup) continue;
                                if (qr_overlap(Q, qs_make(__float_as_uint(r0.w), bc, r1, bh))) emit(id);
                            }
                        }
            }
        }
        // static colliders, ascending (ids PHYS_STATIC_ID_BIT | k above every body id)
        for (uint32_t k = 0; k < n_static; ++k) {
            if (FILT && (qf.st[k].x & qm) == 0u) continue;
            const float4 r0 = st_rec[3 * (size_t)k], r1 = st_rec[3 * (size_t)k + 1], r2 = st_rec[3 * (size_t)k + 2];
            const v3 bc = v3_make(r0.x, r0.y, r0.z), bh = v3_make(r2.x, r2.y, r2.z);
            aabb_t b;
            if (!rc_aabb_of(bc, r1, bh, __float_as_uint(r0.w), &b) || !aabb_touch(b, qa)) continue;
            if (qr_overlap(Q, qs_make(__float_as_uint(r0.w), bc, r1, bh))) emit(__float_as_uint(r2.w));
        }
        // the ground half-space y <= ground_y: the query's lowest point is its AABB's low y
        if (ground && (!FILT || (qf.ground & qm) != 0u) && qa.lo.y <= ground_y) emit(kRayGround);
    }
    if (!FILL) count[q] = cnt;
}

// each query's segment of tmp, ascending, into out (ids of a segment are distinct)
__global__ __launch_bounds__(kOvSortThreads) void k_ov_order(uint32_t nq, const unsigned long long* __restrict__ offsets,
                                                            const uint32_t* __restrict__ tmp, uint32_t* __restrict__ out) {
    __shared__ uint32_t s[kOvSortLds];
    const uint32_t lane = threadIdx.x;
    for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const unsigned long long b = offsets[q];
        const uint32_t len = (uint32_t)(offsets[q + 1] - b);
        bool desc = false;
        for (uint32_t j = lane; j + 1 < len; j += kOvSortThreads) desc = desc || tmp[b + j] > tmp[b + j + 1];
        if (!__any(desc)) {  // already ascending (every direct-path list, the single ids, the statics and the ground)
            for (uint32_t j = lane; j < len; j += kOvSortThreads) out[b + j] = tmp[b + j];
            continue;
        }
        if (len <= kOvSortLds) {
            uint32_t p = 1;
            while (p < len) p <<= 1;
            for (uint32_t j = lane; j < p; j += kOvSortThreads) s[j] = j < len ? tmp[b + j] : 0xFFFFFFFFu;
            __syncthreads();
            for (uint32_t k = 2; k <= p; k <<= 1)
                for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
                    for (uint32_t i = lane; i < p; i += kOvSortThreads) {
                        const uint32_t l = i ^ jj;
                        if (l > i) {
                            const uint32_t x = s[i], y = s[l];
                            if ((x > y) == ((i & k) == 0)) { s[i] = y; s[l] = x; }
                        }
                    }
                    __syncthreads();
                }
            for (uint32_t j = lane; j < len; j += kOvSortThreads) out[b + j] = s[j];
            __syncthreads();
        } else {
            // long lists: the rank of an id is the number of ids below it, counted through LDS tiles
            for (uint32_t j0 = 0; j0 < len; j0 += kOvSortThreads) {
                const uint32_t j = j0 + lane;
                const uint32_t x = j < len ? tmp[b + j] : 0u;
                uint32_t rank = 0;
                for (uint32_t t0 = 0; t0 < len; t0 += kOvSortLds) {
                    const uint32_t tl = min(kOvSortLds, len - t0);
                    for (uint32_t m = lane; m < tl; m += kOvSortThreads) s[m] = tmp[b + t0 + m];
                    __syncthreads();
                    for (uint32_t m = 0; m < tl; ++m) rank += s[m] < x ? 1u : 0u;
                    __syncthreads();
                }
                if (j < len && rank < len) out[b + rank] = x;
            }
        }
    }
}

}  // namespace

int32_t launch_overlap(phys_world* w, uint64_t n, const uint32_t* shape_type, const float* pos, const float* rot, const float* half_extent,
                       const uint32_t* ignore_body, uint64_t cap, uint64_t* offsets_out, uint32_t* ids_out, const uint16_t* query_mask) {
    hipStream_t s = w->stream;
    uint32_t bits = 12;
    int32_t rc = launch_query_grid(w, nullptr, nullptr, 0, &bits); if (rc) return rc;
    const RcHeader* hdr = reinterpret_cast<const RcHeader*>(w->rc_header.p);
    PHYS_HIP_TRY(w->qr_count.resize(n));
    PHYS_HIP_TRY(w->qr_off.resize(n + 1));
    const unsigned blocks = (unsigned)((n + kOvThreads - 1) / kOvThreads);
    const int ground = (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) ? 1 : 0;
    const uint32_t nb = (uint32_t)w->n_owned;
    const float4* st = reinterpret_cast<const float4*>(w->st_rc.p);
    const float4* rec = reinterpret_cast<const float4*>(w->rc_records.p);
    const QueryFilters qf = query_filters(w, query_mask);
    // (the filtered instances take `qf` as one more argument; the unfiltered ones are launched exactly as before filters)
#define PHYS_OV_LAUNCH(FILL, FILT, count, offsets, ids, ...)                                                                 \
    hipLaunchKernelGGL((k_ov_query<FILL, FILT>), dim3(blocks), dim3(kOvThreads), 0, s, (uint32_t)n, shape_type, pos, rot, half_extent, \
                       ignore_body, hdr, bits, (const uint32_t*)w->rc_start.p, rec, nb, w->pos.p, w->rot.p, w->half_extent.p,      \
                       w->shape.p, ground, w->cfg.ground_height, st, (uint32_t)w->n_static, count, offsets, ids, ##__VA_ARGS__)
    if (query_mask) PHYS_OV_LAUNCH(false, true, w->qr_count.p, (const unsigned long long*)nullptr, (uint32_t*)nullptr, qf);
    else PHYS_OV_LAUNCH(false, false, w->qr_count.p, (const unsigned long long*)nullptr, (uint32_t*)nullptr);
    PHYS_HIP_TRY(hipGetLastError());
    // exclusive scan on the host: the offsets are an output of the call anyway
    std::vector<uint32_t> cnt((size_t)n);
    PHYS_HIP_TRY(hipMemcpyAsync(cnt.data(), w->qr_count.p, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
    PHYS_HIP_TRY(hipStreamSynchronize(s));
    uint64_t run = 0;
    for (size_t i = 0; i < (size_t)n; ++i) { offsets_out[i] = run; run += cnt[i]; }
    offsets_out[n] = run;
    if (run > cap) {
        set_error("phys_overlap: the ids need offsets_out[n] slots, more than cap");
        return PHYS_ERR_CAPACITY;
    }
    if (run == 0) return PHYS_OK;
    PHYS_HIP_TRY(w->qr_ids.resize(2 * (size_t)run));
    uint32_t* tmp = w->qr_ids.p;
    uint32_t* out = w->qr_ids.p + run;
    PHYS_HIP_TRY(hipMemcpyAsync(w->qr_off.p, offsets_out, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, s));
    if (query_mask) PHYS_OV_LAUNCH(true, true, (uint32_t*)nullptr, (const unsigned long long*)w->qr_off.p, tmp, qf);
    else PHYS_OV_LAUNCH(true, false, (uint32_t*)nullptr, (const unsigned long long*)w->qr_off.p, tmp);
#undef PHYS_OV_LAUNCH
    hipLaunchKernelGGL(k_ov_order, dim3((unsigned)std::min<uint64_t>(n, kOvMaxSortBlocks)), dim3(kOvSortThreads), 0, s, (uint32_t)n,
                       (const unsigned long long*)w->qr_off.p, (const uint32_t*)tmp, out);
    PHYS_HIP_TRY(hipGetLastError());
    PHYS_HIP_TRY(hipMemcpyAsync(ids_out, out, 4 * (size_t)run, hipMemcpyDeviceToHost, s));
    PHYS_HIP_TRY(hipStreamSynchronize(s));
    return PHYS_OK;
}

}  // namespace phys
