// ccd.hip — continuous collision: the bodies listed by phys_set_ccd_bodies are swept along this update's
// motion against the static colliders and the ground, and a body that would pass through one is advanced only to its time of
// impact. An add-on stage like the force fields, the liquids and the triggers: a kernel of its own between the solver and the
// position half, so no kernel of the narrow phase, the colouring, the row build or the solve changes. A world without a list
// launches nothing of this file, and its position half is the instance it always was.
//
//   k_ccd_sweep   one lane per list entry. The lane loads its body once (pose, shape, half extent, the velocity the solver left,
//                 its filter) and makes the mover (include/spec/ccd.h). The statics travel through LDS in tiles of kCcdTile: the
//                 48-byte ray-cast record, the fattened AABB and, in the filtered instance, the filter word. Per static the lane
//                 first rejects by its swept AABB against the static's box; the survivors get ccd_static_test (one bx_test).
//                 The winner is the least (t, id), so neither the tile order nor the launch shape decides a bit. It writes the
//                 entry's share of dt into ccd_frac[body], the entry's read-out record and its cumulative count.
//
// The arithmetic is include/spec/ccd.h's, called from here and compiled alone by tests/cpp/ccd_probe.cpp.
#include "../../include/spec/ccd.h"
#include "kernels.hpp"

namespace phys {

namespace {

static_assert(CCD_SHAPE_NONE == PHYS_SHAPE_NONE && CCD_MISS == PHYS_RAY_MISS && CCD_GROUND == PHYS_RAY_GROUND && CCD_STATIC_BIT == PHYS_STATIC_ID_BIT,
              "ids and shape codes mismatch");

constexpr int kCcdThreads = 64;     // one wave: a list is hundreds of bodies, so many small workgroups spread over the CUs
constexpr uint32_t kCcdTile = 64;   // statics per LDS tile: 64 x (48 + 32 + 8) bytes = 5.5 KB

struct CcdTile {
    float4 rec[3 * kCcdTile];  // {centre, shape} {rot} {half extent, id}
    float4 box[2 * kCcdTile];  // {lo, -} {hi, -}
    uint2 filt[kCcdTile];
};

template <bool FILT>
__global__ __launch_bounds__(kCcdThreads) void k_ccd_sweep(uint32_t n_list, const uint32_t* __restrict__ ids, float dt,
                                                           const float* __restrict__ pos, const float* __restrict__ rot,
                                                           const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                           const float* __restrict__ vel, const uint2* __restrict__ filt,
                                                           const float4* __restrict__ st_rec, const float4* __restrict__ st_box,
                                                           const uint2* __restrict__ st_filt, uint32_t n_static, int ground, float ground_y,
                                                           uint2 ground_filt, float* __restrict__ frac, uint32_t* __restrict__ hit,
                                                           uint32_t* __restrict__ count) {
    __shared__ CcdTile tile;
    const uint32_t e = blockIdx.x * kCcdThreads + threadIdx.x;
    const bool live = e < n_list;  // (no early return: the tiles have barriers)
    const uint32_t i = live ? ids[e] : 0u;
    quat q;
    q.i = q.j = q.k = 0.0f; q.w = 1.0f;
    v3 x = v3_make(0.0f, 0.0f, 0.0f), h = x, v = x;
    uint32_t sh = PHYS_SHAPE_NONE;
    uint2 bf = make_uint2(kFilterDefaultWord, 0u);
    if (live) {
        const float4 q4 = reinterpret_cast<const float4*>(rot)[i];
        q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
        x = ld3(pos, i); h = ld3(he, i); sh = shape[i];
        const float4 v4 = reinterpret_cast<const float4*>(vel)[2 * (size_t)i];
        v = v3_make(v4.x, v4.y, v4.z);
        if (FILT) bf = filt[i];
    }
    const ccd_mover mv = ccd_mover_make(sh, x, q, h, v, dt);
    ccd_result best = ccd_result_none();
    v3 lo, hi;
    ccd_swept_aabb(&mv, &lo, &hi);
    if (mv.swept && ground && (!FILT || ccd_filter_pass(bf.x, bf.y, ground_filt.x, ground_filt.y))) {
        float t = 0.0f;
        const int res = ccd_ground_test(&mv, ground_y, &t);
        ccd_take(&best, &mv, res, t, v3_make(0.0f, 1.0f, 0.0f), CCD_GROUND);
    }
    for (uint32_t t0 = 0; t0 < n_static; t0 += kCcdTile) {
        const uint32_t tn = min(kCcdTile, n_static - t0);
        __syncthreads();  // the previous tile has been read by everybody
        for (uint32_t k = threadIdx.x; k < 3u * tn; k += kCcdThreads) tile.rec[k] = st_rec[3 * (size_t)t0 + k];
        for (uint32_t k = threadIdx.x; k < 2u * tn; k += kCcdThreads) tile.box[k] = st_box[2 * (size_t)t0 + k];
        if (FILT)
            for (uint32_t k = threadIdx.x; k < tn; k += kCcdThreads) tile.filt[k] = st_filt[(size_t)t0 + k];
        __syncthreads();
        if (!mv.swept) continue;
        for (uint32_t k = 0; k < tn; ++k) {
            const float4 blo = tile.box[2 * k], bhi = tile.box[2 * k + 1];
            if (ccd_aabb_apart(lo, hi, v3_make(blo.x, blo.y, blo.z), v3_make(bhi.x, bhi.y, bhi.z))) continue;
            if (FILT) {
                const uint2 sf = tile.filt[k];
                if (!ccd_filter_pass(bf.x, bf.y, sf.x, sf.y)) continue;
            }
            const float4 a = tile.rec[3 * k], q4 = tile.rec[3 * k + 1], c = tile.rec[3 * k + 2];
            bx_target tg;
            tg.shape = __float_as_uint(a.w);
            tg.c = v3_make(a.x, a.y, a.z);
            tg.q.i = q4.x; tg.q.j = q4.y; tg.q.k = q4.z; tg.q.w = q4.w;
            tg.h = v3_make(c.x, c.y, c.z);
            float t = 0.0f;
            v3 n = v3_make(0.0f, 0.0f, 0.0f);
            const int res = ccd_static_test(&mv, &tg, &t, &n);
            ccd_take(&best, &mv, res, t, n, __float_as_uint(c.w));
        }
    }
    if (!live) return;
    ccd_finish(&best, &mv);
    frac[i] = best.frac;
    hit[e] = __float_as_uint(best.frac);
    hit[(size_t)n_list + e] = best.target;
    st3(reinterpret_cast<float*>(hit) + 2 * (size_t)n_list, e, best.n);
    if (best.target != CCD_MISS) count[e] = count[e] + 1u;
}

__global__ __launch_bounds__(256) void k_ccd_fill(uint32_t n, uint32_t* __restrict__ p, uint32_t value) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = value;
}

}  // namespace

int32_t ccd_set(phys_world* w, std::vector<uint32_t>&& ids) {
    hipStream_t s = w->stream;
    PHYS_HIP_TRY(hipStreamSynchronize(s));  // no update in flight reads the list replaced below
    const uint64_t n = ids.size();
    w->n_ccd = 0;  // (a failure below leaves a world without a list, not half of one)
    if (n == 0) {  // back to launching nothing
        w->ccd_ids.free(); w->ccd_frac.free(); w->ccd_hit.free(); w->ccd_count.free();
        return PHYS_OK;
    }
    PHYS_HIP_TRY(w->ccd_ids.resize(n));
    PHYS_HIP_TRY(w->ccd_frac.resize(w->n_owned));
    PHYS_HIP_TRY(w->ccd_hit.resize(5 * n));
    PHYS_HIP_TRY(w->ccd_count.resize(n));
    PHYS_HIP_TRY(hipMemcpyAsync(w->ccd_ids.p, ids.data(), 4 * n, hipMemcpyHostToDevice, s));
    const unsigned blocks = (unsigned)((w->n_owned + 255) / 256);
    constexpr uint32_t kOne = 0x3F800000u;  // 1.0f
    hipLaunchKernelGGL(k_ccd_fill, dim3(blocks), dim3(256), 0, s, (uint32_t)w->n_owned, reinterpret_cast<uint32_t*>(w->ccd_frac.p), kOne);
    // the read-out before the first sweep: frac 1, no target, no normal, count 0
    hipLaunchKernelGGL(k_ccd_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint32_t)n, w->ccd_hit.p, kOne);
    hipLaunchKernelGGL(k_ccd_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (uint32_t)n, w->ccd_hit.p + n, (uint32_t)PHYS_RAY_MISS);
    PHYS_HIP_TRY(hipMemsetAsync(w->ccd_hit.p + 2 * n, 0, 12 * n, s));
    PHYS_HIP_TRY(hipMemsetAsync(w->ccd_count.p, 0, 4 * n, s));
    PHYS_HIP_TRY(hipGetLastError());
    PHYS_HIP_TRY(hipStreamSynchronize(s));  // the staged ids die with the caller
    w->n_ccd = n;
    return PHYS_OK;
}

void launch_ccd_sweep(phys_world* w, float dt) {
    if (w->n_ccd == 0 || w->n_owned == 0) return;
    const unsigned blocks = (unsigned)((w->n_ccd + kCcdThreads - 1) / kCcdThreads);
    const bool ground = (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) != 0;
    const bool filt = w->body_filters_set || (w->n_static != 0 && w->static_filters_set) || (ground && w->ground_filter_set);
    PHYS_PROF(w, PHYS_STAGE_MISC);
    dispatch_bool(filt, [&](auto f) {
        hipLaunchKernelGGL((k_ccd_sweep<decltype(f)::value>), dim3(blocks), dim3(kCcdThreads), 0, w->stream, (uint32_t)w->n_ccd, w->ccd_ids.p, dt,
                           w->pos.p, w->rot.p, w->half_extent.p, w->shape.p, w->vel.p, reinterpret_cast<const uint2*>(w->filt.p),
                           reinterpret_cast<const float4*>(w->st_rc.p), reinterpret_cast<const float4*>(w->st_box.p),
                           reinterpret_cast<const uint2*>(w->st_filt.p), (uint32_t)w->n_static, ground ? 1 : 0, w->cfg.ground_height,
                           make_uint2(w->ground_filt, 0u), w->ccd_frac.p, w->ccd_hit.p, w->ccd_count.p);
    });
}

int32_t ccd_read(phys_world* w, float* d_frac, uint32_t* d_target, float* d_normal, uint32_t* d_count, bool to_host) {
    const uint64_t n = w->n_ccd;
    if (n == 0) return PHYS_OK;
    hipStream_t s = w->stream;
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (d_frac) PHYS_HIP_TRY(hipMemcpyAsync(d_frac, w->ccd_hit.p, 4 * n, kind, s));
    if (d_target) PHYS_HIP_TRY(hipMemcpyAsync(d_target, w->ccd_hit.p + n, 4 * n, kind, s));
    if (d_normal) PHYS_HIP_TRY(hipMemcpyAsync(d_normal, w->ccd_hit.p + 2 * n, 12 * n, kind, s));
    if (d_count) PHYS_HIP_TRY(hipMemcpyAsync(d_count, w->ccd_count.p, 4 * n, kind, s));
    return PHYS_OK;
}

}  // namespace phys
