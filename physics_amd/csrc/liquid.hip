// liquid.hip — liquids: oriented boxes whose +y face is a surface, and buoyancy and drag from the part of
// each body's shape below it. The twin of the force fields (fields.hip): evaluated by a kernel of their own in front of every
// update, behind the fields' kernel, so no kernel of the step changes - the step kernels' FORCES instances read and zero what
// this one adds. A world without liquids launches nothing of this file. The records (lq_record) are built on the host
// (setup.hpp liquid_records).
//
//   k_liquid_apply       one lane per owned body, a loop over the liquids: the records travel through LDS in tiles of 32 (every
//                        lane reads the same record: a broadcast). A lane loads its shape, half extent and rotation once, then
//                        walks the records: mask, AABB against its bounding radius, footprint, then its shape's rule. It loads
//                        its accumulators when the first liquid acts on it and stores them only then.
//   k_liquid_submersion  the read-out (phys_get_submersion): the same walk over the same functions, writing frac and the index
//                        of the lowest-index liquid that acts, and nothing to the accumulators.
//
// The arithmetic is include/spec/liquid.h's, called from here and compiled alone by tests/cpp/liquid_probe.cpp: ascending
// liquid index per body, no atomics, nothing that depends on another lane, so the bits do not depend on the launch shape.
#include "kernels.hpp"

namespace phys {

namespace {

constexpr int kLqThreads = 256;
constexpr uint32_t kLqTile = 32;  // liquids per LDS tile
static_assert(kLqTile * LQ_REC_VEC <= (uint32_t)kLqThreads, "one 16-byte vector per thread stages a tile");
static_assert(sizeof(lq_record) == 16 * LQ_REC_VEC, "records are whole 16-byte vectors");

// what a lane reads of its body, once. VEL: the set holds a nonzero drag; without it the 32-byte velocity record is not loaded.
// MASKED: the set has masks; without it no filter is loaded.
template <bool MASKED, bool VEL>
__device__ __forceinline__ lq_body lq_load_body(bool live, uint32_t i, const float* __restrict__ pos, const float* __restrict__ rot,
                                                const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                const float* __restrict__ vel, const uint2* __restrict__ filt) {
    const v3 zero = v3_make(0.0f, 0.0f, 0.0f);
    quat q;
    q.i = q.j = q.k = 0.0f; q.w = 1.0f;
    if (!live) return lq_body_make(PHYS_SHAPE_NONE, zero, q, zero, zero, zero, 0xFFFFu);
    const float4 q4 = reinterpret_cast<const float4*>(rot)[i];
    q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
    v3 v = zero, w = zero;
    if (VEL) {
        const BodyVel bv = ld_vel(vel, i);
        v = bv.v; w = bv.w;
    }
    return lq_body_make(shape[i], ld3(pos, i), q, ld3(he, i), v, w, MASKED ? (filt[i].x & 0xFFFFu) : 0xFFFFu);
}

template <bool MASKED, bool VEL>
__global__ __launch_bounds__(kLqThreads) void k_liquid_apply(uint32_t n, const float* __restrict__ pos, const float* __restrict__ rot,
                                                             const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                             const float* __restrict__ vel, const uint2* __restrict__ filt,
                                                             const lq_record* __restrict__ rec, uint32_t T, float* __restrict__ force,
                                                             float* __restrict__ torque) {
    __shared__ lq_record tile[kLqTile];
    const uint32_t i = blockIdx.x * kLqThreads + threadIdx.x;
    const bool live = i < n;  // (no early return: the tiles have barriers)
    const lq_body b = lq_load_body<MASKED, VEL>(live, i, pos, rot, he, shape, vel, filt);
    lq_sum sum;
    sum.F = sum.T = v3_make(0.0f, 0.0f, 0.0f);
    sum.acted = 0;
    const v3* acc_F = reinterpret_cast<const v3*>(force) + (live ? i : 0u);
    const v3* acc_T = reinterpret_cast<const v3*>(torque) + (live ? i : 0u);
    for (uint32_t t0 = 0; t0 < T; t0 += kLqTile) {
        const uint32_t tn = min(kLqTile, T - t0);
        tile_stage<LQ_REC_VEC>(reinterpret_cast<vol_f4*>(tile), reinterpret_cast<const vol_f4*>(rec), t0, tn);
        if (live) lq_accumulate(tile, tn, &b, MASKED ? 1 : 0, VEL ? 1 : 0, acc_F, acc_T, &sum);
    }
    if (sum.acted) {
        st3(force, i, sum.F);
        st3(torque, i, sum.T);
    }
}

template <bool MASKED>
__global__ __launch_bounds__(kLqThreads) void k_liquid_submersion(uint32_t n, const float* __restrict__ pos, const float* __restrict__ rot,
                                                                  const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                                  const uint2* __restrict__ filt, const lq_record* __restrict__ rec,
                                                                  uint32_t T, float* __restrict__ frac_out, uint32_t* __restrict__ liquid_out) {
    __shared__ lq_record tile[kLqTile];
    const uint32_t i = blockIdx.x * kLqThreads + threadIdx.x;
    const bool live = i < n;
    const lq_body b = lq_load_body<MASKED, false>(live, i, pos, rot, he, shape, nullptr, filt);
    float frac = 0.0f;
    uint32_t liquid = LQ_NONE;
    for (uint32_t t0 = 0; t0 < T; t0 += kLqTile) {
        const uint32_t tn = min(kLqTile, T - t0);
        tile_stage<LQ_REC_VEC>(reinterpret_cast<vol_f4*>(tile), reinterpret_cast<const vol_f4*>(rec), t0, tn);
        if (live) lq_submersion(tile, tn, t0, &b, MASKED ? 1 : 0, &frac, &liquid);
    }
    if (live) {
        if (frac_out) frac_out[i] = frac;
        if (liquid_out) liquid_out[i] = liquid;
    }
}

}  // namespace

int32_t liquids_set(phys_world* w, LiquidStaging&& staged) {
    const uint64_t n = staged.staged.size();
    w->n_liquids = 0;  // (a failure below leaves a world without liquids, not half a set)
    w->lq_masked = staged.masked; w->lq_drag = staged.drag;
    w->lq_host = std::move(staged.staged);
    if (n == 0) {  // back to launching nothing
        w->lq_rec.free();
        return PHYS_OK;
    }
    PHYS_TRY(upload_records(w, w->lq_rec, liquid_records(w->lq_host)));
    w->n_liquids = n;
    return PHYS_OK;
}

int32_t liquids_rebuild(phys_world* w) {
    if (w->n_liquids == 0) return PHYS_OK;
    w->lq_drag = liquids_have_drag(w->lq_host);
    return upload_records(w, w->lq_rec, liquid_records(w->lq_host));  // on the world's stream: behind the updates already enqueued
}

void launch_liquids(phys_world* w) {
    if (w->n_liquids == 0 || w->n_owned == 0) return;
    const unsigned blocks = (unsigned)((w->n_owned + kLqThreads - 1) / kLqThreads);
    PHYS_PROF(w, PHYS_STAGE_MISC);
    dispatch_bool(w->lq_masked, [&](auto masked) {
        dispatch_bool(w->lq_drag, [&](auto vel) {
            hipLaunchKernelGGL((k_liquid_apply<decltype(masked)::value, decltype(vel)::value>), dim3(blocks), dim3(kLqThreads), 0, w->stream,
                               (uint32_t)w->n_owned, w->pos.p, w->rot.p, w->half_extent.p, w->shape.p, w->vel.p,
                               reinterpret_cast<const uint2*>(w->filt.p), reinterpret_cast<const lq_record*>(w->lq_rec.p),
                               (uint32_t)w->n_liquids, w->force.p, w->torque.p);
        });
    });
    w->forces_dirty = true;
}

// frac and liquid index per owned body into device arrays (either may be null); a world without liquids answers 0 and LQ_NONE
void launch_submersion(phys_world* w, float* d_frac, uint32_t* d_liquid) {
    if (w->n_owned == 0) return;
    const unsigned blocks = (unsigned)((w->n_owned + kLqThreads - 1) / kLqThreads);
    PHYS_PROF(w, PHYS_STAGE_MISC);
    dispatch_bool(w->lq_masked && w->n_liquids != 0, [&](auto masked) {
        hipLaunchKernelGGL((k_liquid_submersion<decltype(masked)::value>), dim3(blocks), dim3(kLqThreads), 0, w->stream, (uint32_t)w->n_owned,
                           w->pos.p, w->rot.p, w->half_extent.p, w->shape.p, reinterpret_cast<const uint2*>(w->filt.p),
                           reinterpret_cast<const lq_record*>(w->lq_rec.p), (uint32_t)w->n_liquids, d_frac, d_liquid);
    });
}

}  // namespace phys
