// fields.hip — force fields: volumes that add to the force / torque accumulators of the bodies whose
// centre lies inside them. The writing twin of the trigger volumes (trigger.hip): evaluated by a kernel of their own in front
// of every update, so no kernel of the step changes - the step kernels' FORCES instances read and zero what this one adds. A
// world without fields launches nothing of this file. The records (ff_record) are built on the host (setup.hpp field_records).
//
//   k_field_apply  one lane per owned body, a loop over the fields: the records travel through LDS in tiles of 32 (every lane
//                  reads the same record: a broadcast), a lane rejects by mask, then by its centre against the record's AABB,
//                  then runs the exact point test and the law. A lane loads its accumulators when the first field acts on it
//                  and stores them only then: everyone else's stay the zeros they are.
//
// The arithmetic is include/spec/force_field.h's, called from here and compiled alone by tests/cpp/field_probe.cpp: ascending
// field index per body, no atomics, nothing that depends on another lane, so the bits do not depend on the launch shape.
#include "kernels.hpp"

namespace phys {

namespace {

constexpr int kFfThreads = 256;
constexpr uint32_t kFfTile = 32;  // fields per LDS tile
static_assert(kFfTile * FF_REC_VEC <= (uint32_t)kFfThreads, "one 16-byte vector per thread stages a tile");
static_assert(sizeof(ff_record) == 16 * FF_REC_VEC, "records are whole 16-byte vectors");

// MASKED: the set has masks - field k acts on body i only if (category[i] & mask[k]) != 0; without it no filter is loaded.
// VEL: the set holds a DRAG field; without it the 32-byte velocity record is not loaded (need_mass: an ACCEL field wants the
// mass, one float of that record).
template <bool MASKED, bool VEL>
__global__ __launch_bounds__(kFfThreads) void k_field_apply(uint32_t n, const float* __restrict__ pos, const float* __restrict__ vel,
                                                            const uint2* __restrict__ filt, const ff_record* __restrict__ rec, uint32_t T,
                                                            uint32_t need_mass, float* __restrict__ force, float* __restrict__ torque) {
    __shared__ ff_record tile[kFfTile];
    const uint32_t i = blockIdx.x * kFfThreads + threadIdx.x;
    const bool live = i < n;  // (no early return: the tiles have barriers)
    ff_body b;
    b.x = b.v = b.w = v3_make(0.0f, 0.0f, 0.0f);
    b.mass = 0.0f;
    b.category = 0xFFFFu;
    if (live) {
        b.x = ld3(pos, i);
        if (VEL) {
            const BodyVel bv = ld_vel(vel, i);
            b.v = bv.v; b.w = bv.w; b.mass = bv.mass;
        } else if (need_mass) {
            b.mass = vel[8 * (size_t)i + 7];
        }
        if (MASKED) b.category = filt[i].x & 0xFFFFu;
    }
    ff_sum sum;
    sum.F = sum.T = v3_make(0.0f, 0.0f, 0.0f);
    sum.acted = 0;
    const v3* acc_F = reinterpret_cast<const v3*>(force) + (live ? i : 0u);
    const v3* acc_T = reinterpret_cast<const v3*>(torque) + (live ? i : 0u);
    for (uint32_t t0 = 0; t0 < T; t0 += kFfTile) {
        const uint32_t tn = min(kFfTile, T - t0);
        tile_stage<FF_REC_VEC>(reinterpret_cast<vol_f4*>(tile), reinterpret_cast<const vol_f4*>(rec), t0, tn);
        if (live) ff_accumulate(tile, tn, &b, MASKED ? 1 : 0, acc_F, acc_T, &sum);
    }
    if (sum.acted) {
        st3(force, i, sum.F);
        st3(torque, i, sum.T);
    }
}

}  // namespace

int32_t fields_set(phys_world* w, FieldStaging&& staged) {
    const uint64_t n = staged.staged.size();
    w->n_fields = 0;  // (a failure below leaves a world without fields, not half a set)
    w->ff_masked = staged.masked; w->ff_drag = staged.drag; w->ff_accel = staged.accel;
    w->ff_host = std::move(staged.staged);
    if (n == 0) {  // back to launching nothing
        w->ff_rec.free();
        return PHYS_OK;
    }
    PHYS_TRY(upload_records(w, w->ff_rec, field_records(w->ff_host)));
    w->n_fields = n;
    return PHYS_OK;
}

int32_t fields_rebuild(phys_world* w) {
    if (w->n_fields == 0) return PHYS_OK;
    return upload_records(w, w->ff_rec, field_records(w->ff_host));  // on the world's stream: behind the updates already enqueued
}

void launch_force_fields(phys_world* w) {
    if (w->n_fields == 0 || w->n_owned == 0) return;
    const unsigned blocks = (unsigned)((w->n_owned + kFfThreads - 1) / kFfThreads);
    PHYS_PROF(w, PHYS_STAGE_MISC);
    dispatch_bool(w->ff_masked, [&](auto masked) {
        dispatch_bool(w->ff_drag, [&](auto vel) {
            hipLaunchKernelGGL((k_field_apply<decltype(masked)::value, decltype(vel)::value>), dim3(blocks), dim3(kFfThreads), 0, w->stream,
                               (uint32_t)w->n_owned, w->pos.p, w->vel.p, reinterpret_cast<const uint2*>(w->filt.p),
                               reinterpret_cast<const ff_record*>(w->ff_rec.p), (uint32_t)w->n_fields, w->ff_accel ? 1u : 0u, w->force.p,
                               w->torque.p);
        });
    });
    w->forces_dirty = true;
}

}  // namespace phys
