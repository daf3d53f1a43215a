// edit.hip — in-place body edits: poses, velocities, impulses and forces by id list, and the read-back
// of a few bodies' states. Their kernels sit outside the step, as the triggers' and the force fields' do: nothing in the
// solver, the narrow phase or the plan changes, and a world that never calls them launches exactly what it launched before.
//
// One design for every edit, no atomics and no per-body table: the entries reach the device ordered by id (the host calls
// sort them, setup.hpp edit_order; the device calls ask the caller for it), so the entries of one body form a run. One lane
// per entry, workgroups of 256:
//   * lane i LEADS a run iff i == 0 or ids[i - 1] != ids[i]; everyone else returns;
//   * a leader walks forward while the id repeats, applies the run's entries in entry order in registers, and so reads the
//     body's state once and writes it once (a set call writes the run's last entry: the last entry of a body wins);
//   * a lane whose id is not below n_owned skips its entry, and it or a lane that sees ids[i - 1] > ids[i] raises kOvfBadEdit in
//     the STICKY overflow word alone (phys_sync: PHYS_ERR_INVALID_ARG). Nothing is ever written outside the arrays: every
//     store is indexed by an id that was compared with n_owned, or by the lane's own entry index below n.
// These are memory-bound scatters: there is nothing to tune beyond that. The arithmetic is include/spec/body_edit.h's, called
// from here and compiled alone by tests/cpp/body_edit_probe.cpp.
#include "kernels.hpp"

namespace phys {

namespace {

constexpr int kEditThreads = 256;

// a caller's quaternion array (device calls: any 4-byte aligned pointer) as one 16-byte access per lane
struct alignas(4) packed4 { float x, y, z, w; };

// entry i of the batch: its id, whether it is refused (flagged), and whether this lane applies a run
__device__ __forceinline__ bool edit_leads(const uint32_t* __restrict__ ids, uint32_t n_owned, uint32_t i, StepCounters* __restrict__ ctr,
                                           uint32_t& id) {
    id = ids[i];
    const bool in_range = id < n_owned;
    if (!in_range || be_out_of_order(ids, i)) atomicOr(&ctr->sticky_overflow, kOvfBadEdit);
    return in_range && be_leads(ids, i);
}

__global__ __launch_bounds__(kEditThreads) void k_edit_poses(uint32_t n, uint32_t n_owned, const uint32_t* __restrict__ ids,
                                                             const float* __restrict__ pos_in, const float* __restrict__ rot_in,
                                                             float* __restrict__ pos, float* __restrict__ rot, StepCounters* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t id;
    if (!edit_leads(ids, n_owned, i, ctr, id)) return;
    const uint32_t last = be_run_end(ids, n, i) - 1u;
    if (pos_in) st3(pos, id, ld3(pos_in, last));
    if (rot_in) {  // stored as given: the integrator never renormalises either
        const packed4 q = reinterpret_cast<const packed4*>(rot_in)[last];
        reinterpret_cast<float4*>(rot)[id] = make_float4(q.x, q.y, q.z, q.w);
    }
}

// only v and w of the 32-byte record are rewritten: inv_mass and mass travel through
__global__ __launch_bounds__(kEditThreads) void k_edit_velocities(uint32_t n, uint32_t n_owned, const uint32_t* __restrict__ ids,
                                                                  const float* __restrict__ lin_in, const float* __restrict__ ang_in,
                                                                  float* __restrict__ vel, StepCounters* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t id;
    if (!edit_leads(ids, n_owned, i, ctr, id)) return;
    const uint32_t last = be_run_end(ids, n, i) - 1u;
    BodyVel bv = ld_vel(vel, id);
    if (lin_in) bv.v = ld3(lin_in, last);
    if (ang_in) bv.w = ld3(ang_in, last);
    st_vel(vel, id, bv);
}

// DIAG: every tensor is diagonal and `inertia` is the compact diagonal array, read at id * inertia_stride (0: one shared
// tensor) as the integrator reads it; otherwise the full 3x3 per body
template <bool DIAG>
__global__ __launch_bounds__(kEditThreads) void k_edit_impulses(uint32_t n, uint32_t n_owned, const uint32_t* __restrict__ ids,
                                                                const float* __restrict__ impulse, const float* __restrict__ point,
                                                                const float* __restrict__ ang_impulse, const float* __restrict__ pos,
                                                                float* __restrict__ vel, const float* __restrict__ inertia,
                                                                uint32_t inertia_stride, StepCounters* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t id;
    if (!edit_leads(ids, n_owned, i, ctr, id)) return;
    const uint32_t end = be_run_end(ids, n, i);
    BodyVel bv = ld_vel(vel, id);
    const v3 x = point ? ld3(pos, id) : v3_make(0.0f, 0.0f, 0.0f);
    const m33 I = ld_inertia<DIAG>(inertia, DIAG ? id * inertia_stride : id);
    const v3 d = v3_make(I.m[0], I.m[4], I.m[8]);
    for (uint32_t j = i; j < end; ++j) {
        const v3 J = ld3(impulse, j);
        v3 p = v3_make(0.0f, 0.0f, 0.0f), a = v3_make(0.0f, 0.0f, 0.0f);
        if (point) p = ld3(point, j);
        if (ang_impulse) a = ld3(ang_impulse, j);
        be_impulse(x, bv.inv_mass, DIAG ? 1 : 0, d, &I, J, point != nullptr, p, ang_impulse != nullptr, a, &bv.v, &bv.w);
    }
    st_vel(vel, id, bv);
}

__global__ __launch_bounds__(kEditThreads) void k_edit_forces(uint32_t n, uint32_t n_owned, const uint32_t* __restrict__ ids,
                                                              const float* __restrict__ f_in, const float* __restrict__ point,
                                                              const float* __restrict__ torque_in, const float* __restrict__ pos,
                                                              float* __restrict__ force, float* __restrict__ torque,
                                                              StepCounters* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t id;
    if (!edit_leads(ids, n_owned, i, ctr, id)) return;
    const uint32_t end = be_run_end(ids, n, i);
    v3 F = ld3(force, id), T = ld3(torque, id);
    const v3 x = point ? ld3(pos, id) : v3_make(0.0f, 0.0f, 0.0f);
    for (uint32_t j = i; j < end; ++j) {
        const v3 f = ld3(f_in, j);
        v3 p = v3_make(0.0f, 0.0f, 0.0f), t = v3_make(0.0f, 0.0f, 0.0f);
        if (point) p = ld3(point, j);
        if (torque_in) t = ld3(torque_in, j);
        be_force(x, f, point != nullptr, p, torque_in != nullptr, t, &F, &T);
    }
    st3(force, id, F);
    st3(torque, id, T);
}

// the states of the bodies named, ids in any order and with repeats: entry i's outputs are lane i's
__global__ __launch_bounds__(kEditThreads) void k_get_states(uint32_t n, uint32_t n_owned, const uint32_t* __restrict__ ids,
                                                             const float* __restrict__ pos, const float* __restrict__ rot,
                                                             const float* __restrict__ vel, float* __restrict__ pos_out,
                                                             float* __restrict__ rot_out, float* __restrict__ lin_out,
                                                             float* __restrict__ ang_out, StepCounters* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t id = ids[i];
    if (id >= n_owned) {  // skipped: its outputs stay as they were
        atomicOr(&ctr->sticky_overflow, kOvfBadEdit);
        return;
    }
    if (pos_out) st3(pos_out, i, ld3(pos, id));
    if (rot_out) {
        const float4 q = reinterpret_cast<const float4*>(rot)[id];
        packed4 o; o.x = q.x; o.y = q.y; o.z = q.z; o.w = q.w;
        reinterpret_cast<packed4*>(rot_out)[i] = o;
    }
    if (lin_out || ang_out) {
        const BodyVel bv = ld_vel(vel, id);
        if (lin_out) st3(lin_out, i, bv.v);
        if (ang_out) st3(ang_out, i, bv.w);
    }
}

}  // namespace

// one edit batch on device arrays (arguments checked by the caller: setup.hpp edit_args_error), enqueued on the world's stream
int32_t launch_edit(phys_world* w, EditKind kind, const EditBatch& b) {
    if (b.n == 0) return PHYS_OK;
    const uint32_t n = (uint32_t)b.n, n_owned = (uint32_t)w->n_owned;
    const dim3 grid((unsigned)((b.n + kEditThreads - 1) / kEditThreads)), block(kEditThreads);
    hipStream_t s = w->stream;
    StepCounters* ctr = w->counters.p;
    PHYS_PROF(w, PHYS_STAGE_MISC);
    switch (kind) {
        case EditKind::Poses:
            hipLaunchKernelGGL(k_edit_poses, grid, block, 0, s, n, n_owned, b.ids, b.a[0], b.a[1], w->pos.p, w->rot.p, ctr);
            // what is derived from the poses and kept: the AABBs and the two grids of the last broad phase (phys_broadphase,
            // phys_get_aabbs and the halo entry points then see the new poses). geo, the query grid, the triggers and the fields
            // are rebuilt from pos / rot by their next use
            w->aabbs_valid = false;
            w->grid_valid = false;
            w->sorted_grid_valid = false;
            break;
        case EditKind::Velocities:
            hipLaunchKernelGGL(k_edit_velocities, grid, block, 0, s, n, n_owned, b.ids, b.a[0], b.a[1], w->vel.p, ctr);
            break;
        case EditKind::Impulses: {
            const uint32_t stride = (w->all_diag_inertia && w->uniform_inertia) ? 0u : 1u;  // integrate.hip make_params
            dispatch_bool(w->all_diag_inertia, [&](auto diag) {
                constexpr bool kDiag = decltype(diag)::value;
                hipLaunchKernelGGL((k_edit_impulses<kDiag>), grid, block, 0, s, n, n_owned, b.ids, b.a[0], b.a[1], b.a[2], w->pos.p, w->vel.p,
                                   kDiag ? w->inv_inertia_diag.p : w->inv_inertia.p, stride, ctr);
            });
            break;
        }
        case EditKind::Forces:
            hipLaunchKernelGGL(k_edit_forces, grid, block, 0, s, n, n_owned, b.ids, b.a[0], b.a[1], b.a[2], w->pos.p, w->force.p, w->torque.p,
                               ctr);
            w->forces_dirty = true;
            break;
    }
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

int32_t launch_get_states(phys_world* w, uint64_t n, const uint32_t* ids, float* pos_out, float* rot_out, float* lin_out, float* ang_out) {
    if (n == 0) return PHYS_OK;
    const dim3 grid((unsigned)((n + kEditThreads - 1) / kEditThreads)), block(kEditThreads);
    PHYS_PROF(w, PHYS_STAGE_MISC);
    hipLaunchKernelGGL(k_get_states, grid, block, 0, w->stream, (uint32_t)n, (uint32_t)w->n_owned, ids, w->pos.p, w->rot.p, w->vel.p, pos_out,
                       rot_out, lin_out, ang_out, w->counters.p);
    PHYS_HIP_TRY(hipGetLastError());
    return PHYS_OK;
}

}  // namespace phys
