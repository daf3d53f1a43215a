/* body_edit.h — normative scalar definition of the in-place body edits (physics_hip.h, phys_set_body_poses ...
 * phys_get_body_states): what one entry of an impulse or force batch does to the body it names, and
 * how a batch ordered by body id splits into runs.
 *
 * The reference (martingoe/physics) can only add a force to a body (rigid_body.rs:43-62), so for the impulses this header is
 * the specification itself; for the forces it restates apply_force_at_position and the plain accumulator sums. The HIP kernels
 * (physics_amd/csrc/edit.hip) call exactly these functions, and a host compiler reads the header alone
 * (tests/cpp/body_edit_probe.cpp), so a GPU run and a sequential CPU run agree bit for bit. Build with -ffp-contract=off.
 *
 * Order: a call behaves as if its entries were applied one after another in the order given. Entries reach the device ordered
 * by id (a stable sort), so the entries of one body form a run in entry order: one lane applies a run from first to last,
 * reading the body's state once and writing it once. Nothing depends on any other body.
 */
#ifndef PHYS_SPEC_BODY_EDIT_H
#define PHYS_SPEC_BODY_EDIT_H

#include <stdint.h>

#include "vec.h"

/* ---- runs of a batch ordered by id ---- */
/* entry i is the first of its body's run */
PHYS_HD int be_leads(const uint32_t* ids, uint32_t i) { return i == 0u || ids[i - 1u] != ids[i]; }
/* entry i breaks the order the device calls ask for (non-decreasing ids) */
PHYS_HD int be_out_of_order(const uint32_t* ids, uint32_t i) { return i != 0u && ids[i - 1u] > ids[i]; }
/* one past the last entry of the run that entry i leads */
PHYS_HD uint32_t be_run_end(const uint32_t* ids, uint32_t n, uint32_t i) {
    uint32_t j = i + 1u;
    while (j < n && ids[j] == ids[i]) ++j;
    return j;
}

/* ---- the inverse inertia times an angular impulse, as the integrator's velocity half applies it ----
 * diag != 0: the tensor is diagonal and d holds its diagonal (the gemv row sum reduces to the diagonal product); else the
 * full row-major 3x3. */
PHYS_HD v3 be_inv_inertia_mul(int diag, v3 d, const m33* I, v3 L) {
    if (diag) return v3_make(d.x * L.x, d.y * L.y, d.z * L.z);
    return m33_mul_v3(I, L);
}

/* ---- one impulse entry on a body at x with velocities *v, *w ----
 * r = point - x (zero without a point), L = ang_impulse + r x J (ang_impulse zero when absent),
 * v = v + J * inv_mass, w = w + I^-1 L. */
PHYS_HD void be_impulse(v3 x, float inv_mass, int diag, v3 d, const m33* I, v3 J, int has_point, v3 point, int has_ang, v3 ang_impulse,
                        v3* v, v3* w) {
    const v3 r = has_point ? v3_sub(point, x) : v3_make(0.0f, 0.0f, 0.0f);
    const v3 a = has_ang ? ang_impulse : v3_make(0.0f, 0.0f, 0.0f);
    const v3 L = v3_add(a, v3_cross(r, J));
    *v = v3_add(*v, v3_scale(J, inv_mass));
    *w = v3_add(*w, be_inv_inertia_mul(diag, d, I, L));
}

/* ---- one force entry on a body at x with accumulators *F, *T ----
 * RigidBody::apply_force_at_position (T += (point - x) x f, F += f) or, without a point, apply_force_centre_of_gravity
 * (F += f); then T += torque if given. */
PHYS_HD void be_force(v3 x, v3 f, int has_point, v3 point, int has_torque, v3 torque, v3* F, v3* T) {
    if (has_point) *T = v3_add(*T, v3_cross(v3_sub(point, x), f));
    *F = v3_add(*F, f);
    if (has_torque) *T = v3_add(*T, torque);
}

#endif /* PHYS_SPEC_BODY_EDIT_H */
