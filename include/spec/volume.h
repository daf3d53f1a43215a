/* volume.h — the record of a volume in the world: a SPHERE, BOX or CAPSULE at a pose that is no body and no static, but is
 * evaluated against the bodies by a kernel of its own. A trigger volume (physics_amd/csrc/trigger.hip)
 * is exactly this record; a force field (force_field.h; section 22) is this record plus one vector of its law. This is the ONE
 * statement of the layout: the host builds the records (physics_amd/csrc/setup.hpp trigger_records, field_records), the
 * kernels and the CPU probes read them through the accessors below. Scalar f32 with a fixed operation order; build with
 * -ffp-contract=off, and host and device give the same bits. */
#ifndef PHYS_SPEC_VOLUME_H
#define PHYS_SPEC_VOLUME_H

#include <stdint.h>

#include "collide.h"

/* 16 bytes, aligned: one vector load or store on the device */
typedef struct __attribute__((aligned(16))) { float x, y, z, w; } vol_f4;

/* One volume as an evaluation reads it, 96 bytes:
 *   r[0] = {AABB lo, shape}   r[1] = {AABB hi, mask}
 *   r[2] = {centre, h.x}   r[3] = {R row 0, h.y}   r[4] = {R row 1, h.z}   r[5] = {R row 2, 0}
 * The AABB is the volume's exact box (body_aabb, margin 0); a volume whose box is not finite gets an inverted one and touches
 * nothing. R is the rotation matrix of the quaternion, row-major. Integers travel as the bits of a float. r[0].w and r[5].w
 * are the two words a user of the record may take for itself (force_field.h does). */
#define VOL_REC_VEC 6
typedef struct { vol_f4 r[VOL_REC_VEC]; } vol_record;

PHYS_HD float vol_u2f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
PHYS_HD uint32_t vol_f2u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
PHYS_HD vol_f4 vol_f4_make(float x, float y, float z, float w) { vol_f4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

PHYS_HD vol_record vol_record_make(uint32_t shape, uint32_t mask, v3 c, quat q, v3 h) {
    aabb_t b = body_aabb(c, q, h, shape, 0.0f);
    const float sum = ((b.lo.x + b.lo.y) + (b.lo.z + b.hi.x)) + (b.hi.y + b.hi.z);
    if (!(det_absf(sum) <= 3.0e38f)) { /* NaN or infinite: touches nothing */
        b.lo = v3_make(3.0e38f, 3.0e38f, 3.0e38f);
        b.hi = v3_make(-3.0e38f, -3.0e38f, -3.0e38f);
    }
    m33 R;
    quat_to_m33(q, &R);
    vol_record r;
    r.r[0] = vol_f4_make(b.lo.x, b.lo.y, b.lo.z, vol_u2f(shape));
    r.r[1] = vol_f4_make(b.hi.x, b.hi.y, b.hi.z, vol_u2f(mask));
    r.r[2] = vol_f4_make(c.x, c.y, c.z, h.x);
    r.r[3] = vol_f4_make(R.m[0], R.m[1], R.m[2], h.y);
    r.r[4] = vol_f4_make(R.m[3], R.m[4], R.m[5], h.z);
    r.r[5] = vol_f4_make(R.m[6], R.m[7], R.m[8], 0.0f);
    return r;
}

/* ---- what an evaluation reads, by the vectors it has to load for it: r[0] and r[1] reject by mask and box, and only a
 * survivor loads r[2] to r[5] ---- */
PHYS_HD uint32_t vol_word(vol_f4 r0) { return vol_f2u(r0.w); } /* the shape, or what the record's user packed there */
PHYS_HD uint32_t vol_mask(vol_f4 r1) { return vol_f2u(r1.w); }
PHYS_HD v3 vol_lo(vol_f4 r0) { return v3_make(r0.x, r0.y, r0.z); }
PHYS_HD v3 vol_hi(vol_f4 r1) { return v3_make(r1.x, r1.y, r1.z); }
/* the volume's box against the box [lo, hi] (a point: lo == hi); a non-finite coordinate on either side fails */
PHYS_HD int vol_box_meets(vol_f4 r0, vol_f4 r1, v3 lo, v3 hi) {
    return r0.x <= hi.x && lo.x <= r1.x && r0.y <= hi.y && lo.y <= r1.y && r0.z <= hi.z && lo.z <= r1.z;
}
PHYS_HD v3 vol_centre(vol_f4 r2) { return v3_make(r2.x, r2.y, r2.z); }
PHYS_HD v3 vol_half_extent(vol_f4 r2, vol_f4 r3, vol_f4 r4) { return v3_make(r2.w, r3.w, r4.w); }
PHYS_HD m33 vol_rotation(vol_f4 r3, vol_f4 r4, vol_f4 r5) {
    const m33 R = {{r3.x, r3.y, r3.z, r4.x, r4.y, r4.z, r5.x, r5.y, r5.z}};
    return R;
}

#endif /* PHYS_SPEC_VOLUME_H */
