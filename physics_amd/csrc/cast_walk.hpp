// cast_walk.hpp — one query's walk through the query grid, shared by the cast kernel (raycast.hip k_rc_trace: ray casts, sphere
// casts, capsule casts) and move-and-slide (slide.hip k_slide, which casts again and again from registers): the exact tests of a
// ray and of a swept ball against one record, and rc_walk: the ground, the statics, the clip to the grid box, the DDA and, for a
// capsule cast, the contact at the end. There is one copy of it; the kernels load a query, call it and store the answer.
#pragma once
#include "capsule_cast.hpp"

namespace phys {
namespace {

// exact test of one record; accepted into `best` when t <= tmax and (t, id) beats it
__device__ __forceinline__ void rc_test(const float4* __restrict__ rec, uint32_t k, float ox, float oy, float oz, float ux, float uy,
                                        float uz, float tmax, uint32_t ignore, RayHit& best) {
    const float4 a = rec[3 * (size_t)k];
    const float4 c = rec[3 * (size_t)k + 2];
    const uint32_t id = __float_as_uint(c.w);
    if (id == ignore) return;
    const float px = ox - a.x, py = oy - a.y, pz = oz - a.z;  // origin relative to the centre
    float t, nx, ny, nz;
    if (__float_as_uint(a.w) == PHYS_SHAPE_SPHERE) {
        if (!ray_ball(px, py, pz, ux, uy, uz, c.x, t, nx, ny, nz)) return;
    } else if (__float_as_uint(a.w) == PHYS_SHAPE_CAPSULE) {
        // radius c.x, core c +- c.y * w, w = column 1 of R
        float wx, wy, wz;
        rc_capsule_axis(rec[3 * (size_t)k + 1], wx, wy, wz);
        if (!ray_capsule(px, py, pz, ux, uy, uz, wx, wy, wz, c.x, c.y, t, nx, ny, nz)) return;
    } else {
        const float4 q4 = rec[3 * (size_t)k + 1];
        quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
        m33 R;
        quat_to_m33(q, &R);  // world = R * local: the local frame is R^T (the conjugate rotation)
        const float lx = (R.m[0] * px + R.m[3] * py) + R.m[6] * pz;
        const float ly = (R.m[1] * px + R.m[4] * py) + R.m[7] * pz;
        const float lz = (R.m[2] * px + R.m[5] * py) + R.m[8] * pz;
        const float dx = (R.m[0] * ux + R.m[3] * uy) + R.m[6] * uz;
        const float dy = (R.m[1] * ux + R.m[4] * uy) + R.m[7] * uz;
        const float dz = (R.m[2] * ux + R.m[5] * uy) + R.m[8] * uz;
        float sx, sy, sz;
        const int res = ray_box_local(lx, ly, lz, dx, dy, dz, c.x, c.y, c.z, t, sx, sy, sz);
        if (res == 0) return;
        if (res == 1) {  // origin inside the closed box
            nx = -ux; ny = -uy; nz = -uz;
        } else {
            // local normal of the entering slab, into the world frame
            nx = (R.m[0] * sx + R.m[1] * sy) + R.m[2] * sz;
            ny = (R.m[3] * sx + R.m[4] * sy) + R.m[5] * sz;
            nz = (R.m[6] * sx + R.m[7] * sy) + R.m[8] * sz;
            const float inv = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);  // R of a nearly-unit quaternion
            nx *= inv; ny *= inv; nz *= inv;
        }
    }
    if (t <= tmax && rc_better(t, id, best)) { best.t = t; best.id = id; best.nx = nx; best.ny = ny; best.nz = nz; }
}

// a ball of radius rad swept from o along u against one record: the ray against the record's shape grown by rad (its
// Minkowski sum with the ball). Sphere r: the ball of r + rad. Capsule r: the capsule of r + rad. Box: the rounded box,
// the union of three boxes each grown by rad along one axis (its flat faces) and of the twelve edge capsules of radius
// rad (the cylinders along the edges; their end balls are the rounded corners): the least t over the fifteen. The normal
// runs from the target's closest point to the centre at t; from inside (t = 0) it is -u.
__device__ __forceinline__ void sc_test(const float4* __restrict__ rec, uint32_t k, float ox, float oy, float oz, float ux, float uy,
                                        float uz, float rad, float tmax, uint32_t ignore, RayHit& best) {
    const float4 a = rec[3 * (size_t)k];
    const float4 c = rec[3 * (size_t)k + 2];
    const uint32_t id = __float_as_uint(c.w);
    if (id == ignore) return;
    const float px = ox - a.x, py = oy - a.y, pz = oz - a.z;
    float t, nx, ny, nz;
    if (__float_as_uint(a.w) == PHYS_SHAPE_SPHERE) {
        if (!ray_ball(px, py, pz, ux, uy, uz, c.x + rad, t, nx, ny, nz)) return;
    } else if (__float_as_uint(a.w) == PHYS_SHAPE_CAPSULE) {
        float wx, wy, wz;
        rc_capsule_axis(rec[3 * (size_t)k + 1], wx, wy, wz);
        if (!ray_capsule(px, py, pz, ux, uy, uz, wx, wy, wz, c.x + rad, c.y, t, nx, ny, nz)) return;
    } else {
        const float4 q4 = rec[3 * (size_t)k + 1];
        quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
        m33 R;
        quat_to_m33(q, &R);
        const float lx = (R.m[0] * px + R.m[3] * py) + R.m[6] * pz;
        const float ly = (R.m[1] * px + R.m[4] * py) + R.m[7] * pz;
        const float lz = (R.m[2] * px + R.m[5] * py) + R.m[8] * pz;
        const float dx = (R.m[0] * ux + R.m[3] * uy) + R.m[6] * uz;
        const float dy = (R.m[1] * ux + R.m[4] * uy) + R.m[7] * uz;
        const float dz = (R.m[2] * ux + R.m[5] * uy) + R.m[8] * uz;
        float sx, sy, sz;
        // the rounded box lies inside the box grown by rad along every axis: a ray that misses that misses it
        if (ray_box_local(lx, ly, lz, dx, dy, dz, c.x + rad, c.y + rad, c.z + rad, t, sx, sy, sz) == 0) return;
        const float gx = fmaxf(fabsf(lx) - c.x, 0.0f), gy = fmaxf(fabsf(ly) - c.y, 0.0f), gz = fmaxf(fabsf(lz) - c.z, 0.0f);
        bool inside = (gx * gx + gy * gy) + gz * gz <= rad * rad;  // the centre starts within rad of the box
        float mx = 0.0f, my = 0.0f, mz = 0.0f;  // local normal of the best part
        t = __builtin_inff();
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            float tb, bx, by, bz;
            const int res = ray_box_local(lx, ly, lz, dx, dy, dz, c.x + (ax == 0 ? rad : 0.0f), c.y + (ax == 1 ? rad : 0.0f),
                                          c.z + (ax == 2 ? rad : 0.0f), tb, bx, by, bz);
            inside = inside || res == 1;
            if (res == 2 && tb < t) { t = tb; mx = bx; my = by; mz = bz; }
        }
        // radius 0: the rounded box is the box (and a zero-radius cylinder is ill-conditioned), so no edges
#pragma unroll
        for (int e = 0; e < (rad > 0.0f ? 12 : 0); ++e) {
            // edge e along axis e / 4, at the corner signs of bits 0 and 1 of e on the other two axes
            const int ax = e >> 2;
            const float s1 = (e & 1) ? 1.0f : -1.0f, s2 = (e & 2) ? 1.0f : -1.0f;
            const float ex = ax == 0 ? 0.0f : s1 * c.x;
            const float ey = ax == 1 ? 0.0f : (ax == 0 ? s1 : s2) * c.y;
            const float ez = ax == 2 ? 0.0f : s2 * c.z;
            const float hl = ax == 0 ? c.x : (ax == 1 ? c.y : c.z);
            float te, ex_n, ey_n, ez_n;
            if (ray_capsule(lx - ex, ly - ey, lz - ez, dx, dy, dz, ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f,
                            rad, hl, te, ex_n, ey_n, ez_n) &&
                te < t) {
                t = te; mx = ex_n; my = ey_n; mz = ez_n;
            }
        }
        if (inside) {
            t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        } else {
            if (!(t < __builtin_inff())) return;
            // the normal runs from the box's closest point to the centre at t: a face and the cylinder beside it give
            // nearly equal t near their seam, and this does not depend on which of them rounding picked (the part's own
            // normal stays for a centre that rounding put within rad / 2 of the box)
            const float cx = lx + t * dx, cy = ly + t * dy, cz = lz + t * dz;
            const float vx = cx - fminf(fmaxf(cx, -c.x), c.x), vy = cy - fminf(fmaxf(cy, -c.y), c.y), vz = cz - fminf(fmaxf(cz, -c.z), c.z);
            if ((vx * vx + vy * vy) + vz * vz > 0.25f * (rad * rad)) { mx = vx; my = vy; mz = vz; }
            nx = (R.m[0] * mx + R.m[1] * my) + R.m[2] * mz;
            ny = (R.m[3] * mx + R.m[4] * my) + R.m[5] * mz;
            nz = (R.m[6] * mx + R.m[7] * my) + R.m[8] * mz;
            const float inv = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);
            nx *= inv; ny *= inv; nz *= inv;
        }
    }
    if (t <= tmax && rc_better(t, id, best)) { best.t = t; best.id = id; best.nx = nx; best.ny = ny; best.nz = nz; }
}

__device__ __forceinline__ float rc_plane_t(int i, bool up, float lo, float cell, float o, float inv_u) {
    return ((lo + (float)(i + (up ? 1 : 0)) * cell) - o) * inv_u;
}

// the length of a cast's direction: this expression everywhere (include/spec/slide.h sl_length restates it)
__device__ __forceinline__ float rc_length(v3 d) { return sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z); }

// One query from o along d, up to tmax, in registers: its answer in best (a miss: kRayMiss, +inf, zeros) and, for a capsule
// cast, the touched point. len: rc_length(d), which the caller has (move-and-slide needs it for its own rule).
// SWEEP: a sphere cast (radius rad; the grid was grown by the largest valid radius, so the walk of the centre line meets every
// target the ball can touch); otherwise a ray cast (rad unused, the arithmetic of the ray cast unchanged).
// FILT: a target whose category misses the query's mask qm is skipped before its exact test.
// CAPS (SWEEP instances only): the capsule cast. A query with a half-length hq above 0 along the unit axis a tests with cc_test
// and finds its contact after the walk, the others are sphere casts with a touched point; cap_ok: hq and the rot a came from
// are usable (otherwise the query misses).
// ign: a body id that is never reported (0xFFFFFFFF: none). STATS: cells visited and candidates tested are added up.
// hdr, bits, start, rec: the grid of launch_query_grid; st_rec, n_static: the statics; ground, ground_y: the ground plane. (Plain
// arguments, not a struct: the grid's sizes then stay in scalar registers, as they did while the walk was the kernel's body.)
template <bool STATS, bool SWEEP, bool FILT, bool CAPS>
__device__ __forceinline__ void rc_walk(const RcHeader* __restrict__ hdr, uint32_t bits, const uint32_t* __restrict__ start,
                                        const float4* __restrict__ rec, int ground, float ground_y, const float4* __restrict__ st_rec,
                                        uint32_t n_static, const QueryFilters& qf, uint32_t qm, v3 o, v3 d, float len, float tmax,
                                        uint32_t ign, float rad, float hq, float ax, float ay, float az, bool cap_ok, RayHit& best_out,
                                        v3& point_out, uint32_t& cells, uint32_t& cands) {
    RayHit best;
    best.t = __builtin_inff(); best.id = kRayMiss; best.nx = 0.0f; best.ny = 0.0f; best.nz = 0.0f;
    v3 point = v3_make(0.0f, 0.0f, 0.0f);
    const float sum = ((o.x + o.y) + (o.z + d.x)) + (d.y + d.z);
    const bool rad_ok = !SWEEP || (rad >= 0.0f && rad <= 3.4e38f);  // a negative, NaN or infinite radius misses
    bool best_st = false;
    uint32_t best_k = 0;
    if (len > 0.0f && len <= 3.0e38f && isfinite(sum) && tmax >= 0.0f && rad_ok && cap_ok) {
        const float ux = d.x / len, uy = d.y / len, uz = d.z / len;
        // the ground: the solid half-space y <= ground_y (for a ball: its centre reaches y = ground_y + rad; for a capsule:
        // its lowest point, hq |a.y| + rad below the centre)
        float gy = SWEEP ? ground_y + rad : ground_y;
        if (CAPS && hq > 0.0f) gy = ground_y + (rad + hq * fabsf(ay));
        if (ground && (!FILT || (qf.ground & qm) != 0u)) {
            float tg = -1.0f;
            if (o.y <= gy) { tg = 0.0f; best.nx = -ux; best.ny = -uy; best.nz = -uz; }
            else if (uy < 0.0f) { tg = (gy - o.y) / uy; best.nx = 0.0f; best.ny = 1.0f; best.nz = 0.0f; }
            if (tg >= 0.0f && tg <= tmax) { best.t = tg; best.id = kRayGround; }
            else { best.nx = 0.0f; best.ny = 0.0f; best.nz = 0.0f; }
        }
        // static colliders (records of phys_set_static_bodies, id PHYS_STATIC_ID_BIT | k): every one tested, before the bodies'
        // walk so that a static hit shortens it; bodies still win exact ties (smaller ids), the ground loses them
        for (uint32_t k = 0; k < n_static; ++k) {
            if (FILT && (qf.st[k].x & qm) == 0u) continue;
            if (CAPS && hq > 0.0f) cc_test(st_rec, k, true, o.x, o.y, o.z, ux, uy, uz, ax, ay, az, hq, rad, tmax, 0xFFFFFFFFu, best, best_k, best_st);
            else if (SWEEP) sc_test(st_rec, k, o.x, o.y, o.z, ux, uy, uz, rad, tmax, 0xFFFFFFFFu, best);
            else rc_test(st_rec, k, o.x, o.y, o.z, ux, uy, uz, tmax, 0xFFFFFFFFu, best);
        }
        const RcGrid g = rc_grid(hdr);
        // clip to the grid box and to [0, min(max_t, best)] (bodies win ties with the ground: best.t itself stays in)
        const float iux = 1.0f / ux, iuy = 1.0f / uy, iuz = 1.0f / uz;  // +-inf on a zero component
        const float hx = g.lox + (float)g.nx * g.cell, hy = g.loy + (float)g.ny * g.cell, hz = g.loz + (float)g.nz * g.cell;
        float t0 = 0.0f, t1 = fminf(tmax, best.t);
        bool hit_box = g.valid;
        if (ux == 0.0f) hit_box = hit_box && o.x >= g.lox && o.x <= hx;
        else { const float a = (g.lox - o.x) * iux, b = (hx - o.x) * iux; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (uy == 0.0f) hit_box = hit_box && o.y >= g.loy && o.y <= hy;
        else { const float a = (g.loy - o.y) * iuy, b = (hy - o.y) * iuy; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (uz == 0.0f) hit_box = hit_box && o.z >= g.loz && o.z <= hz;
        else { const float a = (g.loz - o.z) * iuz, b = (hz - o.z) * iuz; t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (hit_box && t0 <= t1) {
            const float tlim = fminf(tmax, best.t);
            int ix = rc_coord(o.x + t0 * ux, g.lox, g.inv, g.nx);
            int iy = rc_coord(o.y + t0 * uy, g.loy, g.inv, g.ny);
            int iz = rc_coord(o.z + t0 * uz, g.loz, g.inv, g.nz);
            const bool upx = ux > 0.0f, upy = uy > 0.0f, upz = uz > 0.0f;
            const int sx = upx ? 1 : (ux < 0.0f ? -1 : 0), sy = upy ? 1 : (uy < 0.0f ? -1 : 0), sz = upz ? 1 : (uz < 0.0f ? -1 : 0);
            const float inf = __builtin_inff();
            float tx = sx ? rc_plane_t(ix, upx, g.lox, g.cell, o.x, iux) : inf;
            float ty = sy ? rc_plane_t(iy, upy, g.loy, g.cell, o.y, iuy) : inf;
            float tz = sz ? rc_plane_t(iz, upz, g.loz, g.cell, o.z, iuz) : inf;
            // a walk never takes more steps than the grid has cells along the three axes (also bounds a NaN walk)
            for (int steps = g.nx + g.ny + g.nz + 3; steps > 0; --steps) {
                const float texit = fminf(tx, fminf(ty, tz));
                const uint32_t bk = rc_bucket(ix, iy, iz, bits);
                const uint32_t b0 = start[bk], b1 = start[bk + 1];
                if (STATS) { cells += 1; cands += b1 - b0; }
                for (uint32_t k = b0; k < b1; ++k) {
                    if (FILT && (qf.body[__float_as_uint(rec[3 * (size_t)k + 2].w)].x & qm) == 0u) continue;
                    if (CAPS && hq > 0.0f) cc_test(rec, k, false, o.x, o.y, o.z, ux, uy, uz, ax, ay, az, hq, rad, tlim, ign, best, best_k, best_st);
                    else if (SWEEP) sc_test(rec, k, o.x, o.y, o.z, ux, uy, uz, rad, tlim, ign, best);
                    else rc_test(rec, k, o.x, o.y, o.z, ux, uy, uz, tlim, ign, best);
                }
                if (best.t <= texit || texit > t1) break;
                const bool stepx = tx <= ty && tx <= tz, stepy = !stepx && ty <= tz, stepz = !stepx && !stepy;
                ix += stepx ? sx : 0; iy += stepy ? sy : 0; iz += stepz ? sz : 0;
                if (ix < 0 || ix >= g.nx || iy < 0 || iy >= g.ny || iz < 0 || iz >= g.nz) break;
                tx = stepx ? rc_plane_t(ix, upx, g.lox, g.cell, o.x, iux) : tx;
                ty = stepy ? rc_plane_t(iy, upy, g.loy, g.cell, o.y, iuy) : ty;
                tz = stepz ? rc_plane_t(iz, upz, g.loz, g.cell, o.z, iuz) : tz;
            }
        }
        if constexpr (CAPS) {
            // the contact, once per query: the touched point and, for a capsule, the normal from the closest points at t
            if (best.id == kRayGround && best.t > 0.0f) {
                // the lower end of the core (the centre for a level one) at t, projected onto the plane
                const float e = ay > 0.0f ? -hq : (ay < 0.0f ? hq : 0.0f);
                point = v3_make((o.x + best.t * ux) + e * ax, ground_y, (o.z + best.t * uz) + e * az);
            } else if (best.id != kRayMiss && best.t > 0.0f) {
                if (hq > 0.0f) cc_contact(best_st ? st_rec : rec, best_k, o.x, o.y, o.z, ux, uy, uz, ax, ay, az, hq, rad, best.t, best.nx, best.ny, best.nz, point);
                else point = v3_make(o.x + (best.t * ux - rad * best.nx), o.y + (best.t * uy - rad * best.ny), o.z + (best.t * uz - rad * best.nz));
            }
        }
    }
    best_out = best;
    point_out = point;
}

}  // namespace
}  // namespace phys
