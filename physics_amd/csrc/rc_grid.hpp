// rc_grid.hpp — what the read-only queries share: the per-call query grid (raycast.hip builds it; ray casts, sphere casts
// and overlap queries walk it) and the exact ray tests against one sphere, capsule or box. A sphere cast is a ray cast
// against the target grown by the ball's radius, so it calls the same tests with grown sizes (DESIGN.md sections 9, 12).
// At the end: what the capsule query kernels share (the load of a lane's query, the slot writer) and the host's QueryGrid.
#pragma once
#include "kernels.hpp"

namespace phys {
namespace {

constexpr int kRcThreads = 256;
constexpr uint32_t kRcMaxCellsPerAxis = 1u << 20;
constexpr uint32_t kRayMiss = PHYS_RAY_MISS, kRayGround = PHYS_RAY_GROUND;

// k_rc_bounds' result: order-preserving keys (0 = nothing seen, which no finite float maps to); the low corner as the
// key of -x so that every slot is a max and one memset to zero resets them all. grow: the bits of the non-negative float
// every body AABB is grown by before it is measured and inserted (0 for ray casts and overlap queries, the call's largest
// radius for sphere casts): the header is zeroed, so a call that never writes it grows nothing.
struct RcHeader {
    uint32_t neg_lo[3];
    uint32_t hi[3];
    uint32_t edge;
    uint32_t grow;
};

__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the grid every kernel derives from the header (same arithmetic everywhere, so insertion and walk agree on every cell)
struct RcGrid {
    float lox, loy, loz;  // grid origin = scene bounds - pad
    float cell, inv, pad;
    int nx, ny, nz;       // cells per axis
    bool valid;           // some owned body has a shape
};

__device__ __forceinline__ int rc_dim(float span, float inv) {
    float c = floorf(span * inv) + 1.0f;
    c = c < 1.0f ? 1.0f : (c > (float)kRcMaxCellsPerAxis + 1.0f ? (float)kRcMaxCellsPerAxis + 1.0f : c);
    return (int)c;
}

__device__ __forceinline__ RcGrid rc_grid(const RcHeader* __restrict__ h) {
    RcGrid g;
    g.valid = h->hi[0] != 0u;
    const float lx = -key2f(h->neg_lo[0]), ly = -key2f(h->neg_lo[1]), lz = -key2f(h->neg_lo[2]);
    const float hx = key2f(h->hi[0]), hy = key2f(h->hi[1]), hz = key2f(h->hi[2]);
    const float e = g.valid ? key2f(h->edge) : 0.0f;
    float m = fmaxf(fmaxf(fabsf(lx), fabsf(hx)), fmaxf(fmaxf(fabsf(ly), fabsf(hy)), fmaxf(fabsf(lz), fabsf(hz))));
    if (!g.valid) m = 0.0f;
    // pad: float rounding of an AABB, of a cell coordinate and of the walk's plane crossings is a few ulp of the scene's
    // coordinates; 2^-16 of them is hundreds of ulp. The cell exceeds the padded edge, so a body touches <= 2 cells per axis
    g.pad = 0x1p-16f * (m + e);
    g.lox = lx - g.pad; g.loy = ly - g.pad; g.loz = lz - g.pad;
    const float sx = (hx + g.pad) - g.lox, sy = (hy + g.pad) - g.loy, sz = (hz + g.pad) - g.loz;
    float cell = (e + 2.0f * g.pad) * (1.0f + 0x1p-10f);
    const float span = fmaxf(sx, fmaxf(sy, sz));
    if (span * 0x1p-20f > cell) cell = span * 0x1p-20f;  // a guard: cell >= 2 pad >= 2^-15 m already keeps an axis below 65 474 cells
    g.cell = fmaxf(cell, 1.0e-30f);
    g.inv = 1.0f / g.cell;
    g.nx = g.valid ? rc_dim(sx, g.inv) : 1;
    g.ny = g.valid ? rc_dim(sy, g.inv) : 1;
    g.nz = g.valid ? rc_dim(sz, g.inv) : 1;
    return g;
}

__device__ __forceinline__ int rc_coord(float x, float lo, float inv, int n) {
    float c = floorf((x - lo) * inv);
    c = c < 0.0f ? 0.0f : (c > (float)(n - 1) ? (float)(n - 1) : c);  // NaN stays NaN -> (int) 0 on gfx950, still in range
    const int i = (int)c;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// multiplicative hash of the cell, top `bits` bits
__device__ __forceinline__ uint32_t rc_bucket(int x, int y, int z, uint32_t bits) {
    const uint32_t h = ((uint32_t)x * 73856093u) ^ ((uint32_t)y * 19349663u) ^ ((uint32_t)z * 83492791u);
    return (h * 0x9E3779B1u) >> (32u - bits);
}

// the exact AABB of a target from its shape and pose; false for no shape or a non-finite pose (never inserted, never hit)
__device__ __forceinline__ bool rc_aabb_of(v3 c, float4 q4, v3 h, uint32_t type, aabb_t* out) {
    if (type != PHYS_SHAPE_SPHERE && type != PHYS_SHAPE_BOX && type != PHYS_SHAPE_CAPSULE) return false;
    quat q; q.i = q4.x; q.j = q4.y; q.k = q4.z; q.w = q4.w;
    const aabb_t b = body_aabb(c, q, h, type, 0.0f);
    const float s = ((b.lo.x + b.lo.y) + (b.lo.z + b.hi.x)) + (b.hi.y + b.hi.z);
    if (!isfinite(s)) return false;
    *out = b;
    return true;
}

__device__ __forceinline__ bool rc_aabb(const float* __restrict__ pos, const float* __restrict__ rot, const float* __restrict__ he,
                                        const uint32_t* __restrict__ shape, uint32_t i, aabb_t* out) {
    return rc_aabb_of(ld3(pos, i), reinterpret_cast<const float4*>(rot)[i], ld3(he, i), shape[i], out);
}

// a body AABB grown by the header's grow amount (0 for ray casts: x - 0 == x, the grid and the walk stay as they were)
__device__ __forceinline__ aabb_t rc_grown(aabb_t b, float grow) {
    b.lo = v3_make(b.lo.x - grow, b.lo.y - grow, b.lo.z - grow);
    b.hi = v3_make(b.hi.x + grow, b.hi.y + grow, b.hi.z + grow);
    return b;
}

// the cells a body's records occupy: [x0, x1] x [y0, y1] x [z0, z1], at most two per axis (k_rc_insert's rule; the
// overlap query recomputes it to find the first cell a body shares with a query)
struct RcCells {
    int x0, x1, y0, y1, z0, z1;
};
__device__ __forceinline__ RcCells rc_body_cells(const RcGrid& g, const aabb_t& b) {
    RcCells c;
    c.x0 = rc_coord(b.lo.x - g.pad, g.lox, g.inv, g.nx); c.x1 = min(rc_coord(b.hi.x + g.pad, g.lox, g.inv, g.nx), c.x0 + 1);
    c.y0 = rc_coord(b.lo.y - g.pad, g.loy, g.inv, g.ny); c.y1 = min(rc_coord(b.hi.y + g.pad, g.loy, g.inv, g.ny), c.y0 + 1);
    c.z0 = rc_coord(b.lo.z - g.pad, g.loz, g.inv, g.nz); c.z1 = min(rc_coord(b.hi.z + g.pad, g.loz, g.inv, g.nz), c.z0 + 1);
    return c;
}

struct RayHit {
    float t;
    uint32_t id;
    float nx, ny, nz;
};

__device__ __forceinline__ bool rc_better(float t, uint32_t id, const RayHit& b) { return t < b.t || (t == b.t && id < b.id); }

// --- exact ray tests. p: the origin relative to the shape's centre, u: the unit direction. An origin inside the closed
// shape gives t = 0 and n = -u; otherwise n is the outward unit normal at the hit. false: missed.

// the closed ball of radius r
__device__ __forceinline__ bool ray_ball(float px, float py, float pz, float ux, float uy, float uz, float r, float& t, float& nx,
                                         float& ny, float& nz) {
    const float bb = (px * ux + py * uy) + pz * uz;
    const float cc = ((px * px + py * py) + pz * pz) - r * r;
    if (cc <= 0.0f) {  // origin inside the closed ball
        t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        return true;
    }
    if (bb >= 0.0f) return false;  // outside and moving away
    // distance of the line from the centre without cancellation: |p - (p.u) u|^2
    const float lx = px - bb * ux, ly = py - bb * uy, lz = pz - bb * uz;
    const float disc = r * r - ((lx * lx + ly * ly) + lz * lz);
    if (disc < 0.0f) return false;
    const float q = -bb + sqrtf(disc);  // the far root (> 0); the near one is cc / q (no cancellation)
    t = cc / q;
    const float hx = px + t * ux, hy = py + t * uy, hz = pz + t * uz;
    const float inv = 1.0f / sqrtf((hx * hx + hy * hy) + hz * hz);
    nx = hx * inv; ny = hy * inv; nz = hz * inv;
    return true;
}

// the closed capsule of radius r around the core +- hl * w (w unit): the finite cylinder's side, then the two end balls;
// the first hit of the union is the least of their first hits (a ray that enters through a flat end of the cylinder has
// hit the ball there already)
__device__ __forceinline__ bool ray_capsule(float px, float py, float pz, float ux, float uy, float uz, float wx, float wy, float wz,
                                            float r, float hl, float& t, float& nx, float& ny, float& nz) {
    const float rr = r * r;
    const float pd = (px * wx + py * wy) + pz * wz;
    const float sp = fminf(fmaxf(pd, -hl), hl);
    const float qx = px - sp * wx, qy = py - sp * wy, qz = pz - sp * wz;
    if ((qx * qx + qy * qy) + qz * qz <= rr) {  // origin inside the closed capsule
        t = 0.0f; nx = -ux; ny = -uy; nz = -uz;
        return true;
    }
    t = __builtin_inff();
    // side: the components of p and u across the axis
    const float ud = (ux * wx + uy * wy) + uz * wz;
    const float ax = ux - ud * wx, ay = uy - ud * wy, az = uz - ud * wz;
    const float bx = px - pd * wx, by = py - pd * wy, bz = pz - pd * wz;
    const float A = (ax * ax + ay * ay) + az * az;
    const float B = (ax * bx + ay * by) + az * bz;
    const float C = ((bx * bx + by * by) + bz * bz) - rr;
    if (A > 1.0e-12f && B < 0.0f) {
        // B^2 - A C = A (r^2 - |l|^2), l = b - (B / A) a the part of b across the ray: as in ray_ball, the distance of the
        // line from the axis without cancellation (B^2 and A C are both |p|^2-sized: from 200 away their difference had
        // lost all but two digits of a radius of 0.5)
        const float s = B / A;
        const float lx = bx - s * ax, ly = by - s * ay, lz = bz - s * az;
        const float disc = A * (rr - ((lx * lx + ly * ly) + lz * lz));
        if (disc >= 0.0f) {
            const float q = -B + sqrtf(disc);  // > 0; the near root is C / q (no cancellation)
            const float tc = C / q;
            if (tc >= 0.0f && fabsf(pd + tc * ud) <= hl) t = tc;
        }
    }
    // end balls at -hl w and +hl w (the ray-ball test above)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float s = e == 0 ? -hl : hl;
        const float ex = px - s * wx, ey = py - s * wy, ez = pz - s * wz;
        const float bb = (ex * ux + ey * uy) + ez * uz;
        const float cc = ((ex * ex + ey * ey) + ez * ez) - rr;
        if (bb < 0.0f) {
            const float lx = ex - bb * ux, ly = ey - bb * uy, lz = ez - bb * uz;
            const float disc = rr - ((lx * lx + ly * ly) + lz * lz);
            if (disc >= 0.0f) t = fminf(t, cc / (-bb + sqrtf(disc)));
        }
    }
    if (!(t < __builtin_inff())) return false;  // missed
    // normal: from the closest point of the core to the hit
    const float hx = px + t * ux, hy = py + t * uy, hz = pz + t * uz;
    const float sh = fminf(fmaxf((hx * wx + hy * wy) + hz * wz, -hl), hl);
    const float dx = hx - sh * wx, dy = hy - sh * wy, dz = hz - sh * wz;
    const float inv = 1.0f / sqrtf((dx * dx + dy * dy) + dz * dz);
    nx = dx * inv; ny = dy * inv; nz = dz * inv;
    return true;
}

// the closed box [-h, h] in its own frame: l = origin, d = direction, both in that frame. 0: missed, 1: origin inside,
// 2: hit at t through the face of local outward normal (sx, sy, sz) (the slab the ray enters last; ties x, then y, then z)
__device__ __forceinline__ int ray_box_local(float lx, float ly, float lz, float dx, float dy, float dz, float hx, float hy, float hz,
                                             float& t, float& sx, float& sy, float& sz) {
    if (fabsf(lx) <= hx && fabsf(ly) <= hy && fabsf(lz) <= hz) { t = 0.0f; return 1; }  // origin inside the closed box
    // slabs; an axis the ray is parallel to either always holds the ray (|l| <= h) or never (the box is missed)
    const bool px0 = dx == 0.0f, py0 = dy == 0.0f, pz0 = dz == 0.0f;
    if ((px0 && fabsf(lx) > hx) || (py0 && fabsf(ly) > hy) || (pz0 && fabsf(lz) > hz)) return 0;
    const float ix = 1.0f / dx, iy = 1.0f / dy, iz = 1.0f / dz;
    // entering face of each slab: the one facing the ray (-sign(d) h)
    const float ex = px0 ? -3.0e38f : (dx > 0.0f ? (-hx - lx) : (hx - lx)) * ix;
    const float fx = px0 ? 3.0e38f : (dx > 0.0f ? (hx - lx) : (-hx - lx)) * ix;
    const float ey = py0 ? -3.0e38f : (dy > 0.0f ? (-hy - ly) : (hy - ly)) * iy;
    const float fy = py0 ? 3.0e38f : (dy > 0.0f ? (hy - ly) : (-hy - ly)) * iy;
    const float ez = pz0 ? -3.0e38f : (dz > 0.0f ? (-hz - lz) : (hz - lz)) * iz;
    const float fz = pz0 ? 3.0e38f : (dz > 0.0f ? (hz - lz) : (-hz - lz)) * iz;
    const float tn = fmaxf(ex, fmaxf(ey, ez));
    const float tf = fminf(fx, fminf(fy, fz));
    if (!(tn <= tf) || tf < 0.0f || tn < 0.0f) return 0;
    t = tn;
    const bool ax = ex == tn, ay = !ax && ey == tn, az = !ax && !ay;
    sx = ax ? (dx > 0.0f ? -1.0f : 1.0f) : 0.0f;
    sy = ay ? (dy > 0.0f ? -1.0f : 1.0f) : 0.0f;
    sz = az ? (dz > 0.0f ? -1.0f : 1.0f) : 0.0f;
    return 2;
}

// core axis of a capsule's rotation: column 1 of R (R.m[1], R.m[4], R.m[7] of quat_to_m33)
__device__ __forceinline__ void rc_capsule_axis(float4 q4, float& wx, float& wy, float& wz) {
    const float qi = q4.x, qj = q4.y, qk = q4.z, qw = q4.w;
    wx = (qi * qj * 2.0f) - (qw * qk * 2.0f);
    wy = (((qw * qw) - (qi * qi)) + (qj * qj)) - (qk * qk);
    wz = (qw * qi * 2.0f) + (qj * qk * 2.0f);
}

// --- what the capsule query kernels share (k_slide, k_character, k_depen: one capsule per lane, hit slots iteration-major)

// a lane's query as they load it: its mask (0xFFFF without filtering), where it stands and, with MOTION, its motion (zero
// otherwise: depenetration has none), radius and half-length, the body it never reports (0xFFFFFFFF: none, also for an id that
// is no owned body's), rot as given or the identity; the loads in the order the three kernels made them
struct CapsuleQuery {
    uint32_t qm;
    v3 p, m;
    float rad, hq;
    uint32_t ign;
    quat q;
};
template <bool FILT, bool MOTION>
__device__ __forceinline__ CapsuleQuery capsule_query(uint32_t i, const QueryFilters& qf, const float* __restrict__ pos,
                                                      const float* __restrict__ motion, const float* __restrict__ rot,
                                                      const float* __restrict__ radius, const float* __restrict__ half_length,
                                                      const uint32_t* __restrict__ ignore_body, uint32_t n_bodies) {
    CapsuleQuery c;
    c.qm = FILT ? (uint32_t)qf.query_mask[i] : 0xFFFFu;
    c.p = ld3(pos, i);
    c.m = v3_make(0.0f, 0.0f, 0.0f);
    if constexpr (MOTION) c.m = ld3(motion, i);
    c.rad = radius[i]; c.hq = half_length[i];
    c.ign = ignore_body && ignore_body[i] < n_bodies ? ignore_body[i] : 0xFFFFFFFFu;
    c.q.i = 0.0f; c.q.j = 0.0f; c.q.k = 0.0f; c.q.w = 1.0f;
    if (rot) { c.q.i = rot[4 * (size_t)i]; c.q.j = rot[4 * (size_t)i + 1]; c.q.k = rot[4 * (size_t)i + 2]; c.q.w = rot[4 * (size_t)i + 3]; }
    return c;
}

// one slot (a hit, or the character's floor): id, normal and a last value - the touched point, or the depth for
// depenetration - each where its array is wanted
__device__ __forceinline__ void slot_put(float* a, size_t at, v3 v) { a[3 * at] = v.x; a[3 * at + 1] = v.y; a[3 * at + 2] = v.z; }
__device__ __forceinline__ void slot_put(float* a, size_t at, float v) { a[at] = v; }
template <typename T>
__device__ __forceinline__ void query_slot(uint32_t* body, float* normal, float* last, size_t at, uint32_t id, v3 n, T v) {
    if (body) body[at] = id;
    if (normal) slot_put(normal, at, n);
    if (last) slot_put(last, at, v);
}
// the kernels write every slot: of the `count` slots of query i of n that begin at slot `first`, those from `used` on, which no
// round used, are empty (`zero`: the last value's)
template <typename T>
__device__ __forceinline__ void query_slots_empty(uint32_t* body, float* normal, float* last, uint32_t first, uint32_t used,
                                                  uint32_t count, uint32_t n, uint32_t i, T zero) {
    for (uint32_t e = used; e < count; ++e)
        query_slot(body, normal, last, (size_t)(first + e) * n + i, kRayMiss, v3_make(0.0f, 0.0f, 0.0f), zero);
}

// host: what a query kernel takes of the world, as launch_query_grid has just left it: the grid (header, log2 of the bucket
// table, bucket starts, records), the ground, the statics' records. The kernels take the members as plain arguments.
struct QueryGrid {
    const RcHeader* hdr;
    uint32_t bits;
    const uint32_t* start;
    const float4* rec;
    uint32_t n_bodies;
    int ground;
    float ground_y;
    const float4* st_rec;
    uint32_t n_static;
};
inline int32_t query_grid(phys_world* w, const float* grow_radius, const float* grow_half_length, uint64_t n_grow, QueryGrid* g,
                          const float* grow_half_extent = nullptr) {
    uint32_t bits = 12;
    PHYS_TRY(launch_query_grid(w, grow_radius, grow_half_length, n_grow, &bits, grow_half_extent));
    *g = {reinterpret_cast<const RcHeader*>(w->rc_header.p), bits, (const uint32_t*)w->rc_start.p,
          reinterpret_cast<const float4*>(w->rc_records.p), (uint32_t)w->n_owned, (w->cfg.flags & PHYS_FLAG_GROUND_PLANE) ? 1 : 0,
          w->cfg.ground_height, reinterpret_cast<const float4*>(w->st_rc.p), (uint32_t)w->n_static};
    return PHYS_OK;
}
inline unsigned rc_blocks(uint64_t n) { return (unsigned)((n + kRcThreads - 1) / kRcThreads); }

}  // namespace
}  // namespace phys
