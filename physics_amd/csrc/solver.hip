// solver.hip — sequential-impulse contact solver for gfx950. No reference
// counterpart; the arithmetic is include/spec/contact_solve.h (solver_prep / solve_manifold).
//
// Order of work = the spec's: iterations outermost, colours ascending, manifolds of one colour in
// parallel (they share no body, so there are no float atomics and the result is independent of the
// schedule), points of a manifold in index order inside one lane.
//
// Row storage: after colouring, manifolds are renumbered colour-major (row d = colour start + slot in
// colour). Everything a solve needs per row is kept as 16-BYTE elements in plane-major arrays over d (stride =
// cap), so a lane fetches a row with ~10 dwordx4 loads (a wave: 1 KiB contiguous per load) instead of ~45
// dword loads - the row solve is a long dependent chain at one wave per SIMD, and the number of memory
// instructions in front of it is what its latency is made of. The planes and what each element holds: records.hpp
// (the prepared rows).
// Only the body velocities (32-byte records) and the inverse inertia are gathered by body id.
// Algorithmic bytes per manifold per iteration: ids, count, normal 24 + per point 40 (rA, rB,
// masses, bias) + 12 R + 12 W (accumulated impulses), + per body 48 (v, w R+W) + 4 (inv mass) + 12 / 36
// (inverse inertia diagonal / full).
#include <cstdlib>

#include "handoff.hpp"

namespace phys {

// warm starting (contact_solve.h): where the impulses a solve ends with go, and where a row's starting impulses come from
struct WarmJob {
    const uint32_t* man_prev;  // null: warm starting is off (rows start from zero, no sweep 0); otherwise only a flag
    const float* geo_prev;     // 128-byte manifold records of the previous update
    const float* imp_prev;     // 12 floats per manifold: what its solve ended with
    float* imp;                // this update's (written by the last sweep of whichever solver kernel runs)
    const uint32_t* row_src;   // row -> manifold
};
__device__ __forceinline__ void store_final_impulses(const WarmJob& wj, uint32_t d, const solver_manifold_t& sm) {
    const float pn[4] = {sm.row[0].pn, sm.row[1].pn, sm.row[2].pn, sm.row[3].pn};
    const float pt0[4] = {sm.row[0].pt[0], sm.row[1].pt[0], sm.row[2].pt[0], sm.row[3].pt[0]};
    const float pt1[4] = {sm.row[0].pt[1], sm.row[1].pt[1], sm.row[2].pt[1], sm.row[3].pt[1]};
    float4 o0, o1, o2;
    impulses_pack(pn, pt0, pt1, o0, o1, o2);
    float4* o = reinterpret_cast<float4*>(wj.imp) + kImpulseVecs * (size_t)wj.row_src[d];
    o[0] = o0; o[1] = o1; o[2] = o2;
}
// ... and lane q of a four-lane kernel: point q's three floats of that record (zeros beyond the count)
__device__ __forceinline__ void store_final_point_impulses(const WarmJob& wj, uint32_t d, uint32_t q, v3 imp) {
    st3(wj.imp + kImpulseFloats * (size_t)wj.row_src[d] + impulses_point_offset(q), 0, imp);
}

struct RowArrays {
    float4* all;  // the kRowPlanes planes in one piece: plane p of row d = all[p * cap + d]; below, where its groups begin (records.hpp)
    uint4* hdr;
    float4* n;
    float4* pt;
    float4* tb;
    float4* acc;
    uint64_t cap;
};

// MAT: the material instance. It combines the two sides' materials into the manifold's friction `mu`,
// which rides in the row (prepared rows: row_n.w, which is the cluster info and 0 outside cluster steps; compact rows: the
// whole of hdr.z, the point count moving into spare ticket bits - see cluster.hip), and gives a point that bounces the
// restitution bias of contact_solve.h. Only a row whose restitution is not zero reads more of its bodies than before.
// The material arguments travel as a parameter pack that is empty in the plain instance, which keeps its kernel
// arguments and its instructions (the technique of section 13).
template <bool DIAG, bool MAT, typename... Mat>
__global__ __launch_bounds__(256) void k_rows_build(StepCounters* __restrict__ ctr, RowArrays rows, solve_params_t sp,
                                                    const uint32_t* __restrict__ row_src,
                                                    const float* __restrict__ man_geo /* 128-byte records */,
                                                    const float* __restrict__ pos,
                                                    const float* __restrict__ vel,
                                                    const float* __restrict__ inv_inertia, uint32_t inertia_stride,
                                                    const uint32_t* __restrict__ man_color,
                                                    const unsigned long long* __restrict__ used,
                                                    int flow /* 1: k_solve_flow runs this step (tickets, no zeroed impulses) */,
                                                    ColorTableJob table, const uint32_t* __restrict__ cluster_slot,
                                                    const uint32_t* __restrict__ body_shared,
                                                    uint32_t cluster_slots /* 0: not a cluster-solver step */, uint32_t cluster_count,
                                                    WarmJob warm, Mat... mat /* MAT: one RowMaterials */) {
    static_assert(sizeof...(Mat) == (MAT ? 1u : 0u), "one RowMaterials argument exactly in the material instance");
    RowMaterials mt{};
    if constexpr (MAT) mt = material_arg(mat...);
    if (ctr->overflow) return;  // never solve a truncated set; phys_sync / phys_get_stats report it
    const uint32_t M = ctr->n_manifolds;
    const uint64_t cap = rows.cap;
    for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < M; d += gridDim.x * blockDim.x) {
        const uint32_t m = row_src[d];
        manifold_t g;
        const float4* rec = reinterpret_cast<const float4*>(man_geo) + kManifoldVecs * (size_t)m;  // ONE line through the row permutation
        const float4 r1 = rec[kManifoldVecNormal];
        const ManifoldHead head = manifold_head_decode(rec[kManifoldVecHead]);
        const uint32_t a = head.a, b = head.b;
        g.count = (int)head.count;
        g.normal = v3_make(r1.x, r1.y, r1.z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 p = rec[kManifoldVecPoint + k];
            g.pt[k] = v3_make(p.x, p.y, p.z);
            g.depth[k] = p.w;
        }
        const int has_b = !PHYS_IS_STATIC_PARTNER(b);
        // warm starting: the impulses this row starts from = what the same pair's manifold of the previous update ended
        // with, matched point by point (contact_solve.h warm_match); zero for a new pair or with warm starting off
        float w_pn[4] = {0.0f, 0.0f, 0.0f, 0.0f}, w_pt0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, w_pt1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (warm.man_prev) {
            const uint32_t pm = manifold_prev_index(r1);  // index of the pair's manifold in the previous update (narrow phase)
            if (pm != kNoPrevManifold) {
                const float4* prec = reinterpret_cast<const float4*>(warm.geo_prev) + kManifoldVecs * (size_t)pm;
                const float4* pimp = reinterpret_cast<const float4*>(warm.imp_prev) + kImpulseVecs * (size_t)pm;
                const float4 q0 = prec[kManifoldVecHead], q1 = prec[kManifoldVecNormal], i0 = pimp[0], i1 = pimp[1], i2 = pimp[2];
                warm_t wt;
                wt.count = (int)manifold_head_decode(q0).count;
                wt.normal = v3_make(q1.x, q1.y, q1.z);
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float4 p = prec[kManifoldVecPoint + k]; wt.pt[k] = v3_make(p.x, p.y, p.z); }
                impulses_unpack(i0, i1, i2, wt.pn, wt.pt0, wt.pt1);
                warm_match(&g, &wt, w_pn, w_pt0, w_pt1);
            }
        }
        // persistent colouring: a manifold that is new in this update enters the colour table (kernels.hpp)
        if (table.tab && (table.all || head.color == kUncolored)) color_table_insert(table, a, b, m, ctr);
        // a kept colour came with the record; a new manifold's was made by the colouring rounds since
        const uint32_t color_m = head.color != kUncolored ? head.color : man_color[m];
        uint32_t ticket = 0;  // the ticket word (records.hpp)
        if (flow) {
            // the colours in use at a body are exactly the colours of its manifolds (all distinct), so the rank of
            // this row among the body's manifolds in solve order = number of its colours below this one
            const unsigned long long below = (1ull << color_m) - 1ull;
            const unsigned long long ua = used[a];
            RowTicket tk{(uint32_t)__popcll(ua & below), (uint32_t)__popcll(ua), 0u, 0u};
            if (has_b) {
                const unsigned long long ub = used[b];
                tk.rankB = (uint32_t)__popcll(ub & below); tk.degB = (uint32_t)__popcll(ub);
            }
            ticket = ticket_encode(tk);
            if (flow == 2 && d == 0) ticket += 1;  // fault injection (PHYS_DEBUG_FLOW_STALL): row 0 waits for a turn that never comes
        }
        // materials: the manifold's friction and restitution; a row that bounces needs the velocities the solve starts from
        float mu = 0.0f, rest = 0.0f;
        v3 m_xA = v3_make(0.0f, 0.0f, 0.0f), m_vA = m_xA, m_wA = m_xA, m_xB = m_xA, m_vB = m_xA, m_wB = m_xA;
        if constexpr (MAT) {
            const float2 ma = mt.body[a];
            // (three assignments, not one conditional expression: that selects between ADDRESSES, and the argument struct
            // went to scratch memory for it)
            float2 mb = mt.ground;
            if (has_b) mb = mt.body[b];
            else if (b != PHYS_GROUND_ID) mb = mt.st[b & ~PHYS_STATIC_ID_BIT];
            mu = material_friction(ma.x, mb.x);
            rest = material_restitution(ma.y, mb.y);
            if (rest > 0.0f) {
                const BodyVel A = ld_vel(vel, a);
                m_xA = ld3(pos, a); m_vA = A.v; m_wA = A.w;
                if (has_b) { const BodyVel B = ld_vel(vel, b); m_xB = ld3(pos, b); m_vB = B.v; m_wB = B.w; }
            }
        }
        // bias of point k (contact_solve.h); rB = 0 for a body B that does not move, as solver_prep has it
        auto point_bias = [&](v3 pt, float depth) -> float {
            if constexpr (MAT) {
                if (rest > 0.0f) {
                    const v3 rA = v3_sub(pt, m_xA);
                    const v3 rB = has_b ? v3_sub(pt, m_xB) : v3_make(0.0f, 0.0f, 0.0f);
                    const float vn = contact_normal_velocity(g.normal, m_vA, m_wA, rA, m_vB, m_wB, rB);
                    return contact_bias_restitution(depth, vn, rest, mt.threshold, &sp);
                }
            }
            return contact_bias(depth, &sp);
        };
        if constexpr (MAT) {
            if (cluster_slots)  // compact rows: mu takes hdr.z; the count rides in the ticket word
                rows.hdr[d] = make_uint4(a, b, __float_as_uint(mu), ticket_with_count(ticket, (uint32_t)g.count));
            else
                rows.hdr[d] = make_uint4(a, b, (uint32_t)g.count, ticket);
        } else {
            rows.hdr[d] = make_uint4(a, b, (uint32_t)g.count, ticket);
        }
        uint32_t info = 0;
        if (cluster_slots) {
            // cluster solver (cluster.hip): where each side's velocity lives - the side word (records.hpp).
            // publish: the body's NEXT update in solve order (next colour in use at the body, cyclically) belongs to a
            // remote row, so this update must be written to the granules for it
            const unsigned long long bitc = 1ull << color_m;
            const uint32_t ha = cluster_home(cluster_slot, a, cluster_slots);
            const uint32_t hb = has_b ? cluster_home(cluster_slot, b, cluster_slots) : kNoHome;
            const uint32_t owner = cluster_row_owner(a, ha, hb, cluster_count);
            // one side: {slot | publish | mode} of body x whose home is `hx`
            auto side = [&](uint32_t x, uint32_t hx) -> uint32_t {
                if (hx != owner) return cluster_side_encode(0u, 0u, kSideForeign);  // homeless, or at home elsewhere
                const unsigned long long rem = ((unsigned long long)body_shared[2 * (size_t)x + 1] << 32) | body_shared[2 * (size_t)x];
                uint32_t pub = 0;
                if (rem) {
                    const unsigned long long ux = used[x];
                    const unsigned long long above = ux & ~(bitc | (bitc - 1ull));
                    const unsigned long long next = above ? (above & (~above + 1ull)) : (ux & (~ux + 1ull));  // lowest colour above, else the first
                    pub = (rem & next) ? 1u : 0u;
                }
                return cluster_side_encode(cluster_slot[x] - hx * cluster_slots, pub, rem ? kSideShared : kSideOwn);
            };
            info = cluster_sides_encode(side(a, ha), has_b ? side(b, hb) : cluster_side_encode(0u, 0u, kSideNone));
        }
        if constexpr (MAT) rows.n[d] = make_float4(g.normal.x, g.normal.y, g.normal.z, cluster_slots ? __uint_as_float(info) : mu);
        else rows.n[d] = make_float4(g.normal.x, g.normal.y, g.normal.z, __uint_as_float(info));
        if (cluster_slots) {
            // compact rows of the cluster solver (cluster.hip): the contact points themselves and the bias; lever arms and
            // row masses are remade there from the body positions it keeps in LDS. Nothing of the bodies is read here.
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < g.count)
                    rows.all[(size_t)(kClusterPlaneGeo + k) * cap + d] = make_float4(g.pt[k].x, g.pt[k].y, g.pt[k].z, MAT ? point_bias(g.pt[k], g.depth[k]) : contact_bias(g.depth[k], &sp));
            if (warm.man_prev) {  // the starting impulses, packed like the solver packs them (read in sweep 0)
                float4 a0, a1, a2;
                impulses_pack(w_pn, w_pt0, w_pt1, a0, a1, a2);
                rows.all[(size_t)(kClusterPlaneAcc + 0) * cap + d] = a0;
                rows.all[(size_t)(kClusterPlaneAcc + 1) * cap + d] = a1;
                rows.all[(size_t)(kClusterPlaneAcc + 2) * cap + d] = a2;
            }
            if (cluster_side_rides(info, true)) {
                // body B belongs to another cluster: what does not change during the solve rides with the row, or fetching
                // it by body id would be a second dependent round trip in every colour step of the solver
                const v3 xb = ld3(pos, b);
                rows.all[(size_t)kClusterPlaneForeignB * cap + d] = make_float4(xb.x, xb.y, xb.z, vel[8 * (size_t)b + 3]);
                if (DIAG) rows.all[(size_t)(kClusterPlaneForeignB + 1) * cap + d] = reinterpret_cast<const float4*>(inv_inertia)[b * inertia_stride];
            }
            if (cluster_side_rides(info, false)) {
                // body A has no home (dynamic clusters beyond their capacity): the same for A
                const v3 xa = ld3(pos, a);
                rows.all[(size_t)kClusterPlaneForeignA * cap + d] = make_float4(xa.x, xa.y, xa.z, vel[8 * (size_t)a + 3]);
                if (DIAG) rows.all[(size_t)(kClusterPlaneForeignA + 1) * cap + d] = reinterpret_cast<const float4*>(inv_inertia)[a * inertia_stride];
            }
            continue;
        }
        // DIAG: 16 bytes per body instead of 36 (and none at all when every body shares one tensor: stride 0);
        // the zero off-diagonals are put back, so solver_prep's arithmetic is the general path's
        const m33 IA = ld_inertia<DIAG>(inv_inertia, a * inertia_stride);
        m33 IB;
#pragma unroll
        for (int k = 0; k < 9; ++k) IB.m[k] = 0.0f;
        float imb = 0.0f;
        v3 xB = v3_make(0.0f, 0.0f, 0.0f);
        if (has_b) { IB = ld_inertia<DIAG>(inv_inertia, b * inertia_stride); imb = vel[8 * (size_t)b + 3]; xB = ld3(pos, b); }
        solver_manifold_t sm;
        solver_prep(&g, has_b, ld3(pos, a), xB, vel[8 * (size_t)a + 3], &IA, imb, &IB, &sp, &sm);
        if constexpr (MAT) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < sm.count) sm.row[k].bias = point_bias(g.pt[k], g.depth[k]);
        }
        RowPoint rp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const contact_row_t& c = sm.row[k];
            rp[k] = RowPoint{{c.rA.x, c.rA.y, c.rA.z}, {c.rB.x, c.rB.y, c.rB.z}, c.normal_mass, c.tangent_mass[0], c.tangent_mass[1], c.bias};
            if (k < sm.count) {
                float4 pa, pb;
                row_point_encode(rp[k], pa, pb);
                rows.pt[(size_t)row_pt_plane_a(k) * cap + d] = pa;
                rows.pt[(size_t)row_pt_plane_b(k) * cap + d] = pb;
                // accumulated impulses of point k: zero, or where the previous update left off. (The dataflow kernels read
                // these with plain loads in their first sweep only when warm starting is on; tag 0 = no epoch ever.)
                if (!flow || warm.man_prev) rows.acc[(size_t)k * cap + d] = make_float4(w_pn[k], w_pt0[k], w_pt1[k], 0.0f);
            }
        }
        float4 t01, t23;
        row_tb_encode(rp[0], rp[1], t01);
        row_tb_encode(rp[2], rp[3], t23);
        rows.tb[(size_t)row_tb_plane(0) * cap + d] = t01;
        if (sm.count > 2) rows.tb[(size_t)row_tb_plane(2) * cap + d] = t23;
    }
}

// one manifold row d of the colour-major numbering, in registers
struct RowRegs {
    uint32_t a, b, ticket;
    solver_manifold_t sm;
};
// ... and as its planes come from memory: header, normal, the two tb planes, the eight pt planes
struct FlowRowRaw { uint4 h; float4 nn, t01, t23, p[8]; };

// The ONE unpack of a prepared row: everything of it that does not depend on body velocities. ACC: with the accumulated
// impulses out of the acc elements of its points; otherwise they start at zero and `acc` is not looked at (k_solve_flow
// receives them as tagged granules). Elements of points beyond the count are not looked at either. live = false: a lane
// without a row (no points, no body B). (A template flag, not a pointer that may be null: the arrays went to scratch memory for that.)
template <bool ACC>
__device__ __forceinline__ void row_unpack(const FlowRowRaw& raw, const float4 (&acc)[4], bool live, RowRegs& R) {
    R.a = raw.h.x; R.b = raw.h.y; R.ticket = raw.h.w;
    solver_manifold_t& sm = R.sm;
    sm.count = live ? (int)raw.h.z : 0;
    sm.has_b = live && !PHYS_IS_STATIC_PARTNER(R.b);
    sm.n = v3_make(raw.nn.x, raw.nn.y, raw.nn.z);
    if (!live) sm.n = v3_make(0.0f, 1.0f, 0.0f);
    tangent_basis(sm.n, &sm.t1, &sm.t2);  // same inputs as solver_prep => same bits as the basis used there
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        contact_row_t& c = sm.row[k];
        if (k < sm.count) {
            const RowPoint p = row_point_decode(k, raw.p[row_pt_plane_a(k)], raw.p[row_pt_plane_b(k)], row_tb_plane(k) == 0 ? raw.t01 : raw.t23);
            c.rA = v3_make(p.rA[0], p.rA[1], p.rA[2]); c.normal_mass = p.normal_mass;
            c.rB = v3_make(p.rB[0], p.rB[1], p.rB[2]); c.tangent_mass[0] = p.tangent_mass0;
            c.tangent_mass[1] = p.tangent_mass1;
            c.bias = p.bias;
            if (ACC) { c.pn = acc[k].x; c.pt[0] = acc[k].y; c.pt[1] = acc[k].z; }
            else { c.pn = 0.0f; c.pt[0] = 0.0f; c.pt[1] = 0.0f; }
        } else {
            c.pn = 0.0f; c.pt[0] = 0.0f; c.pt[1] = 0.0f;
            c.rA = v3_make(0.0f, 0.0f, 0.0f); c.rB = v3_make(0.0f, 0.0f, 0.0f);
            c.normal_mass = 0.0f; c.tangent_mass[0] = 0.0f; c.tangent_mass[1] = 0.0f; c.bias = 0.0f;
        }
    }
}

// row d from memory. ACC: also the accumulated impulses (plain loads; k_solve_flow receives them as tagged granules instead)
// EAGER: every plane of the row is fetched at once, whatever the point count turns out to be (planes beyond it hold
// stale but readable data that is then ignored): no load waits for the header. For the per-colour kernel of large
// scenes, where a launch is one wave per SIMD and a second dependent round trip to memory is ~1.5 us of every launch.
// Returns the normal element's .w: the manifold's friction where the material instance of k_rows_build wrote the row (0 in plain rows).
template <bool ACC, bool EAGER = false>
__device__ __forceinline__ float load_row(RowRegs& R, uint32_t d, const RowArrays& rows) {
    const uint64_t cap = rows.cap;
    FlowRowRaw raw;  // (elements of points beyond the count stay unset: row_unpack does not look at them)
    float4 acc[4], e_t23;
    if (EAGER) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            raw.p[row_pt_plane_a(k)] = rows.pt[(size_t)row_pt_plane_a(k) * cap + d];
            raw.p[row_pt_plane_b(k)] = rows.pt[(size_t)row_pt_plane_b(k) * cap + d];
            if (ACC) acc[k] = rows.acc[(size_t)k * cap + d];
        }
        e_t23 = rows.tb[(size_t)row_tb_plane(2) * cap + d];
    }
    raw.h = rows.hdr[d];
    raw.nn = rows.n[d];
    raw.t01 = rows.tb[(size_t)row_tb_plane(0) * cap + d];
    const int count = (int)raw.h.z;
    raw.t23 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (count > 2) raw.t23 = EAGER ? e_t23 : rows.tb[(size_t)row_tb_plane(2) * cap + d];
    if (!EAGER) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < count) {
                raw.p[row_pt_plane_a(k)] = rows.pt[(size_t)row_pt_plane_a(k) * cap + d];
                raw.p[row_pt_plane_b(k)] = rows.pt[(size_t)row_pt_plane_b(k) * cap + d];
                if (ACC) acc[k] = rows.acc[(size_t)k * cap + d];
            }
        }
    }
    row_unpack<ACC>(raw, acc, true, R);
    return raw.nn.w;
}

// gather the two bodies, solve_manifold, write velocities and accumulated impulses back
// MAT: the friction is the row's own, not the kernel argument
template <bool DIAG, bool EAGER = false, bool MAT = false>
__device__ __forceinline__ void solve_row(uint32_t d, const RowArrays& rows, float friction,
                                          const float* __restrict__ inv_inertia,
                                          uint32_t inertia_stride /* 0: one tensor shared by every body */,
                                          float* __restrict__ vel, int apply_only /* sweep 0 of a warm-started solve */,
                                          int last /* the solve's last sweep: the impulses are remembered */, const WarmJob& wj) {
    RowRegs R;
    const float row_mu = load_row<true, EAGER>(R, d, rows);
    solver_manifold_t& sm = R.sm;
    const uint32_t a = R.a, b = R.b;
    const m33 IA = ld_inertia<DIAG>(inv_inertia, a * inertia_stride);
    BodyVel A = ld_vel(vel, a);
    const float ima = A.inv_mass;
    v3 vA = A.v, wA = A.w;
    m33 IB;
#pragma unroll
    for (int k = 0; k < 9; ++k) IB.m[k] = 0.0f;
    float imb = 0.0f;
    v3 vB = v3_make(0.0f, 0.0f, 0.0f), wB = v3_make(0.0f, 0.0f, 0.0f);
    BodyVel B = A;
    if (sm.has_b) { IB = ld_inertia<DIAG>(inv_inertia, b * inertia_stride); B = ld_vel(vel, b); imb = B.inv_mass; vB = B.v; wB = B.w; }
    // rows made on the way: these kernels are throughput-bound and want the registers (k_solve_flow makes them all
    // beforehand, while it waits; same arithmetic)
    solve_manifold_lazy(&sm, MAT ? row_mu : friction, ima, &IA, imb, &IB, &vA, &wA, &vB, &wB, apply_only);
    A.v = vA; A.w = wA;
    st_vel(vel, a, A);
    if (sm.has_b) { B.v = vB; B.w = wB; st_vel(vel, b, B); }
    if (!apply_only) {  // (sweep 0 changes no impulse)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < sm.count)
                rows.acc[(size_t)k * rows.cap + d] = make_float4(sm.row[k].pn, sm.row[k].pt[0], sm.row[k].pt[1], 0.0f);
    }
    if (last && wj.man_prev) store_final_impulses(wj, d, sm);
}

// Tiles of `tile_rows` consecutive items handed to the workgroups of a launch so that the workgroups sharing an XCD
// (equal blockIdx % 8 under the dispatcher's round-robin placement: a label, never relied on for correctness) cover
// one contiguous eighth of the range. Every tile is visited exactly once for any grid size.
struct XcdTiles {
    uint32_t tile, last, step;
    __device__ __forceinline__ XcdTiles(uint32_t items, uint32_t tile_rows) {
        const uint32_t tiles = (items + tile_rows - 1) / tile_rows;
        if (gridDim.x < 8u) {  // fewer workgroups than labels: plain striding (some labels would have nobody)
            tile = blockIdx.x; last = tiles; step = gridDim.x;
            return;
        }
        const uint32_t per = (tiles + 7u) / 8u;                       // tiles per label
        const uint32_t label = blockIdx.x & 7u, j = blockIdx.x >> 3;  // j-th workgroup of its label
        step = (gridDim.x - label + 7u) / 8u;                         // workgroups carrying this label
        tile = label * per + j;
        const uint32_t stop = (label + 1u) * per;
        last = stop < tiles ? stop : tiles;
    }
    __device__ __forceinline__ bool valid() const { return tile < last; }
    __device__ __forceinline__ void next() { tile += step; }
};

// one colour of one iteration; the row range comes from the device-side colour table
template <bool DIAG, bool MAT>
__global__ __launch_bounds__(256) void k_solve_color(const StepCounters* __restrict__ ctr, uint32_t col, RowArrays rows,
                                                     float friction, const float* __restrict__ inv_inertia,
                                                     uint32_t inertia_stride, float* __restrict__ vel, int apply_only, int last, WarmJob wj) {
    if (ctr->overflow) return;
    const uint32_t start = ctr->color_start[col], end = ctr->color_start[col + 1];
    // XCD-aware tiles: the rows of a colour are in emission (= spatial) order, so a contiguous range of them touches a
    // compact set of bodies. Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the L2 they share),
    // so the workgroups of one label take ONE contiguous eighth of the colour: the 128-byte lines of the gathered body
    // records are then fetched into one L2 instead of into all eight (PMC, C5: 22 MB of line fetches per launch for
    // 5.6 MB of gathered records when tiles were dealt in plain blockIdx order). Speed only: any mapping is correct.
    for (XcdTiles t(end - start, blockDim.x); t.valid(); t.next()) {
        const uint32_t d = start + t.tile * blockDim.x + threadIdx.x;
        if (d < end) solve_row<DIAG, true, MAT>(d, rows, friction, inv_inertia, inertia_stride, vel, apply_only, last, wj);
    }
}

// The colour classes [first, n_colours) of one iteration in ONE launch of ONE workgroup: colours in
// ascending order with a workgroup barrier between them (all waves share this CU's L1, so a barrier orders
// the body-velocity writes of one colour before the reads of the next). Same order of work as one launch per
// colour, without paying a ~8 us launch for a few hundred manifolds. `first` is a host HINT (the small
// colours of the previous step); any value gives the same result, only the speed changes.
constexpr int kTailThreads = 512;  // 2 waves per SIMD: the row solve needs >128 VGPRs, 1024 threads would spill
template <bool DIAG, bool MAT>
__global__ __launch_bounds__(kTailThreads) void k_solve_tail(const StepCounters* __restrict__ ctr, uint32_t first, RowArrays rows,
                                                            float friction, const float* __restrict__ inv_inertia,
                                                            uint32_t inertia_stride, float* __restrict__ vel, int apply_only,
                                                            int last_sweep, WarmJob wj) {
    if (ctr->overflow) return;
    const uint32_t last = ctr->n_colors;
    if (first >= last) return;
    // the colour table goes to LDS once: a scalar load from global memory per colour phase would put a full
    // memory round trip in front of every phase
    __shared__ uint32_t s_start[PHYS_MAX_COLORS + 1];
    if (threadIdx.x <= (uint32_t)PHYS_MAX_COLORS) s_start[threadIdx.x] = ctr->color_start[threadIdx.x];
    __syncthreads();
    for (uint32_t col = first; col < last; ++col) {
        const uint32_t start = s_start[col], end = s_start[col + 1];
        for (uint32_t d = start + threadIdx.x; d < end; d += kTailThreads)
            solve_row<DIAG, false, MAT>(d, rows, friction, inv_inertia, inertia_stride, vel, apply_only, last_sweep, wj);
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------
// Single-launch dataflow solver. Same arithmetic and the same ORDER OF UPDATES PER BODY as the per-colour launches (iterations
// outermost, colours ascending), so the results are bit-identical; what changes is how the order is enforced. Instead of a
// kernel boundary after every colour of every iteration (8 x n_colours dependent launches of 5-20 us), the k-th update of
// body A in solve order may only be made by the row holding ticket k for A (k = iteration * deg(A) + rank of the row's colour
// among A's colours; k_rows_build): a row waits for its bodies' tagged granules and publishes them with the next tag, and the
// accumulated impulses cross sweeps the same way (the hand-off: handoff.hpp). One hop costs ~0.7-1.0 us
// (tools/hop_bench.hip) instead of a launch, and rows of different colours / iterations overlap wherever the contact graph
// allows. Work items (iteration, chunk of blockDim rows) are handed out by an atomic ticket in solve order, so every dependency
// of an item was taken EARLIER by a workgroup that is running: no co-residency assumption, no deadlock by construction.
// Work items are SOFTWARE-PIPELINED inside a workgroup: while item k waits for its bodies and is solved, the rows of
// item k + 1 (its ticket is taken one item ahead) are already on their way, and so are - issued once those rows have
// arrived, i.e. behind the Jacobians of item k - the records of its bodies. At one wave per SIMD nobody else hides
// these two dependent round trips (~4.5 us of the ~14 us an item cost on the 1M-cube scene: 11.5k items over 256
// workgroups). A workgroup still finishes its items in ticket order, so the earliest unfinished item of the solve is
// always somebody's CURRENT item: the no-deadlock argument above holds. `pipeline` = 0 takes the next item only when
// the current one is done: holding an item ahead means it cannot go to whichever workgroup is free first, and where a
// colour class is much smaller than the launch (C3: 64 items per colour, 256 workgroups) the solve is bound by the
// chain of hand-offs, not by item throughput - there the look-ahead costs 10 % instead of saving it (launch_solver).
struct FlowBodies { m33 IA, IB; float ima, imb, massA, massB; v3 vA, wA, vB, wB; };

template <bool DIAG, bool MAT>
__global__ __launch_bounds__(256) void k_solve_flow(StepCounters* __restrict__ ctr, uint32_t iterations, uint32_t epoch,
                                                    RowArrays rows, float friction,
                                                    const float* __restrict__ inv_inertia, uint32_t inertia_stride,
                                                    float* vel, float* flow_vel, uint32_t n_bodies, long long timeout_ticks,
                                                    uint32_t pipeline, uint32_t warm_sweep /* sweep 0 applies the starting impulses;
                                                    `iterations` counts it */, WarmJob wj) {
    __shared__ uint32_t s_item;
    if (ctr->overflow) return;
    const uint32_t M = ctr->n_manifolds;
    const uint32_t nchunks = (M + blockDim.x - 1) / blockDim.x;
    const uint32_t total = nchunks * iterations;
    const uint32_t cap = (uint32_t)rows.cap;  // collision_alloc: 64 * cap < 4 GiB (32-bit buffer offsets)
    const Handoff hv = body_handoff(flow_vel, n_bodies, epoch), ha = impulse_handoff(rows.acc, cap, epoch);
    const long long t_start = wall_clock64();
    auto take = [&]() -> uint32_t {  // next work item in solve order (block-uniform)
        __syncthreads();
        if (threadIdx.x == 0) s_item = handoff_abandoned(ctr) ? 0xFFFFFFFFu : atomicAdd(&ctr->flow_ticket, 1u);
        __syncthreads();
        return s_item;
    };
    auto row_of = [&](uint32_t L) -> uint32_t {  // this lane's row of item L (>= M: none)
        if (L >= total) return 0xFFFFFFFFu;
        const uint32_t it = L / nchunks;
        return (L - it * nchunks) * blockDim.x + threadIdx.x;
    };
    auto fetch_row = [&](uint32_t d, FlowRowRaw& r) {
        // every plane at once, whatever the point count turns out to be: ONE round trip
        r.h = rows.hdr[d];
        r.nn = rows.n[d];
        r.t01 = rows.tb[(uint32_t)row_tb_plane(0) * cap + d];
        r.t23 = rows.tb[(uint32_t)row_tb_plane(2) * cap + d];
#pragma unroll
        for (int k = 0; k < kRowPtPlanes; ++k) r.p[k] = rows.pt[(size_t)k * cap + d];
    };
    auto fetch_bodies = [&](const FlowRowRaw& r, FlowBodies& g) {
        // everything of the two bodies that is constant during the solve; v, w are the body's state only for ticket 0
        g.IA = ld_inertia<DIAG>(inv_inertia, r.h.x * inertia_stride);
        const BodyVel A0 = ld_vel(vel, r.h.x);
        g.ima = A0.inv_mass; g.massA = A0.mass; g.vA = A0.v; g.wA = A0.w;
        if (!PHYS_IS_STATIC_PARTNER(r.h.y)) {
            g.IB = ld_inertia<DIAG>(inv_inertia, r.h.y * inertia_stride);
            const BodyVel B0 = ld_vel(vel, r.h.y);
            g.imb = B0.inv_mass; g.massB = B0.mass; g.vB = B0.v; g.wB = B0.w;
        }
    };
    auto clear_bodies = [&](FlowBodies& g) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { g.IA.m[k] = 0.0f; g.IB.m[k] = 0.0f; }
        g.ima = 0.0f; g.imb = 0.0f; g.massA = 0.0f; g.massB = 0.0f;
        g.vA = v3_make(0.0f, 0.0f, 0.0f); g.wA = g.vA; g.vB = g.vA; g.wB = g.vA;
    };
    auto clear_row = [&](FlowRowRaw& r) {
        r.h = make_uint4(0u, PHYS_GROUND_ID, 0u, 0u);
        r.nn = make_float4(0.0f, 0.0f, 0.0f, 0.0f); r.t01 = r.nn; r.t23 = r.nn;
#pragma unroll
        for (int k = 0; k < 8; ++k) r.p[k] = r.nn;
    };
    // prologue: the first item with its rows and bodies
    uint32_t L = take();
    FlowRowRaw raw, raw_next;
    FlowBodies bod, bod_next;
    clear_row(raw); clear_bodies(bod);
    {
        const uint32_t d0 = row_of(L);
        if (d0 < M) { fetch_row(d0, raw); fetch_bodies(raw, bod); }
    }
    while (L < total) {
        uint32_t L_next = 0xFFFFFFFFu, d_next = 0xFFFFFFFFu;
        clear_row(raw_next); clear_bodies(bod_next);
        if (pipeline) {
            L_next = take();
            d_next = row_of(L_next);
            if (d_next < M) fetch_row(d_next, raw_next);
        }
        // ---- item L: unpack the row
        const uint32_t it = L / nchunks;
        const bool last_it = it + 1 == iterations;
        const uint32_t d = (L - it * nchunks) * blockDim.x + threadIdx.x;
        bool done = d >= M;
        RowRegs R;
        float4 no_acc[4];  // (never read)
        row_unpack<false>(raw, no_acc, !done, R);
        const bool apply_only = warm_sweep != 0u && it == 0u;
        if (apply_only && !done) {  // the starting impulses k_rows_build left in the impulse planes (plain loads: an earlier kernel wrote them)
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < R.sm.count) {
                const float4 a0 = rows.acc[(size_t)k * cap + d];
                R.sm.row[k].pn = a0.x; R.sm.row[k].pt[0] = a0.y; R.sm.row[k].pt[1] = a0.z;
            }
        }
        const RowTicket tk = ticket_decode(R.ticket);
        const uint32_t rankA = tk.rankA, degA = tk.degA, rankB = tk.rankB, degB = tk.degB;
        const uint32_t tA = done ? 0u : it * degA + rankA, tB = (done || !R.sm.has_b) ? 0u : it * degB + rankB;
        const bool finalA = !done && last_it && rankA + 1 == degA, finalB = !done && R.sm.has_b && last_it && rankB + 1 == degB;
        const m33 IA = bod.IA, IB = bod.IB;
        const float ima = bod.ima, imb = bod.imb, massA = bod.massA, massB = bod.massB;
        v3 vA = bod.vA, wA = bod.wA, vB = bod.vB, wB = bod.wB;
        // the velocity-independent part of every row, while the row waits: the chain behind the wait is short
        solver_jac_t J;
        solver_jacobians(&R.sm, ima, &IA, imb, &IB, &J);
        // the rows of the next item have arrived by now (they were asked for before all of the above): its bodies
        if (pipeline && d_next < M) fetch_bodies(raw_next, bod_next);
        // what is still missing (a matched granule cannot change any more: this row is its next writer)
        bool needA = !done && tA != 0, needB = !done && R.sm.has_b && tB != 0, needAcc = !done && it != 0;
        uint32_t sweeps = 0;
        for (;;) {
            uint32_t gap = 0;
            if (!done) {
                BodyGranules a, b; u32x4 p[4];
                if (needA) a = ld_body(hv, R.a);
                if (needB) b = ld_body(hv, R.b);
                if (needAcc) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (k < R.sm.count) p[k] = ld_granule(ha.buf, impulse_granule(k, cap, d));
                }
                if (needA) needA = !take_body(hv, a, tA, vA, wA, gap);
                if (needB) { uint32_t g = 0; needB = !take_body(hv, b, tB, vB, wB, g); gap = g > gap ? g : gap; }
                if (needAcc) {
                    bool all = true;
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (k < R.sm.count) all = all && p[k].w == ha.tag(it);
                    if (all) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (k < R.sm.count) {
                            R.sm.row[k].pn = __uint_as_float(p[k].x);
                            R.sm.row[k].pt[0] = __uint_as_float(p[k].y);
                            R.sm.row[k].pt[1] = __uint_as_float(p[k].z);
                        }
                        needAcc = false;
                    } else if (gap == 0) {
                        gap = 1;
                    }
                }
                if (!needA && !needB && !needAcc) {
                    if constexpr (MAT) solve_manifold(&R.sm, &J, raw.nn.w, &vA, &wA, &vB, &wB, apply_only ? 1 : 0);  // the row's own friction
                    else solve_manifold(&R.sm, &J, friction, &vA, &wA, &vB, &wB, apply_only ? 1 : 0);
                    // publish: bodies first (they are what other rows wait for)
                    if (finalA) { BodyVel o; o.v = vA; o.inv_mass = ima; o.w = wA; o.mass = massA; st_vel(vel, R.a, o); }
                    else publish_body(hv, R.a, vA, wA, tA + 1u);
                    if (R.sm.has_b) {
                        if (finalB) { BodyVel o; o.v = vB; o.inv_mass = imb; o.w = wB; o.mass = massB; st_vel(vel, R.b, o); }
                        else publish_body(hv, R.b, vB, wB, tB + 1u);
                    }
                    if (!last_it) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) if (k < R.sm.count)
                            ha.publish(impulse_granule(k, cap, d), v3_make(R.sm.row[k].pn, R.sm.row[k].pt[0], R.sm.row[k].pt[1]), it + 1u);
                    } else if (wj.man_prev) {  // the solve's last sweep: remembered for the next update
                        store_final_impulses(wj, d, R.sm);
                    }
                    done = true;
                }
            }
            if (__all(done)) break;
            if (flow_backoff(ctr, done, gap, sweeps, t_start, timeout_ticks)) done = true;
        }
        if (!pipeline) {
            L_next = take();
            d_next = row_of(L_next);
            if (d_next < M) { fetch_row(d_next, raw_next); fetch_bodies(raw_next, bod_next); }
        }
        L = L_next;
        raw = raw_next;
        bod = bod_next;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The FOUR-LANE ROW CORE of k_solve_flow_quad and k_solve_color_quad. At one wave per SIMD the one-lane row solve is
// VALU-issue-bound (~65 instructions per row x 12 rows, ~2/3 of a hop in k_solve_flow). A row is four dot products, a
// scalar update and four axpys over {vA, wA, vB, wB}: lane q of a quad owns ONE of those vectors with its Jacobian
// column and response (made beforehand: quad_lane_setup), so a row costs each lane one dot product, two cross-lane
// adds (DPP inside the quad: no LDS), the scalar update and one axpy - about a third of the instructions
// (quad_lane_solve). The partial sums are combined in the order of the spec ((dir.vB + aB.wB) - (dir.vA + aA.wA)), so
// the bits are those of the one-lane kernels. Both kernels run this one copy; what differs is where the rows and the
// accumulated impulses come from and where the results go.
template <int CTRL>
__device__ __forceinline__ float quad_perm(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int quad_perm_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }
constexpr int kQuadXor1 = 0xB1;  // quad_perm [1, 0, 3, 2]
constexpr int kQuadXor2 = 0x4E;  // quad_perm [2, 3, 0, 1]

// one lane's share of a manifold, in registers: its vector, its Jacobian column and (signed) response for the 12 rows;
// replicated over the quad: the row scalars and the accumulated impulses. All zero for a lane without a row.
// (quad_lane_setup / quad_lane_solve work on `x` and `count` in locals: read through the struct inside their loops they
// stayed in memory until the loops were unrolled, and both kernels came out 2-6 VGPRs and up to 100 instructions longer.
// The Jacobian columns are picked by selects, not branches: linear and angular lanes share every wave, so a branch ran
// both sides anyway, and k_solve_flow_quad lost 1 % on C2 with it.)
struct QuadLane {
    v3 x, Jv[4][3], Rs[4][3];
    float nm[4], tm0[4], tm1[4], bias[4], pn[4], pt0[4], pt1[4];
    float keep_w;  // the other float of the lane's half of the velocity record ({v, 1/m} or {w, m}): stored back as it was
    uint32_t body, count;
    bool has_body;
    __device__ __forceinline__ QuadLane() : keep_w(0.0f), body(0), count(0), has_body(false) {
        x = v3_make(0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nm[k] = 0.0f; tm0[k] = 0.0f; tm1[k] = 0.0f; bias[k] = 0.0f; pn[k] = 0.0f; pt0[k] = 0.0f; pt1[k] = 0.0f;
#pragma unroll
            for (int t = 0; t < 3; ++t) { Jv[k][t] = x; Rs[k][t] = x; }
        }
    }
};

// lane q (0 vA, 1 wA, 2 vB, 3 wB) of row {a, b, count} with normal `nn`, the tb elements t01 / t23 (t23 read by the
// caller only for count > 2) and the pt planes (records.hpp), read for the points below `count` only. The accumulated
// impulses are left to the caller.
template <bool DIAG>
__device__ __forceinline__ void quad_lane_setup(QuadLane& s, uint32_t q, uint32_t a, uint32_t b, uint32_t count, float4 nn,
                                                float4 t01, float4 t23, const float4* pt, uint32_t pt_stride, const float* vel,
                                                const float* __restrict__ inv_inertia, uint32_t inertia_stride) {
    const bool side_a = q < 2u, angular = (q & 1u) != 0u;
    const uint32_t body = side_a ? a : b;
    const bool has_body = side_a || !PHYS_IS_STATIC_PARTNER(b);
    s.count = count; s.body = body; s.has_body = has_body;
    v3 dir[3];
    dir[2] = v3_make(nn.x, nn.y, nn.z);
    tangent_basis(dir[2], &dir[0], &dir[1]);  // same inputs as solver_prep => same bits as the basis used there
    m33 I;
#pragma unroll
    for (int k = 0; k < 9; ++k) I.m[k] = 0.0f;
    float inv_m = 0.0f;
    v3 x = v3_make(0.0f, 0.0f, 0.0f);
    if (has_body) {
        // the body's half of the plain velocity record: the state itself where the caller takes it from there, the masses always
        const float4 h0 = reinterpret_cast<const float4*>(vel)[2 * (size_t)body + (angular ? 1 : 0)];
        x = v3_make(h0.x, h0.y, h0.z);
        s.keep_w = h0.w;
        if (angular) I = ld_inertia<DIAG>(inv_inertia, body * inertia_stride); else inv_m = h0.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < (int)count) {
            const RowPoint p = row_point_decode(k, pt[(size_t)row_pt_plane_a(k) * pt_stride], pt[(size_t)row_pt_plane_b(k) * pt_stride],
                                                row_tb_plane(k) == 0 ? t01 : t23);
            s.nm[k] = p.normal_mass; s.tm0[k] = p.tangent_mass0;
            s.tm1[k] = p.tangent_mass1;
            s.bias[k] = p.bias;
            const v3 r = side_a ? v3_make(p.rA[0], p.rA[1], p.rA[2]) : v3_make(p.rB[0], p.rB[1], p.rB[2]);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                if (has_body) {
                    // solver_jacobians: lA = dir * invM; aA = r x dir, mA = I aA. The A side is subtracted by the spec:
                    // its response is stored negated (exact)
                    const v3 jv = angular ? v3_cross_f(r, dir[t]) : dir[t];
                    const v3 rs = angular ? inertia_mul(&I, jv) : v3_scale(dir[t], inv_m);
                    s.Jv[k][t] = jv;
                    s.Rs[k][t] = side_a ? v3_neg(rs) : rs;
                }
            }
        }
    }
    s.x = x;
}

// the 12 rows of solve_manifold on the quad's four lanes; every lane of the quad takes part in the DPP exchanges.
// apply_only: sweep 0 of a warm-started solve - the starting impulses reach the lane's vector, no row is solved
__device__ __forceinline__ void quad_lane_solve(QuadLane& s, float friction, bool apply_only, bool side_a) {
    const uint32_t count = s.count;
    v3 x = s.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < (int)count) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                // row_velocity: (dir.vB + aB.wB) - (dir.vA + aA.wA), the two sums made inside each pair
                float lambda;
                if (apply_only) {
                    lambda = t == 0 ? s.pt0[k] : (t == 1 ? s.pt1[k] : s.pn[k]);
                    x = v3_madd(x, s.Rs[k][t], lambda);
                    continue;
                }
                const float part = v3_dot_f(s.Jv[k][t], x);
                const float mine = part + quad_perm<kQuadXor1>(part);
                const float other = quad_perm<kQuadXor2>(mine);
                const float vrel = side_a ? other - mine : mine - other;
                if (t < 2) lambda = friction_impulse(t == 0 ? s.tm0[k] : s.tm1[k], vrel, friction * s.pn[k], t == 0 ? &s.pt0[k] : &s.pt1[k]);
                else lambda = normal_impulse(s.nm[k], vrel, s.bias[k], &s.pn[k]);
                x = v3_madd(x, s.Rs[k][t], lambda);  // row_apply
            }
        }
    }
    s.x = x;
}

// {pn, pt0, pt1} of contact point q: what lane q publishes and stores
__device__ __forceinline__ v3 quad_point_impulses(const QuadLane& s, uint32_t q) {
    return q == 0 ? v3_make(s.pn[0], s.pt0[0], s.pt1[0])
         : q == 1 ? v3_make(s.pn[1], s.pt0[1], s.pt1[1])
         : q == 2 ? v3_make(s.pn[2], s.pt0[2], s.pt1[2]) : v3_make(s.pn[3], s.pt0[3], s.pt1[3]);
}

// ---------------------------------------------------------------------------------------------------------
// The dataflow solver with FOUR LANES PER MANIFOLD (the row core above), for scenes where the hop latency is
// everything. The granule protocol maps one to one: lane q polls and publishes exactly its own 16-byte granule (v or w
// of A or B), and the impulse granule of contact point q.
template <bool DIAG, bool MAT>
__global__ __launch_bounds__(256) void k_solve_flow_quad(StepCounters* __restrict__ ctr, uint32_t iterations, uint32_t epoch,
                                                         RowArrays rows, float friction,
                                                         const float* __restrict__ inv_inertia, uint32_t inertia_stride,
                                                         float* vel, float* flow_vel, uint32_t n_bodies, long long timeout_ticks,
                                                         uint32_t warm_sweep, WarmJob wj) {
    if (ctr->overflow) return;
    const uint32_t M = ctr->n_manifolds;
    const uint32_t rows_per_item = blockDim.x >> 2;
    const uint32_t nchunks = (M + rows_per_item - 1) / rows_per_item;
    const uint32_t total = nchunks * iterations;
    const uint32_t cap = (uint32_t)rows.cap;
    const Handoff hv = body_handoff(flow_vel, n_bodies, epoch), ha = impulse_handoff(rows.acc, cap, epoch);
    const uint32_t q = threadIdx.x & 3u;     // 0: vA, 1: wA, 2: vB, 3: wB
    const bool side_a = q < 2u, angular = (q & 1u) != 0u;
    const long long t_start = wall_clock64();
    const v3 zero = v3_make(0.0f, 0.0f, 0.0f);
    // Items are dealt STATICALLY here: workgroup g takes items g, g + G, g + 2G, ... in that order. A ticket from a global
    // counter (k_solve_flow keeps it) was one more dependent round trip and two barriers in front of every item of a
    // launch whose whole time is such chains: C2 0.078 -> 0.054 ms per solve, 6400 -> 7700 steps/s. (Measured and dropped:
    // the ticket of the next item asked for when an item begins - an item reserved by a workgroup that is still busy is an
    // item nobody else may start: C2 0.095 ms.)
    // No deadlock PROVIDED every workgroup of the launch gets to run: at most 224 workgroups, three fit a CU (the argument,
    // and why k_solve_flow keeps its tickets: DESIGN.md section 26).
    for (uint32_t L = blockIdx.x;; L += gridDim.x) {
        if (handoff_abandoned(ctr)) return;  // somebody gave up
        if (L >= total) return;
        const uint32_t it = L / nchunks, chunk = L - it * nchunks;
        const bool last_it = it + 1 == iterations;
        const uint32_t d = chunk * rows_per_item + (threadIdx.x >> 2);
        bool done = d >= M;  // the same for the four lanes of a quad
        QuadLane s;
        uint32_t ticket = 0;
        bool final_update = false;
        float mu = friction;  // MAT: the row's own
        if (!done) {
            const uint4 h = rows.hdr[d];
            const uint32_t tk = ticket_side(h.w, !side_a);
            const uint32_t rank = ticket_side_rank(tk), deg = ticket_side_degree(tk);
            ticket = it * deg + rank;
            final_update = last_it && rank + 1 == deg;
            const float4 nn = rows.n[d], t01 = rows.tb[(uint32_t)row_tb_plane(0) * cap + d];
            float4 t23 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (h.z > 2) t23 = rows.tb[(uint32_t)row_tb_plane(2) * cap + d];
            if constexpr (MAT) mu = nn.w;
            quad_lane_setup<DIAG>(s, q, h.x, h.y, h.z, nn, t01, t23, rows.pt + d, cap,
                                  vel, inv_inertia, inertia_stride);
        }
        const bool apply_only = warm_sweep != 0u && it == 0u;
        bool need = !done && s.has_body && ticket != 0;
        bool need_acc = !done && it != 0 && q < s.count;  // lane q fetches the impulses of contact point q
        v3 my_acc = zero;
        if (apply_only && !done && q < s.count) {  // the starting impulses of point q (plain load: k_rows_build wrote them)
            const float4 a0 = rows.acc[(size_t)q * cap + d];
            my_acc = v3_make(a0.x, a0.y, a0.z);
        }
        uint32_t sweeps = 0;
        for (;;) {
            uint32_t gap = 0;
            if (!done) {
                u32x4 g, p;
                if (need) g = ld_granule(hv.buf, body_granule(s.body, angular));
                if (need_acc) p = ld_granule(ha.buf, impulse_granule(q, cap, d));
                if (need) need = !hv.take(g, ticket, s.x, gap);
                if (need_acc) {
                    if (p.w == ha.tag(it)) { my_acc = granule_v3(p); need_acc = false; }
                    else if (gap == 0) gap = 1;
                }
            }
            // the manifold goes when its four lanes have what they need
            int ready = (!need && !need_acc) ? 1 : 0;
            ready &= quad_perm_i<kQuadXor1>(ready);
            ready &= quad_perm_i<kQuadXor2>(ready);
            if (!done && ready) {
                if (it != 0 || apply_only) {  // everybody needs every point's accumulated impulses
                    s.pn[0] = quad_perm<0x00>(my_acc.x); s.pt0[0] = quad_perm<0x00>(my_acc.y); s.pt1[0] = quad_perm<0x00>(my_acc.z);
                    s.pn[1] = quad_perm<0x55>(my_acc.x); s.pt0[1] = quad_perm<0x55>(my_acc.y); s.pt1[1] = quad_perm<0x55>(my_acc.z);
                    s.pn[2] = quad_perm<0xAA>(my_acc.x); s.pt0[2] = quad_perm<0xAA>(my_acc.y); s.pt1[2] = quad_perm<0xAA>(my_acc.z);
                    s.pn[3] = quad_perm<0xFF>(my_acc.x); s.pt0[3] = quad_perm<0xFF>(my_acc.y); s.pt1[3] = quad_perm<0xFF>(my_acc.z);
                }
                quad_lane_solve(s, mu, apply_only, side_a);
                if (s.has_body) {
                    if (final_update)
                        reinterpret_cast<float4*>(vel)[2 * (size_t)s.body + (angular ? 1 : 0)] = make_float4(s.x.x, s.x.y, s.x.z, s.keep_w);
                    else
                        hv.publish(body_granule(s.body, angular), s.x, ticket + 1u);
                }
                if (!last_it && q < s.count) ha.publish(impulse_granule(q, cap, d), quad_point_impulses(s, q), it + 1u);
                if (last_it && wj.man_prev) store_final_point_impulses(wj, d, q, quad_point_impulses(s, q));
                done = true;
            }
            if (__all(done)) break;
            if (flow_backoff(ctr, done, gap, sweeps, t_start, timeout_ticks)) done = true;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// One colour of one iteration with FOUR LANES PER MANIFOLD (the row core above) and the rows staged through LDS: the
// per-colour kernel for colour classes too small to fill the chip with one lane per manifold. k_solve_color runs one
// lane per manifold: a colour of 60-70k manifolds is then ~270 workgroups = one wave per SIMD, each lane a chain of
// header load -> ~20 dependent dwordx4 loads -> ~1200 VALU instructions -> stores with nothing to overlap it
// (17 us per launch for 26-33 MB, 19-24 % of the HBM rate). Here
//   * a workgroup owns 64 consecutive rows; every 16-byte element of the 16 row planes of those rows is loaded
//     ONCE (wave w fetches planes 4w..4w+3, 1 KiB contiguous per instruction, all issued before anything
//     else: no load depends on the header any more) and parked in LDS (16 KiB);
//   * quad_lane_setup / quad_lane_solve as in k_solve_flow_quad: a third of the VALU chain per lane, four times the
//     waves to overlap memory with arithmetic, and a gather of ONE 16-byte half record per lane.
// Rows of one colour share no body, so the plain loads / stores of `vel` need no ordering inside a launch.
template <bool DIAG, bool MAT>
__global__ __launch_bounds__(256) void k_solve_color_quad(StepCounters* ctr, uint32_t col, RowArrays rows,
                                                          float friction, const float* __restrict__ inv_inertia,
                                                          uint32_t inertia_stride, float* __restrict__ vel, uint32_t n_bodies,
                                                          int apply_only, int last, WarmJob wj) {
    __shared__ float4 s_rows[kRowPlanes][kQuadRowsPerGroup];  // [plane][row of this workgroup]
    constexpr uint32_t kPlanesPerWave = kRowPlanes / 4;       // four waves stage the planes
    static_assert(kPlanesPerWave == 4, "a wave stages four planes below");
    if (ctr->overflow) return;
    const uint32_t start = ctr->color_start[col], end = ctr->color_start[col + 1];
    const uint32_t cap = (uint32_t)rows.cap;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t q = threadIdx.x & 3u, r = threadIdx.x >> 2;  // q: 0 vA, 1 wA, 2 vB, 3 wB
    const bool side_a = q < 2u, angular = (q & 1u) != 0u;
    // the four planes this wave stages: kPlanesPerWave * wave + j of the ONE row allocation.
    // Plain arithmetic on purpose: written as `if (wave == 0) {pointers..} else if ..` over the five arrays, hipcc
    // (ROCm 7.2) lost one case of the pointer selection (wave 3 staged from a null pointer: memory access fault)
    const float4* pl = rows.all + (size_t)(kPlanesPerWave * wave) * cap;
    for (XcdTiles tl(end - start, kQuadRowsPerGroup); tl.valid(); tl.next()) {  // XCD-aware: see k_solve_color
        const uint32_t base = start + tl.tile * kQuadRowsPerGroup;
        {
            // rows beyond `end` belong to later colours (read only, never used); beyond the arrays: clamp
            uint32_t e = base + lane;
            e = e < cap ? e : cap - 1u;
            const float4 t0 = pl[e], t1 = pl[(size_t)cap + e], t2 = pl[2 * (size_t)cap + e], t3 = pl[3 * (size_t)cap + e];
            s_rows[kPlanesPerWave * wave + 0][lane] = t0; s_rows[kPlanesPerWave * wave + 1][lane] = t1;
            s_rows[kPlanesPerWave * wave + 2][lane] = t2; s_rows[kPlanesPerWave * wave + 3][lane] = t3;
        }
        __syncthreads();
        const uint32_t d = base + r;
        const bool live = d < end;  // the same for the four lanes of a quad
        QuadLane s;
        const float4 hraw = s_rows[kRowPlaneHdr][r];
        const uint32_t ha = __float_as_uint(hraw.x), hb = __float_as_uint(hraw.y), count = __float_as_uint(hraw.z);
        // a row header that names no body of this world must never become an address (a faulting kernel can take the
        // whole node down): flag the step (bit 5) and skip the row
        const bool bad = live && (count > 4u || ha >= n_bodies || (!PHYS_IS_STATIC_PARTNER(hb) && hb >= n_bodies));
        if (bad) {
            flag_overflow(ctr, kOvfCorruptRow);
            corrupt_row_note_encode(CorruptRowNote{d, ha, hb, count, start, end, col, base}, ctr->debug);
        }
        if (live && !bad) {
            float4 t23 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (count > 2) t23 = s_rows[kRowPlaneTb + row_tb_plane(2)][r];
            quad_lane_setup<DIAG>(s, q, ha, hb, count, s_rows[kRowPlaneN][r], s_rows[kRowPlaneTb + row_tb_plane(0)][r], t23, &s_rows[kRowPlanePt][r], kQuadRowsPerGroup,
                                  vel, inv_inertia, inertia_stride);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < (int)count) {  // the accumulated impulses of point k
                    const float4 ac = s_rows[kRowPlaneAcc + k][r];
                    s.pn[k] = ac.x; s.pt0[k] = ac.y; s.pt1[k] = ac.z;
                }
            }
        }
        // dead quads carry zeros (and, MAT, a clean friction: their slot of the tile holds another colour's row or stale memory)
        quad_lane_solve(s, MAT ? (live ? s_rows[kRowPlaneN][r].w : 0.0f) : friction, apply_only != 0, side_a);
        if (live) {
            if (s.has_body)
                reinterpret_cast<float4*>(vel)[2 * (size_t)s.body + (angular ? 1 : 0)] = make_float4(s.x.x, s.x.y, s.x.z, s.keep_w);
            if (q < s.count) {
                const v3 mine = quad_point_impulses(s, q);
                rows.acc[(size_t)q * cap + d] = make_float4(mine.x, mine.y, mine.z, 0.0f);
            }
            if (last && wj.man_prev) store_final_point_impulses(wj, d, q, quad_point_impulses(s, q));
        }
        __syncthreads();  // the LDS tile is restaged by the next trip
    }
}

// Launch sizes come from the plan (plan.hpp plan_solver: the HINT, counters of an earlier step read back asynchronously);
// every kernel takes its real ranges from the device-side counters, so a stale hint costs speed, never correctness.
void launch_solver(phys_world* w, float dt, const SolverPlan& plan, const ColorPlan& coloring) {
    if (w->n == 0) return;
    solve_params_t sp;
    sp.dt = dt;
    sp.baumgarte = w->cfg.baumgarte;
    sp.slop = w->cfg.slop;
    sp.friction = w->cfg.friction;
    sp.max_bias = w->cfg.max_bias;
    hipStream_t s = w->stream;
    const uint64_t cap = w->max_manifolds;
    const dim3 tb(256);
    const bool diag = w->all_diag_inertia;
    // every body shares one diagonal tensor (the reference's only case, identity): all lanes read entry 0
    const float* inertia = diag ? w->inv_inertia_diag.p : w->inv_inertia.p;
    const uint32_t stride = diag && w->uniform_inertia ? 0u : 1u;
    RowArrays rows;
    rows.all = reinterpret_cast<float4*>(w->row_all.p);
    rows.hdr = reinterpret_cast<uint4*>(rows.all + (size_t)kRowPlaneHdr * cap);
    rows.n = rows.all + (size_t)kRowPlaneN * cap;
    rows.tb = rows.all + (size_t)kRowPlaneTb * cap;
    rows.pt = rows.all + (size_t)kRowPlanePt * cap;
    rows.acc = rows.all + (size_t)kRowPlaneAcc * cap;
    rows.cap = cap;
    const bool cluster = plan.path == SolverPath::Cluster, flow = plan.flow();
    // warm starting (contact_solve.h): one sweep more, in front - it applies the impulses the rows start from
    WarmJob warm{};
    if (w->warm) {
        warm.man_prev = w->man_prev.p; warm.geo_prev = w->man_geo_prev.p; warm.imp_prev = w->man_imp_prev.p;
        warm.imp = w->man_imp.p; warm.row_src = w->row_src.p;
    }
    const uint32_t warm_sweep = w->warm ? 1u : 0u;
    const uint32_t sweeps = w->cfg.solver_iterations + warm_sweep;
    // the colouring stage's job for k_rows_build: this update's new manifolds - all of them on a rebuild - go into the colour table
    ColorTableJob table{};
    table.tab = reinterpret_cast<ulonglong2*>(w->ctab.p);
    table.mask = w->ctab_mask;
    table.stamp = coloring.stamp;
    table.all = coloring.rebuild ? 1u : 0u;
    table.man_color = w->man_color.p; table.man_prio = w->man_prio.p;
    const EpochStep next = flow ? handoff_epoch_next(w->flow_epoch) : EpochStep{w->flow_epoch, false};
    w->flow_epoch = next.epoch;
    if (next.clear) {
        // tags would repeat: forget every old one. AHEAD of k_rows_build: on a cluster step that kernel writes the constants
        // of foreign bodies into the impulse planes (with flow != 0 it never writes the impulses there), and a memset
        // behind it wiped them - every 65535th solve ran with x = 0, 1/m = 0, I^-1 = 0 for those rows
        PHYS_PROF(w, PHYS_STAGE_MISC);
        (void)hipMemsetAsync(w->flow_vel.p, 0, kBodyGranuleBytes * w->n, s);
        (void)hipMemsetAsync(rows.acc, 0, row_plane_floats(kRowAccPlanes, cap) * sizeof(float), s);
    }
    // materials: once a material call was made, the material instances of every kernel below - same
    // path choice, same launch sizes; they take the friction from the row. With every material at its default they give the
    // plain instances' bits.
    RowMaterials mats{};
    mats.body = reinterpret_cast<const float2*>(w->mat.p);
    mats.st = reinterpret_cast<const float2*>(w->st_mat.p);
    mats.ground = make_float2(w->ground_mat_set ? w->ground_mat[0] : w->cfg.friction, w->ground_mat_set ? w->ground_mat[1] : 0.0f);
    mats.threshold = w->restitution_threshold;
    dispatch_bool(diag, [&](auto diag_t) { dispatch_bool(plan.materials, [&](auto mat_t) {  // every kernel below in this world's instantiation
        constexpr bool DIAG = decltype(diag_t)::value, MAT = decltype(mat_t)::value;
        { PHYS_PROF(w, PHYS_STAGE_ROWS);
          auto rows_build = [&](auto... mat) {
              hipLaunchKernelGGL((k_rows_build<DIAG, MAT, decltype(mat)...>), dim3(plan.rows_blocks), tb, 0, s, w->counters.p, rows, sp, w->row_src.p, w->man_geo.p,
                                 w->pos.p, w->vel.p, inertia, stride, w->man_color.p,
                                 w->color_state.p, flow ? (plan.stall ? 2 : 1) : 0, table, w->cluster_slot.p, w->body_shared.p,
                                 cluster ? w->cluster_slots : 0u, w->cluster_count, warm, mat...);
          };
          if constexpr (MAT) rows_build(mats); else rows_build(); }
        if (cluster) {
            PHYS_PROF(w, PHYS_STAGE_SOLVE_CLUSTER);
            launch_solve_cluster(w, plan, rows.all, cap, sp.friction, inertia, stride, diag);
            return;
        }
        if (flow) {
            const dim3 items(plan.items), threads(256);
            PHYS_PROF(w, PHYS_STAGE_SOLVE_FLOW);
            if (plan.path == SolverPath::FlowQuad)
                hipLaunchKernelGGL((k_solve_flow_quad<DIAG, MAT>), items, threads, 0, s, w->counters.p, sweeps, w->flow_epoch,
                                   rows, sp.friction, inertia, stride, w->vel.p, w->flow_vel.p, (uint32_t)w->n, plan.timeout_ticks, warm_sweep, warm);
            else
                hipLaunchKernelGGL((k_solve_flow<DIAG, MAT>), items, threads, 0, s, w->counters.p, sweeps, w->flow_epoch,
                                   rows, sp.friction, inertia, stride, w->vel.p, w->flow_vel.p, (uint32_t)w->n, plan.timeout_ticks, plan.pipeline,
                                   warm_sweep, warm);
            return;
        }
        // colours [0, big) get a launch each; [big, n_colours) go through the single-workgroup tail
        for (uint32_t it = 0; it < sweeps; ++it) {
            const int apply_only = warm_sweep && it == 0 ? 1 : 0, last = it + 1 == sweeps ? 1 : 0;
            for (uint32_t col = 0; col < plan.big; ++col) {
                PHYS_PROF(w, PHYS_STAGE_SOLVE);
                if (plan.color_quad[col])  // four lanes per manifold
                    hipLaunchKernelGGL((k_solve_color_quad<DIAG, MAT>), dim3(plan.color_blocks[col]), tb, 0, s, w->counters.p, col, rows,
                                       sp.friction, inertia, stride, w->vel.p, (uint32_t)w->n, apply_only, last, warm);
                else
                    hipLaunchKernelGGL((k_solve_color<DIAG, MAT>), dim3(plan.color_blocks[col]), tb, 0, s, w->counters.p, col, rows,
                                       sp.friction, inertia, stride, w->vel.p, apply_only, last, warm);
            }
            PHYS_PROF(w, PHYS_STAGE_SOLVE_TAIL);
            hipLaunchKernelGGL((k_solve_tail<DIAG, MAT>), dim3(1), dim3(kTailThreads), 0, s, w->counters.p, plan.big, rows, sp.friction,
                               inertia, stride, w->vel.p, apply_only, last, warm);
        }
    }); });
}

}  // namespace phys
