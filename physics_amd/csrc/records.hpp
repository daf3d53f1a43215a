// records.hpp — the records the collision kernels hand to each other, each stated ONCE: its constants, one encode and one
// decode. DESIGN.md section 21 is the table of them. Host-compilable like plan.hpp (no HIP header), held to
// tests/cpp/records_probe.cpp; every kernel and host function that produces or consumes one of these goes through here.
// A 16-byte element is whatever four-float vector the caller has (`V`: fields x, y, z, w): the functions only name its
// fields, so a kernel's loads and stores of it stay the single 16-byte accesses they are.
#pragma once
#include <cstddef>
#include <cstdint>

#include "plan.hpp"

#ifdef __HIPCC__
#define PHYS_REC __host__ __device__ __forceinline__
#else
#define PHYS_REC inline
#endif

namespace phys {

PHYS_REC uint32_t rec_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
PHYS_REC float rec_float(uint32_t u) { return __builtin_bit_cast(float, u); }

// ---- ticket word (row header .w): which update of each of its two bodies a row makes -------------------------------------
// Per side 16 bits: rank (the row's place among the body's rows in solve order) in bits 0-5, the body's degree in bits 8-14;
// side A in the low half, side B in the high half. A rank is below kMaxColors and a degree at most kMaxColors, so bits 6, 7
// and 15 are never set: the compact rows of material worlds keep the row's point count (0..4) there, their header .z being
// taken by the friction.
struct RowTicket { uint32_t rankA, degA, rankB, degB; };
constexpr uint32_t kTicketCountBits = 0x000080C0u;  // bits 6, 7 (the count's low two bits) and 15 (its bit 2)
static_assert(((uint32_t)(kMaxColors - 1) & kTicketCountBits) == 0u && (((uint32_t)kMaxColors << 8) & kTicketCountBits) == 0u &&
                  (uint32_t)kMaxColors == 64u,
              "rank < 64 and degree <= 64 leave ticket bits 6, 7 and 15 clear");
PHYS_REC uint32_t ticket_side_encode(uint32_t rank, uint32_t deg) { return rank | (deg << 8); }
PHYS_REC uint32_t ticket_encode(RowTicket t) { return ticket_side_encode(t.rankA, t.degA) | (ticket_side_encode(t.rankB, t.degB) << 16); }
// one side alone: {rank, degree} in rankA, degA
PHYS_REC uint32_t ticket_side(uint32_t word, bool side_b) { return side_b ? word >> 16 : word; }
PHYS_REC uint32_t ticket_side_rank(uint32_t side) { return side & 0xFFu; }
PHYS_REC uint32_t ticket_side_degree(uint32_t side) { return (side >> 8) & 0xFFu; }
// the plain decode: of a word without count bits
PHYS_REC RowTicket ticket_decode(uint32_t word) {
    return {ticket_side_rank(word), ticket_side_degree(word), ticket_side_rank(word >> 16), word >> 24};
}
// material compact rows: the count rides along, and comes off again
PHYS_REC uint32_t ticket_with_count(uint32_t ticket, uint32_t count) { return ticket | ((count & 3u) << 6) | ((count >> 2) << 15); }
PHYS_REC uint32_t ticket_count(uint32_t word) { return ((word >> 6) & 3u) | ((word >> 13) & 4u); }
PHYS_REC uint32_t ticket_without_count(uint32_t word) { return word & ~kTicketCountBits; }

// ---- cluster side word (compact row normal .w): where each side's velocity lives --------------------------------------------
// Per side 16 bits: slot in the owning workgroup's LDS (13) | publish (1) | mode (2); side A low, side B high.
// publish: the body's NEXT update in solve order belongs to another workgroup's row, so this one must reach the granules.
constexpr uint32_t kSideOwn = 0;      // own cluster, never updated by another workgroup: LDS only
constexpr uint32_t kSideShared = 1;   // own cluster, shared: LDS while its tag is current, granules otherwise
constexpr uint32_t kSideForeign = 2;  // another cluster's body, or one without a home: granules only; its constants ride with the row
constexpr uint32_t kSideNone = 3;     // no body (ground, static collider)
constexpr uint32_t kSideSlots = 1u << 13;
struct ClusterSide { uint32_t slot, publish, mode; };
PHYS_REC uint32_t cluster_side_encode(uint32_t slot, uint32_t publish, uint32_t mode) { return slot | (publish << 13) | (mode << 14); }
PHYS_REC uint32_t cluster_sides_encode(uint32_t side_a, uint32_t side_b) { return side_a | (side_b << 16); }
PHYS_REC ClusterSide cluster_side_decode(uint32_t word, bool side_b) {
    const uint32_t s = side_b ? word >> 16 : word;
    return {s & (kSideSlots - 1u), (s >> 13) & 1u, (s >> 14) & 3u};
}
// this side's constants (position, 1/m, inverse inertia diagonal) ride with the row, in its foreign planes
PHYS_REC bool cluster_side_rides(uint32_t word, bool side_b) { return cluster_side_decode(word, side_b).mode == kSideForeign; }
PHYS_REC bool cluster_side_at_home(uint32_t mode) { return mode == kSideOwn || mode == kSideShared; }

// ---- hand-off tag (.w of a granule of the single-launch solvers) ---------------------------------------
// epoch of the solve in the high half | updates applied to the body (impulse granules: sweeps finished) in the low half
constexpr uint32_t kTagHalfBits = 16, kTagHalfMask = 0xFFFFu, kHandoffEpochMax = kTagHalfMask;
constexpr uint32_t kGranuleBytes = 16, kBodyGranuleBytes = 2 * kGranuleBytes;  // a body in flow_vel: {v, tag} {w, tag}
static_assert(((kHandoffIterationsEnd - 1u) + 1u /* the warm sweep */) * (uint32_t)kMaxColors <= kTagHalfMask,
              "a body is updated at most once per sweep and colour: the count fits its half of the tag");
PHYS_REC constexpr uint32_t handoff_tag(uint32_t epoch, uint32_t updates) { return (epoch << kTagHalfBits) | updates; }
PHYS_REC constexpr uint32_t handoff_tag_from(uint32_t tag0, uint32_t updates) { return tag0 | updates; }  // tag0 = handoff_tag(epoch, 0), kept by the kernels
PHYS_REC constexpr uint32_t handoff_tag_epoch(uint32_t tag) { return tag >> kTagHalfBits; }
PHYS_REC constexpr uint32_t handoff_tag_updates(uint32_t tag) { return tag & kTagHalfMask; }
// how many updates a row holding `ticket` is away from what it saw: another epoch's tag counts as nothing seen; never below 1
PHYS_REC constexpr uint32_t handoff_gap(uint32_t seen_tag, uint32_t epoch, uint32_t ticket) {
    const uint32_t seen = handoff_tag_epoch(seen_tag) == epoch ? handoff_tag_updates(seen_tag) : 0u;
    return ticket > seen ? ticket - seen : 1u;
}
// the host's step from one solve's epoch to the next; clear: tags would repeat, so every granule is zeroed first
struct EpochStep { uint32_t epoch; bool clear; };
PHYS_REC constexpr EpochStep handoff_epoch_next(uint32_t epoch) { return epoch + 1u > kHandoffEpochMax ? EpochStep{1u, true} : EpochStep{epoch + 1u, false}; }

// ---- colour-table value word (the second 8 bytes of a table slot) ---------------------------------------------------------
// stamp of the update that wrote it (32) | index of the pair's manifold in that update (26) | colour (6)
constexpr uint32_t kUncolored = 0xFFFFFFFFu;  // man_color of a manifold that kept no colour (narrowphase.hip -> coloring.hip)
constexpr uint32_t kTableIndexBits = 26, kTableColorBits = 6, kTableColorMask = (1u << kTableColorBits) - 1u;
static_assert((1u << kTableColorBits) == (uint32_t)kMaxColors, "a colour fits its field exactly");
struct TableValue { uint32_t stamp, index, color; };
// a colour that may be kUncolored (an update whose colouring gave up) must not reach the index and stamp bits
PHYS_REC uint32_t table_color_field(uint32_t color) { return color & kTableColorMask; }
PHYS_REC unsigned long long table_value_encode(uint32_t stamp, uint32_t index, uint32_t color /* below kMaxColors */) {
    return ((unsigned long long)stamp << 32) | ((unsigned long long)(index & ((1u << kTableIndexBits) - 1u)) << kTableColorBits) | color;
}

PHYS_REC uint32_t table_value_stamp(unsigned long long v) { return (uint32_t)(v >> 32); }
PHYS_REC uint32_t table_value_index(unsigned long long v) { return (uint32_t)v >> kTableColorBits; }
PHYS_REC uint32_t table_value_color(unsigned long long v) { return table_color_field((uint32_t)v); }
PHYS_REC TableValue table_value_decode(unsigned long long v) { return {table_value_stamp(v), table_value_index(v), table_value_color(v)}; }

// ---- impulse record: 48 bytes per manifold, {pn, pt0, pt1} of points 0..3 packed into three 16-byte elements ----------------
// Point k's three floats are floats 3k, 3k + 1, 3k + 2. The same packing holds the starting / accumulated impulses and the
// row masses {t1, t2, n} in the compact rows (planes kClusterPlaneAcc.., kClusterPlaneMass..).
constexpr uint32_t kImpulseFloats = 12, kImpulseFloatsPerPoint = 3, kImpulseVecs = 3;
template <class V>
PHYS_REC void impulses_pack(const float pn[4], const float pt0[4], const float pt1[4], V& o0, V& o1, V& o2) {
    o0.x = pn[0]; o0.y = pt0[0]; o0.z = pt1[0]; o0.w = pn[1];
    o1.x = pt0[1]; o1.y = pt1[1]; o1.z = pn[2]; o1.w = pt0[2];
    o2.x = pt1[2]; o2.y = pn[3]; o2.z = pt0[3]; o2.w = pt1[3];
}
template <class V>
PHYS_REC void impulses_unpack(const V& i0, const V& i1, const V& i2, float pn[4], float pt0[4], float pt1[4]) {
    pn[0] = i0.x; pt0[0] = i0.y; pt1[0] = i0.z; pn[1] = i0.w;
    pt0[1] = i1.x; pt1[1] = i1.y; pn[2] = i1.z; pt0[2] = i1.w;
    pt1[2] = i2.x; pn[3] = i2.y; pt0[3] = i2.z; pt1[3] = i2.w;
}
// where the four-lane kernels' lane q writes {pn, pt0, pt1} of point q, in floats from the record's start
PHYS_REC constexpr uint32_t impulses_point_offset(uint32_t q) { return kImpulseFloatsPerPoint * q; }
// one float of the record, for a reader that wants a few of them (pn of point k: float impulses_point_offset(k))
template <class V>
PHYS_REC float impulses_float(const V& i0, const V& i1, const V& i2, uint32_t f) {
    const V& v = f < 4u ? i0 : (f < 8u ? i1 : i2);
    return (f & 3u) == 0u ? v.x : ((f & 3u) == 1u ? v.y : ((f & 3u) == 2u ? v.z : v.w));
}

// ---- manifold record: 128 bytes = eight 16-byte elements, six used -----------------------------------------------------------
//   element 0      {body a, body b, point count, kept colour + 1 (0: new in this update, coloured later)}   as bits
//   element 1      {normal xyz, index of the pair's manifold in the previous update (bits) or kNoPrevManifold}
//   elements 2-5   {contact point xyz, depth} of points 0..3
constexpr uint32_t kManifoldVecs = 8, kManifoldFloats = 32, kManifoldBytes = 128;
constexpr uint32_t kManifoldVecHead = 0, kManifoldVecNormal = 1, kManifoldVecPoint = 2;
constexpr uint32_t kManifoldWordA = 0, kManifoldWordB = 1, kManifoldWordCount = 2, kManifoldWordKept = 3, kManifoldWordNormal = 4,
                   kManifoldWordPrev = 7, kManifoldWordPoints = 8, kManifoldWordsUsed = 24;
constexpr uint32_t kNoPrevManifold = 0xFFFFFFFFu;
struct ManifoldHead { uint32_t a, b, count, color; /* the kept colour, or kUncolored */ };
template <class V>
PHYS_REC void manifold_head_encode(ManifoldHead h, V& o) {
    o.x = rec_float(h.a); o.y = rec_float(h.b); o.z = rec_float(h.count); o.w = rec_float(h.color != kUncolored ? h.color + 1u : 0u);
}
template <class V>
PHYS_REC ManifoldHead manifold_head_decode(const V& r) {
    return {rec_bits(r.x), rec_bits(r.y), rec_bits(r.z), rec_bits(r.w) != 0u ? rec_bits(r.w) - 1u : kUncolored};
}
template <class V>
PHYS_REC uint32_t manifold_prev_index(const V& normal_vec) { return rec_bits(normal_vec.w); }

// ---- the two plane numberings of the row allocation: 16 planes of `cap` 16-byte elements, plane p of row d at [p * cap + d] ----
// prepared rows (every solver kernel but the cluster solver's):
//   hdr {body a, body b, point count, ticket word}; n {normal xyz, side word bits / the manifold's friction in material worlds};
//   tb  plane j: {tangent mass 1, bias} of points 2j and 2j + 1;  pt plane 2k: {rA xyz, normal mass}, 2k + 1: {rB xyz, tangent mass 0};
//   acc plane k: {pn, pt0, pt1, tag} of point k
constexpr int kRowPlanes = 16;
// where plane p of an allocation of `cap` rows begins, in floats from its start (a plane is cap 16-byte elements)
PHYS_REC constexpr size_t row_plane_floats(int plane, uint64_t cap) { return 4 * (size_t)plane * (size_t)cap; }
constexpr int kRowPlaneHdr = 0, kRowPlaneN = 1, kRowPlaneTb = 2, kRowPlanePt = 4, kRowPlaneAcc = 12;
constexpr int kRowTbPlanes = 2, kRowPtPlanes = 8, kRowAccPlanes = 4;
// within the tb, pt and acc planes: where point k's elements are
PHYS_REC constexpr int row_tb_plane(int k) { return k >> 1; }
PHYS_REC constexpr int row_pt_plane_a(int k) { return 2 * k; }
PHYS_REC constexpr int row_pt_plane_b(int k) { return 2 * k + 1; }
// one point of a prepared row: {rA, normal mass} {rB, tangent mass 0} and its half of a tb element
struct RowPoint { float rA[3], rB[3], normal_mass, tangent_mass0, tangent_mass1, bias; };
template <class V>
PHYS_REC RowPoint row_point_decode(int k, const V& pa, const V& pb, const V& tb) {
    return {{pa.x, pa.y, pa.z}, {pb.x, pb.y, pb.z}, pa.w, pb.w, (k & 1) ? tb.z : tb.x, (k & 1) ? tb.w : tb.y};
}
template <class V>
PHYS_REC void row_point_encode(const RowPoint& p, V& pa, V& pb) {
    pa.x = p.rA[0]; pa.y = p.rA[1]; pa.z = p.rA[2]; pa.w = p.normal_mass;
    pb.x = p.rB[0]; pb.y = p.rB[1]; pb.z = p.rB[2]; pb.w = p.tangent_mass0;
}
template <class V>
PHYS_REC void row_tb_encode(const RowPoint& even, const RowPoint& odd, V& tb) {
    tb.x = even.tangent_mass1; tb.y = even.bias; tb.z = odd.tangent_mass1; tb.w = odd.bias;
}
static_assert(kRowPlaneHdr == 0 && kRowPlaneN == kRowPlaneHdr + 1 && kRowPlaneTb == kRowPlaneN + 1 && kRowPlanePt == kRowPlaneTb + kRowTbPlanes &&
                  kRowPlaneAcc == kRowPlanePt + kRowPtPlanes && kRowPlaneAcc + kRowAccPlanes == kRowPlanes,
              "the prepared-row planes partition 0..15");
// compact rows (cluster solver: k_rows_build on a cluster step -> k_solve_cluster):
//   hdr as above (material worlds: .z the friction, the count in the ticket word); n {normal xyz, side word};
//   geo plane k: {contact point xyz, bias} of point k; acc, mass: impulse-record packing; foreign B / A: {position, 1/m}
//   {inverse inertia diagonal} of a side whose constants ride with the row
constexpr int kClusterPlaneHdr = 0, kClusterPlaneN = 1, kClusterPlaneGeo = 2, kClusterPlaneAcc = 6, kClusterPlaneMass = 9,
              kClusterPlaneForeignB = 12, kClusterPlaneForeignA = 14;
constexpr int kClusterGeoPlanes = 4, kClusterForeignPlanes = 2;
static_assert(kClusterPlaneHdr == 0 && kClusterPlaneN == kClusterPlaneHdr + 1 && kClusterPlaneGeo == kClusterPlaneN + 1 &&
                  kClusterPlaneAcc == kClusterPlaneGeo + kClusterGeoPlanes && kClusterPlaneMass == kClusterPlaneAcc + (int)kImpulseVecs &&
                  kClusterPlaneForeignB == kClusterPlaneMass + (int)kImpulseVecs &&
                  kClusterPlaneForeignA == kClusterPlaneForeignB + kClusterForeignPlanes &&
                  kClusterPlaneForeignA + kClusterForeignPlanes == kRowPlanes,
              "the compact-row planes partition 0..15");
static_assert(kClusterPlaneForeignB >= kRowPlaneAcc, "the foreign constants lie in the impulse planes, which a dataflow step's k_rows_build leaves alone");

// ---- the eight debug words (StepCounters::debug) behind two overflow bits, as phys_sync's text reads them ---------------------
// kOvfCorruptRow: the row k_solve_color_quad refused
struct CorruptRowNote { uint32_t row, a, b, count, color_start, color_end, color, tile_base; };
PHYS_REC void corrupt_row_note_encode(const CorruptRowNote& n, uint32_t g[8]) {
    g[0] = n.row; g[1] = n.a; g[2] = n.b; g[3] = n.count; g[4] = n.color_start; g[5] = n.color_end; g[6] = n.color; g[7] = n.tile_base;
}
PHYS_REC CorruptRowNote corrupt_row_note_decode(const uint32_t g[8]) { return {g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7]}; }
// kOvfHandoff with word 0 == kClusterTimeoutMark: what the first lane of k_solve_cluster to give up was waiting for. Word 0 is
// claimed by a compare-and-swap at the site (0 -> the mark); the encode fills words 1..7. Tickets and the cluster count are
// 16-bit fields, colour and iteration 8-bit.
constexpr uint32_t kClusterTimeoutMark = 0xC1u;
struct ClusterTimeoutNote { uint32_t cluster, clusters, row, a, b, ticketA, ticketB, waitA, waitB, modeA, modeB, color, iteration; };
PHYS_REC void cluster_timeout_note_encode(const ClusterTimeoutNote& n, uint32_t g[8]) {
    g[1] = n.cluster | (n.clusters << 16);
    g[2] = n.row; g[3] = n.a; g[4] = n.b;
    g[5] = (n.ticketA & 0xFFFFu) | (n.ticketB << 16);
    g[6] = n.waitA | (n.waitB << 1) | (n.modeA << 4) | (n.modeB << 8);
    g[7] = (n.color & 0xFFu) | ((n.iteration & 0xFFu) << 8);
}
PHYS_REC ClusterTimeoutNote cluster_timeout_note_decode(const uint32_t g[8]) {
    return {g[1] & 0xFFFFu, g[1] >> 16, g[2], g[3], g[4], g[5] & 0xFFFFu, g[5] >> 16, g[6] & 1u, (g[6] >> 1) & 1u,
            (g[6] >> 4) & 3u, (g[6] >> 8) & 3u, g[7] & 0xFFu, (g[7] >> 8) & 0xFFu};
}

}  // namespace phys
