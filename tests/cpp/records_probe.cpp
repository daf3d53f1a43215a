// records_probe.cpp — the records the collision kernels exchange (physics_amd/csrc/records.hpp) against their stated layouts.
// Built by a host compiler alone (tests/test_records_cpu.py); exits non-zero at the first mismatch. Every expected bit
// position and word offset below is written out from the format's description, never taken from the
// header's constants, and every word's encode-then-decode is the identity over its whole domain.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../physics_amd/csrc/readout.hpp"
#include "../../physics_amd/csrc/records.hpp"

using namespace phys;

static long long g_checks = 0;
#define CHECK(what, got, want)                                                                                          \
    do {                                                                                                                \
        ++g_checks;                                                                                                     \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                  \
        if (g_ != w_) {                                                                                                 \
            std::printf("MISMATCH %s:%d  %s: %s = %lld, expected %lld\n", __FILE__, __LINE__, what, #got, g_, w_);      \
            std::exit(1);                                                                                               \
        }                                                                                                               \
    } while (0)

struct Vec4 { float x, y, z, w; };  // the 16-byte element as a host sees it
static_assert(sizeof(Vec4) == 16, "four floats");
static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static void ticket() {
    // rank A bits 0-5 | degree A bits 8-14 | rank B bits 16-21 | degree B bits 24-30; the count of a material compact row in
    // bits 6, 7 (its low two bits) and 15 (its bit 2)
    CHECK("count bits", kTicketCountBits, (1u << 6) | (1u << 7) | (1u << 15));
    CHECK("ticket", ticket_encode(RowTicket{5, 9, 63, 64}), 5u | (9u << 8) | (63u << 16) | (64u << 24));
    CHECK("ticket + count", ticket_with_count(0u, 4u), 1u << 15);
    CHECK("ticket + count", ticket_with_count(0u, 3u), (1u << 6) | (1u << 7));
    for (uint32_t ra = 0; ra < 64; ++ra)
        for (uint32_t da = 1; da <= 64; ++da)
            for (uint32_t rb = 0; rb < 64; ++rb)
                for (uint32_t db = 1; db <= 64; ++db) {
                    const uint32_t w = ticket_encode(RowTicket{ra, da, rb, db});
                    if ((w & kTicketCountBits) != 0u) CHECK("count bits stay clear", w & kTicketCountBits, 0);
                    const RowTicket t = ticket_decode(w);
                    if (t.rankA != ra || t.degA != da || t.rankB != rb || t.degB != db) CHECK("ticket round trip", 0, 1);
                    const uint32_t sa = ticket_side(w, false), sb = ticket_side(w, true);
                    if (ticket_side_rank(sa) != ra || ticket_side_degree(sa) != da || ticket_side_rank(sb) != rb || ticket_side_degree(sb) != db)
                        CHECK("ticket sides", 0, 1);
                    // the material form only where something differs per side B (the count bits lie in side A's half)
                    if (rb == 0 && db == 1) {
                        for (uint32_t c = 0; c <= 4; ++c) {
                            const uint32_t m = ticket_with_count(w, c);
                            if (ticket_count(m) != c || ticket_without_count(m) != w) CHECK("material ticket", 0, 1);
                            const RowTicket p = ticket_decode(ticket_without_count(m));  // the plain decode, count bits masked
                            if (p.rankA != ra || p.degA != da || p.rankB != rb || p.degB != db) CHECK("material ticket, plain decode", 0, 1);
                        }
                    }
                }
    // ... and the count with every side B at its extremes
    for (uint32_t c = 0; c <= 4; ++c)
        for (uint32_t rb : {0u, 63u})
            for (uint32_t db : {1u, 64u}) {
                const uint32_t w = ticket_encode(RowTicket{63, 64, rb, db}), m = ticket_with_count(w, c);
                CHECK("material ticket", ticket_count(m), c); CHECK("material ticket", ticket_without_count(m), w);
            }
    g_checks += 64ll * 64 * 64 * 64;
}

static void side_word() {
    // per side: slot bits 0-12 | publish bit 13 | mode bits 14-15; side B sixteen bits up
    CHECK("side", cluster_side_encode(8191u, 1u, 3u), 0xFFFFu);
    CHECK("side", cluster_sides_encode(cluster_side_encode(5u, 0u, 1u), cluster_side_encode(7u, 1u, 2u)),
          5u | (1u << 14) | (7u << 16) | (1u << 29) | (2u << 30));
    CHECK("modes", kSideOwn, 0); CHECK("modes", kSideShared, 1); CHECK("modes", kSideForeign, 2); CHECK("modes", kSideNone, 3);
    // side A over its whole domain against side B at its corners, and the other way round
    const ClusterSide corner[4] = {{0, 0, 0}, {8191, 1, 3}, {4096, 0, 2}, {1, 1, 1}};
    for (uint32_t slot = 0; slot < 8192; ++slot)
        for (uint32_t pub = 0; pub < 2; ++pub)
            for (uint32_t mode = 0; mode < 4; ++mode)
                for (const ClusterSide& o : corner)
                    for (int swap = 0; swap < 2; ++swap) {
                        const uint32_t mine = cluster_side_encode(slot, pub, mode), other = cluster_side_encode(o.slot, o.publish, o.mode);
                        const uint32_t w = swap ? cluster_sides_encode(other, mine) : cluster_sides_encode(mine, other);
                        const ClusterSide m = cluster_side_decode(w, swap != 0), p = cluster_side_decode(w, swap == 0);
                        if (m.slot != slot || m.publish != pub || m.mode != mode || p.slot != o.slot || p.publish != o.publish || p.mode != o.mode)
                            CHECK("side round trip", 0, 1);
                        if (cluster_side_rides(w, swap != 0) != (mode == 2u) || cluster_side_rides(w, swap == 0) != (o.mode == 2u))
                            CHECK("constants ride with the row iff mode 2", 0, 1);
                        ++g_checks;
                    }
    CHECK("at home", cluster_side_at_home(0) && cluster_side_at_home(1) && !cluster_side_at_home(2) && !cluster_side_at_home(3), 1);
}

static void handoff_tag_word() {
    // epoch bits 16-31 | updates applied bits 0-15; a body's granules in flow_vel: 32 bytes, two of 16
    CHECK("tag", handoff_tag(0xABCDu, 0x1234u), 0xABCD1234u);
    CHECK("halves", kTagHalfBits, 16); CHECK("halves", kTagHalfMask, 65535); CHECK("largest epoch", kHandoffEpochMax, 65535);
    CHECK("granule", kGranuleBytes, 16); CHECK("a body's granules", kBodyGranuleBytes, 32);
    for (uint32_t epoch = 0; epoch <= 0xFFFFu; ++epoch)
        for (uint32_t updates : {0u, 1u, 63u, 64u, 64000u, 0xFFFFu}) {
            const uint32_t t = handoff_tag(epoch, updates);
            CHECK("tag round trip", handoff_tag_epoch(t), epoch); CHECK("tag round trip", handoff_tag_updates(t), updates);
            CHECK("tag from the epoch in place", handoff_tag_from(handoff_tag(epoch, 0u), updates), t);
        }
    // the gap of a row holding `ticket` in epoch 7: {tag seen, ticket, gap}
    const uint32_t gaps[][3] = {
        {(7u << 16) | 12u, 10u, 1u},     // same epoch, ahead of the ticket (cannot happen; never below 1)
        {(7u << 16) | 3u, 10u, 7u},      // same epoch, behind it
        {(7u << 16) | 9u, 10u, 1u},      // ... by one
        {(7u << 16) | 10u, 10u, 1u},     // equal (the other granule of the body is the one that lags)
        {(7u << 16) | 0u, 64000u, 64000u},
        {(6u << 16) | 9u, 10u, 10u},     // a foreign epoch: nothing seen
        {(0x8007u << 16) | 9u, 10u, 10u},
        {0u, 10u, 10u}, {0u, 1u, 1u},    // tag 0: a cleared buffer
    };
    for (const auto& g : gaps) CHECK("gap", handoff_gap(g[0], 7u, g[1]), g[2]);
    CHECK("gap in epoch 0 from a cleared buffer", handoff_gap(0u, 0u, 5u), 5);
    // the sweep limit: (999 iterations + the warm sweep) x 64 colours of updates fit 16 bits; 1024 sweeps would not
    CHECK("iterations end", kHandoffIterationsEnd, 1000);
    CHECK("largest update count", (999 + 1) * 64, 64000); CHECK("fits", (999 + 1) * 64 <= 65535, 1); CHECK("1024 sweeps do not", 1024 * 64 > 65535, 1);
    // the host's epoch step: {epoch, next, clear}
    const uint32_t steps[][3] = {{0u, 1u, 0u}, {1u, 2u, 0u}, {0xFFFEu, 0xFFFFu, 0u}, {0xFFFFu, 1u, 1u}};
    for (const auto& s : steps) {
        const EpochStep n = handoff_epoch_next(s[0]);
        CHECK("epoch step", n.epoch, s[1]); CHECK("epoch step, clear", n.clear, s[2]);
    }
}

static void table_value() {
    // stamp bits 32-63 | manifold index bits 6-31 | colour bits 0-5
    CHECK("table", table_value_encode(0xDEADBEEFu, 0x2ABCDEFu, 37u), (0xDEADBEEFull << 32) | (0x2ABCDEFull << 6) | 37ull);
    const uint32_t index[3] = {0u, 1u, (1u << 26) - 1u}, stamp[3] = {0u, 1u, 0xFFFFFFFFu};
    for (uint32_t color = 0; color < 64; ++color)
        for (uint32_t i : index)
            for (uint32_t s : stamp) {
                const unsigned long long v = table_value_encode(s, i, color);
                const TableValue t = table_value_decode(v);
                CHECK("table round trip", t.stamp, s); CHECK("table round trip", t.index, i); CHECK("table round trip", t.color, color);
                CHECK("table stamp", table_value_stamp(v), s);
            }
    CHECK("an index beyond 26 bits stays out of the stamp", table_value_stamp(table_value_encode(7u, 0xFFFFFFFFu, 0u)), 7);
    CHECK("no colour stays out of the index", table_color_field(kUncolored), 63);
}

static void impulses() {
    // pn[k], pt0[k], pt1[k] at floats 3k, 3k + 1, 3k + 2 of the 12
    const float pn[4] = {1.0f, 2.0f, 3.0f, 4.0f}, pt0[4] = {10.0f, 20.0f, 30.0f, 40.0f}, pt1[4] = {100.0f, 200.0f, 300.0f, 400.0f};
    Vec4 v[3];
    impulses_pack(pn, pt0, pt1, v[0], v[1], v[2]);
    float flat[12];
    std::memcpy(flat, v, sizeof flat);
    for (int k = 0; k < 4; ++k) {
        CHECK("impulse record", flat[3 * k], pn[k]); CHECK("impulse record", flat[3 * k + 1], pt0[k]); CHECK("impulse record", flat[3 * k + 2], pt1[k]);
        CHECK("lane q's three floats", impulses_point_offset((uint32_t)k), 3 * k);
    }
    for (uint32_t f = 0; f < 12; ++f) CHECK("one float", impulses_float(v[0], v[1], v[2], f), flat[f]);
    float a[4], b[4], c[4];
    impulses_unpack(v[0], v[1], v[2], a, b, c);
    CHECK("unpack", std::memcmp(a, pn, 16) | std::memcmp(b, pt0, 16) | std::memcmp(c, pt1, 16), 0);
    CHECK("sizes", kImpulseFloats, 12); CHECK("sizes", kImpulseVecs, 3); CHECK("sizes", kImpulseFloatsPerPoint, 3);
}

static void manifold_record() {
    // words: 0 a, 1 b, 2 count, 3 kept colour + 1 (0: none), 4-6 normal, 7 previous index, 8 + 4k .. point k xyz, depth
    CHECK("size", kManifoldBytes, 128); CHECK("size", kManifoldFloats, 32); CHECK("size", kManifoldVecs, 8);
    CHECK("word", kManifoldWordA, 0); CHECK("word", kManifoldWordB, 1); CHECK("word", kManifoldWordCount, 2); CHECK("word", kManifoldWordKept, 3);
    CHECK("word", kManifoldWordNormal, 4); CHECK("word", kManifoldWordPrev, 7); CHECK("word", kManifoldWordPoints, 8);
    CHECK("element", 4 * kManifoldVecHead, kManifoldWordA); CHECK("element", 4 * kManifoldVecNormal, kManifoldWordNormal);
    CHECK("element", 4 * kManifoldVecPoint, kManifoldWordPoints); CHECK("element", 4 * (kManifoldVecPoint + 4), kManifoldWordsUsed);
    Vec4 rec[8];
    std::memset(rec, 0, sizeof rec);
    manifold_head_encode(ManifoldHead{11u, 0x80000003u, 4u, 63u}, rec[kManifoldVecHead]);
    uint32_t words[32];
    std::memcpy(words, rec, sizeof words);
    CHECK("head", words[0], 11); CHECK("head", words[1], 0x80000003u); CHECK("head", words[2], 4); CHECK("head", words[3], 64);
    manifold_head_encode(ManifoldHead{0u, 0xFFFFFFFFu, 1u, kUncolored}, rec[kManifoldVecHead]);
    std::memcpy(words, rec, sizeof words);
    CHECK("head, new manifold", words[3], 0); CHECK("head, ground", words[1], 0xFFFFFFFFu);
    for (uint32_t color : {0u, 1u, 63u, kUncolored}) {
        Vec4 h;
        manifold_head_encode(ManifoldHead{5u, 6u, 3u, color}, h);
        const ManifoldHead d = manifold_head_decode(h);
        CHECK("head round trip", d.a, 5); CHECK("head round trip", d.b, 6); CHECK("head round trip", d.count, 3); CHECK("head round trip", d.color, color);
    }
    Vec4 nrm = {0.0f, 1.0f, 0.0f, float_of(123456u)};
    CHECK("previous index", manifold_prev_index(nrm), 123456);
    nrm.w = float_of(0xFFFFFFFFu);
    CHECK("no previous manifold", manifold_prev_index(nrm) == kNoPrevManifold, 1);
    CHECK("bits", rec_bits(1.0f), bits_of(1.0f)); CHECK("bits", bits_of(rec_float(0x7FC00001u)), 0x7FC00001u);
}

static void planes() {
    // prepared rows: 0 hdr, 1 n, 2-3 tb, 4-11 pt, 12-15 acc;  compact rows: 0, 1, 2-5 geo, 6-8 acc, 9-11 mass, 12-13 / 14-15 foreign B / A
    CHECK("prepared", kRowPlaneHdr, 0); CHECK("prepared", kRowPlaneN, 1); CHECK("prepared", kRowPlaneTb, 2); CHECK("prepared", kRowPlanePt, 4);
    CHECK("prepared", kRowPlaneAcc, 12); CHECK("prepared", kRowPlanes, 16);
    CHECK("compact", kClusterPlaneHdr, 0); CHECK("compact", kClusterPlaneN, 1); CHECK("compact", kClusterPlaneGeo, 2); CHECK("compact", kClusterPlaneAcc, 6);
    CHECK("compact", kClusterPlaneMass, 9); CHECK("compact", kClusterPlaneForeignB, 12); CHECK("compact", kClusterPlaneForeignA, 14);
    CHECK("plane offset", row_plane_floats(12, 1000), 48000);
    for (int k = 0; k < 4; ++k) {
        CHECK("pt planes", row_pt_plane_a(k), 2 * k); CHECK("pt planes", row_pt_plane_b(k), 2 * k + 1); CHECK("tb planes", row_tb_plane(k), k / 2);
    }
    // a point of a prepared row: {rA, normal mass} {rB, tangent mass 0}; tb: {tangent mass 1, bias} of the even point, then of the odd one
    const RowPoint even = {{1, 2, 3}, {4, 5, 6}, 7, 8, 9, 10}, odd = {{11, 12, 13}, {14, 15, 16}, 17, 18, 19, 20};
    Vec4 pa, pb, tb;
    row_point_encode(even, pa, pb);
    row_tb_encode(even, odd, tb);
    CHECK("pt a", pa.x == 1 && pa.y == 2 && pa.z == 3 && pa.w == 7, 1); CHECK("pt b", pb.x == 4 && pb.y == 5 && pb.z == 6 && pb.w == 8, 1);
    CHECK("tb", tb.x == 9 && tb.y == 10 && tb.z == 19 && tb.w == 20, 1);
    for (int k = 0; k < 4; ++k) {
        const RowPoint& want = (k & 1) ? odd : even;
        row_point_encode(want, pa, pb);
        const RowPoint got = row_point_decode(k, pa, pb, tb);
        CHECK("point round trip", std::memcmp(&got, &want, sizeof got), 0);
    }
}

static bool has(const std::string& text, const std::string& part) { return text.find(part) != std::string::npos; }

static void debug_notes() {
    uint32_t g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const CorruptRowNote row = {1001, 1002, 0x80000005u, 7, 1005, 1006, 61, 1008};
    corrupt_row_note_encode(row, g);
    const CorruptRowNote r2 = corrupt_row_note_decode(g);
    CHECK("corrupt row round trip", std::memcmp(&r2, &row, sizeof row), 0);
    SyncError e = sync_error(kOvfCorruptRow, g);
    CHECK("corrupt row text", has(e.message, "(row 1001: a 1002, b 2147483653, points 7; colour 61 rows [1005, 1006), tile base 1008)"), 1);

    const ClusterTimeoutNote note = {671, 672, 4000000000u, 123456, 0x80000001u, 65535, 65534, 0, 1, 1, 2, 63, 8};
    uint32_t h[8] = {kClusterTimeoutMark, 0, 0, 0, 0, 0, 0, 0};
    cluster_timeout_note_encode(note, h);
    CHECK("the mark is the site's", h[0], 0xC1);
    const ClusterTimeoutNote n2 = cluster_timeout_note_decode(h);
    CHECK("time-out round trip", std::memcmp(&n2, &note, sizeof note), 0);
    e = sync_error(kOvfHandoff, h);
    CHECK("time-out text", has(e.message, "cluster 671 of 672, row 4000000000, bodies 123456 / 2147483649, tickets 65535 / 65534, waiting A/B 0/1, modes 1/2, "
                                          "iteration 8, colour 63."), 1);
    // every field at both ends of its range
    for (uint32_t lo = 0; lo < 2; ++lo) {
        const ClusterTimeoutNote x = lo ? ClusterTimeoutNote{0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 3, 0, 0}
                                        : ClusterTimeoutNote{65535, 65535, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 65535, 65535, 1, 1, 3, 0, 255, 255};
        cluster_timeout_note_encode(x, h);
        const ClusterTimeoutNote y = cluster_timeout_note_decode(h);
        CHECK("time-out round trip", std::memcmp(&x, &y, sizeof x), 0);
    }
}

int main() {
    ticket();
    side_word();
    handoff_tag_word();
    table_value();
    impulses();
    manifold_record();
    planes();
    debug_notes();
    std::printf("records_probe: %lld checks passed\n", g_checks);
    return 0;
}
