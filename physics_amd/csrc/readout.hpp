// readout.hpp — what the read-out calls compute on the host once the bytes are there: sorted pair lists, the (a, b) order of
// manifolds, the rules and the order of an event drain, the trigger occupancy as CSR, and phys_sync's error text. Host-only like
// setup.hpp (no HIP, no phys_world), held to tests/cpp/setup_probe.cpp. The callers keep the copies and the clears.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "records.hpp"
#include "setup.hpp"

namespace phys {

// m pairs {i, j} in device order -> the first min(m, cap) of them in (i, j) order. A convenience of the read-out calls
// (phys_broadphase, phys_get_cross_pairs); the per-step pipeline never sorts.
inline void sort_pairs(const uint32_t* raw, uint64_t m, uint32_t* out, uint64_t cap) {
    std::vector<uint64_t> keys(m);
    for (uint64_t k = 0; k < m; ++k) keys[k] = ((uint64_t)raw[2 * k] << 32) | raw[2 * k + 1];
    std::sort(keys.begin(), keys.end());
    for (uint64_t k = 0; k < m && k < cap; ++k) {
        out[2 * k] = (uint32_t)(keys[k] >> 32);
        out[2 * k + 1] = (uint32_t)keys[k];
    }
}

// the permutation that puts m manifolds in (a, b) order; a and b are words 0 and 1 of records `stride` words apart (pairs are
// unique, so (a, b) fixes it: phys_get_manifolds and phys_get_contact_impulses agree)
inline std::vector<uint64_t> manifold_order(const uint32_t* ab, size_t stride, uint64_t m) {
    std::vector<uint64_t> order(m);
    for (uint64_t k = 0; k < m; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) {
        return ab[stride * x] < ab[stride * y] || (ab[stride * x] == ab[stride * y] && ab[stride * x + 1] < ab[stride * y + 1]);
    });
    return order;
}

// the order events are handed out in (device order is arbitrary)
inline bool event_before(const phys_contact_event& x, const phys_contact_event& y) {
    if (x.step != y.step) return x.step < y.step;
    if (x.kind != y.kind) return x.kind < y.kind;
    if (x.body_a != y.body_a) return x.body_a < y.body_a;
    return x.body_b < y.body_b;
}
inline bool event_before(const phys_trigger_event& x, const phys_trigger_event& y) {
    if (x.step != y.step) return x.step < y.step;
    if (x.kind != y.kind) return x.kind < y.kind;
    if (x.trigger != y.trigger) return x.trigger < y.trigger;
    return x.body < y.body;
}

// The rules of an event drain (phys_get_contact_events, phys_get_trigger_events), from the cursor - events raised since the
// last drain - and the capacity the device keeps: a count query (no buffer, cap 0) leaves everything as it is; more events
// stored than cap drains nothing; else the stored records are copied out, and only the cursor word is cleared (if non-zero).
struct EventDrain {
    uint64_t stored = 0, dropped = 0;
    bool count_only = false;  // nothing is copied, nothing cleared
    bool too_many = false;    // PHYS_ERR_CAPACITY: nothing is copied, nothing cleared
    bool clear_cursor = false;
};
inline EventDrain drain_rules(uint64_t cursor, uint64_t capacity, bool have_out, uint64_t cap) {
    EventDrain d;
    d.stored = cursor < capacity ? cursor : capacity;
    d.dropped = cursor - d.stored;
    d.count_only = !have_out && cap == 0;
    d.too_many = !d.count_only && d.stored > cap;
    d.clear_cursor = !d.count_only && !d.too_many && cursor != 0;
    return d;
}

// Trigger occupancy, plane-major bit matrix (word wd of body i at bits[wd * n_bodies + i], bit k % 32 of word k / 32 is trigger
// k) -> CSR: offsets[T + 1] always; the body ids of every trigger, ascending, when they fit in cap (the return value). Bits of
// triggers >= T (padding of the last word) are ignored.
inline bool trigger_bits_to_csr(const uint32_t* bits, uint64_t words, uint64_t n_bodies, uint64_t T, uint64_t cap, uint64_t* offsets,
                                uint32_t* ids) {
    std::vector<uint64_t> count((size_t)T, 0);
    for (uint64_t wd = 0; wd < words; ++wd)
        for (uint64_t i = 0; i < n_bodies; ++i)
            for (uint32_t m = bits[(size_t)(wd * n_bodies + i)]; m; m &= m - 1u) {
                const uint64_t k = wd * 32u + (uint32_t)__builtin_ctz(m);
                if (k < T) count[(size_t)k]++;
            }
    uint64_t run = 0;
    for (uint64_t k = 0; k < T; ++k) { offsets[k] = run; run += count[(size_t)k]; }
    offsets[T] = run;
    if (run > cap) return false;
    std::vector<uint64_t> at(offsets, offsets + T);
    for (uint64_t wd = 0; wd < words; ++wd)
        for (uint64_t i = 0; i < n_bodies; ++i)  // bodies ascending: every list ascending
            for (uint32_t m = bits[(size_t)(wd * n_bodies + i)]; m; m &= m - 1u) {
                const uint64_t k = wd * 32u + (uint32_t)__builtin_ctz(m);
                if (k < T) ids[at[(size_t)k]++] = (uint32_t)i;
            }
    return true;
}

// phys_sync: the overflow bits raised since the last call (kOvf*) and the eight debug words -> the code and the text. One error
// per call, in this precedence: corrupt row, hand-off time-out (with k_solve_cluster's note; both notes: records.hpp), colours,
// halo, colour table, then pairs / manifolds (any other bit too), and last a body edit's bad ids (kOvfBadEdit: an argument error
// of a device call, not a capacity).
struct SyncError {
    int32_t code = PHYS_OK;
    std::string message;
};
inline SyncError sync_error(uint32_t bits, const uint32_t g[8]) {
    const auto s = [](uint32_t v) { return std::to_string(v); };
    if (bits & kOvfCorruptRow) {
        const CorruptRowNote n = corrupt_row_note_decode(g);
        return {PHYS_ERR_HIP, "internal error: a solver row names no body of this world and was refused (row " + s(n.row) + ": a " + s(n.a) +
                              ", b " + s(n.b) + ", points " + s(n.count) + "; colour " + s(n.color) + " rows [" + s(n.color_start) + ", " +
                              s(n.color_end) + "), tile base " + s(n.tile_base) + ")"};
    }
    if ((bits & kOvfHandoff) && g[0] == kClusterTimeoutMark) {  // what the first lane of k_solve_cluster to give up was waiting for
        const ClusterTimeoutNote n = cluster_timeout_note_decode(g);
        return {PHYS_ERR_HIP, "contact solver hand-off timed out (k_solve_cluster) in a step since the last phys_sync; velocities "
                              "are invalid from that step on. First lane to give up: cluster " + s(n.cluster) + " of " + s(n.clusters) + ", row " +
                              s(n.row) + ", bodies " + s(n.a) + " / " + s(n.b) + ", tickets " + s(n.ticketA) + " / " + s(n.ticketB) +
                              ", waiting A/B " + s(n.waitA) + "/" + s(n.waitB) + ", modes " + s(n.modeA) + "/" + s(n.modeB) + ", iteration " +
                              s(n.iteration) + ", colour " + s(n.color) +
                              ". If other work shares this GPU with phys_update, create the world WITHOUT PHYS_FLAG_EXCLUSIVE_GPU"};
    }
    if (bits & kOvfHandoff)
        return {PHYS_ERR_HIP, "contact solver hand-off timed out (k_solve_flow) in a step since the last phys_sync; "
                              "velocities are invalid from that step on"};
    if (bits & kOvfColors)
        return {PHYS_ERR_CAPACITY, "a body has more than 64 contact manifolds (PHYS_MAX_COLORS): the contact solve of "
                                   "that step was skipped. This limit is not configurable"};
    if (bits & kOvfHalo)
        return {PHYS_ERR_CAPACITY, "halo record / cross-pair capacity exceeded in a step since the last phys_sync"};
    if (bits & kOvfColorTable)
        return {PHYS_ERR_CAPACITY, "the persistent colour table is full (a look-up or an insert gave up after thousands of "
                                   "slots): the contact solve of that step was skipped. Raise phys_config.max_manifolds"};
    if (bits & ~kOvfBadEdit)
        return {PHYS_ERR_CAPACITY, "pair / manifold capacity exceeded in a step since the last phys_sync (the contact "
                                   "solve of that step was skipped): raise phys_config.max_pairs / max_manifolds"};
    if (bits & kOvfBadEdit)
        return {PHYS_ERR_INVALID_ARG, "a body edit on device arrays since the last phys_sync met ids out of order or out of range: "
                                      "out-of-range entries were skipped, the bodies of out-of-order entries are unspecified"};
    return {};
}

}  // namespace phys
