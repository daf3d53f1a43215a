// trigger.hip — trigger volumes: shapes that report which bodies are inside them and which
// entered or left in an update. Not bodies, not statics: they are evaluated by a kernel of their own against the poses the
// position step leaves, so nothing an update computes depends on them. A world without triggers launches nothing of
// this file. The records (include/spec/volume.h vol_record) are built on the host (setup.hpp trigger_records) and copied here.
//
//   k_trigger_eval   one lane per owned body, a short loop over the triggers: the records travel through LDS in tiles of 32
//                    (every lane reads the same record: a broadcast), a lane rejects by AABB and mask, runs the overlap
//                    queries' exact test (shape_overlap.hpp: trigger = query, body = target), and builds its occupancy 32
//                    triggers at a time. The word is XORed with the word of the previous update: the set bits are the
//                    lane's events, ENTER where the new word has the bit.
//
// Occupancy is a bit matrix that lives across updates, plane-major: word (k / 32) of body i at [(k / 32) * n_owned + i], so
// the loads and stores of one word by a wave are one contiguous 256-byte span. 4 * ceil(T / 32) * n_owned bytes: 128 MB
// for 1M bodies and 1024 triggers.
//
// Events are appended like contact events (events.hip): one reservation per workgroup and trip (wave.hpp
// slots_reserve_count: a wave prefix sum of the lanes' event COUNTS - a lane may hold up to 32 -, per-wave totals in LDS,
// ONE global atomic) because same-address atomics serialise chip-wide. Slots at or beyond the capacity are not written; the cursor keeps counting.
#include <cmath>
#include <vector>

#include "shape_overlap.hpp"

namespace phys {

namespace {

constexpr int kTgThreads = 256;
constexpr int kTgWaves = kTgThreads / 64;
constexpr uint32_t kTgTile = 32;      // triggers per LDS tile = bits per occupancy word
static_assert(kTgTile * VOL_REC_VEC <= (uint32_t)kTgThreads, "one 16-byte vector per thread stages a tile");
static_assert(sizeof(vol_record) == 16 * VOL_REC_VEC, "records are whole 16-byte vectors");

// MASKED: the trigger set has masks - body i is seen by trigger k iff (category[i] & mask[k]) != 0; without it no filter is
// loaded. EVENTS: trigger events are on (the occupancy is kept either way).
template <bool MASKED, bool EVENTS>
__global__ __launch_bounds__(kTgThreads) void k_trigger_eval(uint32_t n, const float* __restrict__ pos, const float* __restrict__ rot,
                                                             const float* __restrict__ he, const uint32_t* __restrict__ shape,
                                                             const uint2* __restrict__ filt, const float4* __restrict__ rec, uint32_t T,
                                                             uint32_t* __restrict__ bits, uint32_t step,
                                                             unsigned long long* __restrict__ cursor, uint4* __restrict__ ev_buf,
                                                             uint64_t capacity) {
    __shared__ vol_f4 tile[kTgTile * VOL_REC_VEC];
    __shared__ SlotAppend<kTgWaves> sh;
    const uint32_t i = blockIdx.x * kTgThreads + threadIdx.x;
    const bool live = i < n;  // (no early return: the tiles and the reservation have barriers)
    bool shaped = false;      // SPHERE, BOX or CAPSULE at a finite pose: what can be an occupant at all
    aabb_t ba;
    ba.lo = ba.hi = v3_make(0.0f, 0.0f, 0.0f);
    QShape B;
    B.type = PHYS_SHAPE_NONE;
    B.c = B.h = v3_make(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 9; ++k) B.R.m[k] = 0.0f;
    uint32_t category = 0xFFFFu;
    if (live) {
        const uint32_t type = shape[i];
        const v3 c = ld3(pos, i), h = ld3(he, i);
        const float4 q4 = reinterpret_cast<const float4*>(rot)[i];
        shaped = rc_aabb_of(c, q4, h, type, &ba);
        if (shaped) B = qs_make(type, c, q4, h);
        if (MASKED) category = filt[i].x & 0xFFFFu;
    }
    const uint32_t words = (T + kTgTile - 1) / kTgTile;
    for (uint32_t wd = 0; wd < words; ++wd) {
        const uint32_t t0 = wd * kTgTile;
        const uint32_t tn = min(kTgTile, T - t0);
        tile_stage<VOL_REC_VEC>(tile, reinterpret_cast<const vol_f4*>(rec), t0, tn);
        uint32_t now = 0;
        if (shaped) {
#pragma unroll 1
            for (uint32_t k = 0; k < tn; ++k) {
                const vol_f4 a0 = tile[VOL_REC_VEC * k], a1 = tile[VOL_REC_VEC * k + 1];
                if (MASKED && (category & vol_mask(a1)) == 0u) continue;
                if (!vol_box_meets(a0, a1, ba.lo, ba.hi)) continue;
                const vol_f4 r2 = tile[VOL_REC_VEC * k + 2], r3 = tile[VOL_REC_VEC * k + 3], r4 = tile[VOL_REC_VEC * k + 4],
                             r5 = tile[VOL_REC_VEC * k + 5];
                QShape Q;
                Q.type = vol_word(a0);
                Q.c = vol_centre(r2);
                Q.h = vol_half_extent(r2, r3, r4);
                Q.R = vol_rotation(r3, r4, r5);
                if (qr_overlap(Q, B)) now |= 1u << k;
            }
        }
        uint32_t diff = 0;
        if (live) {
            uint32_t* word = bits + (size_t)wd * n + i;
            diff = *word ^ now;
            if (diff) *word = now;
        }
        if (EVENTS) {
            unsigned long long slot = slots_reserve_count<kTgWaves>((uint32_t)__popc(diff), wd, sh, cursor);
            while (diff) {
                const uint32_t b = (uint32_t)__ffs((int)diff) - 1u;
                diff &= diff - 1u;
                if (slot < capacity) ev_buf[slot] = make_uint4(t0 + b, i, ((now >> b) & 1u) ? PHYS_TRIGGER_ENTER : PHYS_TRIGGER_EXIT, step);
                ++slot;
            }
        }
    }
}

}  // namespace

// an empty occupancy for the world's current trigger and body counts, and no pending events
int32_t triggers_reset(phys_world* w) {
    if (w->tg_cursor.p) PHYS_HIP_TRY(hipMemsetAsync(w->tg_cursor.p, 0, sizeof(unsigned long long), w->stream));
    if (w->n_triggers == 0) return PHYS_OK;
    const size_t words = (size_t)((w->n_triggers + kTgTile - 1) / kTgTile) * (size_t)w->n_owned;
    PHYS_HIP_TRY(w->tg_bits.resize(words));
    w->tg_bits_bodies = w->n_owned;
    if (words) PHYS_HIP_TRY(hipMemsetAsync(w->tg_bits.p, 0, 4 * words, w->stream));
    return PHYS_OK;
}

int32_t triggers_set(phys_world* w, TriggerStaging&& staged) {
    const uint64_t n = staged.staged.size();
    if (n != w->n_triggers) w->tg_bits.free();  // another word count: another layout
    w->n_triggers = 0;  // (a failure below leaves a world without triggers, not half a set)
    w->tg_masked = staged.masked;
    w->tg_host = std::move(staged.staged);
    if (n == 0) {  // back to launching nothing
        w->tg_rec.free();
        w->tg_bits_bodies = 0;
        if (w->tg_capacity == 0) w->tg_cursor.free();
        return triggers_reset(w);
    }
    PHYS_HIP_TRY(w->tg_cursor.resize(1));
    PHYS_TRY(upload_records(w, w->tg_rec, trigger_records(w->tg_host)));
    w->n_triggers = n;
    return triggers_reset(w);
}

int32_t triggers_rebuild(phys_world* w) {
    if (w->n_triggers == 0) return PHYS_OK;
    return upload_records(w, w->tg_rec, trigger_records(w->tg_host));  // on the world's stream: behind the updates already enqueued
}

// `step`: phys_stats.steps after this update (low 32 bits)
void launch_triggers(phys_world* w, uint32_t step) {
    if (w->n_triggers == 0 || w->n_owned == 0) return;  // (tg_bits is laid out for n_owned: triggers_reset behind every change of either)
    const unsigned blocks = (unsigned)((w->n_owned + kTgThreads - 1) / kTgThreads);
    PHYS_PROF(w, PHYS_STAGE_MISC);
    dispatch_bool(w->tg_masked, [&](auto masked) {
        dispatch_bool(w->tg_capacity != 0, [&](auto events) {
            hipLaunchKernelGGL((k_trigger_eval<decltype(masked)::value, decltype(events)::value>), dim3(blocks), dim3(kTgThreads), 0, w->stream,
                               (uint32_t)w->n_owned, w->pos.p, w->rot.p, w->half_extent.p, w->shape.p,
                               reinterpret_cast<const uint2*>(w->filt.p), reinterpret_cast<const float4*>(w->tg_rec.p),
                               (uint32_t)w->n_triggers, w->tg_bits.p, step, w->tg_cursor.p, reinterpret_cast<uint4*>(w->tg_buf.p),
                               w->tg_capacity);
        });
    });
}

}  // namespace phys

using namespace phys;

extern "C" {

int32_t phys_trigger_events_enable(phys_world* w, uint64_t capacity) {
    ENTER(w);
    if (capacity >= (1ull << 31)) return fail(PHYS_ERR_INVALID_ARG, "phys_trigger_events_enable: capacity must be below 2^31");
    if (capacity == w->tg_capacity) return PHYS_OK;
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    w->tg_capacity = capacity;
    w->tg_buf.free();  // a new capacity: a buffer of exactly that size; off: freed, pending events gone
    if (capacity == 0) {
        if (w->n_triggers == 0) w->tg_cursor.free();
    } else {
        PHYS_HIP_TRY(w->tg_buf.resize(4 * (size_t)capacity));
        PHYS_HIP_TRY(w->tg_cursor.resize(1));
    }
    // a new capacity drops the pending events, nothing else: the occupancy stays
    if (w->tg_cursor.p) PHYS_HIP_TRY(hipMemsetAsync(w->tg_cursor.p, 0, sizeof(unsigned long long), w->stream));
    return PHYS_OK;
}

int32_t phys_get_trigger_events(phys_world* w, phys_trigger_event* out, uint64_t cap, uint64_t* n, uint64_t* n_dropped) {
    ENTER(w);
    if (!n) return fail(PHYS_ERR_INVALID_ARG, "phys_get_trigger_events: null n");
    if (cap && !out) return fail(PHYS_ERR_INVALID_ARG, "phys_get_trigger_events: null out with cap > 0");
    if (w->tg_capacity == 0) return fail(PHYS_ERR_UNSUPPORTED, "trigger events are off (phys_trigger_events_enable)");
    return drain_events(w, w->tg_cursor.p, w->tg_capacity, w->tg_buf.p, out, cap, n, n_dropped,
                        "phys_get_trigger_events: more events stored than cap (*n says how many); nothing was drained");
}

int32_t phys_get_trigger_overlaps(phys_world* w, uint64_t cap, uint64_t* offsets_out, uint32_t* ids_out) {
    ENTER(w);
    if (!offsets_out) return fail(PHYS_ERR_INVALID_ARG, "phys_get_trigger_overlaps: null offsets_out");
    if (cap && !ids_out) return fail(PHYS_ERR_INVALID_ARG, "phys_get_trigger_overlaps: null ids_out with cap > 0");
    const uint64_t T = w->n_triggers, nb = w->n_owned;
    for (uint64_t k = 0; k <= T; ++k) offsets_out[k] = 0;
    if (T == 0 || nb == 0 || !w->tg_bits.p || w->tg_bits_bodies != nb) return PHYS_OK;
    // the bit matrix to the host, one plane of 32 triggers at a time; not a hot path
    const uint64_t words = (T + kTgTile - 1) / kTgTile;
    std::vector<uint32_t> h((size_t)(words * nb));
    PHYS_HIP_TRY(hipMemcpyAsync(h.data(), w->tg_bits.p, 4 * h.size(), hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    if (!trigger_bits_to_csr(h.data(), words, nb, T, cap, offsets_out, ids_out))
        return fail(PHYS_ERR_CAPACITY, "phys_get_trigger_overlaps: the ids need offsets_out[n] slots, more than cap");
    return PHYS_OK;
}

}  // extern "C"
