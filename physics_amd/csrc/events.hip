// events.hip — contact events: which pairs began and stopped touching in an update, read off
// what the collision stage leaves on the device anyway. Two streaming kernels behind the solve of every update of a
// world with events on; a world that never enables them launches nothing of this file.
//
//   k_events_begin  over this update's manifolds: a manifold whose pair had one in the previous update (the narrow phase
//                   wrote that manifold's index into the record, from the persistent colour table) stamps
//                   ev_matched[index]; one whose pair had none raises BEGIN with its deepest point, its normal and the
//                   normal impulses its solve ended with.
//   k_events_end    over the previous update's manifolds: one that nobody stamped raises END.
//
// Events are appended to one buffer that lives across updates (also inside a phys_update_n batch). The cursor is
// reserved once per workgroup and trip (wave.hpp slots_reserve_flag: wave ballot + popcount, per-wave totals in LDS, ONE
// global atomic) because same-address atomics serialise chip-wide (~88 per microsecond). Slots at or beyond the capacity are not written; the
// cursor keeps counting, and the drain reports the difference as dropped.
#include "kernels.hpp"

namespace phys {

constexpr int kEventWaves = kEventThreads / 64;

// device words of the event state: {cursor (64 bits), manifold count of the even updates, ... of the odd updates}
struct EventState {
    unsigned long long cursor;  // events raised since the last drain (stored ones: the first `capacity` of them)
    uint32_t count[2];          // stored manifolds of the last two updates with events, by the update's parity
};

__device__ __forceinline__ void event_store(uint32_t* __restrict__ ev_buf, unsigned long long slot, uint4 w0, uint4 w1, uint4 w2) {
    uint4* o = reinterpret_cast<uint4*>(ev_buf) + 3 * slot;  // 48 bytes = phys_contact_event
    o[0] = w0; o[1] = w1; o[2] = w2;
}

__global__ __launch_bounds__(kEventThreads) void k_events_begin(const StepCounters* __restrict__ ctr, uint64_t max_manifolds,
                                                                const float* __restrict__ man_geo /* 128-byte records */,
                                                                const float* __restrict__ man_imp /* 12 floats per manifold */,
                                                                uint32_t* __restrict__ ev_matched, uint32_t stamp, uint32_t step,
                                                                uint32_t parity, EventState* __restrict__ st,
                                                                uint32_t* __restrict__ ev_buf, uint64_t capacity) {
    __shared__ SlotAppend<kEventWaves> sh;
    const uint32_t n = ctr->n_manifolds;  // final: the narrow phase ended launches ago
    const uint32_t M = (uint64_t)n < max_manifolds ? n : (uint32_t)max_manifolds;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->count[parity] = M;  // what the next update's k_events_end runs over
    const uint32_t stride = gridDim.x * kEventThreads;
    const uint32_t trips = (M + stride - 1) / stride;  // the same for every thread: the reservation has barriers
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint32_t m = trip * stride + blockIdx.x * kEventThreads + threadIdx.x;
        bool emit = false;
        uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0, w2 = w0;
        if (m < M) {
            const float4* rec = reinterpret_cast<const float4*>(man_geo) + kManifoldVecs * (size_t)m;
            const float4 r0 = rec[kManifoldVecHead], r1 = rec[kManifoldVecNormal];
            const uint32_t prev_m = manifold_prev_index(r1);
            if (prev_m != kNoPrevManifold) {
                // pairs are unique: no two lanes write one word
                if ((uint64_t)prev_m < max_manifolds) ev_matched[prev_m] = stamp;
            } else {
                emit = true;
                const ManifoldHead head = manifold_head_decode(r0);
                const uint32_t count = head.count;
                const float4 p0 = rec[kManifoldVecPoint], p1 = rec[kManifoldVecPoint + 1], p2 = rec[kManifoldVecPoint + 2], p3 = rec[kManifoldVecPoint + 3];
                const float4* imp = reinterpret_cast<const float4*>(man_imp) + kImpulseVecs * (size_t)m;
                const float4 i0 = imp[0], i1 = imp[1], i2 = imp[2];
                const float pn[4] = {impulses_float(i0, i1, i2, impulses_point_offset(0)), impulses_float(i0, i1, i2, impulses_point_offset(1)),
                                     impulses_float(i0, i1, i2, impulses_point_offset(2)), impulses_float(i0, i1, i2, impulses_point_offset(3))};
                // the deepest point: largest depth, lowest index on a tie
                float4 best = p0;
                if (count > 1u && p1.w > best.w) best = p1;
                if (count > 2u && p2.w > best.w) best = p2;
                if (count > 3u && p3.w > best.w) best = p3;
                const float n0 = count > 0u ? pn[0] : 0.0f, n1 = count > 1u ? pn[1] : 0.0f;
                const float n2 = count > 2u ? pn[2] : 0.0f, n3 = count > 3u ? pn[3] : 0.0f;
                const float impulse = ((n0 + n1) + n2) + n3;
                w0 = make_uint4(head.a, head.b, PHYS_CONTACT_BEGIN, step);
                w1 = make_uint4(__float_as_uint(best.x), __float_as_uint(best.y), __float_as_uint(best.z), __float_as_uint(impulse));
                w2 = make_uint4(__float_as_uint(r1.x), __float_as_uint(r1.y), __float_as_uint(r1.z), 0u);
            }
        }
        const unsigned long long slot = slots_reserve_flag(emit, trip, sh, &st->cursor);
        if (emit && slot < capacity) event_store(ev_buf, slot, w0, w1, w2);
    }
}

__global__ __launch_bounds__(kEventThreads) void k_events_end(uint64_t max_manifolds, const float* __restrict__ man_geo_prev,
                                                              const uint32_t* __restrict__ ev_matched, uint32_t stamp, uint32_t step,
                                                              uint32_t parity_prev, EventState* __restrict__ st,
                                                              uint32_t* __restrict__ ev_buf, uint64_t capacity) {
    __shared__ SlotAppend<kEventWaves> sh;
    const uint32_t n = st->count[parity_prev];  // left by the previous update's k_events_begin; 0 after a reset
    const uint32_t M = (uint64_t)n < max_manifolds ? n : (uint32_t)max_manifolds;
    const uint32_t stride = gridDim.x * kEventThreads;
    const uint32_t trips = (M + stride - 1) / stride;
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint32_t k = trip * stride + blockIdx.x * kEventThreads + threadIdx.x;
        bool emit = false;
        uint4 w0 = make_uint4(0, 0, 0, 0);
        if (k < M && ev_matched[k] != stamp) {
            emit = true;
            static_assert(kManifoldWordA == 0 && kManifoldWordB == 1, "a and b are the record's first eight bytes");
            const uint2 ab = *reinterpret_cast<const uint2*>(man_geo_prev + kManifoldFloats * (size_t)k);
            w0 = make_uint4(ab.x, ab.y, PHYS_CONTACT_END, step);
        }
        const unsigned long long slot = slots_reserve_flag(emit, trip, sh, &st->cursor);
        if (emit && slot < capacity) event_store(ev_buf, slot, w0, make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0));
    }
}

static_assert(sizeof(EventState) == 16, "cursor | two counts");

// (re)allocates what events need for the world's current manifold capacity; the buffers of a world with events off are freed
int32_t events_alloc(phys_world* w) {
    if (w->ev_capacity == 0) {
        w->ev_buf.free(); w->ev_matched.free(); w->ev_state.free();
        return PHYS_OK;
    }
    PHYS_HIP_TRY(w->ev_buf.resize(12 * (size_t)w->ev_capacity));
    PHYS_HIP_TRY(w->ev_state.resize(4));
    if (w->max_manifolds && w->ev_matched.n < w->max_manifolds) {
        PHYS_HIP_TRY(w->ev_matched.resize(w->max_manifolds));
        // no stamp is ever 0 (launch_events), and stamps only grow: zeroed words match no update
        PHYS_HIP_TRY(hipMemsetAsync(w->ev_matched.p, 0, 4 * w->ev_matched.n, w->stream));
    }
    return PHYS_OK;
}

// forget the contact history and the events not yet drained (phys_set_bodies, phys_set_static_bodies: the ids name other things)
int32_t events_reset(phys_world* w) {
    if (w->ev_capacity == 0 || !w->ev_state.p) return PHYS_OK;
    PHYS_HIP_TRY(hipMemsetAsync(w->ev_state.p, 0, sizeof(EventState), w->stream));
    return PHYS_OK;
}

// `step`: phys_stats.steps after this update (low 32 bits)
void launch_events(phys_world* w, uint32_t step, uint32_t blocks) {
    if (w->ev_capacity == 0 || !w->ev_matched.p || w->n == 0) return;
    // The stamp that says "matched in THIS update": a 32-bit count of the updates with events of this world, never 0 (the
    // value of a fresh ev_matched). At its wrap - 2^32 updates, months of stepping - the words are zeroed and the count
    // starts again at 1, so a stamp written 2^32 updates ago can never pass for this update's.
    if (++w->ev_stamp == 0u) {
        PHYS_PROF(w, PHYS_STAGE_MISC);
        (void)hipMemsetAsync(w->ev_matched.p, 0, 4 * w->ev_matched.n, w->stream);
        w->ev_stamp = 1u;
    }
    const uint32_t parity = w->ev_parity;
    w->ev_parity ^= 1u;
    EventState* st = reinterpret_cast<EventState*>(w->ev_state.p);
    { PHYS_PROF(w, PHYS_STAGE_MISC);
      hipLaunchKernelGGL(k_events_begin, dim3(blocks), dim3(kEventThreads), 0, w->stream, w->counters.p, w->max_manifolds,
                         w->man_geo.p, w->man_imp.p, w->ev_matched.p, w->ev_stamp, step, parity, st, w->ev_buf.p, w->ev_capacity); }
    { PHYS_PROF(w, PHYS_STAGE_MISC);
      hipLaunchKernelGGL(k_events_end, dim3(blocks), dim3(kEventThreads), 0, w->stream, w->max_manifolds, w->man_geo_prev.p,
                         w->ev_matched.p, w->ev_stamp, step, parity ^ 1u, st, w->ev_buf.p, w->ev_capacity); }
}

}  // namespace phys

using namespace phys;

extern "C" {

int32_t phys_contact_events_enable(phys_world* w, uint64_t capacity) {
    ENTER(w);
    if (capacity >= (1ull << 31)) return fail(PHYS_ERR_INVALID_ARG, "phys_contact_events_enable: capacity must be below 2^31");
    if (!(w->cfg.flags & PHYS_FLAG_COLLISIONS) || (w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY))
        return fail(PHYS_ERR_UNSUPPORTED, "contact events need PHYS_FLAG_COLLISIONS without PHYS_FLAG_BROADPHASE_ONLY");
    // the previous update's records and the impulse records exist only in worlds with warm starting (w->warm once bodies are set)
    const uint64_t cap_cfg = w->cfg.max_manifolds;
    if ((w->cfg.flags & PHYS_FLAG_NO_WARM_START) || (w->n ? !w->warm : cap_cfg >= (1ull << 26)))
        return fail(PHYS_ERR_UNSUPPORTED, "contact events need warm starting: no PHYS_FLAG_NO_WARM_START, manifold capacity below 2^26");
    if (capacity == w->ev_capacity) return PHYS_OK;
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    const bool was_on = w->ev_capacity != 0;
    w->ev_capacity = capacity;
    if (capacity == 0) return events_alloc(w);  // off: buffers freed, pending events gone
    w->ev_buf.free();  // a new capacity: a buffer of exactly that size
    PHYS_TRY(events_alloc(w));
    EventState h{};
    if (was_on) {
        PHYS_HIP_TRY(hipMemcpyAsync(&h, w->ev_state.p, sizeof(h), hipMemcpyDeviceToHost, w->stream));
        PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
        h.cursor = 0;  // a new capacity drops the pending events, nothing else
    } else if (w->ctab_valid && w->n) {
        // Enabling resets nothing: the next update reports against the last one, whose records are on the device and whose
        // manifold count is in the step counters (a phys_broadphase call since then has zeroed it: no END events then).
        uint32_t n = 0;
        PHYS_HIP_TRY(hipMemcpyAsync(&n, &w->counters.p->n_manifolds, 4, hipMemcpyDeviceToHost, w->stream));
        PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
        h.count[w->ev_parity ^ 1u] = (uint64_t)n < w->max_manifolds ? n : (uint32_t)w->max_manifolds;
    }
    PHYS_HIP_TRY(hipMemcpyAsync(w->ev_state.p, &h, sizeof(h), hipMemcpyHostToDevice, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));  // `h` dies here
    return PHYS_OK;
}

int32_t phys_get_contact_events(phys_world* w, phys_contact_event* out, uint64_t cap, uint64_t* n, uint64_t* n_dropped) {
    ENTER(w);
    if (!n) return fail(PHYS_ERR_INVALID_ARG, "phys_get_contact_events: null n");
    if (cap && !out) return fail(PHYS_ERR_INVALID_ARG, "phys_get_contact_events: null out with cap > 0");
    if (w->ev_capacity == 0) return fail(PHYS_ERR_UNSUPPORTED, "contact events are off (phys_contact_events_enable)");
    static_assert(offsetof(EventState, cursor) == 0, "the cursor is the first word of the event state");
    return drain_events(w, w->ev_state.p, w->ev_capacity, w->ev_buf.p, out, cap, n, n_dropped,
                        "phys_get_contact_events: more events stored than cap (*n says how many); nothing was drained");
}

int32_t phys_get_contact_impulses(phys_world* w, float* out, uint64_t cap, uint64_t* n_manifolds) {
    ENTER(w);
    if (!n_manifolds) return fail(PHYS_ERR_INVALID_ARG, "phys_get_contact_impulses: null n_manifolds");
    if (!w->warm || !(w->cfg.flags & PHYS_FLAG_COLLISIONS) || (w->cfg.flags & PHYS_FLAG_BROADPHASE_ONLY))
        return fail(PHYS_ERR_UNSUPPORTED, "contact impulses are kept only in worlds with collisions and warm starting");
    uint32_t counted = 0;
    PHYS_HIP_TRY(hipMemcpyAsync(&counted, &w->counters.p->n_manifolds, 4, hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    const uint64_t m = (uint64_t)counted < w->max_manifolds ? counted : w->max_manifolds;
    *n_manifolds = m;
    if (!out || m == 0) return PHYS_OK;
    // the head element of every manifold record and the impulse records (records.hpp), storage order
    std::vector<uint32_t> head(4 * m);
    std::vector<float> imp(kImpulseFloats * m);
    PHYS_HIP_TRY(hipMemcpy2DAsync(head.data(), 16, w->man_geo.p + 4 * kManifoldVecHead, kManifoldBytes, 16, m, hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipMemcpyAsync(imp.data(), w->man_imp.p, kImpulseFloats * sizeof(float) * m, hipMemcpyDeviceToHost, w->stream));
    PHYS_HIP_TRY(hipStreamSynchronize(w->stream));
    const std::vector<uint64_t> order = manifold_order(head.data() + kManifoldWordA, 4, m);  // phys_get_manifolds' order
    for (uint64_t k = 0; k < m && k < cap; ++k) {
        const uint64_t s = order[k];
        const uint32_t count = head[4 * s + kManifoldWordCount];
        for (uint32_t q = 0; q < kImpulseFloats; ++q)
            out[kImpulseFloats * k + q] = q / kImpulseFloatsPerPoint < count ? imp[kImpulseFloats * s + q] : 0.0f;
    }
    return PHYS_OK;
}

}  // extern "C"
