// handoff.hpp — how k_solve_flow, k_solve_flow_quad (solver.hip) and k_solve_cluster (cluster.hip) pass body velocities and
// accumulated impulses between workgroups: the only text that addresses, loads, compares and stores a granule. The protocol
// and each kernel's no-deadlock argument are told once; the tag word and its limits: records.hpp.
#pragma once
#include "kernels.hpp"

namespace phys {

// A granule is {x, y, z, tag}, written by ONE 16-byte store and read by 16-byte loads only: the tag is the data's ready flag.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 ld_granule(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
    // sc0 | sc1 (what the volatile form emits): read past this XCD's L2. With sc1 alone ("agent scope") a poll could keep
    // hitting a line its own XCD had cached before the other XCD's write-through store landed: one run in two of two
    // worlds stepping side by side ended in the hand-off time-out (tools/ghost_cluster_stress.py), none with this form -
    // and the scope made no difference in time. (Volatile also makes the compiler re-issue the load in every sweep.)
    return __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, (int)0x80000010);
}
__device__ __forceinline__ void st_granule(__amdgpu_buffer_rsrc_t r, uint32_t byte_off, v3 v, uint32_t tag) {
    u32x4 g;
    g.x = __float_as_uint(v.x); g.y = __float_as_uint(v.y); g.z = __float_as_uint(v.z); g.w = tag;
    __builtin_amdgcn_raw_buffer_store_b128(g, r, byte_off, 0, 16);  // sc1: write-through
}
__device__ __forceinline__ v3 granule_v3(u32x4 g) { return v3_make(__uint_as_float(g.x), __uint_as_float(g.y), __uint_as_float(g.z)); }

// One kernel's view of one granule buffer in one solve: its raw-buffer descriptor and the solve's epoch, kept in place as tag 0.
struct Handoff {
    __amdgpu_buffer_rsrc_t buf;
    uint32_t epoch, tag0;
    __device__ __forceinline__ uint32_t tag(uint32_t updates) const { return handoff_tag_from(tag0, updates); }
    // one granule: taken into `x` if it carries update `ticket`, else `gap` says how many updates away it is
    __device__ __forceinline__ bool take(u32x4 g, uint32_t ticket, v3& x, uint32_t& gap) const {
        if (g.w == tag(ticket)) { x = granule_v3(g); return true; }
        gap = handoff_gap(g.w, epoch, ticket);
        return false;
    }
    __device__ __forceinline__ void publish(uint32_t byte_off, v3 x, uint32_t updates) const { st_granule(buf, byte_off, x, tag(updates)); }
};
__device__ __forceinline__ Handoff handoff_over(void* base, uint32_t bytes, uint32_t epoch) { return {__builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000), epoch, handoff_tag(epoch, 0u)}; }
// the bodies' granules (flow_vel) and the impulse granules {pn, pt0, pt1, tag = sweeps finished} of the prepared rows' acc planes
__device__ __forceinline__ Handoff body_handoff(float* flow_vel, uint32_t n_bodies, uint32_t epoch) { return handoff_over(flow_vel, n_bodies * kBodyGranuleBytes, epoch); }
__device__ __forceinline__ Handoff impulse_handoff(float4* acc, uint32_t cap, uint32_t epoch) { return handoff_over(acc, cap * (kGranuleBytes * kRowAccPlanes), epoch); }
__device__ __forceinline__ uint32_t body_granule(uint32_t body, bool angular) { return body * kBodyGranuleBytes + (angular ? kGranuleBytes : 0u); }
__device__ __forceinline__ uint32_t impulse_granule(uint32_t k, uint32_t cap, uint32_t d) { return (k * cap + d) * kGranuleBytes; }

// A body's two granules, in two steps so that a kernel can issue every load of a sweep before its first compare.
struct BodyGranules { u32x4 lin, ang; };
__device__ __forceinline__ BodyGranules ld_body(const Handoff& h, uint32_t body) {
    return {ld_granule(h.buf, body_granule(body, false)), ld_granule(h.buf, body_granule(body, true))};
}
// taken into v, w if BOTH carry update `ticket`; else the gap (read off the linear one)
__device__ __forceinline__ bool take_body(const Handoff& h, const BodyGranules& g, uint32_t ticket, v3& v, v3& w, uint32_t& gap) {
    const uint32_t want = h.tag(ticket);
    if (g.lin.w == want && g.ang.w == want) { v = granule_v3(g.lin); w = granule_v3(g.ang); return true; }
    gap = handoff_gap(g.lin.w, h.epoch, ticket);
    return false;
}
__device__ __forceinline__ void publish_body(const Handoff& h, uint32_t body, v3 v, v3 w, uint32_t updates) {
    h.publish(body_granule(body, false), v, updates);
    h.publish(body_granule(body, true), w, updates);
}
// Every wait is a bounded spin. Somebody gave up (overflow bit kOvfHandoff): nobody waits or starts an item any more.
__device__ __forceinline__ bool handoff_abandoned(const StepCounters* ctr) { return (__hip_atomic_load(&ctr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kOvfHandoff) != 0u; }
// the give-up condition of a waiter (looked at every 64th sweep of a spin); whoever sees it flags kOvfHandoff
__device__ __forceinline__ bool handoff_give_up(const StepCounters* ctr, long long t_start, long long timeout_ticks) { return (wall_clock64() - t_start > timeout_ticks) || handoff_abandoned(ctr); }
// back-off of a waiting dataflow wave, in proportion to how many hops away the nearest waiting lane is, and its bounded
// spin: true when the wave gives up (flagged by lane 0). Waiting waves cost issue slots and L2 bandwidth, so the flow
// launches are sized to about one wave per SIMD (plan_solver) and waiters back off by their distance in hops.
__device__ __forceinline__ bool flow_backoff(StepCounters* ctr, bool done, uint32_t gap, uint32_t& sweeps, long long t_start, long long timeout_ticks) {
    if (__any(!done && gap <= 1u)) __builtin_amdgcn_s_sleep(1);
    else if (__any(!done && gap <= 4u)) __builtin_amdgcn_s_sleep(40);
    else __builtin_amdgcn_s_sleep(127);
    if ((++sweeps & 63u) != 0u) return false;
    const bool dead = handoff_give_up(ctr, t_start, timeout_ticks);
    if (dead && (threadIdx.x & 63u) == 0u) flag_overflow(ctr, kOvfHandoff);  // wave-uniform: both inputs are
    return dead;
}
// k_solve_cluster's waiters sleep a constant: 1 or 32 units instead of 8 changed nothing on C3 (0.630 / 0.627 ms)
constexpr int kClusterPollSleep = 8;

}  // namespace phys
