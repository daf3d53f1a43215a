/* physics_hip_boxcast.h - the four entry points of the box cast. Part of physics_hip.h, which includes it beside phys_capsulecast
 * and documents the call there (semantics, arguments, errors): include physics_hip.h, not this file. It relies on what
 * physics_hip.h has declared by then (stdint.h, phys_world, the extern "C" block it is included in). */
#ifndef PHYSICS_HIP_BOXCAST_H
#define PHYSICS_HIP_BOXCAST_H
#ifndef PHYSICS_HIP_H
#error "include physics_hip.h, which includes this header"
#endif

int32_t phys_boxcast(phys_world* w, uint64_t n, const float* origin /*3n*/, const float* dir /*3n*/,
                     const float* rot_ijkw /*4n, NULL = identity*/, const float* half_extent /*3n*/,
                     const float* max_t /*n, NULL = +inf*/, const uint32_t* ignore_body /*n, NULL = none*/,
                     uint32_t* body_out /*n*/, float* t_out /*n*/, float* normal_out /*3n, may be NULL*/,
                     float* point_out /*3n, may be NULL*/);
int32_t phys_boxcast_device(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                            const float* half_extent, const float* max_t, const uint32_t* ignore_body,
                            uint32_t* body_out, float* t_out, float* normal_out, float* point_out);
int32_t phys_boxcast_filtered(phys_world* w, uint64_t n, const float* origin /*3n*/, const float* dir /*3n*/,
                              const float* rot_ijkw /*4n, NULL = identity*/, const float* half_extent /*3n*/,
                              const float* max_t /*n, NULL = +inf*/, const uint32_t* ignore_body /*n, NULL = none*/,
                              const uint16_t* query_mask /*n, NULL = no filtering*/,
                              uint32_t* body_out /*n*/, float* t_out /*n*/, float* normal_out /*3n, may be NULL*/,
                              float* point_out /*3n, may be NULL*/);
int32_t phys_boxcast_device_filtered(phys_world* w, uint64_t n, const float* origin, const float* dir, const float* rot_ijkw,
                                     const float* half_extent, const float* max_t, const uint32_t* ignore_body,
                                     const uint16_t* query_mask, uint32_t* body_out, float* t_out, float* normal_out,
                                     float* point_out);

#endif /* PHYSICS_HIP_BOXCAST_H */
