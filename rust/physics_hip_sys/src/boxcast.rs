//! The box cast's four entry points (include/physics_hip_boxcast.h, which include/physics_hip.h includes and documents):
//! re-exported from the crate root like every other declaration. They stand in a file of their own as their C declarations do.
use super::phys_world;

extern "C" {
    pub fn phys_boxcast(w: *mut phys_world, n: u64, origin: *const f32, dir: *const f32, rot_ijkw: *const f32, half_extent: *const f32,
                        max_t: *const f32, ignore_body: *const u32, body_out: *mut u32, t_out: *mut f32, normal_out: *mut f32,
                        point_out: *mut f32) -> i32;
    pub fn phys_boxcast_device(w: *mut phys_world, n: u64, origin: *const f32, dir: *const f32, rot_ijkw: *const f32,
                               half_extent: *const f32, max_t: *const f32, ignore_body: *const u32, body_out: *mut u32,
                               t_out: *mut f32, normal_out: *mut f32, point_out: *mut f32) -> i32;
    pub fn phys_boxcast_filtered(w: *mut phys_world, n: u64, origin: *const f32, dir: *const f32, rot_ijkw: *const f32,
                                 half_extent: *const f32, max_t: *const f32, ignore_body: *const u32, query_mask: *const u16,
                                 body_out: *mut u32, t_out: *mut f32, normal_out: *mut f32, point_out: *mut f32) -> i32;
    pub fn phys_boxcast_device_filtered(w: *mut phys_world, n: u64, origin: *const f32, dir: *const f32, rot_ijkw: *const f32,
                                        half_extent: *const f32, max_t: *const f32, ignore_body: *const u32, query_mask: *const u16,
                                        body_out: *mut u32, t_out: *mut f32, normal_out: *mut f32, point_out: *mut f32) -> i32;
}
