// physics_backend.rs — the patch a maintainer of martingoe/physics adds as `src/physics/hip_backend.rs`
// (UNCOMPILED SOURCE: no Rust toolchain on the build machines). It replaces the bodies of
// PhysicsState::update / apply_gravity / step (src/physics.rs:41-55, 87-99) with calls into
// libphysics_hip.so and leaves get_render_data (physics.rs:58-85) and all of src/rendering untouched.
//
// It has to live INSIDE the physics module tree because RigidBody is repr(Rust) and `inertia_tensor` is
// private to rigid_body.rs (:15), `mass/force/torque` are pub(crate) (:7,12,13): the gather below reads
// them through one accessor added to rigid_body.rs:
//     impl RigidBody { pub(crate) fn inertia_row_major(&self) -> [f32; 9] { /* transpose of as_slice() */ } }
use crate::physics::constraints::Constraints;
use crate::physics::PhysicsState;
use physics_hip_sys as ffi;
use std::ffi::CStr;
use std::time::Duration;

pub struct HipBackend {
    world: *mut ffi::phys_world,
    uploaded_bodies: usize,
    uploaded_constraints: usize,
}

fn check(rc: i32) {
    if rc != ffi::PHYS_OK {
        // the reference panics in the same situations (unwrap at rigid_body.rs:31, index at physics.rs:48)
        let msg = unsafe { CStr::from_ptr(ffi::phys_last_error()) }.to_string_lossy().into_owned();
        panic!("physics_hip error {rc}: {msg}");
    }
}

impl HipBackend {
    pub fn new() -> Self {
        let mut cfg = std::mem::MaybeUninit::<ffi::phys_config>::uninit();
        let mut world = std::ptr::null_mut();
        unsafe {
            ffi::phys_config_default(cfg.as_mut_ptr()); // reference constants: gravity (0,-9.81,0) at (0,0,1.5), CG 1000/1e-2/1e-3
            // the frame loop renders on the same GPU (wgpu) while the next update may already run: the default (guarded start of
            // the contact solver's one big launch) is the right one; a headless batch run that has
            // the GPU to itself may add ffi::PHYS_FLAG_EXCLUSIVE_GPU
            check(ffi::phys_create(cfg.as_ptr(), &mut world));
        }
        Self { world, uploaded_bodies: usize::MAX, uploaded_constraints: usize::MAX }
    }

    /// gather `entities` (AoS, repr(Rust)) into the flat arrays phys_set_bodies copies
    fn upload(&mut self, state: &PhysicsState) {
        let n = state.entities.len();
        let (mut pos, mut rot, mut lin, mut ang) = (Vec::with_capacity(3 * n), Vec::with_capacity(4 * n), Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        let (mut mass, mut inertia, mut force, mut torque) = (Vec::with_capacity(n), Vec::with_capacity(9 * n), Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for e in &state.entities {
            let b = &e.body;
            pos.extend_from_slice(b.position.as_slice());
            rot.extend_from_slice(b.rotation.coords.as_slice()); // nalgebra order [i, j, k, w]
            lin.extend_from_slice(b.lin_velocity.as_slice());
            ang.extend_from_slice(b.angular_velocity.as_slice());
            mass.push(b.mass);
            inertia.extend_from_slice(&b.inertia_row_major());
            force.extend_from_slice(b.force.as_slice());
            torque.extend_from_slice(b.torque.as_slice());
        }
        unsafe {
            check(ffi::phys_set_bodies(self.world, n as u64, pos.as_ptr(), rot.as_ptr(), lin.as_ptr(), ang.as_ptr(),
                                       mass.as_ptr(), inertia.as_ptr(), std::ptr::null(), std::ptr::null()));
            check(ffi::phys_set_forces(self.world, force.as_ptr(), torque.as_ptr()));
            check(ffi::phys_clear_constraints(self.world));
            for c in &state.constraint_solver.constraints {
                match c {
                    Constraints::FixedPosition(c) => check(ffi::phys_add_constraint_fix_point(self.world, c.rigid_body as u64, c.position.as_slice().as_ptr())),
                    Constraints::FixedOrientation(c) => check(ffi::phys_add_constraint_fix_orientation(self.world, c.rigid_body as u64, c.position.as_slice().as_ptr())),
                }
            }
        }
        self.uploaded_bodies = n;
        self.uploaded_constraints = state.constraint_solver.constraints.len();
    }

    /// scatter the device state back so get_render_data reads body.position / body.rotation as before
    fn download(&mut self, state: &mut PhysicsState) {
        let n = state.entities.len();
        let (mut pos, mut rot, mut lin, mut ang) = (vec![0f32; 3 * n], vec![0f32; 4 * n], vec![0f32; 3 * n], vec![0f32; 3 * n]);
        unsafe {
            check(ffi::phys_get_transforms(self.world, pos.as_mut_ptr(), rot.as_mut_ptr()));
            check(ffi::phys_get_velocities(self.world, lin.as_mut_ptr(), ang.as_mut_ptr()));
        }
        for (i, e) in state.entities.iter_mut().enumerate() {
            let b = &mut e.body;
            b.position.copy_from_slice(&pos[3 * i..3 * i + 3]);
            b.rotation = nalgebra::Unit::new_unchecked(nalgebra::Quaternion::new(rot[4 * i + 3], rot[4 * i], rot[4 * i + 1], rot[4 * i + 2]));
            b.lin_velocity.copy_from_slice(&lin[3 * i..3 * i + 3]);
            b.angular_velocity.copy_from_slice(&ang[3 * i..3 * i + 3]);
            b.force.fill(0.0);  // rigid_body.rs:38-39
            b.torque.fill(0.0);
        }
    }

    /// Closest hit of every ray against the bodies as the last update left them (phys_raycast): per ray the entity
    /// index, or None for a miss / Some(u32::MAX) = ffi::PHYS_RAY_GROUND for the ground, with t and the surface normal.
    /// `max_t` and `ignore` are optional per-ray slices of the same length as `origins`.
    pub fn raycast(&self, origins: &[[f32; 3]], dirs: &[[f32; 3]], max_t: Option<&[f32]>, ignore: Option<&[u32]>)
                   -> Vec<(Option<u32>, f32, [f32; 3])> {
        let n = origins.len();
        assert_eq!(dirs.len(), n);
        assert!(max_t.map_or(true, |m| m.len() == n) && ignore.map_or(true, |g| g.len() == n));
        let (mut body, mut t, mut normal) = (vec![0u32; n], vec![0f32; n], vec![[0f32; 3]; n]);
        if n > 0 {
            unsafe {
                check(ffi::phys_raycast(self.world, n as u64, origins.as_ptr() as *const f32, dirs.as_ptr() as *const f32,
                                        max_t.map_or(std::ptr::null(), |m| m.as_ptr()), ignore.map_or(std::ptr::null(), |g| g.as_ptr()),
                                        body.as_mut_ptr(), t.as_mut_ptr(), normal.as_mut_ptr() as *mut f32));
            }
        }
        (0..n).map(|i| (if body[i] == ffi::PHYS_RAY_MISS { None } else { Some(body[i]) }, t[i], normal[i])).collect()
    }

    /// First target a ball of `radius[i]` touches moving from `origins[i]` along `dirs[i]` (phys_spherecast): as `raycast`,
    /// t being the distance the centre travelled and the normal the target's outward normal at the contact.
    pub fn spherecast(&self, origins: &[[f32; 3]], dirs: &[[f32; 3]], radius: &[f32], max_t: Option<&[f32]>,
                      ignore: Option<&[u32]>) -> Vec<(Option<u32>, f32, [f32; 3])> {
        let n = origins.len();
        assert!(dirs.len() == n && radius.len() == n);
        assert!(max_t.map_or(true, |m| m.len() == n) && ignore.map_or(true, |g| g.len() == n));
        let (mut body, mut t, mut normal) = (vec![0u32; n], vec![0f32; n], vec![[0f32; 3]; n]);
        if n > 0 {
            unsafe {
                check(ffi::phys_spherecast(self.world, n as u64, origins.as_ptr() as *const f32, dirs.as_ptr() as *const f32,
                                           radius.as_ptr(), max_t.map_or(std::ptr::null(), |m| m.as_ptr()),
                                           ignore.map_or(std::ptr::null(), |g| g.as_ptr()), body.as_mut_ptr(), t.as_mut_ptr(),
                                           normal.as_mut_ptr() as *mut f32));
            }
        }
        (0..n).map(|i| (if body[i] == ffi::PHYS_RAY_MISS { None } else { Some(body[i]) }, t[i], normal[i])).collect()
    }

    /// Every target each query shape intersects (phys_overlap): per query the ascending ids (entity index,
    /// ffi::PHYS_STATIC_ID_BIT | k, ffi::PHYS_RAY_GROUND). `rot` is optional (identity); retries once on capacity.
    pub fn overlap(&self, shape_type: &[u32], pos: &[[f32; 3]], rot: Option<&[[f32; 4]]>, half_extent: &[[f32; 3]],
                   ignore: Option<&[u32]>) -> Vec<Vec<u32>> {
        let n = pos.len();
        assert!(shape_type.len() == n && half_extent.len() == n);
        assert!(rot.map_or(true, |r| r.len() == n) && ignore.map_or(true, |g| g.len() == n));
        let mut offsets = vec![0u64; n + 1];
        let mut ids = vec![0u32; 8 * n + 64];
        for attempt in 0..2 {
            let rc = unsafe {
                ffi::phys_overlap(self.world, n as u64, shape_type.as_ptr(), pos.as_ptr() as *const f32,
                                  rot.map_or(std::ptr::null(), |r| r.as_ptr() as *const f32), half_extent.as_ptr() as *const f32,
                                  ignore.map_or(std::ptr::null(), |g| g.as_ptr()), ids.len() as u64, offsets.as_mut_ptr(),
                                  ids.as_mut_ptr())
            };
            if rc == ffi::PHYS_ERR_CAPACITY && attempt == 0 {
                ids.resize(offsets[n] as usize, 0);
                continue;
            }
            check(rc);
            break;
        }
        (0..n).map(|i| ids[offsets[i] as usize..offsets[i + 1] as usize].to_vec()).collect()
    }

    /// PhysicsState::update (physics.rs:41-55). `dirty` = the caller touched entities/constraints since the
    /// last frame (lib.rs does at start-up only); when false the bodies stay resident on the GPU.
    pub fn update(&mut self, state: &mut PhysicsState, dt: &Duration, dirty: bool) {
        if dirty || self.uploaded_bodies != state.entities.len() || self.uploaded_constraints != state.constraint_solver.constraints.len() {
            self.upload(state);
        }
        unsafe { check(ffi::phys_update(self.world, dt.as_nanos() as u64)) }; // nanoseconds: as_secs_f32 is redone on the other side (quirk Q7)
        self.download(state);
    }
}

impl Drop for HipBackend {
    fn drop(&mut self) {
        unsafe { ffi::phys_destroy(self.world) };
    }
}
