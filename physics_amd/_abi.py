"""ctypes view of include/physics_hip.h (structs, constants, prototypes) and the loader of
libphysics_hip.so. There is no CPU fallback: if the HIP library is missing or no gfx950 device is
usable, creation fails loudly."""
import ctypes as C
import os

PHYS_ABI_VERSION = 2

PHYS_OK = 0
PHYS_ERR_INVALID_ARG = -1
PHYS_ERR_NO_DEVICE = -2
PHYS_ERR_HIP = -3
PHYS_ERR_SINGULAR_INERTIA = -4
PHYS_ERR_CAPACITY = -5
PHYS_ERR_OUT_OF_RANGE = -6
PHYS_ERR_UNSUPPORTED = -7
PHYS_ERR_NO_BODIES = -8

SHAPE_NONE, SHAPE_SPHERE, SHAPE_BOX = 0, 1, 2
# radius half_extent[0], core half-length half_extent[1] along the body's local y axis (include/physics_hip.h)
SHAPE_CAPSULE = 3
FLAG_COLLISIONS, FLAG_GROUND_PLANE, FLAG_EXACT_ROTATION, FLAG_BROADPHASE_ONLY = 1, 2, 4, 8
FLAG_SOLVER_PER_COLOR = 16
FLAG_SHARED_GPU = 32
FLAG_SOLVER_CLUSTER = 64
FLAG_EXCLUSIVE_GPU = 128
FLAG_NO_WARM_START = 256
GROUND_ID = 0xFFFFFFFF
RAY_MISS = 0xFFFFFFFE    # PHYS_RAY_MISS: no hit within max_t
RAY_GROUND = 0xFFFFFFFF  # PHYS_RAY_GROUND: the ground plane
STATIC_ID_BIT = 0x80000000  # PHYS_STATIC_ID_BIT: manifold body_b / ray body = STATIC_ID_BIT | k for static collider k
# collision filters (include/physics_hip.h): category u16, mask u16, group i16; these are the defaults (group 0)
FILTER_DEFAULT_CATEGORY = 0x0001
FILTER_DEFAULT_MASK = 0xFFFF
# contact events (include/physics_hip.h): phys_contact_event.kind
CONTACT_BEGIN, CONTACT_END = 1, 2
# trigger volumes (include/physics_hip.h): the most a world keeps, and phys_trigger_event.kind
MAX_TRIGGERS = 1024
TRIGGER_ENTER, TRIGGER_EXIT = 1, 2
# force fields (include/physics_hip.h): the most a world keeps, and the kinds of law
MAX_FORCE_FIELDS = 1024
FIELD_ACCEL, FIELD_DRAG, FIELD_RADIAL = 0, 1, 2
# liquids (include/physics_hip.h): the most a world keeps, and the read-out's "no liquid"
MAX_LIQUIDS = 1024
NO_LIQUID = 0xFFFFFFFF

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
u16p = C.POINTER(C.c_uint16)
i16p = C.POINTER(C.c_int16)


class PhysConfig(C.Structure):
    """struct phys_config (include/physics_hip.h)."""
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("device", C.c_int32),
        ("flags", C.c_uint32),
        ("gravity_force", C.c_float * 3),
        ("gravity_offset", C.c_float * 3),
        ("cg_max_iterations", C.c_uint32),
        ("cg_max_error", C.c_float),
        ("cg_min_error", C.c_float),
        ("solver_iterations", C.c_uint32),
        ("baumgarte", C.c_float),
        ("slop", C.c_float),
        ("friction", C.c_float),
        ("contact_margin", C.c_float),
        ("ground_height", C.c_float),
        ("max_bias", C.c_float),
        ("max_pairs", C.c_uint64),
        ("max_manifolds", C.c_uint64),
        ("max_ghosts", C.c_uint64),
    ]


class PhysStats(C.Structure):
    _fields_ = [
        ("n_bodies", C.c_uint64),
        ("n_pairs", C.c_uint64),
        ("n_manifolds", C.c_uint64),
        ("n_contacts", C.c_uint64),
        ("n_colors", C.c_uint32),
        ("color_rounds", C.c_uint32),
        ("cg_iterations", C.c_uint32),
        ("cg_converged", C.c_int32),
        ("steps", C.c_uint64),
        ("overflow", C.c_uint32),
        ("n_ground_manifolds", C.c_uint32),
        ("max_extent", C.c_float),
        ("n_halo_records", C.c_uint32),
        ("n_cross_pairs", C.c_uint64),
        ("n_ghosts", C.c_uint32),
        ("n_new_manifolds", C.c_uint32),
    ]


STAGE_COUNT = 14
STAGE_NAMES = ["step_full", "velocity_aabb", "grid", "pairs", "narrow", "color", "rows", "solve", "position",
               "constraints", "misc", "solve_tail", "solve_flow", "solve_cluster"]


class PhysProfile(C.Structure):
    _fields_ = [("ms", C.c_double * STAGE_COUNT), ("launches", C.c_uint64 * STAGE_COUNT), ("steps", C.c_uint64)]


class PhysDeviceView(C.Structure):
    _fields_ = [
        ("n", C.c_uint64),
        ("pos", C.c_void_p),
        ("rot", C.c_void_p),
        ("lin_vel", C.c_void_p),
        ("ang_vel", C.c_void_p),
        ("aabb", C.c_void_p),
        ("stream", C.c_void_p),
        ("vel_stride", C.c_uint64),
    ]


class PhysContactEvent(C.Structure):
    """struct phys_contact_event (include/physics_hip.h), 48 bytes."""
    _fields_ = [
        ("body_a", C.c_uint32),
        ("body_b", C.c_uint32),
        ("kind", C.c_uint32),
        ("step", C.c_uint32),
        ("point", C.c_float * 3),
        ("impulse", C.c_float),
        ("normal", C.c_float * 3),
        ("reserved", C.c_uint32),
    ]


class PhysTriggerEvent(C.Structure):
    """struct phys_trigger_event (include/physics_hip.h), 16 bytes."""
    _fields_ = [("trigger", C.c_uint32), ("body", C.c_uint32), ("kind", C.c_uint32), ("step", C.c_uint32)]


def default_config(**overrides):
    """Reference defaults, identical to phys_config_default() (checked by tests/test_abi.py)."""
    cfg = PhysConfig()
    cfg.abi_version = PHYS_ABI_VERSION
    cfg.device = 0
    cfg.flags = 0
    cfg.gravity_force[:] = (0.0, -9.81, 0.0)   # physics.rs:90
    cfg.gravity_offset[:] = (0.0, 0.0, 1.5)    # physics.rs:91
    cfg.cg_max_iterations = 1000               # sle_solver.rs:5
    cfg.cg_max_error = 1e-2                    # sle_solver.rs:6
    cfg.cg_min_error = 1e-3                    # sle_solver.rs:7
    cfg.solver_iterations = 8
    cfg.baumgarte = 0.2
    cfg.slop = 0.01
    cfg.friction = 0.5
    cfg.contact_margin = 0.02
    cfg.ground_height = 0.0
    cfg.max_bias = 3.0
    cfg.max_pairs = 0
    cfg.max_manifolds = 0
    cfg.max_ghosts = 0
    for k, v in overrides.items():
        if k in ("gravity_force", "gravity_offset"):
            getattr(cfg, k)[:] = tuple(v)
        else:
            setattr(cfg, k, v)
    return cfg


# name -> (restype, argtypes); every symbol include/physics_hip.h declares
PROTOTYPES = {
    "phys_config_default": (None, [C.POINTER(PhysConfig)]),
    "phys_last_error": (C.c_char_p, []),
    "phys_abi_version": (C.c_uint32, []),
    "phys_create": (C.c_int32, [C.POINTER(PhysConfig), C.POINTER(C.c_void_p)]),
    "phys_destroy": (C.c_int32, [C.c_void_p]),
    "phys_set_bodies": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p, f32p, f32p, f32p, f32p, u32p, f32p]),
    "phys_add_constraint_fix_point": (C.c_int32, [C.c_void_p, C.c_uint64, f32p]),
    "phys_add_constraint_fix_orientation": (C.c_int32, [C.c_void_p, C.c_uint64, f32p]),
    "phys_clear_constraints": (C.c_int32, [C.c_void_p]),
    "phys_apply_force_centre_of_gravity": (C.c_int32, [C.c_void_p, C.c_uint64, f32p]),
    "phys_apply_force_at_position": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_apply_force_at_offset": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_set_forces": (C.c_int32, [C.c_void_p, f32p, f32p]),
    "phys_update": (C.c_int32, [C.c_void_p, C.c_uint64]),
    "phys_apply_gravity": (C.c_int32, [C.c_void_p]),
    "phys_step": (C.c_int32, [C.c_void_p, C.c_uint64]),
    "phys_update_n": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint32]),
    "phys_sync": (C.c_int32, [C.c_void_p]),
    "phys_get_transforms": (C.c_int32, [C.c_void_p, f32p, f32p]),
    "phys_get_velocities": (C.c_int32, [C.c_void_p, f32p, f32p]),
    "phys_get_forces": (C.c_int32, [C.c_void_p, f32p, f32p]),
    "phys_get_instance_matrices": (C.c_int32, [C.c_void_p, f32p]),
    "phys_get_lambda": (C.c_int32, [C.c_void_p, f32p, C.c_uint64, u64p]),
    "phys_block_spmv": (C.c_int32, [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, u64p, f32p, f32p, C.c_uint64, C.c_int32, f32p]),
    "phys_broadphase": (C.c_int32, [C.c_void_p, u32p, C.c_uint64, u64p]),
    "phys_get_aabbs": (C.c_int32, [C.c_void_p, f32p]),
    "phys_get_manifolds": (C.c_int32, [C.c_void_p, u32p, u32p, f32p, f32p, C.c_uint64, u64p]),
    "phys_get_stats": (C.c_int32, [C.c_void_p, C.POINTER(PhysStats)]),
    "phys_get_color_counts": (C.c_int32, [C.c_void_p, u32p]),
    "phys_overlap": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p, f32p, u32p, C.c_uint64, u64p, u32p]),
    "phys_set_static_bodies": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p, u32p, f32p]),
    "phys_set_body_filters": (C.c_int32, [C.c_void_p, C.c_uint64, u16p, u16p, i16p]),
    "phys_get_body_filters": (C.c_int32, [C.c_void_p, u16p, u16p, i16p]),
    "phys_set_static_filters": (C.c_int32, [C.c_void_p, C.c_uint64, u16p, u16p, i16p]),
    "phys_set_ground_filter": (C.c_int32, [C.c_void_p, C.c_uint16, C.c_uint16]),
    "phys_overlap_filtered": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p, f32p, u32p, u16p, C.c_uint64, u64p, u32p]),
    "phys_set_body_materials": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_get_body_materials": (C.c_int32, [C.c_void_p, f32p, f32p]),
    "phys_set_static_materials": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_set_ground_material": (C.c_int32, [C.c_void_p, C.c_float, C.c_float]),
    "phys_set_restitution_threshold": (C.c_int32, [C.c_void_p, C.c_float]),
    "phys_get_static_stats": (C.c_int32, [C.c_void_p, u64p, u64p, u64p]),
    "phys_contact_events_enable": (C.c_int32, [C.c_void_p, C.c_uint64]),
    "phys_get_contact_events": (C.c_int32, [C.c_void_p, C.POINTER(PhysContactEvent), C.c_uint64, u64p, u64p]),
    "phys_get_contact_impulses": (C.c_int32, [C.c_void_p, f32p, C.c_uint64, u64p]),
    "phys_set_triggers": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p, f32p, u16p]),
    "phys_set_trigger_poses": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_trigger_events_enable": (C.c_int32, [C.c_void_p, C.c_uint64]),
    "phys_get_trigger_events": (C.c_int32, [C.c_void_p, C.POINTER(PhysTriggerEvent), C.c_uint64, u64p, u64p]),
    "phys_get_trigger_overlaps": (C.c_int32, [C.c_void_p, C.c_uint64, u64p, u32p]),
    "phys_set_force_fields": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, u32p, f32p, f32p, f32p, u16p, f32p, f32p, u32p]),
    "phys_set_force_field_poses": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_set_force_field_params": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_apply_force_fields": (C.c_int32, [C.c_void_p]),
    "phys_set_liquids": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p, f32p, u16p, f32p, f32p, f32p, f32p]),
    "phys_set_liquid_poses": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p]),
    "phys_set_liquid_params": (C.c_int32, [C.c_void_p, C.c_uint64, f32p, f32p, f32p, f32p]),
    "phys_apply_liquids": (C.c_int32, [C.c_void_p]),
    "phys_get_submersion": (C.c_int32, [C.c_void_p, f32p, u32p]),
    "phys_get_submersion_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "phys_set_ccd_bodies": (C.c_int32, [C.c_void_p, C.c_uint64, u32p]),
    "phys_get_ccd_hits": (C.c_int32, [C.c_void_p, f32p, u32p, f32p, u32p]),
    "phys_get_ccd_hits_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "phys_set_body_poses": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p]),
    "phys_set_body_velocities": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p]),
    "phys_apply_impulses": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p, f32p]),
    "phys_apply_forces": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p, f32p]),
    "phys_get_body_states": (C.c_int32, [C.c_void_p, C.c_uint64, u32p, f32p, f32p, f32p, f32p]),
    # the same five on device arrays: every pointer a c_void_p
    "phys_set_body_poses_device": (C.c_int32, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 3),
    "phys_set_body_velocities_device": (C.c_int32, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 3),
    "phys_apply_impulses_device": (C.c_int32, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4),
    "phys_apply_forces_device": (C.c_int32, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4),
    "phys_get_body_states_device": (C.c_int32, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 5),
    "phys_profile_enable": (C.c_int32, [C.c_void_p, C.c_int32]),
    "phys_profile_get": (C.c_int32, [C.c_void_p, C.POINTER(PhysProfile)]),
    "phys_get_device_view": (C.c_int32, [C.c_void_p, C.POINTER(PhysDeviceView)]),
    "phys_set_global_ids": (C.c_int32, [C.c_void_p, u32p]),
    "phys_halo_pack": (C.c_int32, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_uint64, u64p]),
    "phys_halo_pairs": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, u64p]),
    "phys_get_cross_pairs": (C.c_int32, [C.c_void_p, u32p, C.c_uint64, u64p]),
    "phys_set_slab": (C.c_int32, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "phys_halo_pack_bodies": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "phys_halo_pack_bodies_face": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "phys_halo_unpack_ghosts": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]),
    "phys_get_global_ids": (C.c_int32, [C.c_void_p, u32p]),
    "phys_comm_unique_id": (C.c_int32, [C.POINTER(C.c_uint8)]),
    "phys_comm_create": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]),
    "phys_comm_create_local": (C.c_int32, [C.POINTER(C.c_void_p), C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]),
    "phys_comm_destroy": (C.c_int32, [C.c_void_p]),
    "phys_comm_set_neighbours": (C.c_int32, [C.c_void_p, C.c_int32]),
    "phys_halo_exchange": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "phys_halo_exchange_all": (C.c_int32, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int32]),
    "phys_slab_histogram": (C.c_int32, [f32p, C.c_uint64, C.c_float, C.c_float, C.c_uint32, u64p]),
    "phys_slab_cuts": (C.c_int32, [u64p, C.c_uint32, C.c_float, C.c_float, C.c_int32, f32p]),
    "phys_slab_owners": (C.c_int32, [f32p, C.c_uint64, f32p, C.c_int32, C.POINTER(C.c_int32)]),
}

# The casts: per kind its input arrays and its output arrays, in the order of the call (the header's names; rot and ignore
# are its rot_ijkw and ignore_body). Every array is float32 but those of CAST_TYPES. Each kind comes four times: on host
# arrays or on device arrays (_device: every array a c_void_p), plain or _filtered (a u16 query_mask behind the inputs).
CASTS = {
    "raycast": (("origin", "dir", "max_t", "ignore"), ("body_out", "t_out", "normal_out")),
    "spherecast": (("origin", "dir", "radius", "max_t", "ignore"), ("body_out", "t_out", "normal_out")),
    "capsulecast": (("origin", "dir", "rot", "radius", "half_length", "max_t", "ignore"),
                    ("body_out", "t_out", "normal_out", "point_out")),
    "boxcast": (("origin", "dir", "rot", "half_extent", "max_t", "ignore"), ("body_out", "t_out", "normal_out", "point_out")),
}
CAST_TYPES = {"ignore": u32p, "body_out": u32p}

# The box cast's four prototypes come from the same table, into a dict of their own: PROTOTYPES mirrors the declarations that
# stand in include/physics_hip.h itself, BOXCAST_PROTOTYPES those of include/physics_hip_boxcast.h, which that header includes
# (the reason is said there). load_library() sets both.
BOXCAST_PROTOTYPES = {}

for _kind, (_ins, _outs) in CASTS.items():
    for _device in ("", "_device"):
        for _mask in ((), (u16p,)):
            _args = [CAST_TYPES.get(k, f32p) for k in _ins] + list(_mask) + [CAST_TYPES.get(k, f32p) for k in _outs]
            (BOXCAST_PROTOTYPES if _kind == "boxcast" else PROTOTYPES)[f"phys_{_kind}{_device}" + ("_filtered" if _mask else "")] = (
                C.c_int32, [C.c_void_p, C.c_uint64] + ([C.c_void_p] * len(_args) if _device else _args))

# The capsule query calls (move-and-slide, character walking, depenetration): per call its input arrays, its per-call scalars
# with their types, and its output arrays, in the order of the call: the inputs, the scalars, ignore, query_mask, the outputs
# (the header's names but rot, ignore and grounded: its rot_ijkw, ignore_body and grounded_in). Every array is float32 but those
# of QUERY_TYPES. Each call comes on host arrays and on device arrays (_device: every array a c_void_p).
SLIDE_MAX_SLIDES = 8
SLIDE_BLOCKED, SLIDE_EXHAUSTED, SLIDE_INVALID = 0x100, 0x200, 0x400
CHAR_BLOCKED, CHAR_EXHAUSTED, CHAR_INVALID = 0x100, 0x200, 0x400
CHAR_GROUNDED, CHAR_STEPPED, CHAR_SNAPPED, CHAR_ON_STEEP, CHAR_HIT_WALL, CHAR_HIT_CEILING = 0x1000, 0x2000, 0x4000, 0x8000, 0x10000, 0x20000
DEPEN_MAX_ITERS = 8
DEPEN_STUCK, DEPEN_INVALID = 0x100, 0x400
QUERIES = {
    "move_and_slide": (("pos", "motion", "rot", "radius", "half_length"), (("skin", C.c_float), ("max_slides", C.c_uint32)),
                       ("pos_out", "remaining_out", "status_out", "hit_body_out", "hit_normal_out", "hit_point_out")),
    "character_move": (("pos", "motion", "rot", "radius", "half_length", "grounded"),
                       (("skin", C.c_float), ("max_slides", C.c_uint32), ("step_height", C.c_float), ("snap_distance", C.c_float),
                        ("min_floor_ny", C.c_float)),
                       ("pos_out", "remaining_out", "status_out", "floor_body_out", "floor_normal_out", "floor_point_out",
                        "hit_body_out", "hit_normal_out", "hit_point_out")),
    "penetration": (("pos", "rot", "radius", "half_length"), (("max_gap", C.c_float),), ("body_out", "depth_out", "normal_out")),
    "depenetrate": (("pos", "rot", "radius", "half_length"), (("skin", C.c_float), ("max_iters", C.c_uint32)),
                    ("pos_out", "status_out", "hit_body_out", "hit_normal_out", "hit_depth_out")),
}
QUERY_TYPES = {"grounded": u32p, "ignore": u32p, "query_mask": u16p, "status_out": u32p, "floor_body_out": u32p, "hit_body_out": u32p,
               "body_out": u32p}

for _call, (_ins, _scalars, _outs) in QUERIES.items():
    for _device in ("", "_device"):
        _args = [C.c_void_p if _device else QUERY_TYPES.get(k, f32p) for k in _ins + ("ignore", "query_mask") + _outs]
        PROTOTYPES[f"phys_{_call}{_device}"] = (
            C.c_int32, [C.c_void_p, C.c_uint64] + _args[:len(_ins)] + [t for _, t in _scalars] + _args[len(_ins):])

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libphysics_hip.so")
_lib = None


class PhysicsHipMissing(RuntimeError):
    pass


def rocm_runtime_mapped():
    """Paths of the HIP runtime(s) mapped into this process (one entry in a healthy process)."""
    try:
        return sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    except OSError:
        return []


def torch_bundled_rocm_dir():
    """Directory of the ROCm runtime a PyTorch wheel ships inside itself, found WITHOUT importing torch."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.origin:
        return None
    d = os.path.join(os.path.dirname(spec.origin), "lib")
    return d if os.path.exists(os.path.join(d, "libamdhip64.so")) else None


def share_rocm_runtime_with_torch():
    """One ROCm runtime per process. The PyTorch wheel of this image ships its OWN libamdhip64.so / libhsa-runtime64.so
    (ROCm 7.0.2, under torch/lib, SONAME libamdhip64.so.7) next to the system's /opt/rocm (7.2.0, same SONAME).
    libphysics_hip.so asks for the SONAME, libtorch_hip.so for the file in its own directory, so the order of loading
    decided what a process got: torch first -> ONE runtime (torch's, found again by SONAME); the library first -> /opt/rocm's
    for the library and then a SECOND runtime for torch, whose initialisation fails with hipErrorNoDevice ("no ROCm-capable
    device is detected", round 1's unexplained failure: two HSA runtimes cannot both own the process's KFD queue state).
    So when a PyTorch with a bundled runtime is installed and no HIP runtime is mapped yet, that bundled runtime is
    loaded first (RTLD_GLOBAL, by path - torch itself need not be imported): library and torch then share it whichever
    comes first. Callers without PyTorch (the Rust / C++ hosts) get the system runtime, alone in its process.
    PHYS_ROCM_RUNTIME=system skips this (a process that will never import torch)."""
    if os.environ.get("PHYS_ROCM_RUNTIME") == "system" or rocm_runtime_mapped():
        return None
    d = torch_bundled_rocm_dir()
    if d is None:
        return None
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(d, name)
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    # the RCCL of this process must be the one built against that runtime (comm.hip loads it on first use)
    rccl = os.path.join(d, "librccl.so")
    if os.path.exists(rccl):
        os.environ.setdefault("PHYS_RCCL_PATH", rccl)
    return d


def load_library():
    """Load libphysics_hip.so (built in-tree by __graft_entry__.build()). Raises if absent: the
    product path has no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PhysicsHipMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). physics_amd has no CPU fallback.")
    share_rocm_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(PROTOTYPES.items()) + list(BOXCAST_PROTOTYPES.items()):
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
