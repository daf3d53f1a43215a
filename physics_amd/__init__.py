"""physics_amd — MI355X (gfx950) backend for the per-frame rigid-body step of martingoe/physics.

Host-side mirror of the reference's `PhysicsState` surface over the C ABI of libphysics_hip.so
(include/physics_hip.h). The compute path is hand-written HIP; there is no CPU fallback."""
from ._abi import (CONTACT_BEGIN, CONTACT_END, MAX_TRIGGERS, TRIGGER_ENTER, TRIGGER_EXIT, MAX_FORCE_FIELDS, FIELD_ACCEL, FIELD_DRAG, FIELD_RADIAL, FILTER_DEFAULT_CATEGORY, FILTER_DEFAULT_MASK, FLAG_BROADPHASE_ONLY, FLAG_COLLISIONS, FLAG_EXACT_ROTATION,
                   FLAG_GROUND_PLANE, FLAG_EXCLUSIVE_GPU, FLAG_NO_WARM_START, FLAG_SHARED_GPU, FLAG_SOLVER_CLUSTER, FLAG_SOLVER_PER_COLOR, GROUND_ID,
                   RAY_GROUND, RAY_MISS, SHAPE_BOX, SHAPE_CAPSULE, STATIC_ID_BIT, SHAPE_NONE, SHAPE_SPHERE, SLIDE_BLOCKED, SLIDE_EXHAUSTED, SLIDE_INVALID, SLIDE_MAX_SLIDES,
                   DEPEN_INVALID, DEPEN_MAX_ITERS, DEPEN_STUCK, PhysicsHipMissing,
                   default_config)
from . import filters  # noqa: F401  (numpy statement of the collision filter rule)
from .scenes import capsule_inertia
from .world import CONTACT_EVENT_DTYPE, TRIGGER_EVENT_DTYPE, Comm, PhysError, World, block_spmv

__all__ = ["World", "Comm", "block_spmv", "PhysError", "PhysicsHipMissing", "default_config", "FLAG_COLLISIONS", "FLAG_GROUND_PLANE",
           "FLAG_EXACT_ROTATION", "FLAG_BROADPHASE_ONLY", "FLAG_SOLVER_PER_COLOR", "FLAG_SHARED_GPU", "FLAG_SOLVER_CLUSTER", "FLAG_EXCLUSIVE_GPU", "FLAG_NO_WARM_START", "SHAPE_NONE", "SHAPE_SPHERE", "SHAPE_BOX", "SHAPE_CAPSULE", "GROUND_ID",
           "RAY_MISS", "RAY_GROUND", "STATIC_ID_BIT", "FILTER_DEFAULT_CATEGORY", "FILTER_DEFAULT_MASK", "capsule_inertia", "CONTACT_BEGIN",
           "CONTACT_END", "CONTACT_EVENT_DTYPE", "MAX_TRIGGERS", "TRIGGER_ENTER", "TRIGGER_EXIT", "TRIGGER_EVENT_DTYPE", "MAX_FORCE_FIELDS",
           "FIELD_ACCEL", "FIELD_DRAG", "FIELD_RADIAL", "SLIDE_BLOCKED", "SLIDE_EXHAUSTED", "SLIDE_INVALID", "SLIDE_MAX_SLIDES",
           "DEPEN_STUCK", "DEPEN_INVALID", "DEPEN_MAX_ITERS"]
