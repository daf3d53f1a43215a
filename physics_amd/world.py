"""World — thin ctypes wrapper over the C ABI (include/physics_hip.h). Every method is one ABI call;
the reference-shaped object model (PhysicsState / Entity / RigidBody) lives in state.py on top."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import STAGE_NAMES, PhysContactEvent, PhysDeviceView, PhysProfile, PhysStats, PhysTriggerEvent, f32p, i16p, u16p, u32p

# one phys_contact_event as a numpy record (the layout of _abi.PhysContactEvent, 48 bytes)
CONTACT_EVENT_DTYPE = np.dtype([("body_a", "<u4"), ("body_b", "<u4"), ("kind", "<u4"), ("step", "<u4"), ("point", "<f4", (3,)),
                                ("impulse", "<f4"), ("normal", "<f4", (3,)), ("reserved", "<u4")])
# one phys_trigger_event as a numpy record (the layout of _abi.PhysTriggerEvent, 16 bytes)
TRIGGER_EVENT_DTYPE = np.dtype([("trigger", "<u4"), ("body", "<u4"), ("kind", "<u4"), ("step", "<u4")])


class PhysError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"physics_hip error {code}: {msg}")
        self.code = code


def _f(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _p(a, t=f32p):
    return None if a is None else a.ctypes.data_as(t)


def _filter_field(a, n, name, lo, hi, dtype):
    """A per-item filter field as a contiguous array of n `dtype` values, or None; out-of-range or non-integer values and a
    wrong length raise before the library is called."""
    if a is None:
        return None
    v = np.asarray(a)
    if v.dtype.kind not in "iub":
        raise ValueError(f"{name}: needs integers")
    v = np.broadcast_to(v, (n,)) if v.ndim == 0 else v
    if v.ndim != 1 or v.shape[0] != n:
        raise ValueError(f"{name}: needs {n} values, got shape {np.shape(a)}")
    if v.size and (v.min() < lo or v.max() > hi):
        raise ValueError(f"{name}: values must lie in [{lo}, {hi}]")
    return np.ascontiguousarray(v, dtype=dtype)


def _material_field(a, n, name, hi):
    """A per-item material field as a contiguous array of n floats, or None; a wrong length, a non-finite or negative
    value, or one above `hi` raises before the library is called."""
    if a is None:
        return None
    v = np.asarray(a)
    if v.dtype.kind not in "fiu":
        raise ValueError(f"{name}: needs numbers")
    v = np.broadcast_to(v, (n,)) if v.ndim == 0 else v
    if v.ndim != 1 or v.shape[0] != n:
        raise ValueError(f"{name}: needs {n} values, got shape {np.shape(a)}")
    v = np.ascontiguousarray(v, dtype=np.float32)
    if v.size and not (np.all(np.isfinite(v)) and v.min() >= 0.0 and v.max() <= hi):
        raise ValueError(f"{name}: values must be finite and lie in [0, {hi}]")
    return v


def _field_law_check(kind, coef):
    """What each force field's law asks of its coefficients (n kinds, (n, 2) coef): DRAG >= 0, RADIAL r0 > 0."""
    if ((kind == _abi.FIELD_DRAG)[:, None] & (coef < 0)).any():
        raise ValueError("coef: a DRAG field's coefficients must be >= 0")
    if ((kind == _abi.FIELD_RADIAL) & ~(coef[:, 1] > 0)).any():
        raise ValueError("coef: a RADIAL field's r0 (coef[1]) must be above 0")


# the arrays of the casts (the names of _abi.CASTS): numpy dtype and columns per query
_CAST_ARRAYS = {
    "origin": (np.float32, 3), "dir": (np.float32, 3), "rot": (np.float32, 4), "radius": (np.float32, 1),
    "half_length": (np.float32, 1), "half_extent": (np.float32, 3), "max_t": (np.float32, 1), "ignore": (np.uint32, 1),
    "body_out": (np.uint32, 1), "t_out": (np.float32, 1), "normal_out": (np.float32, 3), "point_out": (np.float32, 3),
}


def _query_mask(mask, n):
    """The per-query mask of a _filtered query: a scalar or (n,) integers in [0, 0xFFFF]."""
    return _filter_field(mask, n, "mask", 0, 0xFFFF, np.uint16)


def _edit_ids(ids):
    """The body ids of an edit call as a contiguous (n,) uint32 array; non-integers and values outside u32 raise."""
    v = np.asarray(ids)
    if v.size == 0:
        return np.zeros(0, np.uint32)
    if v.dtype.kind not in "iu":
        raise ValueError("ids: needs integers")
    v = v.reshape(-1)
    if v.min() < 0 or v.max() > 0xFFFFFFFF:
        raise ValueError("ids: values must lie in [0, 2^32)")
    return np.ascontiguousarray(v, dtype=np.uint32)


def _device_args(n, items):
    """c_void_p of contiguous 4-byte device tensors of n x cols elements (None passes through)."""
    args = []
    for name, x, cols in items:
        if x is None:
            args.append(None)
            continue
        if not x.is_cuda or not x.is_contiguous() or x.numel() != n * cols or x.element_size() != 4:
            raise ValueError(f"{name}: needs a contiguous 4-byte device tensor of {n} x {cols}")
        args.append(C.c_void_p(x.data_ptr()))
    return args


def _device_mask(mask, n):
    """c_void_p of a contiguous 2-byte device tensor of n query masks."""
    if not mask.is_cuda or not mask.is_contiguous() or mask.numel() != n or mask.element_size() != 2 or mask.is_floating_point():
        raise ValueError(f"mask: needs a contiguous int16 / uint16 device tensor of {n}")
    return C.c_void_p(mask.data_ptr())


# the input arrays of the capsule query calls (the names of _abi.QUERIES): columns per query
_QUERY_COLS = {"pos": 3, "motion": 3, "rot": 4, "radius": 1, "half_length": 1, "grounded": 1, "ignore": 1}


def _query_scalars(call, given):
    """The per-call scalars of a capsule query call (_abi.QUERIES[call] names and orders them), checked before the library is
    called: the count of rounds first, then the lengths. Returns them in the order of the call, and the count of rounds (None
    for a call without one)."""
    scalars = _abi.QUERIES[call][1]
    v, rounds = {}, None
    for k, t in scalars:
        if t is C.c_uint32:
            v[k] = rounds = int(given[k])
            if not 1 <= rounds <= _abi.SLIDE_MAX_SLIDES:  # (= DEPEN_MAX_ITERS)
                raise ValueError(f"{k}: must lie in [1, {_abi.SLIDE_MAX_SLIDES}]")
    for k, t in scalars:
        if t is C.c_float:
            v[k] = float(given[k])
            if k == "min_floor_ny":
                if not 0.0 < v[k] <= 1.0:
                    raise ValueError("min_floor_ny: must lie in (0, 1]")
            elif not (np.isfinite(v[k]) and v[k] >= 0.0):
                raise ValueError(f"{k}: must be finite and not negative")
    return [v[k] for k, _ in scalars], rounds


class World:
    def __init__(self, cfg=None):
        self.lib = _abi.load_library()
        self.cfg = cfg if cfg is not None else _abi.default_config()
        self.h = C.c_void_p()
        self.n = 0
        self.n_static = 0
        self.n_triggers = 0
        self.n_fields, self._field_kinds = 0, np.zeros(0, np.uint32)
        self.n_liquids = 0
        self.n_ccd = 0
        self._ck(self.lib.phys_create(C.byref(self.cfg), C.byref(self.h)))

    def _ck(self, rc):
        if rc != 0:
            raise PhysError(rc, self.lib.phys_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.phys_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- state upload
    def set_bodies(self, pos, rot=None, lin_vel=None, ang_vel=None, mass=None, inertia=None, shape_type=None,
                   half_extent=None):
        pos = _f(pos).reshape(-1, 3)
        n = pos.shape[0]
        arrs = [pos, _f(rot), _f(lin_vel), _f(ang_vel), _f(mass), _f(inertia)]
        for a, w in zip(arrs[1:], (4, 3, 3, 1, 9)):
            if a is not None and a.size != n * w:
                raise ValueError("array size does not match the body count")
        st = None if shape_type is None else np.ascontiguousarray(shape_type, dtype=np.uint32)
        he = _f(half_extent)
        self._ck(self.lib.phys_set_bodies(self.h, n, *[_p(a) for a in arrs], _p(st, u32p), _p(he)))
        self.n = n
        self.n_ccd = 0  # the library clears the continuous-collision list: its ids are stale

    def set_static_bodies(self, pos, rot=None, shape_type=None, half_extent=None):
        """Replace the static colliders (phys_set_static_bodies): pos (n, 3), rot (n, 4) [i, j, k, w] or None (identity),
        shape_type (n,) SHAPE_SPHERE / SHAPE_BOX / SHAPE_CAPSULE, half_extent (n, 3) (capsule: radius, core half-length along
        the local y axis, unused). An empty pos clears the set. Collider k is named
        STATIC_ID_BIT | k in manifolds and ray hits."""
        pos = _f(pos).reshape(-1, 3)
        n = pos.shape[0]
        rot = _f(rot)
        st = None if shape_type is None else np.ascontiguousarray(shape_type, dtype=np.uint32).reshape(-1)
        he = _f(half_extent)
        for a, w in ((rot, 4), (st, 1), (he, 3)):
            if a is not None and a.size != n * w:
                raise ValueError("array size does not match the static collider count")
        self._ck(self.lib.phys_set_static_bodies(self.h, n, _p(pos), _p(rot), _p(st, u32p), _p(he)))
        self.n_static = n

    # ---- collision filters (include/physics_hip.h): category u16, mask u16, group i16 per body / static
    def set_body_filters(self, category=None, mask=None, group=None):
        """Filters of the owned bodies (phys_set_body_filters): each of category / mask / group a scalar or (n_bodies,)
        integers, or None for the default (category FILTER_DEFAULT_CATEGORY, mask FILTER_DEFAULT_MASK, group 0). Two bodies
        collide iff they share a nonzero group that is positive, or (without one) each one's category meets the other's
        mask. Takes effect at the next update; set_bodies resets the filters."""
        n = self.n
        c = _filter_field(category, n, "category", 0, 0xFFFF, np.uint16)
        m = _filter_field(mask, n, "mask", 0, 0xFFFF, np.uint16)
        g = _filter_field(group, n, "group", -0x8000, 0x7FFF, np.int16)
        self._ck(self.lib.phys_set_body_filters(self.h, n, _p(c, u16p), _p(m, u16p), _p(g, i16p)))

    def get_body_filters(self):
        """(category u16[n], mask u16[n], group i16[n]) of the owned bodies."""
        c = np.empty(self.n, np.uint16)
        m = np.empty(self.n, np.uint16)
        g = np.empty(self.n, np.int16)
        self._ck(self.lib.phys_get_body_filters(self.h, _p(c, u16p), _p(m, u16p), _p(g, i16p)))
        return c, m, g

    def set_static_filters(self, category=None, mask=None, group=None):
        """Filters of the static colliders (phys_set_static_filters), as set_body_filters; set_static_bodies resets them."""
        n = self.n_static
        c = _filter_field(category, n, "category", 0, 0xFFFF, np.uint16)
        m = _filter_field(mask, n, "mask", 0, 0xFFFF, np.uint16)
        g = _filter_field(group, n, "group", -0x8000, 0x7FFF, np.int16)
        self._ck(self.lib.phys_set_static_filters(self.h, n, _p(c, u16p), _p(m, u16p), _p(g, i16p)))

    def set_ground_filter(self, category, mask):
        """The ground plane's category and mask (its group is 0); lasts for the life of the world."""
        for name, v in (("category", category), ("mask", mask)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= 0xFFFF:
                raise ValueError(f"{name}: needs an integer in [0, 65535]")
        self._ck(self.lib.phys_set_ground_filter(self.h, int(category), int(mask)))

    # ---- materials (include/physics_hip.h): friction >= 0 and restitution in [0, 1] per body / static / ground
    def set_body_materials(self, friction=None, restitution=None):
        """Materials of the owned bodies (phys_set_body_materials): each of friction / restitution a scalar or (n_bodies,)
        floats, or None for the default (the config's friction; restitution 0). A manifold's friction is the geometric
        mean of its two sides', its restitution the larger one. Takes effect at the next update; set_bodies resets them."""
        n = self.n
        f = _material_field(friction, n, "friction", np.inf)
        e = _material_field(restitution, n, "restitution", 1.0)
        self._ck(self.lib.phys_set_body_materials(self.h, n, _p(f), _p(e)))

    def get_body_materials(self):
        """(friction f32[n], restitution f32[n]) of the owned bodies."""
        f = np.empty(self.n, np.float32)
        e = np.empty(self.n, np.float32)
        self._ck(self.lib.phys_get_body_materials(self.h, _p(f), _p(e)))
        return f, e

    def set_static_materials(self, friction=None, restitution=None):
        """Materials of the static colliders (phys_set_static_materials), as set_body_materials; set_static_bodies resets them."""
        n = self.n_static
        f = _material_field(friction, n, "friction", np.inf)
        e = _material_field(restitution, n, "restitution", 1.0)
        self._ck(self.lib.phys_set_static_materials(self.h, n, _p(f), _p(e)))

    def set_ground_material(self, friction, restitution=0.0):
        """The ground plane's material; lasts for the life of the world."""
        f = _material_field(friction, 1, "friction", np.inf)
        e = _material_field(restitution, 1, "restitution", 1.0)
        if f is None or e is None:
            raise ValueError("the ground's friction and restitution are numbers")
        self._ck(self.lib.phys_set_ground_material(self.h, float(f[0]), float(e[0])))

    def set_restitution_threshold(self, v):
        """Approach speed along the normal below which no contact bounces (default 1.0); lasts for the life of the world."""
        t = _material_field(v, 1, "threshold", np.inf)
        if t is None:
            raise ValueError("the threshold is a number")
        self._ck(self.lib.phys_set_restitution_threshold(self.h, float(t[0])))

    def get_static_stats(self):
        """(static colliders, (body, static) pairs of the last update, manifolds against statics of the last update)."""
        out = [C.c_uint64() for _ in range(3)]
        self._ck(self.lib.phys_get_static_stats(self.h, *[C.byref(x) for x in out]))
        return tuple(x.value for x in out)

    def add_constraint_fix_point(self, body, target):
        t = _f(target)
        self._ck(self.lib.phys_add_constraint_fix_point(self.h, body, _p(t)))

    def add_constraint_fix_orientation(self, body, target_rpy):
        t = _f(target_rpy)
        self._ck(self.lib.phys_add_constraint_fix_orientation(self.h, body, _p(t)))

    def clear_constraints(self):
        self._ck(self.lib.phys_clear_constraints(self.h))

    def apply_force_centre_of_gravity(self, body, force):
        f = _f(force)
        self._ck(self.lib.phys_apply_force_centre_of_gravity(self.h, body, _p(f)))

    def apply_force_at_position(self, body, force, point):
        f, p = _f(force), _f(point)
        self._ck(self.lib.phys_apply_force_at_position(self.h, body, _p(f), _p(p)))

    def apply_force_at_offset(self, body, force, offset):
        f, o = _f(force), _f(offset)
        self._ck(self.lib.phys_apply_force_at_offset(self.h, body, _p(f), _p(o)))

    def set_forces(self, force=None, torque=None):
        f, t = _f(force), _f(torque)
        self._ck(self.lib.phys_set_forces(self.h, _p(f), _p(t)))

    # ---- in-place body edits (include/physics_hip.h): poses, velocities, impulses, forces and states by id list
    def _edit(self, call, ids, arrays):
        """An edit on host arrays. arrays: (name, values or None, columns) in the call's order. Entries apply in the order
        given; the library checks ids and values before anything is written."""
        ids = _edit_ids(ids)
        n = ids.shape[0]
        a = []
        for name, v, cols in arrays:
            v = None if v is None else _f(v).reshape(-1, cols)
            if v is not None and v.shape[0] != n:
                raise ValueError(f"{name}: needs {n} x {cols} values (one row per id)")
            a.append(v)
        self._ck(getattr(self.lib, call)(self.h, n, _p(ids, u32p), *[_p(v) for v in a]))

    def _edit_device(self, call, ids, arrays):
        """An edit on contiguous torch tensors of the world's device; ids int32 or uint32, non-decreasing. Only enqueues."""
        n = int(ids.numel())
        if ids.is_floating_point():
            raise ValueError("ids: needs an int32 / uint32 device tensor")
        self._ck(getattr(self.lib, call)(self.h, n, *_device_args(n, (("ids", ids, 1),) + tuple(arrays))))

    def set_body_poses(self, ids, pos=None, rot=None):
        """New positions (n, 3) and / or rotations (n, 4) [i, j, k, w] of the bodies `ids` (phys_set_body_poses); None keeps
        that part. The last entry of a body wins. Rotations are stored as given. Warm starting, colours, events and trigger
        occupancy are kept; the next update, broadphase() and the queries see the new poses."""
        self._edit("phys_set_body_poses", ids, (("pos", pos, 3), ("rot", rot, 4)))

    def set_body_velocities(self, ids, lin=None, ang=None):
        """New linear and / or angular velocities (n, 3) of the bodies `ids` (phys_set_body_velocities); masses stay."""
        self._edit("phys_set_body_velocities", ids, (("lin", lin, 3), ("ang", ang, 3)))

    def apply_impulses(self, ids, impulse, point=None, ang_impulse=None):
        """Impulses (n, 3) on the bodies `ids`, at world points (n, 3) or None (the centre), with angular impulses (n, 3) or
        None (phys_apply_impulses): v += J / m, w += I^-1 (ang_impulse + (point - x) x J), entries of one body in order."""
        if impulse is None:
            raise ValueError("impulse is required")
        self._edit("phys_apply_impulses", ids, (("impulse", impulse, 3), ("point", point, 3), ("ang_impulse", ang_impulse, 3)))

    def apply_forces(self, ids, force, point=None, torque=None):
        """Forces (n, 3) on the bodies `ids` into the accumulators, at world points or None (the centre), with torques or
        None (phys_apply_forces): one launch that equals the same apply_force_at_position calls bit for bit."""
        if force is None:
            raise ValueError("force is required")
        self._edit("phys_apply_forces", ids, (("force", force, 3), ("point", point, 3), ("torque", torque, 3)))

    def get_body_states(self, ids):
        """(pos (n, 3), rot (n, 4), lin (n, 3), ang (n, 3)) of the bodies `ids`, in any order and with repeats
        (phys_get_body_states)."""
        ids = _edit_ids(ids)
        n = ids.shape[0]
        out = [np.empty((n, c), np.float32) for c in (3, 4, 3, 3)]
        self._ck(self.lib.phys_get_body_states(self.h, n, _p(ids, u32p), *[_p(o) for o in out]))
        return tuple(out)

    def set_body_poses_device(self, ids, pos=None, rot=None):
        """phys_set_body_poses_device on contiguous torch tensors of the world's device: ids int32 / uint32 (n,) in
        non-decreasing order, pos float32 (n, 3) or None, rot float32 (n, 4) or None. Only enqueues on the world's stream;
        ids out of order or out of range make the next sync() raise PHYS_ERR_INVALID_ARG."""
        self._edit_device("phys_set_body_poses_device", ids, (("pos", pos, 3), ("rot", rot, 4)))

    def set_body_velocities_device(self, ids, lin=None, ang=None):
        """phys_set_body_velocities_device, as set_body_poses_device; lin / ang float32 (n, 3) or None."""
        self._edit_device("phys_set_body_velocities_device", ids, (("lin", lin, 3), ("ang", ang, 3)))

    def apply_impulses_device(self, ids, impulse, point=None, ang_impulse=None):
        """phys_apply_impulses_device, as set_body_poses_device; impulse float32 (n, 3), point / ang_impulse (n, 3) or None."""
        if impulse is None:
            raise ValueError("impulse is required")
        self._edit_device("phys_apply_impulses_device", ids, (("impulse", impulse, 3), ("point", point, 3), ("ang_impulse", ang_impulse, 3)))

    def apply_forces_device(self, ids, force, point=None, torque=None):
        """phys_apply_forces_device, as set_body_poses_device; force float32 (n, 3), point / torque (n, 3) or None."""
        if force is None:
            raise ValueError("force is required")
        self._edit_device("phys_apply_forces_device", ids, (("force", force, 3), ("point", point, 3), ("torque", torque, 3)))

    def get_body_states_device(self, ids, pos_out=None, rot_out=None, lin_out=None, ang_out=None):
        """phys_get_body_states_device: the states of the bodies `ids` (any order) into float32 device tensors (n, 3) / (n, 4)
        / (n, 3) / (n, 3), each or None. Only enqueues on the world's stream."""
        self._edit_device("phys_get_body_states_device", ids, (("pos_out", pos_out, 3), ("rot_out", rot_out, 4), ("lin_out", lin_out, 3),
                                                               ("ang_out", ang_out, 3)))

    # ---- stepping
    def apply_gravity(self):
        self._ck(self.lib.phys_apply_gravity(self.h))

    def step(self, dt_nanos):
        self._ck(self.lib.phys_step(self.h, dt_nanos))

    def update(self, dt_nanos):
        self._ck(self.lib.phys_update(self.h, dt_nanos))

    def update_n(self, dt_nanos, n):
        self._ck(self.lib.phys_update_n(self.h, dt_nanos, n))

    def sync(self):
        self._ck(self.lib.phys_sync(self.h))

    # ---- read-back
    def get_transforms(self):
        pos = np.empty((self.n, 3), np.float32)
        rot = np.empty((self.n, 4), np.float32)
        self._ck(self.lib.phys_get_transforms(self.h, _p(pos), _p(rot)))
        return pos, rot

    def get_velocities(self):
        lin = np.empty((self.n, 3), np.float32)
        ang = np.empty((self.n, 3), np.float32)
        self._ck(self.lib.phys_get_velocities(self.h, _p(lin), _p(ang)))
        return lin, ang

    def get_forces(self):
        f = np.empty((self.n, 3), np.float32)
        t = np.empty((self.n, 3), np.float32)
        self._ck(self.lib.phys_get_forces(self.h, _p(f), _p(t)))
        return f, t

    def get_instance_matrices(self):
        m = np.empty((self.n, 16), np.float32)
        self._ck(self.lib.phys_get_instance_matrices(self.h, _p(m)))
        return m

    def get_lambda(self):
        n = C.c_uint64()
        self._ck(self.lib.phys_get_lambda(self.h, None, 0, C.byref(n)))
        out = np.empty(n.value, np.float32)
        if n.value:
            self._ck(self.lib.phys_get_lambda(self.h, _p(out), n.value, C.byref(n)))
        return out

    def get_stats(self):
        s = PhysStats()
        self._ck(self.lib.phys_get_stats(self.h, C.byref(s)))
        return s

    def broadphase(self):
        n = C.c_uint64()
        self._ck(self.lib.phys_broadphase(self.h, None, 0, C.byref(n)))
        out = np.empty((n.value, 2), np.uint32)
        if n.value:
            self._ck(self.lib.phys_broadphase(self.h, _p(out, u32p), n.value, C.byref(n)))
        return out

    def get_aabbs(self):
        out = np.empty((self.n, 6), np.float32)
        self._ck(self.lib.phys_get_aabbs(self.h, _p(out)))
        return out

    def _cast(self, call, noun, origins, dirs, per_query, optional, mask):
        """The casts on host arrays (raycast, spherecast, capsulecast, boxcast). per_query: name -> scalar or (n,) values; optional:
        name -> array or None; the names are those of _CAST_ARRAYS and of _abi.CASTS[call], which orders the arguments.
        Returns the call's outputs."""
        ins, outs = _abi.CASTS[call]
        a = {"origin": _f(origins).reshape(-1, 3), "dir": _f(dirs).reshape(-1, 3)}
        n = a["origin"].shape[0]
        if a["dir"].shape[0] != n:
            raise ValueError("origins and dirs differ in length")
        for k, v in per_query.items():
            a[k] = np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (n,)))
        for k, v in optional.items():
            dtype, cols = _CAST_ARRAYS[k]
            a[k] = None if v is None else np.ascontiguousarray(v, dtype=dtype).reshape(-1, cols)
        for k in optional:
            if a[k] is not None and a[k].size != n * _CAST_ARRAYS[k][1]:
                raise ValueError(f"{' / '.join(optional)} do not match the {noun} count")
        qm = _query_mask(mask, n)
        for k in outs:
            dtype, cols = _CAST_ARRAYS[k]
            a[k] = np.empty(n if cols == 1 else (n, cols), dtype)
        if n:
            ptr = {k: _p(v, _abi.CAST_TYPES.get(k, f32p)) for k, v in a.items()}
            fn = getattr(self.lib, f"phys_{call}" if qm is None else f"phys_{call}_filtered")
            self._ck(fn(self.h, n, *(ptr[k] for k in ins), *(() if qm is None else (_p(qm, u16p),)), *(ptr[k] for k in outs)))
        return tuple(a[k] for k in outs)

    def _cast_device(self, call, origins, inputs, outputs, mask):
        """The casts on device tensors: inputs and outputs as _device_args takes them, in the order of the call."""
        n = int(origins.shape[0])
        args = _device_args(n, inputs)
        out = _device_args(n, outputs)
        if mask is None:
            self._ck(getattr(self.lib, f"phys_{call}_device")(self.h, n, *args, *out))
        else:
            self._ck(getattr(self.lib, f"phys_{call}_device_filtered")(self.h, n, *args, _device_mask(mask, n), *out))

    def raycast(self, origins, dirs, max_t=None, ignore=None, mask=None):
        """Closest hit of every ray against the current poses (phys_raycast): origins / dirs (n, 3), max_t (n,) or None
        (= +inf), ignore (n,) body ids or None. Returns (body u32[n], t f32[n], normal f32[n, 3]); a miss is
        (RAY_MISS, +inf, 0), the ground RAY_GROUND. mask (scalar or (n,) u16): only targets whose filter category meets
        it are seen (phys_raycast_filtered); None: every target."""
        return self._cast("raycast", "ray", origins, dirs, {}, {"max_t": max_t, "ignore": ignore}, mask)

    def raycast_device(self, origins, dirs, body_out, t_out, normal_out=None, max_t=None, ignore=None, mask=None):
        """phys_raycast_device on contiguous torch tensors of the world's device: origins / dirs float32 (n, 3), body_out
        int32 or uint32 (n,), t_out float32 (n,), normal_out float32 (n, 3) or None, max_t float32 (n,) or None, ignore
        int32 / uint32 (n,) or None, mask int16 / uint16 (n,) or None (phys_raycast_device_filtered). Only enqueues on
        the world's stream (device_view().stream): order other streams' work against it yourself."""
        self._cast_device("raycast", origins, (("origins", origins, 3), ("dirs", dirs, 3), ("max_t", max_t, 1), ("ignore", ignore, 1)),
                          (("body_out", body_out, 1), ("t_out", t_out, 1), ("normal_out", normal_out, 3)), mask)

    def spherecast(self, origins, dirs, radius, max_t=None, ignore=None, mask=None):
        """First target a moving ball touches, per ball (phys_spherecast): origins / dirs (n, 3), radius scalar or (n,),
        max_t (n,) or None (= +inf), ignore (n,) body ids or None. Returns (body u32[n], t f32[n], normal f32[n, 3]): t is
        the distance the centre travelled, normal the target's outward normal at the contact (-dir from an overlap at t = 0);
        a miss is (RAY_MISS, +inf, 0). mask: as for raycast (phys_spherecast_filtered)."""
        return self._cast("spherecast", "ball", origins, dirs, {"radius": radius}, {"max_t": max_t, "ignore": ignore}, mask)

    def spherecast_device(self, origins, dirs, radius, body_out, t_out, normal_out=None, max_t=None, ignore=None, mask=None):
        """phys_spherecast_device on contiguous torch tensors of the world's device, as raycast_device; radius float32 (n,).
        Only enqueues on the world's stream (device_view().stream)."""
        self._cast_device("spherecast", origins, (("origins", origins, 3), ("dirs", dirs, 3), ("radius", radius, 1), ("max_t", max_t, 1),
                                                  ("ignore", ignore, 1)),
                          (("body_out", body_out, 1), ("t_out", t_out, 1), ("normal_out", normal_out, 3)), mask)

    def capsulecast(self, origins, dirs, radius, half_length, rot=None, max_t=None, ignore=None, mask=None):
        """First target a moving capsule touches, per capsule (phys_capsulecast): origins / dirs (n, 3), radius and
        half_length scalar or (n,), rot (n, 4) [i, j, k, w] or None (upright: the core along y), max_t (n,) or None
        (= +inf), ignore (n,) body ids or None. Returns (body u32[n], t f32[n], normal f32[n, 3], point f32[n, 3]): t is
        the distance the centre travelled, normal runs from the target's closest point to the capsule's core (-dir from an
        overlap at t = 0), point is the touched point of the target's surface (zeros at t = 0 and on a miss); a miss is
        (RAY_MISS, +inf, 0, 0). mask: as for raycast (phys_capsulecast_filtered)."""
        return self._cast("capsulecast", "capsule", origins, dirs, {"radius": radius, "half_length": half_length},
                          {"rot": rot, "max_t": max_t, "ignore": ignore}, mask)

    def capsulecast_device(self, origins, dirs, radius, half_length, body_out, t_out, normal_out=None, point_out=None, rot=None,
                           max_t=None, ignore=None, mask=None):
        """phys_capsulecast_device on contiguous torch tensors of the world's device, as spherecast_device; radius and
        half_length float32 (n,), rot float32 (n, 4) or None, point_out float32 (n, 3) or None. Only enqueues on the
        world's stream (device_view().stream)."""
        self._cast_device("capsulecast", origins, (("origins", origins, 3), ("dirs", dirs, 3), ("rot", rot, 4), ("radius", radius, 1),
                                                   ("half_length", half_length, 1), ("max_t", max_t, 1), ("ignore", ignore, 1)),
                          (("body_out", body_out, 1), ("t_out", t_out, 1), ("normal_out", normal_out, 3), ("point_out", point_out, 3)),
                          mask)

    def boxcast(self, origins, dirs, half_extent, rot=None, max_t=None, ignore=None, mask=None):
        """First target a moving box touches, per box (phys_boxcast): origins / dirs (n, 3), half_extent (3,) or (n, 3) in the
        frame of rot (n, 4) [i, j, k, w] or None (axis-aligned), max_t (n,) or None (= +inf), ignore (n,) body ids or None.
        Returns (body u32[n], t f32[n], normal f32[n, 3], point f32[n, 3]): t is the distance the centre travelled, normal the
        target's outward normal at the contact (-dir from an overlap at t = 0), point a touched point of the target's surface
        (zeros at t = 0 and on a miss); a miss is (RAY_MISS, +inf, 0, 0). mask: as for raycast (phys_boxcast_filtered)."""
        n = _f(origins).reshape(-1, 3).shape[0]
        he = _f(half_extent)
        if he.shape not in ((3,), (n, 3)):
            raise ValueError("half_extent must be (3,) or (n, 3)")
        he = np.ascontiguousarray(np.broadcast_to(he, (n, 3)))
        return self._cast("boxcast", "box", origins, dirs, {}, {"rot": rot, "half_extent": he, "max_t": max_t, "ignore": ignore}, mask)

    def boxcast_device(self, origins, dirs, half_extent, body_out, t_out, normal_out=None, point_out=None, rot=None, max_t=None,
                       ignore=None, mask=None):
        """phys_boxcast_device on contiguous torch tensors of the world's device, as capsulecast_device; half_extent float32
        (n, 3), rot float32 (n, 4) or None, point_out float32 (n, 3) or None. Only enqueues on the world's stream
        (device_view().stream)."""
        self._cast_device("boxcast", origins, (("origins", origins, 3), ("dirs", dirs, 3), ("rot", rot, 4), ("half_extent", half_extent, 3),
                                               ("max_t", max_t, 1), ("ignore", ignore, 1)),
                          (("body_out", body_out, 1), ("t_out", t_out, 1), ("normal_out", normal_out, 3), ("point_out", point_out, 3)),
                          mask)

    def _query(self, call, noun, given, mask, scalars, shapes):
        """The capsule query calls on host arrays (move_and_slide, character_move, penetration, depenetrate). given: name ->
        array (pos, motion), scalar or (n,) values (radius, half_length), array or None (rot, ignore, grounded); scalars: name
        -> per-call value; the names are those of _abi.QUERIES[call], which orders the arguments. shapes(n, rounds): the shape
        of every output. Returns the call's outputs."""
        ins, _, outs = _abi.QUERIES[call]
        if "motion" not in ins:  # the order of the checks is each call's own: these look at their scalars first
            values, rounds = _query_scalars(call, scalars)
        a = {"pos": _f(given["pos"]).reshape(-1, 3)}
        n = a["pos"].shape[0]
        if "motion" in ins:
            a["motion"] = _f(given["motion"]).reshape(-1, 3)
            if a["motion"].shape[0] != n:
                raise ValueError("pos and motion differ in length")
            values, rounds = _query_scalars(call, scalars)
        for k in ("radius", "half_length"):
            a[k] = np.ascontiguousarray(np.broadcast_to(np.asarray(given[k], np.float32), (n,)))
        optional = [k for k in ("rot", "ignore", "grounded") if k in given]
        for k in optional:
            v = given[k]
            if v is not None and k == "grounded":
                v = np.asarray(v) != 0
            a[k] = None if v is None else np.ascontiguousarray(v, dtype=np.float32 if k == "rot" else np.uint32).reshape(-1, _QUERY_COLS[k])
            if a[k] is not None and a[k].size != n * _QUERY_COLS[k]:
                raise ValueError(f"{' / '.join(optional)} do not match the {noun} count")
        a["query_mask"] = _query_mask(mask, n)
        for k, shape in zip(outs, shapes(n, rounds)):
            a[k] = np.empty(shape, np.uint32 if _abi.QUERY_TYPES.get(k) is u32p else np.float32)
        if n:
            ptr = {k: _p(v, _abi.QUERY_TYPES.get(k, f32p)) for k, v in a.items()}
            self._ck(getattr(self.lib, f"phys_{call}")(self.h, n, *(ptr[k] for k in ins), *values, ptr["ignore"], ptr["query_mask"],
                                                       *(ptr[k] for k in outs)))
        return tuple(a[k] for k in outs)

    def _query_device(self, call, given, mask, scalars, outputs):
        """The capsule query calls on device tensors. given: name -> tensor or None (the inputs of _abi.QUERIES[call] and
        ignore); outputs(rounds): (tensor or None, columns per query) per output, in the order of the call."""
        ins, _, outs = _abi.QUERIES[call]
        n = int(given["pos"].shape[0])
        values, rounds = _query_scalars(call, scalars)
        args = _device_args(n, [(k, given[k], _QUERY_COLS[k]) for k in ins + ("ignore",)])
        out = _device_args(n, [(k, x, cols) for k, (x, cols) in zip(outs, outputs(rounds))])
        self._ck(getattr(self.lib, f"phys_{call}_device")(self.h, n, *args[:-1], *values, args[-1],
                                                          None if mask is None else _device_mask(mask, n), *out))

    def move_and_slide(self, pos, motion, radius, half_length, rot=None, skin=0.01, max_slides=4, ignore=None, mask=None):
        """Capsule characters move, stop `skin` short of what they meet and slide along it (phys_move_and_slide; the rule:
        include/spec/slide.h): pos / motion (n, 3), radius and half_length scalar or (n,), rot (n, 4) [i, j, k, w] or None
        (upright), ignore (n,) body ids or None, mask scalar or (n,) u16 or None (no filtering), max_slides 1 .. 8 casts per
        character, all in one launch. Returns (pos f32[n, 3], remaining f32[n, 3], status u32[n], hit_body u32[max_slides, n],
        hit_normal f32[max_slides, n, 3], hit_point f32[max_slides, n, 3]): status holds the hit count in bits 0-3 and the
        SLIDE_BLOCKED / SLIDE_EXHAUSTED / SLIDE_INVALID flags; an unused hit slot holds RAY_MISS and zeros."""
        return self._query("move_and_slide", "character",
                           dict(pos=pos, motion=motion, radius=radius, half_length=half_length, rot=rot, ignore=ignore), mask,
                           dict(skin=skin, max_slides=max_slides), lambda n, k: ((n, 3), (n, 3), (n,), (k, n), (k, n, 3), (k, n, 3)))

    def move_and_slide_device(self, pos, motion, radius, half_length, pos_out, status_out, remaining_out=None, hit_body_out=None,
                              hit_normal_out=None, hit_point_out=None, rot=None, skin=0.01, max_slides=4, ignore=None, mask=None):
        """phys_move_and_slide_device on contiguous torch tensors of the world's device, as capsulecast_device: pos / motion
        float32 (n, 3), radius and half_length float32 (n,), pos_out float32 (n, 3), status_out int32 / uint32 (n,),
        remaining_out float32 (n, 3) or None, hit_body_out int32 / uint32 (max_slides, n) or None, hit_normal_out and
        hit_point_out float32 (max_slides, n, 3) or None, rot float32 (n, 4) or None, ignore int32 / uint32 (n,) or None, mask
        int16 / uint16 (n,) or None. Only enqueues on the world's stream (device_view().stream)."""
        self._query_device("move_and_slide", dict(pos=pos, motion=motion, rot=rot, radius=radius, half_length=half_length, ignore=ignore), mask,
                           dict(skin=skin, max_slides=max_slides),
                           lambda k: ((pos_out, 3), (remaining_out, 3), (status_out, 1), (hit_body_out, k), (hit_normal_out, 3 * k),
                                      (hit_point_out, 3 * k)))

    def character_move(self, pos, motion, radius, half_length, rot=None, grounded=None, skin=0.01, max_slides=4, step_height=0.3,
                       snap_distance=0.2, min_floor_ny=0.7071068, ignore=None, mask=None):
        """Capsule characters walk (phys_character_move; the rule: include/spec/character.h): move_and_slide on the whole
        motion of the frame, and for a character that stood on a floor (grounded (n,) non-zero, None: nobody) and does not
        move up: no climbing of slopes steeper than min_floor_ny (the cosine of the limit), a step up of at most step_height,
        a snap down of at most snap_distance; then the ground state. pos / motion (n, 3), radius and half_length scalar or
        (n,), rot (n, 4) or None (upright), ignore (n,) body ids or None, mask scalar or (n,) u16 or None. Returns (pos
        f32[n, 3], remaining f32[n, 3], status u32[n], floor_body u32[n], floor_normal f32[n, 3], floor_point f32[n, 3],
        hit_body u32[2 max_slides, n], hit_normal f32[2 max_slides, n, 3], hit_point f32[2 max_slides, n, 3]): status holds
        MOVE's hit count in bits 0-3, the lifted slide's in bits 4-7 and the CHAR_* flags; pass status & CHAR_GROUNDED as the
        next frame's grounded."""
        return self._query("character_move", "character",
                           dict(pos=pos, motion=motion, radius=radius, half_length=half_length, rot=rot, ignore=ignore, grounded=grounded), mask,
                           dict(skin=skin, max_slides=max_slides, step_height=step_height, snap_distance=snap_distance, min_floor_ny=min_floor_ny),
                           lambda n, k: ((n, 3), (n, 3), (n,), (n,), (n, 3), (n, 3), (2 * k, n), (2 * k, n, 3), (2 * k, n, 3)))

    def character_move_device(self, pos, motion, radius, half_length, pos_out, status_out, remaining_out=None, floor_body_out=None,
                              floor_normal_out=None, floor_point_out=None, hit_body_out=None, hit_normal_out=None, hit_point_out=None,
                              rot=None, grounded=None, skin=0.01, max_slides=4, step_height=0.3, snap_distance=0.2,
                              min_floor_ny=0.7071068, ignore=None, mask=None):
        """phys_character_move_device on contiguous torch tensors of the world's device, as move_and_slide_device: grounded
        int32 / uint32 (n,) or None, floor_body_out int32 / uint32 (n,) or None, floor_normal_out and floor_point_out float32
        (n, 3) or None, hit_body_out int32 / uint32 (2 max_slides, n) or None, hit_normal_out and hit_point_out float32
        (2 max_slides, n, 3) or None. Only enqueues on the world's stream (device_view().stream)."""
        self._query_device("character_move",
                           dict(pos=pos, motion=motion, rot=rot, radius=radius, half_length=half_length, grounded=grounded, ignore=ignore), mask,
                           dict(skin=skin, max_slides=max_slides, step_height=step_height, snap_distance=snap_distance, min_floor_ny=min_floor_ny),
                           lambda k: ((pos_out, 3), (remaining_out, 3), (status_out, 1), (floor_body_out, 1), (floor_normal_out, 3),
                                      (floor_point_out, 3), (hit_body_out, 2 * k), (hit_normal_out, 6 * k), (hit_point_out, 6 * k)))

    def penetration(self, pos, radius, half_length, rot=None, max_gap=0.0, ignore=None, mask=None):
        """The deepest target within max_gap of each capsule where it stands (phys_penetration; the rule:
        include/spec/depenetrate.h): pos (n, 3), radius and half_length scalar or (n,), rot (n, 4) [i, j, k, w] or None
        (upright), ignore (n,) body ids or None, mask scalar or (n,) u16 or None (no filtering). Returns (body u32[n], depth
        f32[n], normal f32[n, 3]): depth > 0 is how far the capsule reaches into the target, depth < 0 the clearance, normal
        points out of the target towards the capsule; a miss is (RAY_MISS, -inf, 0). Nothing moves."""
        return self._query("penetration", "capsule", dict(pos=pos, radius=radius, half_length=half_length, rot=rot, ignore=ignore), mask,
                           dict(max_gap=max_gap), lambda n, k: ((n,), (n,), (n, 3)))

    def penetration_device(self, pos, radius, half_length, body_out, depth_out, normal_out=None, rot=None, max_gap=0.0, ignore=None,
                           mask=None):
        """phys_penetration_device on contiguous torch tensors of the world's device, as capsulecast_device: pos float32
        (n, 3), radius and half_length float32 (n,), body_out int32 / uint32 (n,), depth_out float32 (n,), normal_out float32
        (n, 3) or None, rot float32 (n, 4) or None, ignore int32 / uint32 (n,) or None, mask int16 / uint16 (n,) or None. Only
        enqueues on the world's stream (device_view().stream)."""
        self._query_device("penetration", dict(pos=pos, rot=rot, radius=radius, half_length=half_length, ignore=ignore), mask,
                           dict(max_gap=max_gap), lambda k: ((body_out, 1), (depth_out, 1), (normal_out, 3)))

    def depenetrate(self, pos, radius, half_length, rot=None, skin=0.01, max_iters=4, ignore=None, mask=None):
        """Capsules that overlap something are pushed out of it, the deepest target first, until they are skin / 2 clear of
        everything or max_iters (1 .. 8) pushes were made, all in one launch (phys_depenetrate; the rule:
        include/spec/depenetrate.h). Arguments as for penetration. Returns (pos f32[n, 3], status u32[n], hit_body
        u32[max_iters, n], hit_normal f32[max_iters, n, 3], hit_depth f32[max_iters, n]): status holds the push count in bits
        0-3 and the DEPEN_STUCK / DEPEN_INVALID flags; slot k is what penetration reported where push k began, an unused slot
        holds RAY_MISS and zeros."""
        return self._query("depenetrate", "capsule", dict(pos=pos, radius=radius, half_length=half_length, rot=rot, ignore=ignore), mask,
                           dict(skin=skin, max_iters=max_iters), lambda n, k: ((n, 3), (n,), (k, n), (k, n, 3), (k, n)))

    def depenetrate_device(self, pos, radius, half_length, pos_out, status_out, hit_body_out=None, hit_normal_out=None,
                           hit_depth_out=None, rot=None, skin=0.01, max_iters=4, ignore=None, mask=None):
        """phys_depenetrate_device on contiguous torch tensors of the world's device, as penetration_device: pos_out float32
        (n, 3), status_out int32 / uint32 (n,), hit_body_out int32 / uint32 (max_iters, n) or None, hit_normal_out float32
        (max_iters, n, 3) or None, hit_depth_out float32 (max_iters, n) or None. Only enqueues on the world's stream
        (device_view().stream): pos_out may feed move_and_slide_device without a host wait."""
        self._query_device("depenetrate", dict(pos=pos, rot=rot, radius=radius, half_length=half_length, ignore=ignore), mask,
                           dict(skin=skin, max_iters=max_iters),
                           lambda k: ((pos_out, 3), (status_out, 1), (hit_body_out, k), (hit_normal_out, 3 * k), (hit_depth_out, k)))

    def overlap(self, shape_type, pos, rot=None, half_extent=None, ignore=None, cap=None, mask=None):
        """Every target each query shape intersects (phys_overlap): shape_type scalar or (n,) SHAPE_SPHERE / BOX / CAPSULE,
        pos (n, 3), rot (n, 4) [i, j, k, w] or None (identity), half_extent (3,) or (n, 3) with the bodies' conventions,
        ignore (n,) body ids or None. Returns (offsets u64[n + 1], ids u32[offsets[n]]): query i's ids, ascending, are
        ids[offsets[i]:offsets[i + 1]] (bodies, then PHYS_STATIC_ID_BIT | k, then RAY_GROUND). The first call reserves
        `cap` ids (default 8 per query) and, if they do not fit, the call is repeated once with the reported total. mask: as
        for raycast (phys_overlap_filtered)."""
        p = _f(pos).reshape(-1, 3)
        n = p.shape[0]
        if half_extent is None:
            raise ValueError("half_extent is required")
        st = np.ascontiguousarray(np.broadcast_to(np.asarray(shape_type, np.uint32), (n,)))
        he = np.ascontiguousarray(np.broadcast_to(np.asarray(half_extent, np.float32).reshape(-1, 3), (n, 3)))
        r = None if rot is None else _f(rot).reshape(-1, 4)
        ig = None if ignore is None else np.ascontiguousarray(ignore, dtype=np.uint32).reshape(-1)
        for a, k in ((r, 4), (ig, 1)):
            if a is not None and a.size != n * k:
                raise ValueError("rot / ignore do not match the query count")
        qm = _query_mask(mask, n)
        offsets = np.zeros(n + 1, np.uint64)
        cap = 8 * n + 64 if cap is None else int(cap)
        for attempt in range(2):
            ids = np.empty(max(cap, 1), np.uint32)
            if qm is None:
                rc = self.lib.phys_overlap(self.h, n, _p(st, u32p), _p(p), _p(r), _p(he), _p(ig, u32p), cap, _p(offsets, _abi.u64p),
                                           _p(ids, u32p))
            else:
                rc = self.lib.phys_overlap_filtered(self.h, n, _p(st, u32p), _p(p), _p(r), _p(he), _p(ig, u32p), _p(qm, u16p), cap,
                                                    _p(offsets, _abi.u64p), _p(ids, u32p))
            if rc == _abi.PHYS_ERR_CAPACITY and attempt == 0:
                cap = int(offsets[n])
                continue
            self._ck(rc)
            break
        return offsets, ids[:int(offsets[n])]

    def get_manifolds(self):
        n = C.c_uint64()
        self._ck(self.lib.phys_get_manifolds(self.h, None, None, None, None, 0, C.byref(n)))
        m = n.value
        ids = np.empty((m, 2), np.uint32)
        counts = np.empty(m, np.uint32)
        normals = np.empty((m, 3), np.float32)
        points = np.empty((m, 4, 4), np.float32)
        if m:
            self._ck(self.lib.phys_get_manifolds(self.h, _p(ids, u32p), _p(counts, u32p), _p(normals), _p(points), m,
                                                 C.byref(n)))
        return ids, counts, normals, points

    # ---- contact events (include/physics_hip.h): what began / stopped touching per update, and the solver's impulses
    def enable_contact_events(self, capacity):
        """Keep up to `capacity` contact events on the device between two drains (phys_contact_events_enable); 0 turns
        events off. A new capacity drops the events not yet drained."""
        self._ck(self.lib.phys_contact_events_enable(self.h, int(capacity)))

    def get_contact_events(self):
        """(events, n_dropped): every event stored since the last drain as a structured array (CONTACT_EVENT_DTYPE: body_a,
        body_b, kind CONTACT_BEGIN / CONTACT_END, step, point, impulse, normal), sorted by (step, kind, body_a, body_b),
        and the number of events that did not fit the device buffer. Empties the buffer."""
        n, dropped = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.phys_get_contact_events(self.h, None, 0, C.byref(n), C.byref(dropped)))  # count only
        while True:
            out = np.zeros(n.value, CONTACT_EVENT_DTYPE)
            rc = self.lib.phys_get_contact_events(self.h, out.ctypes.data_as(C.POINTER(PhysContactEvent)), out.shape[0],
                                                  C.byref(n), C.byref(dropped))
            if rc != _abi.PHYS_ERR_CAPACITY:  # (more than counted: another thread stepped the world in between; resize)
                self._ck(rc)
                return out[:n.value], dropped.value

    def get_contact_impulses(self):
        """(M, 4, 3) float32: {pn, pt0, pt1} the last update's solve ended with, per point slot of every manifold (zeros beyond
        its count), row for row in get_manifolds' order."""
        n = C.c_uint64()
        self._ck(self.lib.phys_get_contact_impulses(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4, 3), np.float32)
        if n.value:
            self._ck(self.lib.phys_get_contact_impulses(self.h, _p(out), n.value, C.byref(n)))
        return out

    # ---- trigger volumes (include/physics_hip.h): which bodies are inside a shape, and which entered / left per update
    def set_triggers(self, shape_type, pos, rot=None, half_extent=None, mask=None):
        """Replace the trigger volumes (phys_set_triggers): shape_type scalar or (n,) SHAPE_SPHERE / BOX / CAPSULE, pos (n, 3),
        rot (n, 4) [i, j, k, w] or None (identity), half_extent (3,) or (n, 3) with the bodies' conventions, mask a scalar
        or (n,) u16 or None: trigger k sees body i iff category[i] & mask[k] (None: every body). An empty pos clears the
        set. Forgets the occupancy and the pending trigger events; at most MAX_TRIGGERS volumes (the library refuses more)."""
        p = _f(pos).reshape(-1, 3)
        n = p.shape[0]
        if n and half_extent is None:
            raise ValueError("half_extent is required")
        st = np.asarray(shape_type if n else np.zeros(0, np.uint32))
        if st.ndim > 1 or (st.ndim == 1 and st.shape[0] != n):
            raise ValueError(f"shape_type: needs {n} values, got shape {st.shape}")
        st = np.ascontiguousarray(np.broadcast_to(st.astype(np.uint32), (n,)))
        he = np.asarray(half_extent if n else np.zeros((0, 3)), np.float32).reshape(-1, 3)
        if he.shape[0] not in (1, n):
            raise ValueError(f"half_extent: needs 3 or {n} x 3 values, got shape {np.shape(half_extent)}")
        he = np.ascontiguousarray(np.broadcast_to(he, (n, 3)))
        r = None if rot is None else _f(rot).reshape(-1, 4)
        if r is not None and r.shape[0] != n:
            raise ValueError("rot does not match the trigger count")
        m = _filter_field(mask, n, "mask", 0, 0xFFFF, np.uint16)
        self._ck(self.lib.phys_set_triggers(self.h, n, _p(st, u32p), _p(p), _p(r), _p(he), _p(m, u16p)))
        self.n_triggers = n

    def set_trigger_poses(self, pos, rot=None):
        """New positions (n_triggers, 3) and, unless None, rotations (n_triggers, 4) of the trigger volumes
        (phys_set_trigger_poses), from the next update on. Keeps the occupancy: a body left behind raises EXIT."""
        p = _f(pos).reshape(-1, 3)
        r = None if rot is None else _f(rot).reshape(-1, 4)
        if p.shape[0] != self.n_triggers or (r is not None and r.shape[0] != self.n_triggers):
            raise ValueError(f"pos / rot: need {self.n_triggers} rows (the trigger count)")
        self._ck(self.lib.phys_set_trigger_poses(self.h, self.n_triggers, _p(p), _p(r)))

    # ---- force fields (include/physics_hip.h): volumes that push, drag and attract the bodies whose centre is inside
    def set_force_fields(self, kind, shape_type, pos, rot=None, half_extent=None, mask=None, vec=None, coef=None, exponent=None):
        """Replace the force fields (phys_set_force_fields): kind scalar or (n,) FIELD_ACCEL / FIELD_DRAG / FIELD_RADIAL,
        shape_type scalar or (n,) SHAPE_SPHERE / BOX / CAPSULE, pos (n, 3), rot (n, 4) [i, j, k, w] or None (identity),
        half_extent (3,) or (n, 3) with the bodies' conventions, mask a scalar or (n,) u16 or None (every body), vec (3,) or
        (n, 3) (None: zeros), coef (2,) or (n, 2) (ACCEL: unused; DRAG: linear and angular coefficient, >= 0; RADIAL: strength
        and r0 > 0), exponent a scalar or (n,) in 0..2 or None (0). An empty pos clears the set. At most MAX_FORCE_FIELDS."""
        p = _f(pos).reshape(-1, 3)
        n = p.shape[0]
        if n > _abi.MAX_FORCE_FIELDS:
            raise ValueError(f"at most {_abi.MAX_FORCE_FIELDS} force fields")
        if n and (half_extent is None or coef is None):
            raise ValueError("half_extent and coef are required")

        def words(a, name, known):
            v = np.asarray(a if n else np.zeros(0, np.uint32))
            if v.dtype.kind not in "iub":
                raise ValueError(f"{name}: needs integers")
            if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != n):
                raise ValueError(f"{name}: needs {n} values, got shape {v.shape}")
            if v.size and not np.isin(v, known).all():
                raise ValueError(f"{name}: values must be among {known}")
            return np.ascontiguousarray(np.broadcast_to(v.astype(np.uint32), (n,)))

        def rows(a, cols, name):
            v = np.asarray(a if n else np.zeros((0, cols)), np.float32).reshape(-1, cols)
            if v.shape[0] not in (1, n):
                raise ValueError(f"{name}: needs {cols} or {n} x {cols} values, got shape {np.shape(a)}")
            v = np.ascontiguousarray(np.broadcast_to(v, (n, cols)))
            if not np.isfinite(v).all():
                raise ValueError(f"{name}: non-finite value")
            return v

        kd = words(kind, "kind", (_abi.FIELD_ACCEL, _abi.FIELD_DRAG, _abi.FIELD_RADIAL))
        st = words(shape_type, "shape_type", (_abi.SHAPE_SPHERE, _abi.SHAPE_BOX, _abi.SHAPE_CAPSULE))
        ex = None if exponent is None else words(exponent, "exponent", (0, 1, 2))
        he = rows(half_extent, 3, "half_extent")
        vc = rows(np.zeros(3, np.float32) if vec is None else vec, 3, "vec")
        cf = rows(coef, 2, "coef")
        r = None if rot is None else _f(rot).reshape(-1, 4)
        if r is not None and r.shape[0] != n:
            raise ValueError("rot does not match the force field count")
        if not np.isfinite(p).all() or (r is not None and not np.isfinite(r).all()):
            raise ValueError("pos / rot: non-finite value")
        if (he < 0).any():
            raise ValueError("half_extent: negative value")
        _field_law_check(kd, cf)
        m = _filter_field(mask, n, "mask", 0, 0xFFFF, np.uint16)
        self._ck(self.lib.phys_set_force_fields(self.h, n, _p(kd, u32p), _p(st, u32p), _p(p), _p(r), _p(he), _p(m, u16p), _p(vc), _p(cf),
                                                _p(ex, u32p)))
        self.n_fields, self._field_kinds = n, kd

    def set_force_field_poses(self, pos, rot=None):
        """New positions (n_fields, 3) and, unless None, rotations (n_fields, 4) of the force fields
        (phys_set_force_field_poses), from the next update on."""
        p = _f(pos).reshape(-1, 3)
        r = None if rot is None else _f(rot).reshape(-1, 4)
        if p.shape[0] != self.n_fields or (r is not None and r.shape[0] != self.n_fields):
            raise ValueError(f"pos / rot: need {self.n_fields} rows (the force field count)")
        if not np.isfinite(p).all() or (r is not None and not np.isfinite(r).all()):
            raise ValueError("pos / rot: non-finite value")
        self._ck(self.lib.phys_set_force_field_poses(self.h, self.n_fields, _p(p), _p(r)))

    def set_force_field_params(self, vec, coef):
        """New vec (3,) or (n_fields, 3) and coef (2,) or (n_fields, 2) of the force fields (phys_set_force_field_params);
        kinds, volumes and exponents stay. A strength of 0 switches a field off without rebuilding the set."""
        n = self.n_fields
        v = np.asarray(vec, np.float32).reshape(-1, 3)
        c = np.asarray(coef, np.float32).reshape(-1, 2)
        if v.shape[0] not in (1, n) or c.shape[0] not in (1, n):
            raise ValueError(f"vec / coef: need one row or {n} rows (the force field count)")
        v = np.ascontiguousarray(np.broadcast_to(v, (n, 3)))
        c = np.ascontiguousarray(np.broadcast_to(c, (n, 2)))
        if not (np.isfinite(v).all() and np.isfinite(c).all()):
            raise ValueError("vec / coef: non-finite value")
        _field_law_check(self._field_kinds, c)
        self._ck(self.lib.phys_set_force_field_params(self.h, n, _p(v), _p(c)))

    def apply_force_fields(self):
        """Evaluate the force fields now, into the force / torque accumulators (phys_apply_force_fields): the twin of
        apply_gravity for a caller that steps with step()."""
        self._ck(self.lib.phys_apply_force_fields(self.h))

    # ---- liquids (include/physics_hip.h): buoyancy and drag from the part of each body's shape below a liquid's surface
    @staticmethod
    def _liquid_rows(a, n, cols, name, negative_ok=True):
        v = np.asarray(a, np.float32).reshape(-1, cols)
        if v.shape[0] not in (1, n):
            raise ValueError(f"{name}: needs {cols} or {n} x {cols} values, got shape {np.shape(a)}")
        v = np.ascontiguousarray(np.broadcast_to(v, (n, cols)))
        if not np.isfinite(v).all():
            raise ValueError(f"{name}: non-finite value")
        if not negative_ok and (v < 0).any():
            raise ValueError(f"{name}: negative value")
        return v

    def _liquid_params(self, n, density, gravity, flow, drag):
        z3 = np.zeros(3, np.float32)
        return (self._liquid_rows(density, n, 1, "density", negative_ok=False).reshape(n),
                self._liquid_rows(gravity, n, 3, "gravity"), self._liquid_rows(z3 if flow is None else flow, n, 3, "flow"),
                self._liquid_rows(np.zeros(2, np.float32) if drag is None else drag, n, 2, "drag", negative_ok=False))

    def set_liquids(self, pos, rot=None, half_extent=None, mask=None, density=None, gravity=None, flow=None, drag=None):
        """Replace the liquids (phys_set_liquids): oriented boxes at pos (n, 3) with rot (n, 4) [i, j, k, w] or None (identity) and
        half_extent (3,) or (n, 3), whose local +y face is the surface; mask a scalar or (n,) u16 or None (every body); density
        a scalar or (n,), >= 0; gravity (3,) or (n, 3), the acceleration the liquid is weighed by; flow (3,) or (n, 3) (None:
        zeros); drag (2,) or (n, 2), linear and angular, >= 0 (None: zeros). An empty pos clears the set. At most MAX_LIQUIDS."""
        p = _f(pos).reshape(-1, 3)
        n = p.shape[0]
        if n > _abi.MAX_LIQUIDS:
            raise ValueError(f"at most {_abi.MAX_LIQUIDS} liquids")
        if n and (half_extent is None or density is None or gravity is None):
            raise ValueError("half_extent, density and gravity are required")
        if n == 0:
            half_extent, density, gravity = np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3))
            flow, drag = np.zeros((0, 3)), np.zeros((0, 2))
        he = self._liquid_rows(half_extent, n, 3, "half_extent", negative_ok=False)
        dn, gv, fl, dr = self._liquid_params(n, density, gravity, flow, drag)
        r = None if rot is None else _f(rot).reshape(-1, 4)
        if r is not None and r.shape[0] != n:
            raise ValueError("rot does not match the liquid count")
        if not np.isfinite(p).all() or (r is not None and not np.isfinite(r).all()):
            raise ValueError("pos / rot: non-finite value")
        m = _filter_field(mask, n, "mask", 0, 0xFFFF, np.uint16)
        self._ck(self.lib.phys_set_liquids(self.h, n, _p(p), _p(r), _p(he), _p(m, u16p), _p(dn), _p(gv), _p(fl), _p(dr)))
        self.n_liquids = n

    def set_liquid_poses(self, pos, rot=None):
        """New positions (n_liquids, 3) and, unless None, rotations (n_liquids, 4) of the liquids (phys_set_liquid_poses), from
        the next evaluation on: a tide, a sloshing tank."""
        p = _f(pos).reshape(-1, 3)
        r = None if rot is None else _f(rot).reshape(-1, 4)
        if p.shape[0] != self.n_liquids or (r is not None and r.shape[0] != self.n_liquids):
            raise ValueError(f"pos / rot: need {self.n_liquids} rows (the liquid count)")
        if not np.isfinite(p).all() or (r is not None and not np.isfinite(r).all()):
            raise ValueError("pos / rot: non-finite value")
        self._ck(self.lib.phys_set_liquid_poses(self.h, self.n_liquids, _p(p), _p(r)))

    def set_liquid_params(self, density, gravity, flow=None, drag=None):
        """New density, gravity, flow (None: zeros) and drag (None: zeros) of the liquids (phys_set_liquid_params), each one
        row or n_liquids rows; the volumes and masks stay."""
        n = self.n_liquids
        dn, gv, fl, dr = self._liquid_params(n, density, gravity, flow, drag)
        self._ck(self.lib.phys_set_liquid_params(self.h, n, _p(dn), _p(gv), _p(fl), _p(dr)))

    def apply_liquids(self):
        """Evaluate the liquids now, into the force / torque accumulators (phys_apply_liquids): the twin of
        apply_force_fields for a caller that steps with step()."""
        self._ck(self.lib.phys_apply_liquids(self.h))

    def get_submersion(self):
        """(frac (n,) float32, liquid (n,) uint32): per body, the submerged fraction of its volume in the lowest-index liquid
        that acts on it, and that liquid's index; 0 and 0xFFFFFFFF where none does (phys_get_submersion). Evaluates now and
        leaves the accumulators alone."""
        frac = np.zeros(self.n, np.float32)
        liquid = np.full(self.n, _abi.NO_LIQUID, np.uint32)
        self._ck(self.lib.phys_get_submersion(self.h, _p(frac), _p(liquid, u32p)))
        return frac, liquid

    # ---- continuous collision (include/physics_hip.h): listed bodies stop at the statics and the ground they would pass through
    def set_ccd_bodies(self, ids):
        """Replace the list of bodies that are swept along each collision update's motion (phys_set_ccd_bodies): ids, body
        indices in any order, none twice; empty or None clears the list. Entry k of ccd_hits() is ids[k]. Resets every frac to 1
        and every count to 0. set_bodies clears the list, set_static_bodies keeps it."""
        a = np.zeros(0, np.uint32) if ids is None else np.asarray(ids)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("ids: needs integers")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("ids: needs values in [0, 2^32)")
        a = np.ascontiguousarray(a.reshape(-1), dtype=np.uint32)
        self._ck(self.lib.phys_set_ccd_bodies(self.h, a.size, _p(a, u32p)))
        self.n_ccd = int(a.size)

    def ccd_hits(self):
        """(frac (n_ccd,) float32, target (n_ccd,) uint32, normal (n_ccd, 3) float32, count (n_ccd,) uint32) per list entry
        (phys_get_ccd_hits): of the last update that swept, the share of dt the body was advanced by, what stopped it (RAY_MISS,
        RAY_GROUND, STATIC_ID_BIT | k), the normal from that target to the body, and the updates in which the entry was stopped
        since the list was set. Synchronises."""
        n = self.n_ccd
        frac, target = np.ones(n, np.float32), np.full(n, _abi.RAY_MISS, np.uint32)
        normal, count = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        if n:
            self._ck(self.lib.phys_get_ccd_hits(self.h, _p(frac), _p(target, u32p), _p(normal), _p(count, u32p)))
        return frac, target, normal, count

    def ccd_hits_device(self, frac_out=None, target_out=None, normal_out=None, count_out=None):
        """phys_get_ccd_hits_device into contiguous tensors of the world's device: frac_out float32 (n_ccd,), target_out int32 /
        uint32 (n_ccd,), normal_out float32 (n_ccd, 3), count_out int32 / uint32 (n_ccd,); any may be None. Enqueued on the
        world's stream: sync() before reading."""
        ptrs = []
        for name, x, floating, cols in (("frac_out", frac_out, True, 1), ("target_out", target_out, False, 1),
                                        ("normal_out", normal_out, True, 3), ("count_out", count_out, False, 1)):
            if x is not None and (not x.is_contiguous() or x.numel() != cols * self.n_ccd or x.element_size() != 4
                                  or x.is_floating_point() != floating or not x.is_cuda):
                raise ValueError(f"{name}: needs a contiguous 4-byte device tensor of {cols * self.n_ccd} elements")
            ptrs.append(None if x is None or self.n_ccd == 0 else C.c_void_p(x.data_ptr()))
        self._ck(self.lib.phys_get_ccd_hits_device(self.h, *ptrs))

    def get_submersion_device(self, frac_out=None, liquid_out=None):
        """phys_get_submersion_device into contiguous tensors of the world's device: frac_out float32 (n,), liquid_out int32 /
        uint32 (n,), each or None. Only enqueues on the world's stream."""
        for name, x, floating in (("frac_out", frac_out, True), ("liquid_out", liquid_out, False)):
            if x is not None and (not x.is_cuda or not x.is_contiguous() or x.numel() != self.n or x.element_size() != 4
                                  or x.is_floating_point() != floating):
                raise ValueError(f"{name}: needs a contiguous 4-byte {'float' if floating else 'integer'} device tensor of {self.n}")
        self._ck(self.lib.phys_get_submersion_device(self.h, None if frac_out is None else C.c_void_p(frac_out.data_ptr()),
                                                     None if liquid_out is None else C.c_void_p(liquid_out.data_ptr())))

    def enable_trigger_events(self, capacity):
        """Keep up to `capacity` trigger events on the device between two drains (phys_trigger_events_enable); 0 turns
        them off. A new capacity drops the events not yet drained; the occupancy is tracked either way."""
        self._ck(self.lib.phys_trigger_events_enable(self.h, int(capacity)))

    def get_trigger_events(self):
        """(events, n_dropped): every trigger event stored since the last drain as a structured array (TRIGGER_EVENT_DTYPE:
        trigger, body, kind TRIGGER_ENTER / TRIGGER_EXIT, step), sorted by (step, kind, trigger, body), and the number of
        events that did not fit the device buffer. Empties the buffer."""
        n, dropped = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.phys_get_trigger_events(self.h, None, 0, C.byref(n), C.byref(dropped)))  # count only
        while True:
            out = np.zeros(n.value, TRIGGER_EVENT_DTYPE)
            rc = self.lib.phys_get_trigger_events(self.h, out.ctypes.data_as(C.POINTER(PhysTriggerEvent)), out.shape[0],
                                                  C.byref(n), C.byref(dropped))
            if rc != _abi.PHYS_ERR_CAPACITY:  # (more than counted: another thread stepped the world in between; resize)
                self._ck(rc)
                return out[:n.value], dropped.value

    def get_trigger_overlaps(self, cap=None):
        """(offsets u64[n_triggers + 1], ids u32[offsets[-1]]): the occupants of every trigger as of the last update
        (phys_get_trigger_overlaps); trigger k's body ids, ascending, are ids[offsets[k]:offsets[k + 1]]. The first call
        reserves `cap` ids (default 8 per trigger) and, if they do not fit, the call is repeated once with the reported total."""
        n = self.n_triggers
        offsets = np.zeros(n + 1, np.uint64)
        cap = 8 * n + 64 if cap is None else int(cap)
        for attempt in range(2):
            ids = np.empty(max(cap, 1), np.uint32)
            rc = self.lib.phys_get_trigger_overlaps(self.h, cap, _p(offsets, _abi.u64p), _p(ids, u32p))
            if rc == _abi.PHYS_ERR_CAPACITY and attempt == 0:
                cap = int(offsets[n])
                continue
            self._ck(rc)
            break
        return offsets, ids[:int(offsets[n])]

    def get_color_counts(self):
        out = np.zeros(64, np.uint32)
        self._ck(self.lib.phys_get_color_counts(self.h, _p(out, u32p)))
        return out

    def profile_enable(self, on=True):
        self._ck(self.lib.phys_profile_enable(self.h, int(on)))

    def profile_get(self):
        """{stage: (device ms summed, launches)} and the number of profiled updates."""
        p = PhysProfile()
        self._ck(self.lib.phys_profile_get(self.h, C.byref(p)))
        return {STAGE_NAMES[k]: (p.ms[k], p.launches[k]) for k in range(len(STAGE_NAMES)) if p.launches[k]}, p.steps

    def device_view(self):
        v = PhysDeviceView()
        self._ck(self.lib.phys_get_device_view(self.h, C.byref(v)))
        return v

    # ---- sharded broad-phase
    def set_global_ids(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self._ck(self.lib.phys_set_global_ids(self.h, _p(ids, u32p)))

    def halo_pack(self, x_lo, x_hi, reach, dev_ptr, cap, wait=True):
        """wait=False: enqueue only (no host synchronisation), returns None."""
        n = C.c_uint64()
        self._ck(self.lib.phys_halo_pack(self.h, x_lo, x_hi, reach, C.c_void_p(dev_ptr), cap, C.byref(n) if wait else None))
        return n.value if wait else None

    def halo_pairs(self, dev_ptr, n_remote, skip_first=0, skip_count=0, wait=True):
        n = C.c_uint64()
        self._ck(self.lib.phys_halo_pairs(self.h, C.c_void_p(dev_ptr), n_remote, skip_first, skip_count,
                                          C.byref(n) if wait else None))
        return n.value if wait else None

    def get_cross_pairs(self):
        n = C.c_uint64()
        self._ck(self.lib.phys_get_cross_pairs(self.h, None, 0, C.byref(n)))
        out = np.empty((n.value, 2), np.uint32)
        if n.value:
            self._ck(self.lib.phys_get_cross_pairs(self.h, _p(out, u32p), n.value, C.byref(n)))
        return out

    # ---- sharded worlds with ghost bodies (SURVEY §8 rows E + N4)
    def set_slab(self, x_lo, x_hi, reach):
        self._ck(self.lib.phys_set_slab(self.h, x_lo, x_hi, reach))

    def halo_pack_bodies(self, dev_ptr, cap):
        self._ck(self.lib.phys_halo_pack_bodies(self.h, C.c_void_p(dev_ptr), cap))

    def halo_pack_bodies_face(self, dev_ptr, cap, face):
        """face < 0: bodies within reach of the low slab face only, > 0: of the high face, 0: both."""
        self._ck(self.lib.phys_halo_pack_bodies_face(self.h, C.c_void_p(dev_ptr), cap, int(face)))

    def halo_unpack_ghosts(self, dev_ptr, n_records, skip_first=0, skip_count=0):
        self._ck(self.lib.phys_halo_unpack_ghosts(self.h, C.c_void_p(dev_ptr), n_records, skip_first, skip_count))

    def get_global_ids(self):
        out = np.empty(self.n + int(self.cfg.max_ghosts), np.uint32)
        self._ck(self.lib.phys_get_global_ids(self.h, _p(out, u32p)))
        return out

    def halo_exchange(self, comm):
        """pack -> RCCL all-gather -> unpack (ghost worlds: call BEFORE update) / cross pairs (AABB mode: AFTER)."""
        self._ck(self.lib.phys_halo_exchange(self.h, comm.h))


def block_spmv(nrows, ncols, blocks, vec, transpose=False, device=0):
    """SparseMatrix::multiply_vector / tr_multiply_vector (sparse_matrix.rs:25-50) on the device: `blocks` is the
    add_block list as (row, column, 2-D array) triples; returns M v (or M^T v) as float32."""
    lib = _abi.load_library()
    desc = np.array([[i, j, np.shape(b)[0], np.shape(b)[1]] for i, j, b in blocks], np.uint64).reshape(-1)
    data = (np.concatenate([np.asarray(b, np.float32).reshape(-1) for _, _, b in blocks]).astype(np.float32)
            if blocks else np.zeros(0, np.float32))
    vec = _f(vec).reshape(-1)
    out = np.zeros(ncols if transpose else nrows, np.float32)
    rc = lib.phys_block_spmv(device, nrows, ncols, len(blocks), _p(desc, _abi.u64p), _p(data), _p(vec), vec.size,
                             int(bool(transpose)), _p(out))
    if rc != 0:
        raise PhysError(rc, lib.phys_last_error().decode())
    return out


class Comm:
    """One rank of an RCCL communicator behind the C ABI (phys_comm_*): the id travels by whatever the host has."""

    @staticmethod
    def unique_id():
        lib = _abi.load_library()
        buf = (C.c_uint8 * 128)()
        rc = lib.phys_comm_unique_id(buf)
        if rc != 0:
            raise PhysError(rc, lib.phys_last_error().decode())
        return bytes(buf)

    def __init__(self, world, unique_id, rank, n_ranks, capacity, neighbours=False):
        """neighbours: the ranks are x-slabs ordered by rank, none thinner than the reach - exchange with ranks r - 1 and
        r + 1 only (phys_comm_set_neighbours) instead of an all-gather of every rank's block."""
        self.lib = world.lib
        self.h = C.c_void_p()
        self.rank, self.n_ranks, self.capacity, self.neighbours = rank, n_ranks, capacity, bool(neighbours)
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        rc = self.lib.phys_comm_create(world.h, buf, rank, n_ranks, capacity, C.byref(self.h))
        if rc != 0:
            raise PhysError(rc, self.lib.phys_last_error().decode())
        if neighbours:
            rc = self.lib.phys_comm_set_neighbours(self.h, 1)
            if rc != 0:
                raise PhysError(rc, self.lib.phys_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.phys_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
