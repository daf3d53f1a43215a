"""GPU: what the twelve cast entry points (phys_raycast / phys_spherecast / phys_capsulecast, on host or device arrays, plain or
_filtered) check before they touch anything, called through the library directly: a null required array, a count of 2^31, an
empty call, and a call with every optional array null. One query against two bodies and the ground; a null pointer is refused
before any launch, and no call here passes a non-null pointer that is not a valid array of its kind."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# family -> (too many, a null required array): the texts of include/physics_hip.h's three cast families
TEXTS = {
    "raycast": ("phys_raycast: n_rays must be below 2^31", "phys_raycast: null origin, dir, body_out or t_out"),
    "spherecast": ("phys_spherecast: n must be below 2^31", "phys_spherecast: null origin, dir, radius, body_out or t_out"),
    "capsulecast": ("phys_capsulecast: n must be below 2^31", "phys_capsulecast: null origin, dir, radius, half_length, body_out or t_out"),
}
# the arguments behind (world, n), in the order of the call; the _filtered calls take query_mask behind ignore_body
INPUTS = {
    "raycast": ("origin", "dir", "max_t", "ignore_body"),
    "spherecast": ("origin", "dir", "radius", "max_t", "ignore_body"),
    "capsulecast": ("origin", "dir", "rot", "radius", "half_length", "max_t", "ignore_body"),
}
OUTPUTS = {"raycast": ("body_out", "t_out", "normal_out"), "spherecast": ("body_out", "t_out", "normal_out"),
           "capsulecast": ("body_out", "t_out", "normal_out", "point_out")}
REQUIRED = {"raycast": ("origin", "dir", "body_out", "t_out"), "spherecast": ("origin", "dir", "radius", "body_out", "t_out"),
            "capsulecast": ("origin", "dir", "radius", "half_length", "body_out", "t_out")}
# one query straight down from (0, 5, 0) onto body 0, a unit-diameter sphere at (0, 1, 0): its top is at y = 1.5. The ray
# arrives at t = 3.5, the ball of radius 0.25 at 3.25, the upright capsule (radius 0.25, half-length 0.5) at 2.75.
VALUES = {"origin": [0.0, 5.0, 0.0], "dir": [0.0, -1.0, 0.0], "rot": [0.0, 0.0, 0.0, 1.0], "radius": [0.25], "half_length": [0.5],
          "max_t": [100.0], "ignore_body": [1], "query_mask": [0xFFFF]}
T_HIT = {"raycast": 3.5, "spherecast": 3.25, "capsulecast": 2.75}
CALLS = [(family, device, filtered) for family in TEXTS for device in (False, True) for filtered in (False, True)]


@pytest.fixture(scope="module")
def world():
    import physics_amd as pa
    w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0.0, 0.0, 0.0)))
    w.set_bodies(np.array([[0, 1, 0], [3, 1, 0]], np.float32), shape_type=np.array([pa.SHAPE_SPHERE, pa.SHAPE_BOX], np.uint32),
                 half_extent=np.full((2, 3), 0.5, np.float32))
    yield w
    w.close()


def _arrays(family, device, filtered):
    """name -> one-query array of the call, as numpy arrays or as tensors on the GPU; the outputs filled with a pattern"""
    names = INPUTS[family] + (("query_mask",) if filtered else ()) + OUTPUTS[family]
    out = {}
    for k in names:
        if k in ("ignore_body", "body_out"):
            a = np.array(VALUES.get(k, [0x5A5A5A5A]), np.uint32)
        elif k == "query_mask":
            a = np.array(VALUES[k], np.uint16)
        else:
            a = np.array(VALUES.get(k, [-7.0] * (1 if k == "t_out" else 3)), np.float32)
        if device:
            import torch
            a = torch.from_numpy(a.view({2: np.int16, 4: np.int32}[a.itemsize]) if a.dtype.kind == "u" else a).cuda()
        out[k] = a
    return names, out


def _pointer(a, device):
    if a is None:
        return None
    if device:
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.POINTER({"float32": C.c_float, "uint32": C.c_uint32, "uint16": C.c_uint16}[a.dtype.name]))


@pytest.mark.parametrize("family,device,filtered", CALLS, ids=lambda v: str(v))
def test_cast_entry_point_checks(world, family, device, filtered):
    import physics_amd as pa
    w = world
    fn = getattr(w.lib, "phys_" + family + ("_device" if device else "") + ("_filtered" if filtered else ""))
    too_many, null_array = TEXTS[family]
    names, arrays = _arrays(family, device, filtered)

    def call(n, present):
        return fn(w.h, n, *[_pointer(arrays[k], device) if k in present else None for k in names])

    def err():
        return w.lib.phys_last_error().decode()

    # each required array null in turn, everything else given
    for k in REQUIRED[family]:
        assert call(1, set(names) - {k}) == pa._abi.PHYS_ERR_INVALID_ARG, k
        assert err() == null_array, k
    # the count is looked at before the arrays; a null world before either
    assert call(1 << 31, set()) == pa._abi.PHYS_ERR_INVALID_ARG and err() == too_many
    assert fn(None, 1 << 31, *[None] * len(names)) == pa._abi.PHYS_ERR_INVALID_ARG and err() == "null world"
    assert call(0, set()) == 0
    # nothing above wrote an output
    w.sync()
    host = {k: (v.cpu().numpy() if device else v) for k, v in arrays.items()}
    assert host["body_out"].view(np.uint32)[0] == 0x5A5A5A5A and host["t_out"][0] == -7.0
    # every optional array null (a _filtered call's query_mask too: the plain walk then), which writes body_out and t_out;
    # 1e-5 is what the hand scenes of the cast suites allow a closed-form answer
    assert call(1, set(REQUIRED[family])) == 0
    w.sync()
    host = {k: (v.cpu().numpy() if device else v) for k, v in arrays.items()}
    assert host["body_out"].view(np.uint32)[0] == 0
    assert abs(float(host["t_out"][0]) - T_HIT[family]) <= 1e-5
    # ... and with them (ignore_body = 1 hides the other body, the mask sees everything): the same hit, and a normal
    assert call(1, set(names)) == 0
    w.sync()
    host = {k: (v.cpu().numpy() if device else v) for k, v in arrays.items()}
    assert host["body_out"].view(np.uint32)[0] == 0 and abs(float(host["t_out"][0]) - T_HIT[family]) <= 1e-5
    assert np.abs(host["normal_out"] - np.array([0.0, 1.0, 0.0], np.float32)).max() <= 1e-5
