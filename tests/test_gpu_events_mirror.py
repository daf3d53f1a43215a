"""GPU: contact events through the C++ host mirror - include/physics_state.hpp (tests/cpp/events_scene.cpp: enable,
90 updates, one drain, the impulse rows) - against the same scene on a Python World: the same bytes."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 16_666_667


def _by_hand():
    import physics_amd as pa
    w = pa.World(pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0.0, 0.0, 0.0)))
    pos = np.array([[0.0, 0.8, 0.0], [0.1, 2.1, 0.0], [3.0, 1.5, 0.0], [3.2, 3.0, 0.1], [-4.0, 0.5, 2.0]], np.float32)
    lin = np.zeros((5, 3), np.float32)
    lin[4, 1] = 3.0  # touches the ground, leaves it, comes back
    shape = np.array([pa.SHAPE_SPHERE, pa.SHAPE_SPHERE, pa.SHAPE_BOX, pa.SHAPE_SPHERE, pa.SHAPE_SPHERE], np.uint32)
    w.enable_contact_events(4096)  # before the bodies, as the mirror does (it uploads at its first update)
    w.set_bodies(pos, lin_vel=lin, shape_type=shape, half_extent=np.full((5, 3), 0.5, np.float32))
    for _ in range(90):
        w.update(DT)
    ev, dropped = w.get_contact_events()
    imp = w.get_contact_impulses()
    w.sync()
    w.close()
    return ev, dropped, imp


def test_by_hand_scene_has_begins_ends_and_impulses():
    import physics_amd as pa
    ev, dropped, imp = _by_hand()
    assert dropped == 0 and len(imp) >= 5 and imp[:, 0, 0].max() > 0.0
    kinds = set(ev["kind"])
    pairs = {(int(r["body_a"]), int(r["body_b"])) for r in ev[ev["kind"] == pa.CONTACT_BEGIN]}
    assert pa.CONTACT_BEGIN in kinds and pa.CONTACT_END in kinds, ev
    assert (0, pa.GROUND_ID) in pairs and (0, 1) in pairs and (2, 3) in pairs, pairs
    hop = ev[(ev["body_a"] == 4)]
    assert [int(k) for k in hop["kind"][:3]] == [pa.CONTACT_BEGIN, pa.CONTACT_END, pa.CONTACT_BEGIN], hop


def test_cpp_state_mirror_drains_the_same_bytes():
    exe = os.path.join(ROOT, "tests", "cpp", "events_scene")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "events_scene.cpp"), "-o", exe,
                               "-L", os.path.join(ROOT, "physics_amd", "csrc"), "-lphysics_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "physics_amd", "csrc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    r = json.loads(out.stdout.strip().splitlines()[-1])
    ev, dropped, imp = _by_hand()
    assert r["dropped"] == dropped == 0 and r["n"] == len(ev) > 0 and r["after"] == 0
    assert bytes.fromhex(r["events"]) == np.ascontiguousarray(ev).tobytes()
    assert bytes.fromhex(r["impulses"]) == np.ascontiguousarray(imp).tobytes()
