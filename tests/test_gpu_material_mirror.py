"""GPU: materials through the two host mirrors - physics_amd.state.PhysicsState (RigidBody.friction / .restitution,
set_ground_material) and the C++ include/physics_state.hpp (tests/cpp/material_scene.cpp) - against the same sequence of
calls made on a World by hand: first upload, an edit of a material alone, back to the defaults, and a body edit whose
phys_set_bodies resets the materials."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 16_666_667
HE = np.full((2, 3), 0.5, np.float32)


def _cfg():
    import physics_amd as pa
    return pa.default_config(flags=pa.FLAG_COLLISIONS | pa.FLAG_GROUND_PLANE, gravity_offset=(0.0, 0.0, 0.0))


def _by_hand():
    """The scene of material_scene.cpp on a World; returns (pos, lin, per-frame height and speed of the dropped ball)."""
    import physics_amd as pa
    w = pa.World(_cfg())
    shape = np.full(2, pa.SHAPE_SPHERE, np.uint32)
    w.set_bodies(np.array([[0.0, 1.3, 0.0], [4.0, 0.5, 0.0]], np.float32), lin_vel=np.array([[0, 0, 0], [3, 0, 0]], np.float32),
                 shape_type=shape, half_extent=HE)
    w.set_ground_material(0.4, 0.0)
    w.set_body_materials([w.cfg.friction, 0.1], [0.8, 0.0])
    track = []
    for f in range(40):
        if f == 20:
            w.set_body_materials([w.cfg.friction, 0.9], [0.8, 0.0])
        if f == 30:
            w.set_body_materials([w.cfg.friction, w.cfg.friction], [0.0, 0.0])
        if f == 35:
            pos, rot = w.get_transforms()
            lin, ang = w.get_velocities()
            pos[0, 0] = 1.0
            w.set_bodies(pos, rot=rot, lin_vel=lin, ang_vel=ang, shape_type=shape, half_extent=HE)  # resets the materials
        w.update(DT)
        track.append(w.get_velocities()[0][0, 1])
    w.sync()
    out = (w.get_transforms()[0], w.get_velocities()[0], np.array(track))
    w.close()
    return out


def test_by_hand_scene_bounces_and_slides():
    """What the mirrors are compared with does what it should: the ball leaves the ground at about 0.8 of its impact speed
    (it fell 0.8: 3.96), and the sliding ball is slowed by mu = sqrt(0.1 x 0.4) at first."""
    pos, lin, vy = _by_hand()
    assert vy.max() > 0.8 * 3.5 and vy.min() < -3.5
    assert 0.0 < lin[1, 0] < 3.0


def test_python_state_mirror_uploads_materials_like_the_calls_by_hand():
    from physics_amd import state as st
    import physics_amd as pa
    ents = []
    for i in range(2):
        b = st.RigidBody.new(i)
        b.shape_type = pa.SHAPE_SPHERE
        b.half_extent = np.full(3, 0.5, np.float32)
        ents.append(st.Entity(b))
    ents[0].body.position = np.array([0.0, 1.3, 0.0], np.float32)
    ents[0].body.restitution = 0.8
    ents[1].body.position = np.array([4.0, 0.5, 0.0], np.float32)
    ents[1].body.lin_velocity = np.array([3.0, 0.0, 0.0], np.float32)
    ents[1].body.friction = 0.1
    ps = st.PhysicsState(ents, cfg=_cfg())
    ps.set_ground_material(0.4, 0.0)
    for f in range(40):
        if f == 20:
            ps.entities[1].body.friction = 0.9
        if f == 30:
            for e in ps.entities:
                e.body.friction, e.body.restitution = None, 0.0
        if f == 35:
            ps.entities[0].body.position = np.array([1.0, *ps.entities[0].body.position[1:]], np.float32)
        ps.update(DT)
    pos, lin, _ = _by_hand()
    for i, e in enumerate(ps.entities):
        assert np.array_equal(e.body.position, pos[i]) and np.array_equal(e.body.lin_velocity, lin[i]), i


def test_cpp_state_mirror_uploads_materials_like_the_calls_by_hand():
    exe = os.path.join(ROOT, "tests", "cpp", "material_scene")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "material_scene.cpp"), "-o", exe,
                               "-L", os.path.join(ROOT, "physics_amd", "csrc"), "-lphysics_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "physics_amd", "csrc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    r = json.loads(out.stdout.strip().splitlines()[-1])
    pos, lin, _ = _by_hand()
    assert np.array_equal(np.float32(r["pos"]), pos) and np.array_equal(np.float32(r["lin"]), lin), r
