"""CPU: the trigger volumes' reference (tests/trigger_ref.py) on its own, the event struct against the C compiler, and the
Python wrapper's argument checks, which raise before the library is called. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import trigger_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_alone_on_the_ballistic_soup():
    """192 bodies (5 % NONE) at speeds 5 to 15 bouncing in a cage of +-8, six rotated triggers, 48 steps of 1/60 s: bodies
    enter and leave, and the reference's own near-touch pairs (within 1e-4 of touching, where float32 may legitimately
    disagree) stay within the cap the GPU tests allow."""
    sc = tr.soup()
    assert len(sc["pos"]) == 192 and (sc["shape"] == tr.SHAPE_NONE).any()
    speed = np.linalg.norm(sc["vel"], axis=1)
    assert speed.min() >= 5.0 - 1e-3 and speed.max() <= 15.0 + 1e-3
    before, n_events, n_near, kinds = set(), 0, 0, set()
    for pos in tr.ballistic(sc, 48):
        assert np.abs(pos).max() <= sc["cage"]
        now, near = tr.occupancy(sc["triggers"], pos, sc["rot"], sc["shape"], sc["half_extent"])
        ev = tr.events(before, now)
        n_events += len(ev)
        kinds |= {k for k, _, _ in ev}
        n_near += sum(1 for s in near.values() if abs(s) <= tr.NEAR)
        assert all(sc["shape"][i] != tr.SHAPE_NONE for _, i in now)
        before = now
    print(f"reference alone: {n_events} events, {n_near} near-touch pairs")
    assert n_events >= 100 and kinds == {tr.ENTER, tr.EXIT}
    assert n_near <= tr.near_cap(n_events)


def test_reference_masks_and_events():
    trig = dict(shape=np.array([2, 1], np.uint32), pos=np.array([[0, 0, 0], [10, 0, 0]], np.float32), rot=None,
                half_extent=np.array([[1, 1, 1], [2, 0, 0]], np.float32))
    pos = np.array([[0.5, 0, 0], [10, 1, 0], [30, 0, 0], [1.5, 0, 0]], np.float32)
    rot = np.tile([0, 0, 0, 1], (4, 1)).astype(np.float32)
    shape = np.array([1, 2, 1, 0], np.uint32)
    he = np.full((4, 3), 0.25, np.float32)
    a, _ = tr.occupancy(trig, pos, rot, shape, he)
    assert a == {(0, 0), (1, 1)}
    b, _ = tr.occupancy(trig, pos, rot, shape, he, category=[1, 2, 1, 1], mask=[0xFFFF, 1])
    assert b == {(0, 0)}
    assert tr.events(a, b) == [(tr.EXIT, 1, 1)] and tr.events(set(), a) == [(tr.ENTER, 0, 0), (tr.ENTER, 1, 1)]
    pos[2] = [np.nan, 0, 0]
    assert tr.occupancy(trig, pos, rot, shape, he)[0] == a


def test_trigger_event_struct_matches_the_c_compiler(tmp_path):
    from physics_amd import _abi, world
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "physics_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %u %u %u", '
           'sizeof(phys_trigger_event), offsetof(phys_trigger_event, trigger), offsetof(phys_trigger_event, body), '
           'offsetof(phys_trigger_event, kind), offsetof(phys_trigger_event, step), PHYS_MAX_TRIGGERS, PHYS_TRIGGER_ENTER, '
           'PHYS_TRIGGER_EXIT);}')
    exe = str(tmp_path / "trigger_sizes")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[0] == 16
    E = _abi.PhysTriggerEvent
    assert got == [C.sizeof(E), E.trigger.offset, E.body.offset, E.kind.offset, E.step.offset, _abi.MAX_TRIGGERS, _abi.TRIGGER_ENTER,
                   _abi.TRIGGER_EXIT]
    d = world.TRIGGER_EVENT_DTYPE
    assert d.itemsize == 16 and [d.fields[k][1] for k in ("trigger", "body", "kind", "step")] == got[1:5]
    import physics_amd
    assert (physics_amd.MAX_TRIGGERS, physics_amd.TRIGGER_ENTER, physics_amd.TRIGGER_EXIT) == (1024, 1, 2)
    assert physics_amd.TRIGGER_EVENT_DTYPE is d


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _unbound_world(n_triggers=0):
    from physics_amd import World
    w = World.__new__(World)  # no phys_create: there is no GPU here, and the checks under test come before any call
    w.lib, w.h, w.n, w.n_static, w.n_triggers = _NoLibrary(), None, 0, 0, n_triggers
    return w


def test_wrapper_validates_before_the_library_is_called():
    w = _unbound_world(n_triggers=3)
    pos = np.zeros((3, 3), np.float32)
    he = np.ones((3, 3), np.float32)
    with pytest.raises(ValueError):
        w.set_triggers([2, 2], pos, half_extent=he)                      # two shapes for three volumes
    with pytest.raises(ValueError):
        w.set_triggers(2, pos)                                           # no half extents
    with pytest.raises(ValueError):
        w.set_triggers(2, pos, half_extent=np.ones((2, 3), np.float32))  # two half extents for three volumes
    with pytest.raises(ValueError):
        w.set_triggers(2, pos, rot=np.zeros((2, 4), np.float32), half_extent=he)
    with pytest.raises(ValueError):
        w.set_triggers(2, pos, half_extent=he, mask=[1, 2])              # mask length
    with pytest.raises(ValueError):
        w.set_triggers(2, pos, half_extent=he, mask=0x10000)             # mask range
    with pytest.raises(ValueError):
        w.set_triggers(2, pos, half_extent=he, mask=[-1, 1, 1])
    with pytest.raises(ValueError):
        w.set_triggers(2, pos, half_extent=he, mask=[1.0, 1.0, 1.0])     # not integers
    with pytest.raises(ValueError):
        w.set_trigger_poses(np.zeros((2, 3), np.float32))                # the world has three
    with pytest.raises(ValueError):
        w.set_trigger_poses(pos, rot=np.zeros((4, 4), np.float32))
    w.h = None  # (nothing to destroy)
