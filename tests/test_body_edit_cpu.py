"""CPU: the in-place body edits without a GPU. The ten symbols in the library, the ctypes table, the header and the Rust shim;
the Python wrapper's checks; the spec header read by a host compiler alone; the library's own arithmetic
(tests/cpp/body_edit_probe.cpp compiles include/spec/body_edit.h and the setup.hpp ordering with the host compiler, once
under the address and undefined-behaviour sanitizers) against the float64 reference (tests/body_edit_ref.py) within the bound
its docstring derives; the ordering function's hand cases, its refusals and phys_sync's reading of the bad-edit bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import body_edit_probe as bp
import body_edit_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("phys_set_body_poses", "phys_set_body_velocities", "phys_apply_impulses", "phys_apply_forces", "phys_get_body_states")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return bp.build(str(tmp_path_factory.mktemp("body_edit_probe") / "body_edit_probe"))


@pytest.fixture(scope="module")
def probe_sanitized(tmp_path_factory):
    return bp.build(str(tmp_path_factory.mktemp("body_edit_probe_san") / "body_edit_probe"), sanitize=True)


# ---- symbols and wrapper ---------------------------------------------------------------------------------------------------
def test_symbols_exported_bound_and_declared_in_the_rust_shim():
    from physics_amd import World, _abi
    lib = _abi.load_library()
    rust = open(os.path.join(ROOT, "rust", "physics_hip_sys", "src", "lib.rs")).read()
    header = open(os.path.join(ROOT, "include", "physics_hip.h")).read()
    for base in NAMES:
        for name in (base, base + "_device"):
            assert hasattr(lib, name), f"{name} is not exported"
            assert name in _abi.PROTOTYPES and len(re.findall(rf"pub fn {name}\s*\(", rust)) == 1
            assert re.search(rf"int32_t {name}\(", header)
            assert len(_abi.PROTOTYPES[name][1]) == len(_abi.PROTOTYPES[base][1])
        assert callable(getattr(World, base[len("phys_"):])) and callable(getattr(World, base[len("phys_"):] + "_device"))
    assert "#define PHYS_ABI_VERSION 2u" in header


class _NoLibrary:
    """Stands where the loaded library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_validates_shapes_before_the_library_is_called():
    from physics_amd import World
    w = World.__new__(World)  # no phys_create: there is no GPU here, and the checks under test come before any call
    w.lib, w.h, w.n = _NoLibrary(), None, 8
    three = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError):
        w.set_body_poses([0, 1], pos=three)                    # three rows for two ids
    with pytest.raises(ValueError):
        w.set_body_poses([0, 1, 2], rot=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        w.set_body_velocities([0.5, 1.0], lin=three[:2])       # ids are integers
    with pytest.raises(ValueError):
        w.set_body_velocities([-1, 1], lin=three[:2])
    with pytest.raises(ValueError):
        w.apply_impulses([0, 1, 2], None)                      # the impulse is required
    with pytest.raises(ValueError):
        w.apply_impulses([0, 1, 2], three, point=three[:2])
    with pytest.raises(ValueError):
        w.apply_forces([0, 1, 2], None)
    with pytest.raises(ValueError):
        w.apply_forces([0, 1, 2], three, torque=np.zeros((4, 3)))
    w.h = None  # (nothing to destroy)


def test_spec_header_needs_no_hip():
    header = os.path.join(ROOT, "include", "spec", "body_edit.h")
    src = f'#include "{header}"\nint main() {{ uint32_t ids[2] = {{1, 1}}; return be_leads(ids, 1); }}\n'
    for compiler, lang, std in (("gcc", "c", "-std=c99"), ("g++", "c++", "-std=c++17")):
        subprocess.run([compiler, "-x", lang, std, "-Wall", "-Werror", "-fsyntax-only", "-"], input=src.encode(), check=True)
    text = open(header).read()
    assert "hip" not in re.sub(r"/\*.*?\*/", "", text, flags=re.S).lower()
    edit = open(os.path.join(ROOT, "physics_amd", "csrc", "edit.hip")).read()
    for fn in ("be_impulse(", "be_force(", "be_run_end(", "be_leads(", "be_out_of_order("):
        assert fn in edit, f"edit.hip does not call {fn[:-1]}"


# ---- the ordering function, the refusals, the overflow bit (hand cases inside the probe) ---------------------------------------
def test_ordering_refusals_and_the_overflow_bit(probe):
    out = subprocess.run([probe, "--checks"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^\d+ checks passed$", out.stdout.strip()) and int(out.stdout.split()[0]) >= 40


def test_probe_refuses_a_bad_scene_with_the_stated_codes(probe, tmp_path):
    pos = np.zeros((4, 3), np.float32)
    vec = np.ones((2, 3), np.float32)
    for ids, v, code in (([0, 4], vec, -6), ([0, 3], vec * np.float32(np.nan), -1), ([0, 3], vec * np.float32(np.inf), -1)):
        scene = str(tmp_path / "bad.txt")
        bp.write_scene(scene, "impulses", "diag", pos, ids, v)
        out = subprocess.run([probe, scene], capture_output=True, text=True)
        assert out.returncode == 3 and out.stdout.startswith(f"refused {code}:"), out.stdout


# ---- the spec against the float64 reference -------------------------------------------------------------------------------------
def _scene(seed, n, m):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, max(1, n - 3), m)  # the last three bodies stay untouched
    ids[: min(m, 7)] = ids[0]  # seven entries on one body at least, scattered through the batch by the shuffle
    rng.shuffle(ids)
    return dict(rng=rng, ids=ids.astype(np.uint32), pos=rng.uniform(-5, 5, (n, 3)).astype(np.float32),
                vel=rng.normal(size=(n, 3)).astype(np.float32), ang=rng.normal(size=(n, 3)).astype(np.float32),
                mass=rng.uniform(0.5, 3.0, n).astype(np.float32), vec=rng.normal(size=(m, 3)).astype(np.float32) * 3,
                point=rng.uniform(-6, 6, (m, 3)).astype(np.float32), third=rng.normal(size=(m, 3)).astype(np.float32))


@pytest.mark.parametrize("layout", ["shared", "diag", "full"])
@pytest.mark.parametrize("has_point,has_third", [(False, False), (True, False), (False, True), (True, True)])
def test_impulses_against_the_reference(probe, tmp_path, layout, has_point, has_third):
    n, m = 37, 120
    s = _scene(11 + len(layout), n, m)
    inertia = br.inertia_tensors(layout, n, s["rng"])
    point, third = (s["point"] if has_point else None), (s["third"] if has_third else None)
    scene = str(tmp_path / "scene.txt")
    bp.write_scene(scene, "impulses", layout, s["pos"], s["ids"], s["vec"], point, third, vel=s["vel"], ang=s["ang"], mass=s["mass"],
                   inertia=inertia)
    v, w, inv = bp.run(probe, scene)
    if layout == "shared":
        inv = np.broadcast_to(inv[0], inv.shape)
    if layout != "full":
        assert not (inv * (1 - np.eye(3))).any()
    inv_mass = (np.float32(1.0) / s["mass"]).astype(np.float32)
    ref = br.apply_impulses(s["pos"], s["vel"], s["ang"], inv_mass, inv, s["ids"], s["vec"], point, third)
    ev, ew = np.abs(v - ref["v"]), np.abs(w - ref["w"])
    assert (ev <= br.bound(ref["K"], ref["Sv"])).all(), (ev / br.bound(ref["K"], ref["Sv"])).max()
    assert (ew <= br.bound(ref["K"], ref["Sw"])).all(), (ew / br.bound(ref["K"], ref["Sw"])).max()
    untouched = ref["K"] == 0
    assert untouched.any() and np.array_equal(v[untouched], s["vel"][untouched]) and np.array_equal(w[untouched], s["ang"][untouched])
    assert ref["K"].max() >= 7 and (np.abs(v - s["vel"])[~untouched] > 0).any()


@pytest.mark.parametrize("has_point,has_third", [(False, False), (True, False), (False, True), (True, True)])
def test_forces_against_the_reference(probe, tmp_path, has_point, has_third):
    n, m = 37, 120
    s = _scene(23, n, m)
    point, third = (s["point"] if has_point else None), (s["third"] if has_third else None)
    F0, T0 = s["vel"], s["ang"]  # accumulators that are not zero to begin with
    scene = str(tmp_path / "scene.txt")
    bp.write_scene(scene, "forces", "diag", s["pos"], s["ids"], s["vec"], point, third, force=F0, torque=T0)
    F, T, _ = bp.run(probe, scene)
    ref = br.apply_forces(s["pos"], F0, T0, s["ids"], s["vec"], point, third)
    assert (np.abs(F - ref["F"]) <= br.bound(ref["K"], ref["SF"])).all()
    assert (np.abs(T - ref["T"]) <= br.bound(ref["K"], ref["ST"])).all()
    untouched = ref["K"] == 0
    assert np.array_equal(F[untouched], F0[untouched]) and np.array_equal(T[untouched], T0[untouched])
    if not has_point and not has_third:
        assert np.array_equal(T, T0)  # a force at the centre turns nothing


def test_zero_inverse_mass_and_zero_inverse_inertia(probe, tmp_path):
    """inv_mass = 0: the linear velocity stays put, w changes only through I^-1; with I^-1 = 0 as well (a singular tensor is
    staged as zeros) nothing moves at all."""
    n, m = 5, 40
    s = _scene(31, n, m)
    inv_mass = np.zeros(n, np.float32)
    scene = str(tmp_path / "scene.txt")
    inertia = br.inertia_tensors("full", n, s["rng"])
    bp.write_scene(scene, "impulses", "full", s["pos"], s["ids"], s["vec"], s["point"], s["third"], vel=s["vel"], ang=s["ang"],
                   inv_mass=inv_mass, inertia=inertia)
    v, w, inv = bp.run(probe, scene)
    assert np.array_equal(v, s["vel"])
    ref = br.apply_impulses(s["pos"], s["vel"], s["ang"], inv_mass, inv, s["ids"], s["vec"], s["point"], s["third"])
    assert (np.abs(w - ref["w"]) <= br.bound(ref["K"], ref["Sw"])).all() and (w != s["ang"]).any()
    for layout in ("diag", "full"):
        bp.write_scene(scene, "impulses", layout, s["pos"], s["ids"], s["vec"], s["point"], s["third"], vel=s["vel"], ang=s["ang"],
                       inv_mass=inv_mass, inertia=np.zeros((n, 3, 3), np.float32))
        v, w, inv = bp.run(probe, scene)
        assert not inv.any()
        assert np.array_equal(v, s["vel"]) and np.array_equal(w, s["ang"])


def test_known_answers_by_hand(probe, tmp_path):
    """One body at (1, 0, 0), mass 2, inertia diag(2, 4, 8): J = (0, 3, 0) at point (2, 0, 0) gives v += (0, 1.5, 0) and
    L = r x J = (1, 0, 0) x (0, 3, 0) = (0, 0, 3), w += (0, 0, 3 / 8); then an angular impulse (2, 0, 0) alone: w.x += 1."""
    scene = str(tmp_path / "scene.txt")
    inertia = np.diag([2.0, 4.0, 8.0]).astype(np.float32)[None]
    bp.write_scene(scene, "impulses", "diag", [[1, 0, 0]], [0, 0], [[0, 3, 0], [0, 0, 0]], point=[[2, 0, 0], [1, 0, 0]],
                   third=[[0, 0, 0], [2, 0, 0]], mass=[2.0], inertia=inertia)
    v, w, inv = bp.run(probe, scene)
    assert np.array_equal(v, [[0, 1.5, 0]]) and np.array_equal(w, [[1.0, 0, 0.375]])
    assert np.array_equal(np.diag(inv[0]), [0.5, 0.25, 0.125])
    bp.write_scene(scene, "forces", "diag", [[1, 0, 0]], [0, 0], [[0, 3, 0], [1, 0, 0]], point=[[2, 0, 0], [1, 5, 0]],
                   third=[[0, 0, 0], [0, 0, 1]])
    F, T, _ = bp.run(probe, scene)
    # T = (1, 0, 0) x (0, 3, 0) + (0, 5, 0) x (1, 0, 0) + (0, 0, 1) = (0, 0, 3) + (0, 0, -5) + (0, 0, 1)
    assert np.array_equal(F, [[1, 3, 0]]) and np.array_equal(T, [[0, 0, -1]])


# ---- the same under the sanitizers: a stand-alone program, run here --------------------------------------------------------------
def test_probe_runs_clean_under_the_sanitizers(probe, probe_sanitized, tmp_path):
    out = subprocess.run([probe_sanitized, "--checks"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    s = _scene(41, 65, 300)
    scene = str(tmp_path / "scene.txt")
    for mode in ("impulses", "forces"):
        bp.write_scene(scene, mode, "full", s["pos"], s["ids"], s["vec"], s["point"], s["third"], vel=s["vel"], ang=s["ang"], mass=s["mass"],
                       inertia=br.inertia_tensors("full", 65, s["rng"]), force=s["vel"], torque=s["ang"])
        plain, san = bp.run(probe, scene), bp.run(probe_sanitized, scene)
        for a, b in zip(plain, san):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    empty = str(tmp_path / "empty.txt")
    bp.write_scene(empty, "impulses", "shared", np.zeros((3, 3), np.float32), [], np.zeros((0, 3), np.float32))
    v, w, _ = bp.run(probe_sanitized, empty)
    assert not v.any() and not w.any()
