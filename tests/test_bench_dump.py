"""bench.py --dump-outputs: what the timed path computed, written as .npy (float32 / float64, at most 64 MB in all) so
that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs(n, seed=0):
    rng = np.random.default_rng(seed)
    return {"pos": rng.random((n, 3), dtype=np.float32), "rot_ijkw": rng.random((n, 4), dtype=np.float32),
            "lin_vel": rng.random((n, 3), dtype=np.float32), "ang_vel": rng.random((n, 3), dtype=np.float32),
            "scene_stats": np.arange(len(bench.STAT_FIELDS), dtype=np.float64)}


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    o = _outputs(1000)
    bench.dump_outputs(o, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(f"{k}.npy" for k in o)
    for k, v in o.items():
        assert np.array_equal(np.load(tmp_path / f"{k}.npy"), v)


def test_large_outputs_keep_a_seeded_sample_under_the_limit(tmp_path):
    o = _outputs(2_000_000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(o, str(a))
    bench.dump_outputs(o, str(b))
    assert _dir_bytes(a) <= bench.DUMP_LIMIT_BYTES
    idx = np.load(a / "sample_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and len(idx) > 1_000_000
    assert np.array_equal(idx, np.load(b / "sample_index.npy"))
    for k in ("pos", "rot_ijkw", "lin_vel", "ang_vel"):
        assert np.array_equal(np.load(a / f"{k}.npy"), o[k][idx.astype(np.int64)])
    assert np.array_equal(np.load(a / "scene_stats.npy"), o["scene_stats"])


def _run_bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1", "--steps", str(steps), "--warmup", "2",
           "--preroll", "0", "--reps", "1", "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_dump_is_the_same_from_run_to_run(tmp_path):
    """Two fresh bench processes with the same arguments write the same bits; the result line states the steps it
    timed and the time of one of them."""
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    ra = _run_bench(a, 6)
    _run_bench(b, 6)
    _run_bench(c, 7)
    assert ra["steps"] == 6 and ra["ms_per_step"] > 0
    names = sorted(os.listdir(a))
    assert {"pos.npy", "rot_ijkw.npy", "lin_vel.npy", "ang_vel.npy", "scene_stats.npy"} <= set(names)
    assert names == sorted(os.listdir(b))
    for f in names:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64), f
        assert np.array_equal(x, y), f"{f} differs between two runs with the same arguments"
    # one more timed step leaves the world elsewhere: the dump is of the last timed step, not of a fixed state
    assert not np.array_equal(np.load(a / "pos.npy"), np.load(c / "pos.npy"))


HEADLINE_FIELDS = ("metric", "value", "unit", "higher_is_better", "dtype", "steps", "warmup", "ms_per_step", "steps_per_sec",
                   "repetitions", "scene_stats")
FULL_ONLY_FIELDS = ("roofline", "stages", "cpu_baseline", "full_period")


@pytest.mark.gpu
def test_plain_run_times_the_window_and_full_adds_the_rest():
    """A plain run prints the headline figures and nothing that takes worlds of its own; --full adds the period, the
    profiled window and the CPU baseline to the same headline fields."""
    common = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1", "--steps", "4", "--warmup", "2", "--reps", "1"]
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--cpu-steps", "1"])):
        out = subprocess.run(common + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        lines[mode] = json.loads(out.stdout.strip().splitlines()[-1])
    for mode, line in lines.items():
        assert all(k in line for k in HEADLINE_FIELDS), (mode, sorted(line))
        assert line["metric"] == "rigid_body_steps_per_sec" and line["unit"] == "body-steps/s" and line["steps"] == 4
        assert line["value"] > 0 and line["ms_per_step"] > 0
    assert not any(k in lines["plain"] for k in FULL_ONLY_FIELDS), sorted(lines["plain"])
    assert all(k in lines["full"] for k in FULL_ONLY_FIELDS), sorted(lines["full"])
    assert lines["plain"]["scene_stats"] == lines["full"]["scene_stats"]  # the same K steps of the same trajectory


def test_result_line_keeps_the_headline_of_every_workload():
    """The printed line must survive a driver that keeps only the tail of the output: the other workloads appear with
    their headline figures, the flagship record in full."""
    sub = {"workload": "W", "n_bodies": 10, "value": 1.0, "steps_per_sec": 2.0, "ms_per_step": 500.0,
           "roofline": {"note": "x" * 5000}, "stages": {}, "cpu_baseline": {}}
    out = {"metric": "m", "value": 3.0, "steps": 20, "ms_per_step": 1.5, "roofline": {"kernel": "k"},
           "other_workloads": {"a": sub, "b": dict(sub, workload="V")}}
    out["config"] = {"workload": "C", "flags_note": "y" * 400}
    line = bench.result_line(out)
    assert line["config"] == {"workload": "C"} and out["config"]["flags_note"]
    assert {k: v for k, v in line.items() if k not in ("other_workloads", "config")} == \
        {k: v for k, v in out.items() if k not in ("other_workloads", "config")}
    assert line["other_workloads"] == {wl: {k: rr[k] for k in bench.SUMMARY_FIELDS} for wl, rr in out["other_workloads"].items()}
    assert "roofline" in out["other_workloads"]["a"]  # the whole record is left as it was, for --record
    assert bench.result_line({"value": 1.0}) == {"value": 1.0}
