"""ctypes view of tests/cpp/libcolor_probe.so (tests/cpp/color_probe.hip, built by __graft_entry__.build()): the read-out of
the colouring stage and the row sort - manifolds, colours, row_src, the counters, the `used` words, the cluster sort's
segment table - and the ColorPlan of the next update. The product library is loaded first (physics_amd._abi.load_library),
so the process maps one ROCm runtime. The library has no kernel; plan_of() and layout() need no GPU."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "libcolor_probe.so")
_lib = None
PATHS = ("Small", "Known", "Probe")


class ProbeError(RuntimeError):
    pass


class Sizes(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_owned", C.c_uint64), ("max_manifolds", C.c_uint64), ("cluster_count", C.c_uint32),
                ("cluster_slots", C.c_uint32), ("cluster_dynamic", C.c_uint32), ("counters_bytes", C.c_uint32)]


class Plan(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("path", "rounds", "round_blocks", "sort_blocks", "cluster_sort_blocks", "cluster_key_blocks",
                                          "full", "rebuild", "stamp", "wants_cluster", "hint_valid", "hint_n_manifolds",
                                          "hint_color_rounds", "hint_full_rounds", "hint_n_new", "hint_n_colors")] + [("color_epoch", C.c_uint64)]


LAYOUT_FIELDS = ("n_manifolds", "unc_count", "n_uncolored", "n_colors", "color_rounds", "overflow", "n_new_manifolds", "color_count",
                 "color_start", "size")


class Layout(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in LAYOUT_FIELDS]


def load():
    """The probe library. A missing file is an error, not a skip: build() makes it."""
    global _lib
    if _lib is not None:
        return _lib
    from physics_amd import _abi
    _abi.load_library()
    if not os.path.exists(LIB_PATH):
        raise ProbeError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(LIB_PATH)
    p = C.c_void_p
    for name, res, args in (
            ("color_probe_layout_get", None, [C.POINTER(Layout)]),
            ("color_probe_plan_of", C.c_int32, [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Plan)]),
            ("color_probe_sizes_get", C.c_int32, [p, C.POINTER(Sizes)]),
            ("color_probe_next_plan", C.c_int32, [p, C.POINTER(Plan)]),
            ("color_probe_read", C.c_int32, [p, p, C.c_uint64, p, p, p, p, p, p, p])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _ck(rc, what):
    if rc != 0:
        raise ProbeError(f"{what}: {'arguments refused' if rc < 0 else 'hipError_t ' + str(rc)}")


def _plan(p):
    d = {k: int(getattr(p, k)) for k, _ in Plan._fields_}
    d["path"] = PATHS[d["path"]]
    for k in ("full", "rebuild", "wants_cluster", "hint_valid"):
        d[k] = bool(d[k])
    return SimpleNamespace(**d)


def layout():
    out = Layout()
    load().color_probe_layout_get(C.byref(out))
    return SimpleNamespace(**{k: int(getattr(out, k)) for k in LAYOUT_FIELDS})


def plan_of(flags=0, solver_iterations=8, n_owned=0, max_manifolds=0, cluster_count=0, ctab_valid=False, color_epoch=0,
            hint_valid=False, hint_n_manifolds=0, hint_color_rounds=0, hint_full_rounds=0, hint_n_colors=0):
    """plan.hpp plan_coloring on these inputs (default debug switches); no world, no GPU."""
    out = Plan()
    _ck(load().color_probe_plan_of(flags, solver_iterations, n_owned, max_manifolds, cluster_count, int(ctab_valid), color_epoch,
                                   int(hint_valid), hint_n_manifolds, hint_color_rounds, hint_full_rounds, hint_n_colors, C.byref(out)),
        "color_probe_plan_of")
    return _plan(out)


def sizes(world):
    out = Sizes()
    _ck(load().color_probe_sizes_get(world.h, C.byref(out)), "color_probe_sizes_get")
    return SimpleNamespace(**{k: int(getattr(out, k)) for k, _ in Sizes._fields_})


def next_plan(world):
    """The ColorPlan the next update of `world` makes. Call it behind world.sync(), immediately before world.update()."""
    out = Plan()
    _ck(load().color_probe_next_plan(world.h, C.byref(out)), "color_probe_next_plan")
    return _plan(out)


def read(world, cluster=False):
    """What the last update left (the stream is synchronised first): a namespace of man_a, man_b, man_color, row_src (the
    stored manifolds), used (uint64 per body slot), the counters' fields, and for cluster=True cluster_slot, cluster_slots,
    cluster_count and seg_start."""
    lib, lay, sz = load(), layout(), sizes(world)
    raw = np.zeros(lay.size, np.uint8)
    none = C.c_void_p()
    _ck(lib.color_probe_read(world.h, raw.ctypes.data_as(C.c_void_p), 0, none, none, none, none, none, none, none), "color_probe_read")
    word = lambda off, count=1: raw[off:off + 4 * count].view(np.uint32).copy()
    stored = min(int(word(lay.n_manifolds)[0]), sz.max_manifolds)
    arrs = [np.full(max(stored, 1), 0xDEADBEEF, np.uint32) for _ in range(4)]
    used = np.full(max(sz.n, 1), 0xDEADBEEFDEADBEEF, np.uint64)
    slot = np.full(max(sz.n, 1), 0xDEADBEEF, np.uint32) if cluster else None
    seg = np.full(sz.cluster_count * 64 + 1, 0xDEADBEEF, np.uint32) if cluster else None
    ptr = lambda a: none if a is None else a.ctypes.data_as(C.c_void_p)
    _ck(lib.color_probe_read(world.h, ptr(raw), stored, *[ptr(a) for a in arrs], ptr(used), ptr(slot), ptr(seg)), "color_probe_read")
    assert min(int(word(lay.n_manifolds)[0]), sz.max_manifolds) == stored, "the world was updated between the two reads"
    out = SimpleNamespace(M=stored, n_bodies=sz.n, man_a=arrs[0][:stored], man_b=arrs[1][:stored], man_color=arrs[2][:stored],
                          row_src=arrs[3][:stored], used=used[:sz.n], n_manifolds=int(word(lay.n_manifolds)[0]),
                          unc_count=word(lay.unc_count, 3), n_uncolored=int(word(lay.n_uncolored)[0]), n_colors=int(word(lay.n_colors)[0]),
                          color_rounds=int(word(lay.color_rounds)[0]), overflow=int(word(lay.overflow)[0]),
                          n_new_manifolds=int(word(lay.n_new_manifolds)[0]), color_count=word(lay.color_count, 64),
                          color_start=word(lay.color_start, 65))
    if cluster:
        out.cluster_slot, out.seg_start = slot[:sz.n], seg
        out.cluster_slots, out.cluster_count = sz.cluster_slots, sz.cluster_count
    return out
