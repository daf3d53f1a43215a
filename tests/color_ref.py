"""The checker of the colouring stage and the row sort (numpy only): given the read-out of one update (tests/color_probe.py
read(), or any object with the same fields) and the previous update's (sorted keys, colours), every property the solver
kernels rely on is asserted EXACTLY. The colouring itself is contact_ref.color_manifolds (synchronous Jones-Plassmann
rounds restated in numpy; it shares no code with include/spec, the oracle or the kernels); the independence of a colour
class and the row layout are stated here without it.

What holds for `used` (the per-body 64-bit word of coloring.hip): the block it lives in is zeroed at the start of every
update, the narrow phase ORs in the colour of every manifold that KEEPS its colour, and a round's winner stores
used | 1 << colour at its bodies. So after the stage used[body] is exactly the OR of 1 << colour over the manifolds at that
body - on every path, rebuild or not (the rebuild empties the colour TABLE, not `used`). Static partners and the ground have
no word. check_update asserts the equality."""
import numpy as np

import contact_ref as cr

MAX_COLORS = cr.MAX_COLORS
UNCOLORED = 0xFFFFFFFF
NO_HOME = 0xFFFFFFFF
OVF_COLORS = 4  # setup.hpp kOvfColors


class CheckFailed(AssertionError):
    pass


def _need(cond, what):
    if not cond:
        raise CheckFailed(what)


def sort_by_key(a, b, colors):
    """(sorted keys, colours in that order): what the NEXT update's check takes as prev."""
    keys = cr.pair_keys(a, b)
    order = np.argsort(keys, kind="stable")
    return keys[order], np.asarray(colors, np.int64)[order]


def body_incidence(a, b):
    """(body id, manifold index) of every (manifold, body) incidence; static partners and the ground are not bodies."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    dyn = cr.is_body(b)
    m = np.arange(len(a), dtype=np.int64)
    return np.concatenate([a, b[dyn]]), np.concatenate([m, m[dyn]])


def check_independent(a, b, colors):
    """No two manifolds of one colour share a body (stated without the reference colouring)."""
    body, m = body_incidence(a, b)
    pair = body * MAX_COLORS + np.asarray(colors, np.int64)[m]
    uniq, counts = np.unique(pair, return_counts=True)
    bad = uniq[counts > 1]
    _need(len(bad) == 0, f"{len(bad)} (body, colour) cells hold two manifolds or more, e.g. body {bad[:1] // MAX_COLORS}, colour {bad[:1] % MAX_COLORS}")


def used_words(a, b, colors, n_bodies):
    body, m = body_incidence(a, b)
    used = np.zeros(n_bodies, np.uint64)
    np.bitwise_or.at(used, body, np.uint64(1) << np.asarray(colors, np.uint64)[m])
    return used


def check_colors(out, prev=None, expect_overflow=0):
    """Colours of one update; returns the reference's (colors, n_colors, rounds, n_new)."""
    M = out.M
    a, b, col = out.man_a.astype(np.int64), out.man_b.astype(np.int64), out.man_color.astype(np.int64)
    _need(out.overflow == expect_overflow, f"overflow bits {out.overflow:#x}, expected {expect_overflow:#x}")
    _need(out.n_manifolds == M, f"{out.n_manifolds} manifolds found, {M} stored")
    _need(out.n_uncolored == 0, f"n_uncolored = {out.n_uncolored}")
    _need(bool(np.all(out.man_color < MAX_COLORS)), f"{int((out.man_color >= MAX_COLORS).sum())} manifolds without a colour below {MAX_COLORS}")
    _need(bool(np.all(a < out.n_bodies)) and bool(np.all(b[cr.is_body(b)] < out.n_bodies)), "a body id beyond the world")
    keys = cr.pair_keys(a, b)
    _need(len(np.unique(keys)) == M, "a pair occurs twice among the manifolds")
    prev_keys, prev_colors = prev if prev is not None else (None, None)
    ref = cr.color_manifolds(a, b, out.n_bodies, prev_keys, prev_colors)
    ref_colors = ref[0]
    if prev_keys is not None and len(prev_keys) and M:
        at = np.minimum(np.searchsorted(prev_keys, keys), len(prev_keys) - 1)
        kept = prev_keys[at] == keys
        moved = kept & (col != prev_colors[at])
        _need(not moved.any(), f"{int(moved.sum())} manifolds present in the previous update changed colour")
    if not expect_overflow:
        check_independent(a, b, col)
    wrong = col != ref_colors
    _need(not wrong.any(), f"{int(wrong.sum())} of {M} manifolds have another colour than the reference's")
    _need(out.color_rounds == ref[2], f"color_rounds {out.color_rounds}, reference {ref[2]}")
    _need(out.n_new_manifolds == ref[3], f"n_new_manifolds {out.n_new_manifolds}, reference {ref[3]}")
    if getattr(out, "used", None) is not None:  # (the oracle has no such word to show)
        diff = out.used != used_words(a, b, col, out.n_bodies)
        _need(not diff.any(), f"used differs from the OR of the colours at {int(diff.sum())} bodies")
    return ref


def check_counts(out, ref_colors):
    count = np.bincount(np.asarray(ref_colors, np.int64), minlength=MAX_COLORS)[:MAX_COLORS]
    _need(np.array_equal(out.color_count.astype(np.int64), count), "color_count differs from the reference's counts")
    top = int(np.flatnonzero(count).max()) + 1 if count.any() else 0
    _need(out.n_colors == top, f"n_colors {out.n_colors}, highest colour in use + 1 = {top}")


def check_row_src(out):
    """The colour-major layout: row_src a permutation, rows [color_start[c], color_start[c + 1]) exactly colour c's."""
    M = out.M
    start = out.color_start.astype(np.int64)
    _need(start[0] == 0, f"color_start[0] = {start[0]}")
    _need(bool(np.all(np.diff(start) >= 0)), "color_start decreases")
    _need(start[MAX_COLORS] == M, f"color_start[{MAX_COLORS}] = {start[MAX_COLORS]}, {M} manifolds")
    _need(np.array_equal(out.color_count.astype(np.int64), np.diff(start)), "color_count[c] != color_start[c + 1] - color_start[c]")
    rows = out.row_src.astype(np.int64)
    _need(bool(np.all(rows < M)), "row_src names a manifold beyond the stored ones")
    seen = np.bincount(rows, minlength=M)
    _need(bool(np.all(seen == 1)), f"row_src is no permutation: {int((seen == 0).sum())} manifolds missing, {int((seen > 1).sum())} repeated")
    segment = np.searchsorted(start[1:], np.arange(M), side="right")  # the c with start[c] <= r < start[c + 1]
    off = out.man_color.astype(np.int64)[rows] != segment
    _need(not off.any(), f"{int(off.sum())} rows lie in the segment of another colour than their manifold's")


def row_owner(a, b, cluster_slot, slots, clusters):
    """cluster.hip's rule: a row belongs to the home of its body A, else of its body B, else to a hashed cluster."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    slot = np.asarray(cluster_slot, np.int64)
    home = lambda s: np.where(s == NO_HOME, -1, s // max(slots, 1))
    ha = home(slot[a])
    dyn = cr.is_body(b)
    hb = np.where(dyn, home(slot[np.where(dyn, b, 0)]), -1)
    hashed = ((a * 2654435761) % (1 << 32) >> 7) % clusters
    return np.where(ha >= 0, ha, np.where(hb >= 0, hb, hashed))


def check_cluster_rows(out):
    """The (owner cluster, colour) layout: row_src a permutation, rows [seg_start[k * 64 + c], seg_start[k * 64 + c + 1])
    exactly the manifolds of colour c owned by cluster k - so colours ascend inside every cluster's segment."""
    M, bins = out.M, out.cluster_count * MAX_COLORS
    seg = out.seg_start.astype(np.int64)
    _need(len(seg) == bins + 1 and seg[0] == 0 and bool(np.all(np.diff(seg) >= 0)) and seg[bins] == M,
          f"seg_start does not run from 0 to {M} without decreasing")
    rows = out.row_src.astype(np.int64)
    _need(bool(np.all(rows < M)), "row_src names a manifold beyond the stored ones")
    seen = np.bincount(rows, minlength=M)
    _need(bool(np.all(seen == 1)), f"row_src is no permutation: {int((seen == 0).sum())} manifolds missing, {int((seen > 1).sum())} repeated")
    cell = np.searchsorted(seg[1:], np.arange(M), side="right")
    owner = row_owner(out.man_a, out.man_b, out.cluster_slot, out.cluster_slots, out.cluster_count)
    want = owner[rows] * MAX_COLORS + out.man_color.astype(np.int64)[rows]
    off = cell != want
    _need(not off.any(), f"{int(off.sum())} rows lie outside the (cluster, colour) segment of their manifold")
    col = out.man_color.astype(np.int64)[rows]
    same_cluster = (cell[1:] // MAX_COLORS) == (cell[:-1] // MAX_COLORS)
    _need(bool(np.all(col[1:][same_cluster] >= col[:-1][same_cluster])), "colours descend inside a cluster's segment")


def check_update(out, prev=None, cluster=False, expect_overflow=0):
    """Everything above on one update's read-out. Returns (prev for the next update, the reference's tuple)."""
    ref = check_colors(out, prev, expect_overflow)
    check_counts(out, ref[0])
    if cluster:
        check_cluster_rows(out)
    else:
        check_row_src(out)
    return sort_by_key(out.man_a, out.man_b, ref[0]), ref


def round_sizes(a, b, n_bodies, prev=None):
    """Manifolds uncoloured at the start of every round (the lengths of the lists the round kernels walk), restated from
    the definition: a manifold colours in the round in which it has the highest priority among the uncoloured manifolds
    at each of its bodies. Who wins does not depend on the colours, so none are assigned here."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    dyn = cr.is_body(b)
    bb = np.where(dyn, b, 0)
    prio = cr.color_priority(a, b)
    unc = np.ones(len(a), bool)
    if prev is not None and len(prev[0]) and len(a):
        keys = cr.pair_keys(a, b)
        at = np.minimum(np.searchsorted(prev[0], keys), len(prev[0]) - 1)
        unc = prev[0][at] != keys
    sizes = []
    idx = np.flatnonzero(unc)
    while len(idx):
        sizes.append(len(idx))
        top = np.zeros(n_bodies, np.uint64)
        np.maximum.at(top, a[idx], prio[idx])
        d = idx[dyn[idx]]
        np.maximum.at(top, bb[d], prio[d])
        win = (prio[idx] == top[a[idx]]) & (~dyn[idx] | (prio[idx] == top[bb[idx]]))
        idx = idx[~win]
    return sizes


def readout(a, b, colors, n_bodies, rounds, n_new, row_src=True):
    """A read-out as color_probe.read() gives it, made on the host from colours: rows in colour order, the counters
    consistent with them. The CPU tests plant their defects into one of these; the oracle's colours are wrapped in one."""
    from types import SimpleNamespace
    a, b, col = np.asarray(a, np.uint32), np.asarray(b, np.uint32), np.asarray(colors, np.uint32)
    count = np.bincount(col[col < MAX_COLORS], minlength=MAX_COLORS).astype(np.uint32)
    out = SimpleNamespace(M=len(a), n_bodies=n_bodies, man_a=a, man_b=b, man_color=col, n_manifolds=len(a), n_uncolored=0, overflow=0,
                          n_colors=int(np.flatnonzero(count).max()) + 1 if count.any() else 0, color_rounds=rounds,
                          n_new_manifolds=n_new, color_count=count, used=None, row_src=None, color_start=None)
    if row_src:
        out.row_src = np.argsort(col, kind="stable").astype(np.uint32)
        out.color_start = np.concatenate([[0], np.cumsum(count)]).astype(np.uint32)
        out.used = used_words(a, b, col, n_bodies)
    return out
