"""Reference for contact events, written from the definition in include/physics_hip.h and sharing no code with the
product: it imports numpy only. A run is a sequence of per-update manifold id sets; the events of update E are two set
differences against update E - 1.

    BEGIN  pairs of update E that update E - 1 did not have
    END    pairs of update E - 1 that update E does not have

An entry of the sequence is either an (M, 2) array-like of (body_a, body_b) ids - one update - or the string "reset"
(a phys_set_bodies / phys_set_static_bodies between two updates: the history is forgotten, so the next update is all
BEGIN and no END). Steps are numbered from `first_step` (phys_stats.steps after the first update of the sequence)."""
import numpy as np

BEGIN, END = 1, 2
RESET = "reset"
EVENT_KEY = np.dtype([("step", "<u4"), ("kind", "<u4"), ("body_a", "<u4"), ("body_b", "<u4")])


def _pairs(ids):
    a = np.asarray(ids, dtype=np.uint64).reshape(-1, 2)
    keys = (a[:, 0] << np.uint64(32)) | a[:, 1]
    if np.unique(keys).size != keys.size:
        raise ValueError("a pair has one manifold per update: duplicate ids")
    return keys


def expected_events(updates, first_step=1, previous=None):
    """Sorted (step, kind, body_a, body_b) records of the whole sequence; `previous`: the id set of the update before the
    first one (None: none, e.g. a fresh world)."""
    prev = np.zeros(0, np.uint64) if previous is None else _pairs(previous)
    out = []
    step = first_step
    for entry in updates:
        if isinstance(entry, str):
            if entry != RESET:
                raise ValueError(entry)
            prev = np.zeros(0, np.uint64)
            continue
        now = _pairs(entry)
        for kind, keys in ((BEGIN, np.setdiff1d(now, prev)), (END, np.setdiff1d(prev, now))):
            rec = np.zeros(keys.size, EVENT_KEY)
            rec["step"] = step & 0xFFFFFFFF
            rec["kind"] = kind
            rec["body_a"] = (keys >> np.uint64(32)).astype(np.uint32)
            rec["body_b"] = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            out.append(rec)
        prev = now
        step += 1
    if not out:
        return np.zeros(0, EVENT_KEY)
    ev = np.concatenate(out)
    return ev[np.argsort(ev, order=("step", "kind", "body_a", "body_b"), kind="stable")]


def keys_of(events):
    """The (step, kind, body_a, body_b) part of a drained event array, for comparison with expected_events."""
    out = np.zeros(len(events), EVENT_KEY)
    for f in EVENT_KEY.names:
        out[f] = events[f]
    return out
