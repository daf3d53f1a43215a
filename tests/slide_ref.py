"""Float64 statement of the move-and-slide rule (include/physics_hip.h, phys_move_and_slide), written for the tests from the
rule's text: numpy only, one query at a time. An independent restatement: it shares no code with include/spec/slide.h or the
kernels.

    valid(pos, motion, rot, R, h)                                   the query's own values are usable
    step(state, skin, hit)  -> (state, go, branch)                  what one cast's answer does to a state
    slide(cast, pos, motion, skin, max_slides) -> (p, m, status, hits)   the whole loop over a cast function

state: dict(p, m, m0, n_prev (None before the first hit), status). hit: None (a miss) or (id, t, normal). branch names what
decided the step: "miss", "blocked", "plane", "crease", "parallel", and "+turnback" appended where the slide was stopped."""
import numpy as np

BLOCKED, EXHAUSTED, INVALID = 0x100, 0x200, 0x400
PARALLEL = 1e-12
MAX_LENGTH = 3.0e38


def valid(pos, motion, rot, R, h):
    vals = [np.asarray(pos, np.float64), np.asarray(motion, np.float64), np.float64(R), np.float64(h)]
    if rot is not None:
        vals.append(np.asarray(rot, np.float64))
    if not all(np.isfinite(v).all() for v in vals):
        return False
    if R < 0 or h < 0:
        return False
    # the length as float32 arithmetic sees it: squares that overflow float32 make it infinite
    with np.errstate(over="ignore"):
        m = np.asarray(motion, np.float32)
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    return bool(length <= np.float32(MAX_LENGTH))


def begin(pos, motion):
    return dict(p=np.asarray(pos, np.float64), m=np.asarray(motion, np.float64), m0=np.asarray(motion, np.float64), n_prev=None, status=0)


def step(state, skin, hit):
    s = dict(state)
    if hit is None:
        s["p"], s["m"] = s["p"] + s["m"], np.zeros(3)
        return s, False, "miss"
    _, t, n = hit
    n = np.asarray(n, np.float64)
    s["status"] += 1
    if t == 0:
        s["status"] |= BLOCKED
        return s, False, "blocked"
    L = np.linalg.norm(s["m"])
    u = s["m"] / L
    a = min(max(t - skin, 0.0), L)
    s["p"] = s["p"] + a * u
    r = (L - a) * u
    slide_ = r - n * (r @ n)
    branch = "plane"
    if s["n_prev"] is not None and slide_ @ s["n_prev"] < 0:
        c = np.cross(s["n_prev"], n)
        cc = c @ c
        if cc > PARALLEL:
            slide_, branch = c * ((r @ c) / cc), "crease"
        else:
            slide_, branch = np.zeros(3), "parallel"
    if not slide_ @ s["m0"] > 0:
        slide_, branch = np.zeros(3), branch + "+turnback"
    s["n_prev"], s["m"] = n, slide_
    return s, True, branch


def slide(cast, pos, motion, skin, max_slides):
    """cast(p, m, max_t) -> None or (id, t, normal). Returns (p, m, status, [(id, normal)])."""
    s = begin(pos, motion)
    hits = []
    ended = False
    for _ in range(max_slides):
        L = np.linalg.norm(s["m"])
        if not L > 0:
            ended = True
            break
        hit = cast(s["p"], s["m"], L + skin)
        if hit is not None:
            hits.append((hit[0], np.asarray(hit[2], np.float64)))
        s, go, _ = step(s, skin, hit)
        if not go:
            ended = True
            break
    if not ended and np.any(s["m"] != 0):
        s["status"] |= EXHAUSTED
    return s["p"], s["m"], s["status"], hits
