"""Float64 statement of the character walking rule (include/physics_hip.h, phys_character_move), written for the tests from the
rule's text: numpy only, one query at a time. An independent restatement: it shares no code with include/spec/character.h or
the kernels (the slide step between two casts is tests/slide_ref.py's, itself independent of include/spec/slide.h).

    walk(cast, pos, motion, grounded, skin, max_slides, step_height, snap_distance, min_floor_ny) -> dict
    walk_many(cast_many, pos, motion, grounded, ...) -> [dict]     the same walks in lock-step, their casts made in batches

cast(p, d, max_t) -> None or (id, t, normal): the first target a capsule at p meets along d within the distance max_t.
cast_many(rows, p, d, max_t) -> a list of such answers, one per row (rows: which characters ask).
The rule itself is written once, as a generator that yields each cast it needs (steps); walk and walk_many only drive it.
The answer: p, m, status, floor (None or (id, normal)), hits (MOVE's [(id, normal)]), lifted (the lifted slide's), branch (the
names of what decided each phase, in order), audit (the figures the near-tie audit looks at: every |n.y - min_floor_ny| that was
classified, and the two sides of the progress comparison)."""
import numpy as np

import slide_ref

BLOCKED, EXHAUSTED, INVALID = 0x100, 0x200, 0x400
GROUNDED, STEPPED, SNAPPED, ON_STEEP, HIT_WALL, HIT_CEILING = 0x1000, 0x2000, 0x4000, 0x8000, 0x10000, 0x20000
UP, DOWN = np.array([0.0, 1.0, 0.0]), np.array([0.0, -1.0, 0.0])


def classify(n, min_floor_ny):
    return "floor" if n[1] >= min_floor_ny else ("steep" if n[1] > 0 else "wall")


def _slide(p, motion, skin, max_slides, walking, rising, min_floor_ny, audit):
    """slide_ref's loop with the classes and the no-climb rule: (state, hits, flags, branches)"""
    s = slide_ref.begin(p, motion)
    hits, flags, branches = [], 0, []
    ended = False
    for _ in range(max_slides):
        L = np.linalg.norm(s["m"])
        if not L > 0:
            ended = True
            break
        hit = yield (s["p"], s["m"], L + skin)
        if hit is not None:
            hits.append((hit[0], np.asarray(hit[2], np.float64)))
        s, go, branch = slide_ref.step(s, skin, hit)
        if go:
            n = np.asarray(hit[2], np.float64)
            kind = classify(n, min_floor_ny)
            audit["ny"].append(abs(n[1] - min_floor_ny))
            if kind != "floor":
                flags |= HIT_WALL
            if n[1] < 0 and rising:
                flags |= HIT_CEILING
            if walking and kind == "steep" and s["m"][1] > 0:
                h = np.array([s["m"][0], 0.0, s["m"][2]])
                nh = np.array([n[0], 0.0, n[2]])
                nn = nh @ nh
                h = h - nh * ((h @ nh) / nn) if nn > slide_ref.PARALLEL else np.zeros(3)
                if not h @ s["m0"] > 0:
                    h = np.zeros(3)
                s["m"] = h
                branch += "+noclimb"
        branches.append(branch)
        if not go:
            ended = True
            break
    if not ended and np.any(s["m"] != 0):
        s["status"] |= EXHAUSTED
    return s, hits, flags, branches


def steps(pos, motion, grounded, skin, max_slides, step_height, snap_distance, min_floor_ny):
    """the walk as a generator: yields (p, d, max_t) for every cast, is sent its answer, returns the dict"""
    pos, motion = np.asarray(pos, np.float64), np.asarray(motion, np.float64)
    walking = bool(grounded) and not motion[1] > 0
    audit = dict(ny=[], progress=None)
    s, hits, flags, branch = yield from _slide(pos, motion, skin, max_slides, walking, motion[1] > 0, min_floor_ny, audit)
    out = dict(p=s["p"], m=s["m"], status=s["status"] | flags, floor=None, hits=hits, lifted=[], branch=["move:" + ",".join(branch)], audit=audit)
    if s["status"] & BLOCKED:
        return out
    l = np.array([motion[0], 0.0, motion[2]])
    stepped = False
    if walking and step_height > 0 and np.any(l != 0) and flags & HIT_WALL:
        up = yield (pos, UP, step_height + skin)
        lift = step_height if up is None else min(max(up[1] - skin, 0.0), step_height)
        if (up is not None and up[1] == 0) or not lift > 0:
            out["branch"].append("step:no room")
        else:
            b, bhits, bflags, bbranch = yield from _slide(pos + lift * UP, l, skin, max_slides, True, False, min_floor_ny, audit)
            out["lifted"] = bhits
            out["status"] |= (b["status"] & 0xF) << 4
            if b["status"] & BLOCKED:
                out["branch"].append("step:blocked")
            else:
                down = yield (b["p"], DOWN, lift + 2 * skin)
                if down is None or not down[1] > 0:
                    out["branch"].append("step:no landing")
                else:
                    n = np.asarray(down[2], np.float64)
                    audit["ny"].append(abs(n[1] - min_floor_ny))
                    land = b["p"] + max(down[1] - skin, 0.0) * DOWN
                    audit["progress"] = ((land - pos) @ l, (s["p"] - pos) @ l)
                    if classify(n, min_floor_ny) != "floor":
                        out["branch"].append("step:not a floor")
                    elif not audit["progress"][0] > audit["progress"][1]:
                        out["branch"].append("step:no progress")
                    else:
                        stepped = True
                        out["branch"].append("step:taken")
                        out["p"], out["m"] = land, b["m"]
                        out["status"] = (s["status"] & 0xF) | ((b["status"] & 0xF) << 4) | (b["status"] & EXHAUSTED) | bflags | STEPPED | GROUNDED
                        out["floor"] = (down[0], n)
    if not stepped:
        reach = 2 * skin + (snap_distance if walking else 0.0)
        if not reach > 0:
            out["branch"].append("ground:no reach")
        else:
            g = yield (out["p"], DOWN, reach)
            if g is None or not g[1] > 0:
                out["branch"].append("ground:none")
            else:
                n = np.asarray(g[2], np.float64)
                audit["ny"].append(abs(n[1] - min_floor_ny))
                kind = classify(n, min_floor_ny)
                if kind == "floor":
                    out["status"] |= GROUNDED
                    out["floor"] = (g[0], n)
                    if walking and g[1] > 2 * skin:
                        out["p"] = out["p"] + (g[1] - skin) * DOWN
                        out["status"] |= SNAPPED
                        out["branch"].append("ground:snapped")
                    else:
                        out["branch"].append("ground:grounded")
                elif kind == "steep":
                    out["status"] |= ON_STEEP
                    out["floor"] = (g[0], n)
                    out["branch"].append("ground:steep")
                else:
                    out["branch"].append("ground:none")
    return out


def walk(cast, *args):
    gen = steps(*args)
    try:
        req = next(gen)
        while True:
            req = gen.send(cast(*req))
    except StopIteration as done:
        return done.value


def walk_many(cast_many, pos, motion, grounded, *params):
    n = len(pos)
    gens = [steps(pos[i], motion[i], grounded[i], *params) for i in range(n)]
    out, reqs = [None] * n, {}
    for i, g in enumerate(gens):
        try:
            reqs[i] = next(g)
        except StopIteration as done:
            out[i] = done.value
    while reqs:
        rows = sorted(reqs)
        hits = cast_many(np.array(rows), np.array([reqs[i][0] for i in rows]), np.array([reqs[i][1] for i in rows]),
                         np.array([reqs[i][2] for i in rows]))
        for i, hit in zip(rows, hits):
            try:
                reqs[i] = gens[i].send(hit)
            except StopIteration as done:
                out[i] = done.value
                del reqs[i]
    return out
