/* character.h — normative scalar definition of character walking (physics_hip.h, phys_character_move): a
 * capsule character moves and slides (slide.h), does not climb what is too steep, steps up onto low obstacles, stays on the
 * floor it walks down, and learns what it stands on. Up is +y, the ground plane's normal.
 *
 * The reference (martingoe/physics) has no queries, so this header is the specification itself. The walk is a state machine
 * around ONE capsule cast: ch_next says which cast to make next (or that the query is done), ch_answer consumes that cast's
 * answer. The HIP kernel (physics_amd/csrc/character.hip) and a host compiler that reads the header alone
 * (tests/cpp/character_probe.cpp) drive exactly this machine, so one launch and a host loop of phys_capsulecast calls agree
 * bit for bit. Nothing between two casts is arithmetic of the caller's. Build with -ffp-contract=off.
 *
 *   if !ch_valid(...): status = CH_INVALID, pos_out = pos, remaining_out = motion, every slot empty, no ground state
 *   ch_begin(&s, pos, motion, grounded_in, skin, max_slides, step_height, snap_distance, min_floor_ny)
 *   while ch_next(&s, &req):
 *       (id, t, n, point) = capsule cast(origin req.origin, dir req.dir, rot, R, h, max_t = req.max_t, ignore, mask)
 *       if req.slot >= 0 and id != PHYS_RAY_MISS: hit slot req.slot = (id, n, point)
 *       ch_answer(&s, id, t, n, point)
 *       if req.slot == CH_SLOT_FLOOR and ch_floor_found(&s): floor = (id, n, point)
 *   pos_out = s.sl.p, remaining_out = s.sl.m, status_out = s.status
 *
 * A hit normal n is FLOOR when n.y >= min_floor_ny, STEEP when 0 < n.y < min_floor_ny and WALL when n.y <= 0 (ceilings too).
 * The character is WALKING in this call when grounded_in != 0 and !(motion.y > 0).
 *
 * MOVE     the loop of slide.h on the whole motion (sl_length, sl_max_t, sl_miss, sl_hit, sl_ran_out, unchanged), its hits in
 *          slots 0 .. max_slides - 1. While walking only: after sl_hit on a STEEP normal a slide that would gain height
 *          (m.y > 0) is replaced by its horizontal part, less what points into the horizontal part nh of n (nothing where
 *          |nh|^2 <= SL_PARALLEL), and stopped where it turns back against the motion asked for: a walker follows the contour of
 *          a slope that is too steep and never climbs it. Falling onto one keeps the true normal and slides down. For a
 *          character that is not walking MOVE is phys_move_and_slide bit for bit. BLOCKED (t == 0) ends the query.
 * STEP     only when walking, step_height > 0, the horizontal part l = (motion.x, 0, motion.z) is not zero and MOVE met a hit
 *          that is not FLOOR. (a) cast up from pos along (0, 1, 0) with max_t = step_height + skin: lift = step_height on a
 *          miss, else min(max(t - skin, 0), step_height); abandon when t == 0 or !(lift > 0). (b) a fresh slide loop from
 *          pos + lift * up with motion l, the same rules, its hits in slots max_slides .. 2 max_slides - 1; abandon when it is
 *          BLOCKED. (c) cast down along (0, -1, 0) with max_t = lift + 2 skin: accept when it hits with t > 0, the normal is FLOOR
 *          and (p_b - pos) . l > (p_move - pos) . l (the cast is vertical and l horizontal, so where (b) ended stands for the
 *          landing point). Accepted: the character lands max(t - skin, 0) lower, skin above that floor, remaining is what (b)
 *          left, STEPPED and GROUNDED are set and the floor is this hit. Abandoned: MOVE's result stands untouched.
 * GROUND   not after an accepted step or BLOCKED. One cast down along (0, -1, 0) from the position reached with
 *          max_t = reach = 2 skin + (walking ? snap_distance : 0); none when !(reach > 0). A FLOOR hit with t > 0: GROUNDED, the
 *          floor is this hit; when walking and t > 2 skin the character also moves down by t - skin and SNAPPED is set. A STEEP
 *          hit with t > 0: ON_STEEP, the floor outputs report it, not grounded, no snap. Otherwise: no ground state.
 *
 * (c) looks 2 skin beyond the lift, not skin: a character that stands skin above a floor - where a landing or a snap of this very
 * rule leaves it - finds the level it left at t = lift + skin, and with that as the cast's limit rounding would decide whether
 * stepping over a low obstacle onto the same level is a landing. With the band of GROUND as the margin it is one.
 *
 * The vertical casts use unit directions, so their t is a distance and max_t a length as given. At most 2 max_slides + 3 casts.
 *
 * status: MOVE's hit count in bits 0-3, the lifted slide's (b) in bits 4-7 (both count the casts that were made, whether or not
 * the step was accepted; the slots hold them); BLOCKED, EXHAUSTED (slide.h's values), HIT_WALL (a hit that is not FLOOR) and
 * HIT_CEILING (a hit with n.y < 0 while motion.y > 0) describe the slide loop whose result was taken: MOVE's, or (b)'s when
 * STEPPED.
 *
 * skin == 0 is allowed and degenerate as in slide.h: the character rests ON what it hit, the next cast starts touching
 * (BLOCKED), reach is snap_distance alone and a character at rest on a floor finds it at t == 0: not grounded.
 */
#ifndef PHYS_SPEC_CHARACTER_H
#define PHYS_SPEC_CHARACTER_H

#include "vec.h"
#include "slide.h"

#define CH_HITS_SHIFT 4u        /* the lifted slide's hit count: bits 4-7 */
#define CH_BLOCKED SL_BLOCKED
#define CH_EXHAUSTED SL_EXHAUSTED
#define CH_INVALID SL_INVALID
#define CH_GROUNDED 0x1000u     /* a FLOOR within 2 skin (+ snap_distance when walking) below where the character ends */
#define CH_STEPPED 0x2000u      /* the step-up was taken */
#define CH_SNAPPED 0x4000u      /* the character was moved down onto the floor */
#define CH_ON_STEEP 0x8000u     /* what lies below is too steep to stand on */
#define CH_HIT_WALL 0x10000u    /* a hit that is not FLOOR on the path taken */
#define CH_HIT_CEILING 0x20000u /* a hit with n.y < 0 on the path taken while motion.y > 0 */

#define CH_MISS 0xFFFFFFFEu /* PHYS_RAY_MISS */

#define CH_SLOT_NONE (-1)  /* the cast fills nothing */
#define CH_SLOT_FLOOR (-2) /* the cast's hit is the floor when ch_floor_found says so afterwards */

#define CH_MOVE 0u
#define CH_UP 1u
#define CH_LIFTED 2u
#define CH_DOWN 3u
#define CH_GROUND 4u
#define CH_DONE 5u

typedef struct {
    v3 origin, dir;
    float len;   /* sl_length(dir): the cast's own length of dir (1 for the vertical casts) */
    float max_t;
    int slot;    /* the hit slot a hit fills (>= 0), CH_SLOT_NONE or CH_SLOT_FLOOR */
} ch_request;

typedef struct {
    sl_state sl;      /* the slide in progress (MOVE's, then the lifted one's); at the end p and m are the answer */
    v3 pos;           /* where the query began */
    v3 p_move, m_move; /* MOVE's result while the lifted slide runs */
    float lift, L;    /* how far the step lifted; the length of the cast in flight */
    float skin, step_height, snap_distance, min_floor_ny;
    uint32_t max_slides, k; /* k: casts made by the slide in progress */
    uint32_t phase, walking, ended, floor_found;
    uint32_t status;  /* MOVE's from the end of MOVE on, the answer at the end */
} ch_state;

/* sl_valid's rule: the call's own values are checked by the entry point */
PHYS_HD int ch_valid(v3 pos, v3 motion, int has_rot, quat rot, float R, float h) { return sl_valid(pos, motion, has_rot, rot, R, h); }

PHYS_HD void ch_begin(ch_state* s, v3 pos, v3 motion, uint32_t grounded_in, float skin, uint32_t max_slides, float step_height,
                      float snap_distance, float min_floor_ny) {
    sl_begin(&s->sl, pos, motion);
    s->pos = pos;
    s->p_move = pos; s->m_move = motion;
    s->lift = 0.0f; s->L = 0.0f;
    s->skin = skin; s->step_height = step_height; s->snap_distance = snap_distance; s->min_floor_ny = min_floor_ny;
    s->max_slides = max_slides; s->k = 0u;
    s->phase = CH_MOVE;
    s->walking = (grounded_in != 0u && !(motion.y > 0.0f)) ? 1u : 0u;
    s->ended = 0u; s->floor_found = 0u;
    s->status = 0u;
}

PHYS_HD int ch_floor_found(const ch_state* s) { return s->floor_found != 0u; }

/* the next cast of the slide in progress, or 0 when it is over (sl_ran_out applied where the casts ran out) */
PHYS_HD int ch_slide_cast(ch_state* s, ch_request* r, uint32_t first_slot) {
    if (s->ended) return 0;
    if (s->k >= s->max_slides) { sl_ran_out(&s->sl); return 0; }
    const float L = sl_length(s->sl.m);
    if (!(L > 0.0f)) return 0;
    s->L = L;
    r->origin = s->sl.p; r->dir = s->sl.m; r->len = L; r->max_t = sl_max_t(L, s->skin);
    r->slot = (int)(first_slot + s->k);
    return 1;
}

/* the answer of a slide's cast: slide.h's step, the classes of the normal, and the no-climb rule */
PHYS_HD void ch_slide_answer(ch_state* s, int miss, float t, v3 n) {
    if (miss) { sl_miss(&s->sl); s->ended = 1u; return; }
    const int go = sl_hit(&s->sl, s->L, s->skin, t, n);
    s->k += 1u;
    if (!go) { s->ended = 1u; return; }
    if (!(n.y >= s->min_floor_ny)) s->sl.status |= CH_HIT_WALL;
    if (n.y < 0.0f && s->sl.m0.y > 0.0f) s->sl.status |= CH_HIT_CEILING;
    if (s->walking && n.y > 0.0f && n.y < s->min_floor_ny && s->sl.m.y > 0.0f) {
        const v3 nh = v3_make(n.x, 0.0f, n.z);
        const float nn = v3_dot(nh, nh);
        v3 h = v3_make(s->sl.m.x, 0.0f, s->sl.m.z);
        h = nn > SL_PARALLEL ? v3_sub(h, v3_scale(nh, v3_dot(h, nh) / nn)) : v3_make(0.0f, 0.0f, 0.0f);
        if (!(v3_dot(h, s->sl.m0) > 0.0f)) h = v3_make(0.0f, 0.0f, 0.0f);
        s->sl.m = h;
    }
}

PHYS_HD void ch_vertical(ch_request* r, v3 origin, float dy, float max_t, int slot) {
    r->origin = origin; r->dir = v3_make(0.0f, dy, 0.0f); r->len = 1.0f; r->max_t = max_t; r->slot = slot;
}

/* the step is given up: MOVE's result stands, the lifted slide's casts stay counted */
PHYS_HD void ch_abandon(ch_state* s) {
    s->status |= (s->sl.status & SL_HITS_MASK) << CH_HITS_SHIFT;
    s->sl.p = s->p_move; s->sl.m = s->m_move;
    s->phase = CH_GROUND;
}

/* the next cast to make: 1 and *r, or 0 when the query is done */
PHYS_HD int ch_next(ch_state* s, ch_request* r) {
    if (s->phase == CH_MOVE) {
        if (ch_slide_cast(s, r, 0u)) return 1;
        s->status = s->sl.status;
        const int has_l = s->sl.m0.x != 0.0f || s->sl.m0.z != 0.0f;
        if (s->status & CH_BLOCKED) s->phase = CH_DONE;
        else if (s->walking && s->step_height > 0.0f && has_l && (s->status & CH_HIT_WALL)) s->phase = CH_UP;
        else s->phase = CH_GROUND;
    }
    if (s->phase == CH_UP) {
        ch_vertical(r, s->pos, 1.0f, s->step_height + s->skin, CH_SLOT_NONE);
        return 1;
    }
    if (s->phase == CH_LIFTED) {
        if (ch_slide_cast(s, r, s->max_slides)) return 1;
        if (s->sl.status & CH_BLOCKED) ch_abandon(s);
        else s->phase = CH_DOWN;
    }
    if (s->phase == CH_DOWN) {
        ch_vertical(r, s->sl.p, -1.0f, s->lift + 2.0f * s->skin, CH_SLOT_FLOOR);
        return 1;
    }
    if (s->phase == CH_GROUND) {
        const float reach = 2.0f * s->skin + (s->walking ? s->snap_distance : 0.0f);
        if (reach > 0.0f) { ch_vertical(r, s->sl.p, -1.0f, reach, CH_SLOT_FLOOR); return 1; }
        s->phase = CH_DONE;
    }
    return 0;
}

/* the answer of the cast ch_next asked for: id (CH_MISS: nothing was met), t, the normal n and the touched point */
PHYS_HD void ch_answer(ch_state* s, uint32_t id, float t, v3 n, v3 point) {
    const int miss = id == CH_MISS;
    (void)point; /* the driver stores it with the slot or the floor */
    if (s->phase == CH_MOVE || s->phase == CH_LIFTED) {
        ch_slide_answer(s, miss, t, n);
    } else if (s->phase == CH_UP) {
        float lift = s->step_height;
        if (!miss) {
            lift = t - s->skin;
            lift = lift > 0.0f ? lift : 0.0f;
            lift = lift < s->step_height ? lift : s->step_height;
        }
        if ((!miss && t == 0.0f) || !(lift > 0.0f)) { s->phase = CH_GROUND; return; }
        s->lift = lift;
        s->p_move = s->sl.p; s->m_move = s->sl.m;
        const v3 l = v3_make(s->sl.m0.x, 0.0f, s->sl.m0.z);
        sl_begin(&s->sl, v3_make(s->pos.x, s->pos.y + lift, s->pos.z), l);
        s->k = 0u; s->ended = 0u;
        s->phase = CH_LIFTED;
    } else if (s->phase == CH_DOWN) {
        const v3 l = s->sl.m0; /* horizontal: the lifted slide's own motion */
        const int further = v3_dot(v3_sub(s->sl.p, s->pos), l) > v3_dot(v3_sub(s->p_move, s->pos), l);
        if (!miss && t > 0.0f && n.y >= s->min_floor_ny && further) {
            float a = t - s->skin;
            a = a > 0.0f ? a : 0.0f;
            s->sl.p.y = s->sl.p.y - a;
            s->status = (s->status & SL_HITS_MASK) | ((s->sl.status & SL_HITS_MASK) << CH_HITS_SHIFT) |
                        (s->sl.status & (CH_EXHAUSTED | CH_HIT_WALL)) | CH_STEPPED | CH_GROUNDED;
            s->floor_found = 1u;
            s->phase = CH_DONE;
        } else {
            ch_abandon(s);
        }
    } else if (s->phase == CH_GROUND) {
        if (!miss && t > 0.0f) {
            if (n.y >= s->min_floor_ny) {
                s->status |= CH_GROUNDED;
                s->floor_found = 1u;
                if (s->walking && t > 2.0f * s->skin) { s->sl.p.y = s->sl.p.y - (t - s->skin); s->status |= CH_SNAPPED; }
            } else if (n.y > 0.0f) {
                s->status |= CH_ON_STEEP;
                s->floor_found = 1u;
            }
        }
        s->phase = CH_DONE;
    }
}

#endif /* PHYS_SPEC_CHARACTER_H */
