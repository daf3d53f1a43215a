"""GPU: every path of the colouring stage (coloring.hip) and both row sorts, read out manifold by manifold through the probe
library (tests/cpp/color_probe.hip) and held to tests/color_ref.py's checker after EVERY update: the colour of every
manifold equals the numpy restatement's, kept colours stay, no colour class shares a body, row_src is a permutation laid
out exactly by color_start (or by the cluster sort's segment table), the counts, n_colors, color_rounds, n_new_manifolds
and the `used` words are exact, and no update raises an overflow bit (but the one that tests the 64-colour cap).

The scenes (tests/color_cases.py) are built for the branches; each test asserts from the read-out and from the ColorPlan
of the update - plan.hpp's plan_coloring evaluated on the world immediately before it - that its branch was reached, so a
scene that misses fails. Every update prints its path, M, new manifolds, rounds and sort_blocks.

Two conditions of the case table cannot be met and are stated instead (tests/test_color_ref_cpu.py holds both to plan.hpp):
  - an update without new manifolds has 0 rounds and one with a single new manifold has 1, by definition; `rounds >= 3` is
    asserted wherever hundreds of manifolds are new;
  - sort_blocks of 1 and 2 are planned only from hints of at most 6553 manifolds, and every valid hint up to 40 960 selects
    k_color_small, which sorts by itself: k_color_hist / k_color_offsets / k_color_place never run with fewer than 16
    workgroups. They are checked here with 16, 256 and 512."""
import time

import numpy as np
import pytest

import color_cases as cc
import color_probe as cp
import color_ref as cf

pytestmark = pytest.mark.gpu
SMALL_LIMIT = 40 * 1024   # plan.hpp kSmallTrips * kColorThreads
SMALL_LIST = 6144         # coloring.hip kSmallList
STAGE = 8192              # coloring.hip kColorStage


def make_world(scene, flags=0):
    import physics_amd
    ground = physics_amd.FLAG_GROUND_PLANE if scene.ground else 0
    w = physics_amd.World(physics_amd.default_config(flags=physics_amd.FLAG_COLLISIONS | ground | flags, gravity_force=(0, 0, 0),
                                                     gravity_offset=(0, 0, 0)))
    w.set_bodies(**scene.bodies())
    return w


class Run:
    """A world stepped one update at a time: sync, the plan of the next update, the update, sync, read-out, checker."""

    def __init__(self, name, scene, flags=0):
        self.name, self.scene, self.w = name, scene, make_world(scene, flags)
        self.prev, self.log, self.t0 = None, [], time.time()

    def set_statics(self, name):
        self.w.set_static_bodies(**self.scene.statics[name])

    def update(self, expect_overflow=0):
        w = self.w
        if not expect_overflow:
            w.sync()
        plan = cp.next_plan(w)
        # rows by (owner cluster, colour) instead of by colour: the plan's word (static clusters: nobody else has a say)
        cluster = plan.wants_cluster
        assert not (cluster and cp.sizes(w).cluster_dynamic)
        w.update(cc.DT_NANOS)
        if expect_overflow:
            import physics_amd
            with pytest.raises(physics_amd.PhysError) as err:
                w.sync()
            from physics_amd import _abi
            assert err.value.code == _abi.PHYS_ERR_CAPACITY, err.value
        else:
            w.sync()
        out = cp.read(w, cluster=cluster)
        u = len(self.log)
        print(f"\n{self.name} update {u}: path {plan.path}{'+full' if plan.full else ''}{'+rebuild' if plan.rebuild and not plan.full else ''}"
              f"{'+cluster' if cluster else ''}, M {out.M}, new {out.n_new_manifolds}, rounds {out.color_rounds} (launched {plan.rounds}), "
              f"round_blocks {plan.round_blocks}, sort_blocks {plan.sort_blocks}, colours {out.n_colors}", end="")
        try:
            # (a full re-colouring keeps nothing: the colours are a function of this update's manifold set alone)
            self.prev, ref = cf.check_update(out, None if plan.full else self.prev, cluster=cluster, expect_overflow=expect_overflow)
        except cf.CheckFailed as e:
            raise AssertionError(f"{self.name}, update {u} ({plan.path}): {e}") from None
        self.log.append((plan, out, ref))
        return plan, out

    def close(self):
        print(f"\n{self.name}: {len(self.log)} updates checked in {time.time() - self.t0:.2f} s")
        self.w.close()


def relisted(out, prev):
    """k_color_small starts without a list (more than kSmallList uncoloured) and builds one after a later round."""
    sizes = cf.round_sizes(out.man_a, out.man_b, out.n_bodies, prev)
    return sizes[0] > SMALL_LIST and any(0 < s <= SMALL_LIST for s in sizes[1:])


# ---------------------------------------------------------------- 1. Probe: the first update
@pytest.mark.parametrize("M", [1, 1023, 1024, 1025])
def test_probe_path_around_one_workgroup_trip(M):
    run = Run(f"probe M={M}", cc.exact(M))
    plan, out = run.update()
    assert (plan.path, plan.full, plan.rebuild, plan.sort_blocks, plan.hint_valid) == ("Probe", True, True, 512, False)
    assert out.M == M and out.n_new_manifolds == M
    assert out.color_rounds >= 3 or M == 1
    plan, out = run.update()
    assert (plan.path, plan.full, out.M, out.n_new_manifolds, out.color_rounds) == ("Small", False, M, 0, 0)
    run.close()


def test_probe_path_asks_the_device_twice():
    """About 20 000 manifolds and more than 8 rounds: the eight-launches-and-ask loop goes round twice."""
    sc = cc.probe_20k()
    run = Run("probe 20k", sc)
    plan, out = run.update()
    assert plan.path == "Probe" and plan.round_blocks > 1
    assert out.M == sc.expect_M and 19_000 < out.M < 21_000
    assert out.color_rounds > 8
    run.close()


# ---------------------------------------------------------------- 2. Small, incremental
def test_small_path_incremental():
    """k_color_small with nothing new, one new manifold, a few hundred (a list that fits from the start, several rounds)
    and more than kSmallList new ones (no list at first, the re-listing after a later round)."""
    run = Run("small incremental", cc.small_incremental())
    run.update()
    for u in range(1, 7):
        before = run.prev
        plan, out = run.update()
        assert (plan.path, plan.full) == ("Small", False) and out.M <= SMALL_LIMIT
        if u in (1, 4, 6):
            assert (out.n_new_manifolds, out.color_rounds) == (0, 0), u
        if u == 2:
            assert (out.n_new_manifolds, out.color_rounds) == (1, 1)
        if u == 3:
            assert 100 <= out.n_new_manifolds <= 999 and out.color_rounds >= 3
        if u == 5:
            assert out.n_new_manifolds > SMALL_LIST and out.color_rounds >= 3
            assert relisted(out, before)
    run.close()


# ---------------------------------------------------------------- 2b / 3. Small with a full re-colouring
@pytest.mark.parametrize("M", cc.SMALL_FULL_SIZES)
def test_small_path_full_recolouring(M):
    """phys_set_static_bodies clears the colour table and leaves the hint: k_color_small colours all M manifolds. M below
    1024, on both sides of a multiple of 1024 and on it; just above kSmallList (the scan of all manifolds, then the list);
    near the 40 960 the registers hold."""
    run = Run(f"small full M={M}", cc.small_full(M))
    run.update()
    plan, out = run.update()
    assert (plan.path, plan.full, out.M, out.n_new_manifolds) == ("Small", False, M, 0)
    run.set_statics("far")
    plan, out = run.update()
    assert (plan.path, plan.full, plan.rebuild, plan.hint_valid, plan.hint_n_manifolds) == ("Small", True, True, True, M)
    assert out.M == M and out.n_new_manifolds == M and out.color_rounds >= 3
    assert relisted(out, None) == (M > SMALL_LIST)
    plan, out = run.update()
    assert (plan.path, plan.full, out.n_new_manifolds) == ("Small", False, 0)
    run.close()


# ---------------------------------------------------------------- 4. Small chosen, more manifolds than its registers hold
def test_small_path_beyond_its_registers():
    """The hint says 36 480 manifolds, the update stores more than 50 000: in_regs is false and every pass of
    k_color_small takes the strided loops, the counting sort's atomic loads of man_color included."""
    run = Run("small beyond 40960", cc.beyond_registers())
    run.update()
    run.update()
    before = run.prev
    plan, out = run.update()
    assert (plan.path, plan.full) == ("Small", False) and plan.hint_n_manifolds <= SMALL_LIMIT
    assert 50_000 <= out.M <= 60_000 and out.n_new_manifolds > SMALL_LIST and out.color_rounds >= 3
    assert relisted(out, before)
    plan, out = run.update()
    assert plan.path == "Known"
    run.close()


# ---------------------------------------------------------------- 5. Known, incremental
def test_known_path_incremental():
    """Just above 40 960 manifolds, 66 updates: round launches over-hinted (surplus launches exit), exact, and under-hinted
    after nine quiet updates (k_color_finish runs every round itself); the table rebuild of the 65th update and the update
    behind it; the colour sort with 16 workgroups and 64 colours (a hub with 64 partners)."""
    run = Run("known incremental", cc.known_incremental())
    plan, out = run.update()
    assert plan.path == "Probe" and out.n_colors == 64
    for u in range(1, 66):
        plan, out = run.update()
        assert (plan.path, plan.full, plan.sort_blocks) == ("Known", False, 16), u
        assert SMALL_LIMIT < out.M < SMALL_LIMIT + 8192 and out.n_colors == 64, u
        assert plan.rebuild == (u == 64), u
        if u == 2:
            assert (out.n_new_manifolds, out.color_rounds, plan.rounds) == (1, 1, 0)
        if u == 3:  # quiet and over-hinted
            assert out.n_new_manifolds == 0 and out.color_rounds == 0 and plan.rounds >= 1
        if u == 4:  # exact
            assert out.n_new_manifolds == 1 and out.color_rounds == plan.rounds == 1
        if 5 <= u <= 13:
            assert out.n_new_manifolds == 0, u
        if u == 14:  # the burst behind nine quiet updates: nothing launched, k_color_finish runs the rounds
            assert plan.rounds == 0 and out.n_new_manifolds >= 1000 and out.color_rounds >= 3
        if u == 15:  # surplus launches
            assert plan.rounds >= 3 and plan.rounds > out.color_rounds
        if u in (64, 65):
            assert out.n_new_manifolds >= 100 and out.color_rounds >= 3, u
    run.close()


# ---------------------------------------------------------------- 6. Known with a full re-colouring
def test_known_path_full_recolouring():
    """phys_set_static_bodies on the Known path: the round launches come from hint.full_rounds. Once with the manifold set
    of the first update (the count is exact), once with another set - movers have landed and a static slab touches a face -
    so that k_color_finish has rounds left to run."""
    sc = cc.known_full()
    run = Run("known full", sc)
    plan, first = run.update()
    run.update()
    run.set_statics("far")
    plan, out = run.update()
    assert (plan.path, plan.full, plan.rebuild) == ("Known", True, True)
    assert plan.rounds == plan.hint_full_rounds == first.color_rounds == out.color_rounds and out.color_rounds >= 3
    assert out.n_new_manifolds == out.M == first.M
    plan, out = run.update()
    assert (plan.path, plan.full) == ("Known", False) and out.n_new_manifolds >= 1000
    run.set_statics("slab")
    plan, out = run.update()
    assert (plan.path, plan.full) == ("Known", True) and plan.rounds == first.color_rounds
    static = ((out.man_b & cc.STATIC_ID_BIT) != 0) & (out.man_b != cc.GROUND)
    assert static.sum() == sc.slab_manifolds and out.n_new_manifolds == out.M
    assert out.color_rounds != plan.rounds
    run.close()


# ---------------------------------------------------------------- 7. the stage of k_color_round overflows
def test_round_kernel_stage_overflow():
    """A world of 43 680 manifolds gains 546 000 in one update, with round launches sized for the 43 680: the losers of round 0
    outnumber round_blocks x kColorStage, so SOME workgroup has more than its stage holds (whatever the order of the list)
    and appends the surplus directly. The update behind it sorts with 256 workgroups (PHYS_FLAG_SOLVER_PER_COLOR: without
    it that update, of 200 000 bodies and 590 000 manifolds, would take the cluster sort)."""
    import physics_amd
    run = Run("stage overflow", cc.stage_overflow(), flags=physics_amd.FLAG_SOLVER_PER_COLOR)
    for u in range(4):
        run.update()
    before = run.prev
    plan, out = run.update()
    assert (plan.path, plan.full) == ("Known", False) and plan.rounds >= 1
    assert plan.round_blocks == (plan.hint_n_manifolds * 5 // 4 + 1024) // 1024 and plan.hint_n_manifolds < 50_000
    sizes = cf.round_sizes(out.man_a, out.man_b, out.n_bodies, before)
    print(f"\n  round sizes {sizes[:4]}..., stage room {plan.round_blocks} x {STAGE} = {plan.round_blocks * STAGE}", end="")
    assert out.n_new_manifolds == sizes[0] >= 10 * plan.hint_n_manifolds
    assert sizes[1] > plan.round_blocks * STAGE, "the losers of round 0 fit the stages: no workgroup must overflow"
    assert out.color_rounds > plan.rounds + 3
    plan, out = run.update()
    assert (plan.path, plan.sort_blocks, plan.wants_cluster) == ("Known", 256, False)
    run.close()


# ---------------------------------------------------------------- 8. 64 colours and the cap
def test_hub_of_64_partners_uses_every_colour():
    sc = cc.hub_scene(64)
    hub = sc.hub_id
    run = Run("hub 64", sc)
    plan, out = run.update()
    assert (plan.path, plan.sort_blocks) == ("Probe", 512)
    at_hub = (out.man_a == hub[0]) | (out.man_b == hub[0])
    assert at_hub.sum() == 64 and sorted(out.man_color[at_hub]) == list(range(64)) and out.n_colors == 64
    run.update()
    run.close()


def test_hub_of_65_partners_reports_the_cap():
    """The one case with an overflow bit: 65 manifolds at one body. Two of them share colour 63, the update raises bit 2 and
    phys_sync answers PHYS_ERR_CAPACITY; everything else - the sort included - is still held to the checker."""
    sc = cc.hub_scene(65)
    hub = sc.hub_id
    run = Run("hub 65", sc)
    plan, out = run.update(expect_overflow=cf.OVF_COLORS)
    at_hub = (out.man_a == hub[0]) | (out.man_b == hub[0])
    assert at_hub.sum() == 65 and np.bincount(out.man_color[at_hub], minlength=64).tolist() == [1] * 63 + [2]
    run.close()


# ---------------------------------------------------------------- 9. the cluster sort
def test_cluster_sort_rows():
    """32 768 bodies is the least that gets clusters (plan.hpp kClusterMinBodies); a 32^3 lattice has 95 232 manifolds, beyond
    the Small path, and PHYS_FLAG_SOLVER_CLUSTER makes wants_cluster true from the second update on. Rows by (owner cluster,
    colour) over three such updates, the second with new manifolds."""
    import physics_amd
    sc = cc.cluster_scene()
    run = Run("cluster sort", sc, flags=physics_amd.FLAG_SOLVER_CLUSTER)
    sz = cp.sizes(run.w)
    assert sz.cluster_count > 0 and not sz.cluster_dynamic and sz.n_owned == 32768 + 100
    plan, out = run.update()
    assert plan.path == "Probe" and not plan.wants_cluster and out.M == sc.expect_M
    for u in (1, 2, 3):
        plan = cp.next_plan(run.w)
        assert plan.wants_cluster and plan.path == "Known", u
        run.w.profile_enable(True)
        plan, out = run.update()
        assert "solve_cluster" in run.w.profile_get()[0], u
        assert (out.n_new_manifolds >= 300) == (u == 2), (u, out.n_new_manifolds)
        owners = cf.row_owner(out.man_a, out.man_b, out.cluster_slot, out.cluster_slots, out.cluster_count)
        assert len(np.unique(owners)) > 100  # the rows are spread over the clusters
    run.close()
