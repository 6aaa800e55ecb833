"""Proximity sensing of the general-tree engine on the MI355X (so101_tree_proximity, include/so101.h; AlohaEnvironment.proximity) against the
fp64 reference of tests/tree_proximity_ref.py (separated pairs: distance, winner, an algorithm-free certificate on the kernel's witnesses) and
against so101_tree_contacts at the same states (penetrating pairs: the same bits), for both builds of the engine: three hand-over states as one
batch (32-dof build), the settled Dining state (64-dof build).  States, pairs, launches and checks: tests/tree_proximity_cases.py, shared with
tests/test_tree_proximity_emu.py."""
import numpy as np
import pytest

from tests import proximity_cases as px, tree_contact_cases as tc, tree_proximity_cases as tp
from tests.simharness import TreeArraySim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    """ONE pass of every launch the tests below read, and the fp64 side (cached per session)"""
    sim = TreeArraySim(tp.blobs("handover")["f32"], 3, backend="gpu")
    res = tp.run_handover(sim)
    dsim = TreeArraySim(tp.blobs("dining")["f32"], 1, backend="gpu")
    assert (sim.sim.build, dsim.sim.build) == (32, 64)
    return dict(sim=sim, res=res, ref=tp.reference("handover", res["way_adr"]), dining=tp.run_dining(dsim, 3), dref=tp.reference("dining"))


def test_separated_results_match_the_fp64_reference(gpu):
    tp.check_handover_separated(gpu["res"], gpu["ref"])


def test_the_reference_passes_its_own_certificate(gpu):
    tp.check_reference(gpu["ref"], ("group", "big", "single", "way"))
    tp.check_reference(gpu["dref"], ("group",))


def test_penetrating_results_are_the_contact_reports(gpu):
    res = gpu["res"]
    assert tp.check_penetrating(res["group"], res["touch"], res["group_masks"], 3) >= 4


def test_own_q_permutation_swap_and_untouched_state(gpu):
    tp.check_invariants(gpu["res"])


def test_q_moves_what_it_names_and_nothing_else(gpu):
    tp.check_waypoints(gpu["res"], gpu["ref"])


def test_a_group_is_the_minimum_of_its_members(gpu):
    tp.check_members(gpu["res"])


def test_culling_spares_most_of_arms_props(gpu):
    tp.check_culling(gpu["res"])


def test_beyond_outside_and_nan(gpu):
    px.check_beyond(gpu["res"])
    assert gpu["res"]["beyond"]["flags"][1, 0] == 12


def test_dining_through_the_64_dof_build(gpu):
    d, worst = gpu["dining"], dict(dist=0.0, cert=0.0)
    ns, npn = tp.check_separated(d["group"], gpu["dref"]["group"], gpu["dref"]["ref"], "dining", worst)
    assert (ns, npn) == (2, 1), (ns, npn)                      # grippers | object and object | container apart, the props on the table
    assert tp.check_penetrating(d["group"], d["touch"], d["masks"], 1) == 1
    print(f"dining: worst |dist - reference| {worst['dist']:.3e} m, certificate {worst['cert']:.3e} m")


@pytest.mark.parametrize("kind", ["handover", "dining"])
def test_argument_and_state_errors(kind):
    tp.check_argument_errors(kind, "gpu")


def test_aloha_environment_returns_the_raw_calls_tensors(gpu):
    import torch
    from so101_sim_amd import proximity as pr, task_suite
    res = gpu["res"]
    env = task_suite.create_task_env("HandOverBanana", time_limit=10.0, random_state=3, n_envs=3, prefetch_resets=False)
    Q, V, CT, W = tc.states("handover", tp.HANDOVER_STATES)
    for t, a in zip((env.qpos, env.qvel, env.ctrl, env.warm), (Q, V, CT, W)):
        t.copy_(torch.as_tensor(a, dtype=torch.float32, device=env.device))
    rep = env.proximity(tp.GROUP_SPECS, max_dist=tp.GROUP_MAX_DIST)
    assert isinstance(rep, pr.ProximityReport) and rep.dist.device == env.qpos.device
    assert (rep.dist.shape, rep.geom.shape, rep.point.shape, rep.normal.shape, rep.flags.shape) == ((3, 6), (3, 6, 2), (3, 6, 2, 3), (3, 6, 3), (3, 6))
    assert (rep.dist.dtype, rep.geom.dtype, rep.flags.dtype) == (torch.float32, torch.int32, torch.int32)
    for f in ("dist", "geom", "point", "normal", "flags"):
        assert tp.cc.same_bits(getattr(rep, f).cpu().numpy(), res["group"][f]), f
    # the waypoints by tool name and by the chain's addresses: the raw call's bits both ways
    way = tp.waypoints(Q, res["way_adr"])
    ids = [tp.FREE] * 8
    by_name = env.proximity(tp.WAY_SPECS, env_ids=ids, q=way, joints=tp.WAY_TOOL, max_dist=tp.GROUP_MAX_DIST)
    by_adr = env.proximity(tp.WAY_SPECS, env_ids=ids, q=way, joints=env.tool_chain(tp.WAY_TOOL)[1], max_dist=tp.GROUP_MAX_DIST)
    for f in ("dist", "geom", "point", "normal", "flags"):
        assert torch.equal(getattr(by_name, f), getattr(by_adr, f)), f
        assert tp.cc.same_bits(getattr(by_name, f).cpu().numpy(), res["way"][f]), f
    own = env.proximity(tp.GROUP_SPECS, env_ids=[tp.FREE, 0], q=res["own"][[tp.FREE, 0]], max_dist=tp.GROUP_MAX_DIST)      # joints=None: all 16
    assert tp.cc.same_bits(own.dist.cpu().numpy(), res["group"]["dist"][[tp.FREE, 0]])
    # agreement with touch
    touch = env.touch(tp.GROUP_SPECS)
    assert torch.equal(touch.touching, (rep.flags & 1) != 0)
    assert torch.equal(touch.dist[touch.touching], rep.dist[touch.touching])
    recs = pr.records(rep, 0)
    assert len(recs) == 6 and recs[4].penetrating and recs[4].dist == float(res["group"]["dist"][0, 4]) and recs[4].geom1 == int(res["group"]["geom"][0, 4, 0])
    assert recs[0].found and recs[0].point1.shape == (3,)
    with pytest.raises(ValueError, match="max_dist must be"):
        env.proximity(tp.GROUP_SPECS, max_dist=0.0)
    with pytest.raises(ValueError, match="1 .. 16 pairs"):
        env.proximity([("arms", "table")] * 17)
    with pytest.raises(ValueError, match="unknown geom group"):
        env.proximity([("grippers", "no_such_thing")])
    with pytest.raises(ValueError, match="one row of joint values per entry"):
        env.proximity(tp.GROUP_SPECS, q=np.zeros((2, 6), np.float32), joints=tp.WAY_TOOL)
    env.close()
