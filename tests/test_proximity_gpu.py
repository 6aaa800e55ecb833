"""Proximity sensing on the MI355X: the cases and checks of tests/proximity_cases.py (shared with tests/test_proximity_emu.py) through
libso101_hip.so, and the Python layer of BatchedEnvironment.proximity.  One module-scoped fixture does all launches."""
import numpy as np
import pytest

from so101_sim_amd import proximity as px
from tests import contact_cases as cc, proximity_cases as pc
from tests.simharness import ArraySim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(blobs, golden, hip_lib):
    return pc.run(ArraySim(blobs["f32"], pc.N_ENVS, backend="gpu"), blobs, golden)


@pytest.fixture(scope="module")
def ref(blobs, golden):
    return pc.reference(blobs, golden)


def test_argument_and_state_errors(blobs, hip_lib):
    pc.check_argument_errors(ArraySim(blobs["f32"], 2, backend="gpu"), blobs)


def test_separated_results_against_the_reference_and_the_certificate(gpu, ref):
    pc.check_all_separated(gpu, ref)


def test_penetrating_results_are_what_touch_reports(gpu):
    assert pc.check_penetrating(gpu["rich"], gpu["touch"], gpu["group_masks"], 4) >= 3


def test_own_angles_permutation_swap_and_bound_state(gpu):
    pc.check_invariants(gpu)


def test_a_group_is_the_minimum_of_its_members(gpu):
    pc.check_members(gpu)


def test_beyond_max_dist_and_outside_the_batch(gpu):
    pc.check_beyond(gpu)


def test_python_layer(blobs, golden, gpu, hip_lib):
    import torch
    from so101_sim_amd import task_suite
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=3, n_envs=pc.N_ENVS, prefetch_resets=False)
    try:
        Q, V, A, W = pc.states(golden)
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=env.device)
        env.qpos.copy_(f32(Q)); env.qvel.copy_(f32(V)); env.ctrl.copy_(f32(A)); env.warm.copy_(f32(W))
        before = [t.clone() for t in (env.qpos, env.qvel, env.ctrl, env.warm)]
        rep = env.proximity(pc.GROUP_SPECS, env_ids=[0, 1, 2, 3])
        assert isinstance(rep, px.ProximityReport)
        for f, shape, dt in (("dist", (4, 5), torch.float32), ("geom", (4, 5, 2), torch.int32), ("point", (4, 5, 2, 3), torch.float32),
                             ("normal", (4, 5, 3), torch.float32), ("flags", (4, 5), torch.int32)):
            t = getattr(rep, f)
            assert tuple(t.shape) == shape and t.dtype == dt and t.device == env.qpos.device, f
            assert cc.same_bits(t.cpu().numpy(), gpu["rich"][f]), f              # the raw call's bits
        way = env.proximity(list(pc.GROUP_SPECS[:2]) + [pc.GROUP_SPECS[3]], env_ids=[pc.REST] * 8, q=pc.waypoints())
        assert cc.same_bits(way.dist.cpu().numpy(), gpu["way"]["dist"])
        touch = env.touch(pc.GROUP_SPECS, env_ids=[0, 1, 2, 3])
        pen = (rep.flags & 1) != 0
        assert bool(pen.any()) and torch.equal(pen, touch.touching) and torch.equal(rep.dist[pen], touch.dist[pen])
        recs = px.records(rep, 1)
        assert len(recs) == 5 and any(r.penetrating for r in recs) and all(r.found or r.geom1 == -1 for r in recs)
        for a, b in zip(before, (env.qpos, env.qvel, env.ctrl, env.warm)):
            assert torch.equal(a, b)
        for md in (0.0, -1.0, float("nan"), 11.0):
            with pytest.raises(ValueError, match="max_dist must be"):
                env.proximity([("gripper", "object")], max_dist=md)
        with pytest.raises(ValueError, match="1 .. 16 pairs"):
            env.proximity([("gripper", "object")] * 17)
        with pytest.raises(ValueError, match="unknown geom group"):
            env.proximity([("gripper", "nothing_of_that_name")])
        with pytest.raises(ValueError, match="one row of arm joint angles per entry"):
            env.proximity([("gripper", "object")], env_ids=[0, 1], q=np.zeros((3, 6), dtype=np.float32))
    finally:
        env.close()
