"""Depth / segmentation cameras of the general-tree engine on the MI355X (so101_tree_render, include/so101.h) against the fp64 reference of
tests/tree_raycast_ref.py, on the HandOverBanana scene (32-dof build) and the Dining scene (64-dof build).

Acceptance per image (raycast_ref.assert_image): at most 2 % of the pixels are ambiguous (a condition on the view), every other pixel has the
reference's geom id and |z - z64| <= 5e-5 z64, every pixel is well formed."""
import numpy as np
import pytest

from so101_sim_amd import cameras
from tests import raycast_ref as rr
from tests import tree_render_cases as tc
from tests.simharness import TreeArraySim

pytestmark = pytest.mark.gpu
BACKEND = "gpu"
FIVE = ["overhead_cam", "teleoperator_pov", "wrist_cam_left", "wrist_cam_right", tc.FINGER_CAM]
ACTION = np.array([0.3, -0.6, 0.9, 0.2, -0.1, 0.3, 0.5, -0.3, -0.7, 1.0, -0.2, 0.1, -0.3, 0.8], dtype=np.float32)
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _sim(scene, n):
    sim = TreeArraySim(tc.blobs(scene)["f32"], n, backend=BACKEND)
    sim.sim.set_hull_planes(*tc.planes(scene))
    return sim


def test_three_states_five_cameras_on_the_32_dof_build():
    sim = _sim("banana", 3)
    assert sim.sim.build == 32
    sim.set_state(np.stack([tc.STATES[s] for s in tc.STATE_NAMES], axis=1))
    cams = tc.cams_of("banana", FIVE)
    assert cams[-1].body == tc.blobs("banana")["meta"]["body_names"].index("left/left_finger_link")
    depth, seg = tc.render(sim, cams, 48, 64)
    worst = max(tc.check("banana", depth[e], seg[e], tc.STATES[s], cams, s) for e, s in enumerate(tc.STATE_NAMES))
    print(f"worst relative depth error over the 15 images: {worst:.3e}")
    # worms_eye_cam looks along the table's underside: more than 2 % of its pixels are ambiguous, so it is no input for the pixel
    # comparison - its image only has to be well formed
    worm = tc.cams_of("banana", ["worms_eye_cam"])
    d, s = tc.render(sim, worm, 48, 64)
    assert np.all((s >= -1) & (s < sim.sim.ngeom)) and np.array_equal(s == -1, np.isposinf(d)) and not np.any(np.isnan(d)) and np.all(d > 0)
    assert np.isfinite(d).any()


@pytest.mark.parametrize("size", [(30, 44), (1, 1)])
def test_ragged_sizes(size):
    sim = _sim("banana", 1)
    sim.set_state(tc.STATES["bent"][:, None])
    cams = tc.cams_of("banana", tc.RAGGED_CAMS)
    depth, seg = tc.render(sim, cams, *size)
    tc.check("banana", depth[0], seg[0], tc.STATES["bent"], cams, "bent")


def test_dining_scene_on_the_64_dof_build():
    sim = _sim("dining", 1)
    assert sim.sim.build == 64
    sim.set_state(tc.DINING_STATE[:, None])
    cams = tc.cams_of("dining", ["overhead_cam", "wrist_cam_left"])
    depth, seg = tc.render(sim, cams, 48, 64)
    tc.check("dining", depth[0], seg[0], tc.DINING_STATE, cams, "dining")
    ref, meta = tc.reference("dining"), tc.blobs("dining")["meta"]
    props = [meta["body_names"].index(n) for n in ("mug", "pen", "banana", "plate", "bowl", "container")]
    seen = {int(ref.gbody[g]) for g in np.unique(seg) if g >= 0}
    assert len(seen & set(props)) >= 4, sorted(seen)


def test_determinism_across_batch_index_and_camera_count():
    q = np.tile(tc.STATES["home"][:, None], (1, 5))
    q[:, 1], q[:, 4] = tc.STATES["bent"], tc.STATES["reach"]
    sim = _sim("banana", 5)
    sim.set_state(q)
    cams = tc.cams_of("banana", FIVE)
    depth, seg = tc.render(sim, cams, 30, 44)
    pick = [4, 1, 1, 0]
    d2, s2 = tc.render(sim, cams, 30, 44, env_index=pick)
    assert np.array_equal(bits(d2), bits(depth[pick])) and np.array_equal(s2, seg[pick])
    for e in (2, 3):
        assert np.array_equal(bits(depth[e]), bits(depth[0])) and np.array_equal(seg[e], seg[0])
    assert not np.array_equal(seg[1], seg[0]) and not np.array_equal(seg[4], seg[0])
    for k, cam in enumerate(cams):
        d1, s1 = tc.render(sim, [cam], 30, 44, env_index=pick)
        assert np.array_equal(bits(d1[:, 0]), bits(depth[pick, k])) and np.array_equal(s1[:, 0], seg[pick, k]), cam.name
    # an index outside [0, n_envs): an all-miss image, the rows beside it untouched by that
    d3, s3 = tc.render(sim, cams, 30, 44, env_index=[5, 0, -1])
    for row in (0, 2):
        assert np.all(np.isposinf(d3[row])) and np.all(s3[row] == -1)
    assert np.array_equal(bits(d3[1]), bits(depth[0])) and np.array_equal(s3[1], seg[0])


def _env_sim(n, q0, **cfg):
    sim = _sim("banana", n)
    sim.enable_env(physics_state=True, physics_delay_steps=2, n_substeps=2, settle_max_substeps=0, **cfg)
    nv, nu = sim.sim.nv, sim.sim.nu
    sim.set_state(q0, np.zeros((nv, n)), np.zeros((nu, n)), np.zeros((nv, n)))
    sim.begin_episode()
    return sim


def test_delayed_source_reads_the_delayed_physics_state_line():
    q0 = np.stack([tc.STATES["home"], tc.STATES["bent"]], axis=1)
    act = np.stack([ACTION, -ACTION])
    cams = tc.cams_of("banana", ["overhead_cam", "wrist_cam_left"])
    a = _env_sim(2, q0)
    for _ in range(3):
        a.step(act)
    delayed = a._get(a.delayed_physics_state)[:, :a.sim.nq]          # [n_envs][nq] float32: the state of two control steps ago
    now = a._get(a.qpos)
    assert not np.array_equal(bits(delayed.T), bits(now))
    d_del, s_del = tc.render(a, cams, 48, 64, source=1)
    d_now, s_now = tc.render(a, cams, 48, 64, source=0)
    b = _sim("banana", 2)
    b.set_state(delayed.T)
    d_b, s_b = tc.render(b, cams, 48, 64)
    assert np.array_equal(bits(d_del), bits(d_b)) and np.array_equal(s_del, s_b)
    assert not np.array_equal(bits(d_del), bits(d_now))
    # the delayed source with an env index
    d1, s1 = tc.render(a, cams, 48, 64, env_index=[1], source=1)
    assert np.array_equal(bits(d1[0]), bits(d_del[1])) and np.array_equal(s1[0], s_del[1])


def test_rendering_between_steps_changes_nothing():
    q0 = np.stack([tc.STATES["home"], tc.STATES["reach"]], axis=1)
    act = np.stack([ACTION, -ACTION])
    cams = tc.cams_of("banana", ["overhead_cam", tc.FINGER_CAM])

    def run(with_render):
        sim = _env_sim(2, q0)
        for _ in range(2):
            sim.step(act)
        if with_render:
            for source in (0, 1):
                depth, _ = tc.render(sim, cams, 30, 44, source=source)
                assert np.isfinite(depth).any()
        out = sim.step(act)
        return [sim._get(x) for x in (sim.qpos, sim.qvel, sim.warm, sim.ctrl, sim.obs, sim.reward_, sim.discount, sim.step_type,
                                      sim.physics_state, sim.delayed_physics_state, sim.ps_ring, sim.ring_pos, sim.ring_vel, sim.step_count)]

    for x, y in zip(run(True), run(False)):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_aloha_environment_render_depth():
    import torch
    from so101_sim_amd import task_suite
    env = task_suite.create_task_env("HandOverBanana", time_limit=10.0, random_state=7, n_envs=2, settle_max_substeps=100, physics_state=True)
    env.reset()
    depth, seg = env.render_depth("overhead_cam", 48, 64)
    assert depth.shape == seg.shape == (2, 1, 48, 64) and depth.dtype == torch.float32 and seg.dtype == torch.int32
    assert depth.device == env.qpos.device and seg.device == env.qpos.device
    d2, s2 = torch.full_like(depth, float("nan")), torch.full_like(seg, -7)
    env.sim.render([cameras.ALOHA_CAMERAS["overhead_cam"].spec()], 48, 64, None, 2, d2.data_ptr(), s2.data_ptr(), env._stream())
    assert torch.equal(depth.view(torch.int32), d2.view(torch.int32)) and torch.equal(seg, s2)
    names = env.meta["geom_names"]
    seen = {names[i] for i in torch.unique(seg).tolist() if i >= 0}
    assert "table" in seen and int(seg.max()) < len(names)
    # a sequence of cameras (a name whose body is resolved, a Camera on a named body), a subset of envs, no segmentation
    d3, s3 = env.render_depth(["overhead_cam", "wrist_cam_left", tc.FINGER_CAM], 48, 64, env_ids=[1, 0], segmentation=False)
    assert s3 is None and d3.shape == (2, 3, 48, 64)
    assert torch.equal(d3[:, 0].view(torch.int32), depth[[1, 0], 0].view(torch.int32))
    left = env.meta["body_names"].index("left/gripper_base")
    d4 = torch.full((2, 1, 48, 64), float("nan"), device=env.device)
    env.sim.render([cameras.ALOHA_CAMERAS["wrist_cam_left"].with_body_ids(env.meta["body_names"]).spec()], 48, 64, None, 2, d4.data_ptr(), None, env._stream())
    assert cameras.ALOHA_CAMERAS["wrist_cam_left"].with_body_ids(env.meta["body_names"]).body == left
    assert torch.equal(d3[:, 1].view(torch.int32), d4[[1, 0], 0].view(torch.int32))
    # delayed: right after a reset the line holds the reset state, two steps later it lags behind
    dd, sd = env.render_depth("overhead_cam", 48, 64, delayed=True)
    assert torch.equal(dd.view(torch.int32), depth.view(torch.int32)) and torch.equal(sd, seg)
    act = torch.as_tensor(np.stack([ACTION, -ACTION]), device=env.device)
    for _ in range(2):
        env.step(act)
    dd, _ = env.render_depth("overhead_cam", 48, 64, delayed=True)
    dn, _ = env.render_depth("overhead_cam", 48, 64)
    assert torch.equal(dd.view(torch.int32), depth.view(torch.int32)) and not torch.equal(dn.view(torch.int32), depth.view(torch.int32))
    with pytest.raises(ValueError):
        env.render_depth("no_such_cam", 8, 8)
    with pytest.raises(ValueError):
        env.render_depth("overhead_cam", 8, 8, env_ids=[2])
    env.close()
    plain = task_suite.create_task_env("HandOverBanana", time_limit=10.0, random_state=7, n_envs=2, settle_max_substeps=100)
    plain.reset()
    with pytest.raises(ValueError, match="physics_state"):
        plain.render_depth("overhead_cam", 8, 8, delayed=True)
    d5, _ = plain.render_depth("overhead_cam", 48, 64)
    assert torch.equal(d5.view(torch.int32), depth.view(torch.int32))          # the same seed: the same reset state
    plain.close()
