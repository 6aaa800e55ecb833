"""Colour cameras of the general-tree engine on the MI355X (so101_tree_render_color, include/so101.h) against the fp64 reference of
tests/shade_ref.py on tests/tree_raycast_ref.py, on the HandOverBanana scene (32-dof build) and the Dining scene (64-dof build).  The
acceptance per image is that of tests/test_shade_gpu.py (shade_ref.assert_image)."""
import numpy as np
import pytest

from so101_sim_amd import appearance
from tests import shade_cases as sc
from tests import tree_render_cases as tc
from tests.simharness import TreeArraySim

pytestmark = pytest.mark.gpu
BACKEND = "gpu"
# (teleoperator_pov - an exact depth tie between the table and its legs - and worms_eye_cam - more than 4 % ambiguous - are no test views)
FIVE = ["overhead_cam", "collaborator_pov", "wrist_cam_left", "wrist_cam_right", tc.FINGER_CAM]
ACTION = np.array([0.3, -0.6, 0.9, 0.2, -0.1, 0.3, 0.5, -0.3, -0.7, 1.0, -0.2, 0.1, -0.3, 0.8], dtype=np.float32)
SHADING = appearance.ALOHA_SHADING


def _sim(scene, n):
    sim = TreeArraySim(tc.blobs(scene)["f32"], n, backend=BACKEND)
    sim.sim.set_hull_planes(*tc.planes(scene))
    return sim


def _colors(scene):
    return appearance.aloha_colors(tc.blobs(scene)["meta"])


def test_three_states_five_cameras_on_the_32_dof_build():
    sim = _sim("banana", 3)
    assert sim.sim.build == 32
    sim.set_state(np.stack([tc.STATES[s] for s in tc.STATE_NAMES], axis=1))
    cams, colors = tc.cams_of("banana", FIVE), _colors("banana")
    out = sc.render_color(sim, cams, 48, 64, colors, SHADING)
    depth, seg = tc.render(sim, cams, 48, 64)
    assert np.array_equal(sc.bits(out["depth"]), sc.bits(depth)) and np.array_equal(out["seg"], seg)
    worst = max(sc.check(tc.reference("banana"), "tree_banana", out, e, tc.STATES[s], cams, colors, SHADING, s)[0] for e, s in enumerate(tc.STATE_NAMES))
    print(f"worst |n - n64|_inf over the 15 images: {worst:.3e}")
    # rgb alone (depth and seg from the handle's scratch) and per-env colours with an env index
    alone = sc.render_color(sim, cams, 48, 64, colors, SHADING, want=("rgb",))
    assert np.array_equal(alone["rgb"], out["rgb"])
    per_env = np.stack([colors, 1.0 - colors, 0.5 * colors])
    sub = sc.render_color(sim, cams[:2], 48, 64, per_env, SHADING, env_index=[2, 0], per_env=True)
    sc.check(tc.reference("banana"), "tree_banana", sub, 0, tc.STATES[tc.STATE_NAMES[2]], cams[:2], per_env[2], SHADING, "colours of env 2")
    assert np.array_equal(sub["rgb"][1], out["rgb"][0, :2]) and np.array_equal(sc.bits(sub["normal"]), sc.bits(out["normal"][[2, 0], :2]))


def test_dining_scene_on_the_64_dof_build():
    sim = _sim("dining", 1)
    assert sim.sim.build == 64
    sim.set_state(tc.DINING_STATE[:, None])
    cams, colors = tc.cams_of("dining", ["overhead_cam", "wrist_cam_left"]), _colors("dining")
    out = sc.render_color(sim, cams, 48, 64, colors, SHADING)
    worst, _ = sc.check(tc.reference("dining"), "tree_dining", out, 0, tc.DINING_STATE, cams, colors, SHADING, "dining")
    print(f"worst |n - n64|_inf over the 2 images: {worst:.3e}")


def test_delayed_source_and_state_untouched():
    """source 1 shades the delayed physics-state line; a colour render between two steps changes nothing the next step reads or writes"""
    q0 = np.stack([tc.STATES["home"], tc.STATES["bent"]], axis=1)
    act = np.stack([ACTION, -ACTION])
    cams, colors = tc.cams_of("banana", ["overhead_cam", "wrist_cam_left"]), _colors("banana")

    def run(with_render):
        sim = _sim("banana", 2)
        sim.enable_env(physics_state=True, physics_delay_steps=2, n_substeps=2, settle_max_substeps=0)
        nv, nu = sim.sim.nv, sim.sim.nu
        sim.set_state(q0, np.zeros((nv, 2)), np.zeros((nu, 2)), np.zeros((nv, 2)))
        sim.begin_episode()
        for _ in range(3):
            sim.step(act)
        out = None
        if with_render:
            delayed = sim._get(sim.delayed_physics_state)[:, :sim.sim.nq]
            out = delayed, sc.render_color(sim, cams, 48, 64, colors, SHADING, source=1), sc.render_color(sim, cams, 48, 64, colors, SHADING, source=0)
        sim.step(act)
        return out, [sim._get(x) for x in (sim.qpos, sim.qvel, sim.warm, sim.ctrl, sim.obs, sim.reward_, sim.discount, sim.step_type,
                                           sim.physics_state, sim.delayed_physics_state, sim.ps_ring, sim.ring_pos, sim.ring_vel, sim.step_count)]

    (delayed, late, now), after = run(True)
    _, after_plain = run(False)
    for x, y in zip(after, after_plain):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    b = _sim("banana", 2)
    b.set_state(delayed.T)
    want = sc.render_color(b, cams, 48, 64, colors, SHADING)
    for k in sc.OUTPUTS:
        assert np.array_equal(sc.bits(late[k]), sc.bits(want[k])), k
    assert not np.array_equal(late["rgb"], now["rgb"])
    for e in range(2):
        sc.check(tc.reference("banana"), "tree_banana", late, e, delayed[e].astype(np.float64), cams, colors, SHADING, f"delayed env {e}")


def test_aloha_environment_render_color():
    import torch
    from so101_sim_amd import task_suite
    env = task_suite.create_task_env("HandOverBanana", time_limit=10.0, random_state=7, n_envs=2, settle_max_substeps=100, physics_state=True)
    env.reset()
    img = env.render_color("overhead_cam", 48, 64, normals=True, depth=True, segmentation=True)
    assert img.rgb.shape == (2, 1, 48, 64, 3) and img.rgb.dtype == torch.uint8 and img.normal.shape == (2, 1, 48, 64, 3) and img.normal.dtype == torch.float32
    assert all(t.device == env.qpos.device for t in img)
    depth, seg = env.render_depth("overhead_cam", 48, 64)
    assert torch.equal(img.depth.view(torch.int32), depth.view(torch.int32)) and torch.equal(img.seg, seg)
    plain = env.render_color("overhead_cam", 48, 64)
    assert plain.normal is None and plain.depth is None and plain.seg is None and torch.equal(plain.rgb, img.rgb)
    group = env.geom_group("left_gripper")
    over = env.render_color("overhead_cam", 48, 64, colors={"left_gripper": (1.0, 0.0, 1.0)}).rgb
    hit = torch.isin(seg, torch.as_tensor(list(group.geoms), dtype=torch.int32, device=seg.device))
    assert hit.any() and torch.equal(over[~hit], img.rgb[~hit]) and torch.all(over[hit][:, 1] == 0)
    late = env.render_color(["overhead_cam", "wrist_cam_left"], 48, 64, env_ids=[1, 0], delayed=True)
    assert late.rgb.shape == (2, 2, 48, 64, 3) and torch.equal(late.rgb[:, 0], img.rgb[[1, 0], 0])          # right after a reset the line holds the reset state
    with pytest.raises(ValueError):
        env.render_color("no_such_cam", 8, 8)
    env.close()
    bare = task_suite.create_task_env("HandOverBanana", time_limit=10.0, random_state=7, n_envs=2, settle_max_substeps=100)
    bare.reset()
    with pytest.raises(ValueError, match="physics_state"):
        bare.render_color("overhead_cam", 8, 8, delayed=True)
    bare.close()
