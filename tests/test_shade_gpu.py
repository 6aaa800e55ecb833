"""Colour cameras on the MI355X (so101_render_color, include/so101.h) against the fp64 reference of tests/shade_ref.py.

Acceptance per image (shade_ref.assert_image): depth / seg pass raycast_ref.assert_image and equal so101_render's bits; every hit normal is
unit and faces the camera, every miss has normal 0 and the background bytes; on shading-unambiguous pixels |n - n64|_inf <= TOL_N; every
rgb byte is within 1 of the formula evaluated in fp64 on the kernel's own normal and seg; at most 4 % of the pixels are shading-ambiguous
(a condition on the view)."""
import numpy as np
import pytest

from so101_sim_amd import appearance, cameras
from so101_sim_amd.model import blob as blobfmt
from tests import raycast_ref as rr
from tests import shade_cases as sc
from tests import shade_ref as sr
from tests.render_cases import FIVE_CAMS, JAW_CAM, render, scene_planes
from tests.simharness import ArraySim

pytestmark = pytest.mark.gpu
BACKEND = "gpu"
STATE_NAMES = ("home", "grasp", "tilted")
SHADING = appearance.SO100_SHADING


@pytest.fixture(scope="module")
def ref(blobs):
    return rr.RaycastRef(blobs["f64"])


@pytest.fixture(scope="module")
def colors(blobs):
    return appearance.so100_colors(blobs["meta"])


def _sim(blob_f32, n, **cfg):
    sim = ArraySim(blob_f32, n, backend=BACKEND, **cfg)
    sim.sim.set_hull_planes(*scene_planes(blob_f32))
    return sim


def test_three_states_five_cameras(blobs, ref, colors):
    sim = _sim(blobs["f32"], 3)
    sim.set_state(np.stack([rr.STATES[s] for s in STATE_NAMES], axis=1))
    out = sc.render_color(sim, FIVE_CAMS, 48, 64, colors, SHADING)
    depth, seg = render(sim, FIVE_CAMS, 48, 64)
    assert np.array_equal(sc.bits(out["depth"]), sc.bits(depth)) and np.array_equal(out["seg"], seg)
    worst, counts = 0.0, np.zeros(len(sr.FEATURE_NAMES), dtype=np.int64)
    for e, s in enumerate(STATE_NAMES):
        w, c = sc.check(ref, "banana", out, e, rr.STATES[s], FIVE_CAMS, colors, SHADING, s)
        worst, counts = max(worst, w), counts + c
    print(f"worst |n - n64|_inf over the 15 images: {worst:.3e}; unambiguous pixels per feature {dict(zip(sr.FEATURE_NAMES, counts.tolist()))}")
    for f in (sr.F_PLANE, sr.F_BOX, sr.F_HULL, sr.F_CYLINDER_SIDE, sr.F_CYLINDER_CAP, sr.F_CAPSULE_SIDE, sr.F_CAPSULE_END):
        assert counts[f] >= 4, f"the views must show the feature class {sr.FEATURE_NAMES[f]!r}"
    # the wrist camera at the home pose looks past everything: a valid image of background alone
    wrist = [c.name for c in FIVE_CAMS].index("wrist_cam")
    assert np.all(out["seg"][0, wrist] == -1) and not out["normal"][0, wrist].any()
    assert np.all(out["rgb"][0, wrist] == SHADING.background_bytes())


@pytest.mark.parametrize("size", [(30, 44), (1, 1)])
def test_ragged_sizes(blobs, ref, colors, size):
    sim = _sim(blobs["f32"], 1)
    sim.set_state(rr.STATES["tilted"][:, None])
    cams = [cameras.SO100_CAMERAS[n] for n in ("overhead_cam", "front_cam", "side_cam")] + [JAW_CAM]
    out = sc.render_color(sim, cams, *size, colors, SHADING)
    sc.check(ref, "banana", out, 0, rr.STATES["tilted"], cams, colors, SHADING, "tilted")


def _capsule_as_sphere(raw):
    """the blob with its static capsule (the base scene's banana) retyped to a sphere of the capsule's radius"""
    m = blobfmt.unpack(raw)
    real = m["geom_size"].dtype
    t = m["geom_type"].copy()
    g = int(np.flatnonzero(t == rr.CAPSULE)[0])
    assert int(m["geom_body"][g]) not in set(m["arm_body"]) | set(m["free_body"])
    t[g] = rr.SPHERE
    m["geom_type"] = t
    return blobfmt.pack(m, real=real), g


def test_sphere_geom(blobs, colors):
    raw32, g = _capsule_as_sphere(blobs["f32"])
    raw64, g64 = _capsule_as_sphere(blobs["f64"])
    assert g == g64
    sref = rr.RaycastRef(raw64)
    sim = _sim(raw32, 1)
    sim.set_state(rr.STATES["home"][:, None])
    cams = [cameras.SO100_CAMERAS["front_cam"]]
    out = sc.render_color(sim, cams, 48, 64, colors, SHADING)
    worst, counts = sc.check(sref, "banana_sphere", out, 0, rr.STATES["home"], cams, colors, SHADING, "sphere home")
    assert counts[sr.F_SPHERE] >= 4, "the view must show the sphere"


def test_shadings(blobs, ref, colors):
    """no light: rgb = C_g * A; a single headlight; a diffuse sum that clamps: the bytes saturate at 255"""
    sim = _sim(blobs["f32"], 1)
    q = rr.STATES["grasp"]
    sim.set_state(q[:, None])
    cams = [cameras.SO100_CAMERAS["overhead_cam"], cameras.SO100_CAMERAS["front_cam"]]
    out = sc.render_color(sim, cams, 48, 64, colors, sc.NO_LIGHT)
    sc.check(ref, "banana", out, 0, q, cams, colors, sc.NO_LIGHT, "no light")
    flat = sr.to_bytes(colors.astype(np.float64) * np.asarray(sc.NO_LIGHT.ambient))[np.maximum(out["seg"], 0)]
    hit = out["seg"] >= 0
    assert np.abs(out["rgb"][hit].astype(np.int32) - flat[hit].astype(np.int32)).max() <= 1
    head = sc.render_color(sim, cams, 48, 64, colors, sc.HEADLIGHT)
    sc.check(ref, "banana", head, 0, q, cams, colors, sc.HEADLIGHT, "headlight")
    # the table top faces the overhead camera: lit by the headlight it is brighter than its ambient share alone
    table = list(blobs["meta"]["geom_names"]).index("table_surface")
    px = head["seg"][0, 0] == table
    assert px.sum() > 100 and np.all(head["rgb"][0, 0][px][:, 0] > sr.to_bytes(0.8 * 0.1) + 100)
    sat = sc.render_color(sim, cams, 48, 64, colors, sc.SATURATING)
    sc.check(ref, "banana", sat, 0, q, cams, colors, sc.SATURATING, "saturating")
    # the table top under ambient 0.9 + 0.9 + 0.9 cos: 0.4 * 2.67 > 1 in its darkest channel; the background's 1.5 clamps as well
    assert np.all(sat["rgb"][0, 0][px] == 255) and np.array_equal(sc.SATURATING.background_bytes(), [255, 0, 128])
    assert np.array_equal(sc.bits(sat["normal"]), sc.bits(out["normal"])) and np.array_equal(sc.bits(head["normal"]), sc.bits(out["normal"]))


def test_colors_per_env(blobs, ref, colors):
    """3 envs in the same state with different colours per env, env_index = [2, 0]: rows follow the env, not the entry"""
    sim = _sim(blobs["f32"], 3)
    q = rr.STATES["grasp"]
    sim.set_state(np.tile(q[:, None], (1, 3)))
    rng = np.random.RandomState(5)
    per_env = np.stack([colors, rng.uniform(0, 1, colors.shape).astype(np.float32), rng.uniform(0, 1.3, colors.shape).astype(np.float32)])
    cams = [cameras.SO100_CAMERAS["overhead_cam"], JAW_CAM]
    out = sc.render_color(sim, cams, 30, 44, per_env, SHADING, env_index=[2, 0], per_env=True)
    for entry, env in enumerate((2, 0)):
        sc.check(ref, "banana", out, entry, q, cams, per_env[env], SHADING, f"colours of env {env}")
    assert not np.array_equal(out["rgb"][0], out["rgb"][1])
    plain = sc.render_color(sim, cams, 30, 44, colors, SHADING, env_index=[2, 0])
    assert np.array_equal(plain["rgb"][1], out["rgb"][1]) and np.array_equal(plain["rgb"][0], plain["rgb"][1])
    for k in ("normal", "depth", "seg"):
        assert np.array_equal(sc.bits(plain[k]), sc.bits(out[k])), k


def test_determinism_across_batch_index_and_camera_count(blobs, colors):
    N = 130
    q = np.tile(rr.STATES["grasp"][:, None], (1, N))
    q[:, 7], q[:, 129] = rr.STATES["home"], rr.STATES["tilted"]
    sim = _sim(blobs["f32"], N)
    sim.set_state(q)
    want = ("rgb", "normal")
    full = sc.render_color(sim, FIVE_CAMS, 30, 44, colors, SHADING, want=want)
    pick = [129, 7, 0]
    sub = sc.render_color(sim, FIVE_CAMS, 30, 44, colors, SHADING, env_index=pick, want=want)
    same = [e for e in range(N) if e not in (7, 129)]
    assert len(same) == 128
    for k in want:
        assert np.array_equal(sc.bits(sub[k]), sc.bits(full[k][pick])), k
        assert np.all(sc.bits(full[k][same]) == sc.bits(full[k][0])[None]), k
        assert not np.array_equal(sc.bits(full[k][7]), sc.bits(full[k][0])) and not np.array_equal(sc.bits(full[k][129]), sc.bits(full[k][0]))
    for c, cam in enumerate(FIVE_CAMS):
        one = sc.render_color(sim, [cam], 30, 44, colors, SHADING, env_index=pick, want=want)
        for k in want:
            assert np.array_equal(sc.bits(one[k][:, 0]), sc.bits(full[k][pick, c])), (k, cam.name)


def test_render_color_between_steps_changes_nothing(blobs, ref, colors):
    names = ("home", "grasp", "tilted", "grasp")
    q0 = np.stack([rr.STATES[s] for s in names], axis=1)
    act = np.tile(np.array([0.3, -1.2, 1.3, 1.0, -0.5, 0.4], dtype=np.float32), (4, 1))
    cams = [cameras.SO100_CAMERAS["overhead_cam"], JAW_CAM]

    def run(with_render):
        sim = _sim(blobs["f32"], 4, seed=3, last_step=500)
        sim.set_state(q0, np.zeros((18, 4)), np.zeros((6, 4)), np.zeros((18, 4)))
        sim.begin_episode()
        for _ in range(3):
            sim.step(act)
        out = None
        if with_render:
            out = sim.get_state()[0], sc.render_color(sim, cams, 30, 44, colors, SHADING), sc.render_color(sim, cams, 30, 44, colors, SHADING, want=("rgb",))
        sim.step(act)
        return out, [sim._get(a) for a in (sim.qpos, sim.qvel, sim.warm, sim.ctrl, sim.obs)]

    (qpos, out, alone), after = run(True)
    _, after_plain = run(False)
    assert np.array_equal(alone["rgb"], out["rgb"])
    for e in range(4):
        sc.check(ref, "banana", out, e, qpos[:, e], cams, colors, SHADING, f"stepped env {e}")
    for a, b in zip(after, after_plain):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_batched_environment_render_color(blobs):
    import torch
    from so101_sim_amd import task_suite
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=7, n_envs=4, settle_max_substeps=100)
    env.reset_all()
    img = env.render_color("overhead_cam", 48, 64)
    assert isinstance(img, appearance.ColorImages) and img.normal is None and img.depth is None and img.seg is None
    assert img.rgb.shape == (4, 1, 48, 64, 3) and img.rgb.dtype == torch.uint8 and img.rgb.device == env.qpos.device
    full = env.render_color("overhead_cam", 48, 64, normals=True, depth=True, segmentation=True)
    assert full.normal.shape == (4, 1, 48, 64, 3) and full.normal.dtype == torch.float32 and full.normal.device == env.qpos.device
    depth, seg = env.render_depth("overhead_cam", 48, 64)
    assert torch.equal(full.depth.view(torch.int32), depth.view(torch.int32)) and torch.equal(full.seg, seg) and torch.equal(full.rgb, img.rgb)
    assert full.depth.dtype == torch.float32 and full.seg.dtype == torch.int32
    # the scene colours, as an explicit table, per env, and through a dict override that hits exactly the geoms geom_group returns
    scene = appearance.so100_colors(env.meta)
    assert torch.equal(env.render_color("overhead_cam", 48, 64, colors=scene).rgb, img.rgb)
    assert torch.equal(env.render_color("overhead_cam", 48, 64, colors=np.tile(scene, (4, 1, 1))).rgb, img.rgb)
    group = env.geom_group("table")
    assert len(group.geoms) == 5
    changed = scene.copy()
    changed[list(group.geoms)] = (0.0, 1.0, 0.0)
    over = env.render_color("overhead_cam", 48, 64, colors={"table": (0.0, 1.0, 0.0)}).rgb
    assert torch.equal(over, env.render_color("overhead_cam", 48, 64, colors=changed).rgb) and not torch.equal(over, img.rgb)
    on_table = torch.isin(seg, torch.as_tensor(list(group.geoms), dtype=torch.int32, device=seg.device))
    assert on_table.any() and torch.equal(over[~on_table], img.rgb[~on_table]) and torch.all(over[on_table][:, 0] == 0) and torch.all(over[on_table][:, 2] == 0)
    # a sequence of cameras, a subset of envs, another shading
    sub = env.render_color(["overhead_cam", JAW_CAM], 48, 64, env_ids=[2, 0], shading=sc.HEADLIGHT)
    assert sub.rgb.shape == (2, 2, 48, 64, 3)
    assert torch.equal(sub.rgb[:, 0], env.render_color("overhead_cam", 48, 64, shading=sc.HEADLIGHT).rgb[[2, 0], 0])
    with pytest.raises(ValueError):
        env.render_color("no_such_cam", 8, 8)
    with pytest.raises(ValueError):
        env.render_color("overhead_cam", 8, 8, colors=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        env.render_color("overhead_cam", 8, 8, colors={"no_such_geom": (1, 1, 1)})
    env.close()


def test_lerobot_wrapper_images():
    import torch
    from so101_sim_amd.lerobot import SO101LeRobotWrapper
    w = SO101LeRobotWrapper(cameras=("overhead_cam", "front_cam"), camera_resolution=(24, 32), time_limit=10.0, n_envs=3, random_state=3, settle_max_substeps=100)
    spec = w.get_observation_spec()
    assert spec["images"] == {n: {"shape": (3, 24, 32), "dtype": np.float32} for n in ("overhead_cam", "front_cam")}
    act = np.tile(np.array([0.3, -1.2, 1.3, 1.0, -0.5, 0.4], dtype=np.float32), (3, 1))
    for make in (w.reset, lambda: w.step(act)):
        frame = make()
        rgb = w.env.render_color(["overhead_cam", "front_cam"], 24, 32).rgb
        for k, name in enumerate(("overhead_cam", "front_cam")):
            img = frame[f"observation.images.{name}"]
            assert img.shape == (3, 3, 24, 32) and img.dtype == torch.float32 and img.is_cuda
            assert torch.equal(img, rgb[:, k].permute(0, 3, 1, 2) / 255)
            assert float(img.max()) <= 1.0 and float(img.max()) > 0.0
    w.env.close()
    one = SO101LeRobotWrapper(cameras=("overhead_cam",), camera_resolution=(24, 32), time_limit=10.0, n_envs=1, random_state=3, settle_max_substeps=100)
    img = one.reset()["observation.images.overhead_cam"]
    assert img.shape == (3, 24, 32) and img.dtype == torch.float32
    one.env.close()
    with pytest.raises(ValueError, match="no_such_cam"):
        SO101LeRobotWrapper(cameras=("no_such_cam",))
    plain = SO101LeRobotWrapper(time_limit=10.0, n_envs=2, random_state=3, settle_max_substeps=100)
    assert plain.get_observation_spec()["images"] == {}
    assert not any(k.startswith("observation.images") for k in plain.reset())
    plain.env.close()
