"""Depth / segmentation cameras on the MI355X (so101_render, include/so101.h) against the fp64 reference of tests/raycast_ref.py.

Acceptance per image (raycast_ref.assert_image): at most 2 % of the pixels are ambiguous (a condition on the view), every other pixel has the
reference's geom id and |z - z64| <= 5e-5 z64, every pixel is well formed."""
import numpy as np
import pytest

from so101_sim_amd import cameras
from so101_sim_amd.model import blob as blobfmt
from tests import raycast_ref as rr
from tests.render_cases import FIVE_CAMS, JAW_CAM, render, scene_planes
from tests.simharness import ArraySim

pytestmark = pytest.mark.gpu
BACKEND = "gpu"
STATE_NAMES = ("home", "grasp", "tilted")


@pytest.fixture(scope="module")
def ref(blobs):
    return rr.RaycastRef(blobs["f64"])


def _sim(blob_f32, n, **cfg):
    sim = ArraySim(blob_f32, n, backend=BACKEND, **cfg)
    sim.sim.set_hull_planes(*scene_planes(blob_f32))
    return sim


def _check(ref, key, depth, seg, qpos, cams, label):
    H, W = depth.shape[-2:]
    worst = 0.0
    for k, cam in enumerate(cams):
        img = rr.reference_image(ref, key, qpos, rr.cam_tuple(cam), H, W)
        worst = max(worst, rr.assert_image(depth[k], seg[k], img, ref.ngeom, f"{label} {cam.name} {H}x{W}")[1])
    return worst


def test_three_states_five_cameras(blobs, ref):
    sim = _sim(blobs["f32"], 3)
    sim.set_state(np.stack([rr.STATES[s] for s in STATE_NAMES], axis=1))
    depth, seg = render(sim, FIVE_CAMS, 48, 64)
    worst = max(_check(ref, "banana", depth[e], seg[e], rr.STATES[s], FIVE_CAMS, s) for e, s in enumerate(STATE_NAMES))
    print(f"worst relative depth error over the 15 images: {worst:.3e}")
    # the wrist camera at the home pose looks past everything: a valid image without a single hit
    wrist = [c.name for c in FIVE_CAMS].index("wrist_cam")
    assert np.all(np.isposinf(depth[0, wrist])) and np.all(seg[0, wrist] == -1)


@pytest.mark.parametrize("size", [(30, 44), (1, 1)])
def test_ragged_sizes(blobs, ref, size):
    sim = _sim(blobs["f32"], 1)
    sim.set_state(rr.STATES["tilted"][:, None])
    cams = [cameras.SO100_CAMERAS[n] for n in ("overhead_cam", "front_cam", "side_cam")] + [JAW_CAM]
    depth, seg = render(sim, cams, *size)
    _check(ref, "banana", depth[0], seg[0], rr.STATES["tilted"], cams, "tilted")


def test_determinism_across_batch_index_and_camera_count(blobs):
    N = 130
    q = np.tile(rr.STATES["grasp"][:, None], (1, N))
    q[:, 7], q[:, 129] = rr.STATES["home"], rr.STATES["tilted"]
    sim = _sim(blobs["f32"], N)
    sim.set_state(q)
    depth, seg = render(sim, FIVE_CAMS, 30, 44)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    pick = [129, 7, 0]
    d2, s2 = render(sim, FIVE_CAMS, 30, 44, env_index=pick)
    assert np.array_equal(bits(d2), bits(depth[pick])) and np.array_equal(s2, seg[pick])
    same = [e for e in range(N) if e not in (7, 129)]
    assert len(same) == 128
    assert np.all(bits(depth[same]) == bits(depth[0])[None]) and np.all(seg[same] == seg[0][None])
    assert not np.array_equal(seg[7], seg[0]) and not np.array_equal(seg[129], seg[0])
    for k, cam in enumerate(FIVE_CAMS):
        d1, s1 = render(sim, [cam], 30, 44, env_index=pick)
        assert np.array_equal(bits(d1[:, 0]), bits(depth[pick, k])) and np.array_equal(s1[:, 0], seg[pick, k]), cam.name


def test_render_reads_the_bound_state_and_changes_nothing(blobs, ref):
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
            qpos = sim.get_state()[0]
            out = (qpos,) + render(sim, cams, 30, 44)
        sim.step(act)
        return out, [sim._get(a) for a in (sim.qpos, sim.qvel, sim.warm, sim.ctrl, sim.obs)]

    (qpos, depth, seg), after = run(True)
    _, after_plain = run(False)
    assert not np.array_equal(qpos.astype(np.float32), q0.astype(np.float32))
    for e in range(4):
        _check(ref, "banana", depth[e], seg[e], qpos[:, e], cams, f"stepped env {e}")
    for a, b in zip(after, after_plain):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


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


def test_sphere_geom(blobs):
    raw32, g = _capsule_as_sphere(blobs["f32"])
    raw64, g64 = _capsule_as_sphere(blobs["f64"])
    assert g == g64
    sref = rr.RaycastRef(raw64)
    sim = _sim(raw32, 1)
    sim.set_state(rr.STATES["home"][:, None])
    cams = [cameras.SO100_CAMERAS["front_cam"]]
    depth, seg = render(sim, cams, 48, 64)
    _check(sref, "banana_sphere", depth[0], seg[0], rr.STATES["home"], cams, "sphere home")
    img = rr.reference_image(sref, "banana_sphere", rr.STATES["home"], rr.cam_tuple(cams[0]), 48, 64)
    assert np.count_nonzero((img[1] == g) & ~img[2]) >= 4, "the view must show the sphere"
    assert np.array_equal((seg[0, 0] == g) & ~img[2], (img[1] == g) & ~img[2])


def test_batched_environment_render_depth(blobs):
    import torch
    from so101_sim_amd import task_suite
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=7, n_envs=4, settle_max_substeps=100)
    env.reset_all()
    depth, seg = env.render_depth("overhead_cam", 48, 64)
    assert depth.shape == seg.shape == (4, 1, 48, 64) and depth.dtype == torch.float32 and seg.dtype == torch.int32
    assert depth.device == env.qpos.device and seg.device == env.qpos.device
    d2, s2 = torch.full_like(depth, float("nan")), torch.full_like(seg, -7)
    env.sim.render([cameras.SO100_CAMERAS["overhead_cam"].spec()], 48, 64, None, 4, d2.data_ptr(), s2.data_ptr(), env._stream())
    assert torch.equal(depth.view(torch.int32), d2.view(torch.int32)) and torch.equal(seg, s2)
    names = env.meta["geom_names"]
    seen = {names[i] for i in torch.unique(seg).tolist() if i >= 0}
    assert "table_surface" in seen and int(seg.max()) < len(names)
    # a sequence of cameras, a subset of envs, no segmentation
    d3, s3 = env.render_depth(["overhead_cam", JAW_CAM], 48, 64, env_ids=[2, 0], segmentation=False)
    assert s3 is None and d3.shape == (2, 2, 48, 64)
    assert torch.equal(d3[:, 0].view(torch.int32), depth[[2, 0], 0].view(torch.int32))
    with pytest.raises(ValueError):
        env.render_depth("no_such_cam", 8, 8)
    env.close()
