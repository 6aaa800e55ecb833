"""Shared pieces of the tree engine's camera tests (test_tree_render_emu.py on the emulated build, test_tree_render_gpu.py on the MI355X):
the blobs, the states, the cameras with their bodies resolved, one so101_tree_render call through tests/simharness.TreeArraySim.

The states are chosen for what they show, none of them is the result of a step: the arms at the task's home pose and at two bent poses
(fingers at different openings, so the slide joints matter), the props resting on or tilted above the table.  The views they give were
checked against the ambiguity cap of raycast_ref.assert_image with the fp64 reference alone."""
from __future__ import annotations

import functools

import numpy as np

from so101_sim_amd import cameras
from so101_sim_amd.model import scenes
from tests import raycast_ref as rr
from tests import tree_raycast_ref as trr
from tests.render_cases import scene_planes          # (planes as the product computes them: the same helper serves both engines)


@functools.lru_cache(maxsize=None)
def blobs(scene: str):
    """dict(f32, f64, meta) of "banana" (the HandOverBanana scene, 32-dof build) or "dining" (DiningPlaceBananaInBowl, 64-dof build)"""
    load = scenes.load_dining_blob if scene == "dining" else scenes.load_aloha_blob
    raw32, meta = load("banana", "f32")
    return dict(f32=raw32, f64=load("banana", "f64")[0], meta=meta)


@functools.lru_cache(maxsize=None)
def reference(scene: str) -> trr.TreeRaycastRef:
    return trr.TreeRaycastRef(blobs(scene)["f64"])


@functools.lru_cache(maxsize=None)
def planes(scene: str):
    return scene_planes(blobs(scene)["f32"])


def cams_of(scene: str, names):
    """ALOHA_CAMERAS entries (or Camera objects) with their bodies resolved against the scene's body names"""
    return [c.with_body_ids(blobs(scene)["meta"]["body_names"]) for c in cameras.resolve(names, cameras.ALOHA_CAMERAS)]


# on the left arm's left finger (a slide joint below the wrist chain), looking along the finger towards the other arm
FINGER_CAM = cameras.Camera.from_xyaxes("finger_cam", "left/left_finger_link", (0.0, 0.0, 0.03), (0, 1, 0, 0, 0, 1), fovy=70.0)

# Cameras of the ragged-size test.  teleoperator_pov is not among them: from there the front face of the table box (geom "table") and a
# facet of the hull "tablelegs" lie in one plane, an exact tie in depth between two geoms that the +-1e-4 jitter of the reference does not
# flag (fp64 resolves it the same way in all five rays) and fp32 may resolve the other way; at 30 x 44 a pixel row falls on that face.
RAGGED_CAMS = ("overhead_cam", "wrist_cam_left", "wrist_cam_right", FINGER_CAM)

_HOME = np.concatenate([scenes.ALOHA_HOME_QPOS, scenes.ALOHA_HOME_QPOS])
_BENT = np.array([0.35, -0.45, 0.75, 0.4, 0.35, -0.3, 0.030, 0.030, -0.5, -0.2, 0.55, -0.6, 0.5, 0.8, 0.012, 0.012])
_REACH = np.array([-0.3, 0.1, 0.35, 0.2, 0.9, 0.5, 0.02, 0.02, 0.25, -0.7, 1.0, 0.3, 0.1, -0.9, 0.037, 0.037])
_ID = [1.0, 0.0, 0.0, 0.0]
_q = rr._axis_quat

# qpos of the banana hand-over blob: arms (16) | object pos, quat | container pos, quat
STATES = {
    "home": np.r_[_HOME, [0.15, 0.02, 0.06], _ID, [-0.15, -0.03, 0.06], _ID],
    "bent": np.r_[_BENT, [0.10, -0.12, 0.16], _q((1, 2, 0.5), 0.9), [-0.18, 0.08, 0.12], _q((0.3, 1, 0), 0.5)],
    "reach": np.r_[_REACH, [-0.02, 0.15, 0.22], _q((0, 1, 1), -1.2), [0.2, -0.15, 0.09], _q((1, 0, 0.2), 0.35)],
}
STATE_NAMES = ("home", "bent", "reach")

# the Dining blob: arms (16) | mug, pen, banana, plate, bowl, container (pos, quat each): the six props spread over the table, two of them tilted
DINING_STATE = np.r_[_BENT,
                     [-0.25, -0.18, 0.09], _ID, [0.0, -0.17, 0.07], _q((0, 0, 1), 0.7), [0.25, -0.17, 0.08], _q((1, 1, 0), 0.4),
                     [-0.26, 0.15, 0.07], _ID, [0.0, 0.15, 0.09], _q((1, 0, 0), 0.3), [0.26, 0.15, 0.08], _ID]


def render(sim, cams, H, W, env_index=None, source=0):
    """so101_tree_render on a TreeArraySim (either backend) -> numpy depth [n, ncam, H, W] float32, seg int32.  The outputs start as NaN / -7,
    so a pixel the kernel does not write fails every check."""
    n = sim.N if env_index is None else len(env_index)
    shape = (n, len(cams), H, W)
    if sim.backend == "gpu":
        t = sim.torch
        depth = t.full(shape, float("nan"), dtype=t.float32, device=sim.dev)
        seg = t.full(shape, -7, dtype=t.int32, device=sim.dev)
        idx = None if env_index is None else t.as_tensor(np.asarray(env_index, dtype=np.int32)).to(sim.dev)
    else:
        depth, seg = np.full(shape, np.nan, dtype=np.float32), np.full(shape, -7, dtype=np.int32)
        idx = None if env_index is None else np.asarray(env_index, dtype=np.int32)
    sim.sim.render([c.spec() for c in cams], H, W, None if idx is None else sim.ptr(idx), n, sim.ptr(depth), sim.ptr(seg), sim.stream(), source=source)
    return sim._get(depth), sim._get(seg)


def check(scene, depth, seg, qpos, cams, label):
    """assert_image of every camera's image [ncam, H, W] of one env; returns the worst relative depth error"""
    ref = reference(scene)
    H, W = depth.shape[-2:]
    worst = 0.0
    for k, cam in enumerate(cams):
        img = rr.reference_image(ref, "tree_" + scene, qpos, rr.cam_tuple(cam), H, W)
        worst = max(worst, rr.assert_image(depth[k], seg[k], img, ref.ngeom, f"{label} {cam.name} {H}x{W}")[1])
    return worst
