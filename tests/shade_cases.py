"""Shared pieces of the colour-camera tests (test_shade_emu.py on the emulated build; test_shade_gpu.py and test_tree_shade_gpu.py on the
MI355X): one so101_render_color / so101_tree_render_color call through tests/simharness, the acceptance of a batch of images against
tests/shade_ref.py, a few shadings."""
from __future__ import annotations

import numpy as np

from so101_sim_amd import appearance
from tests import raycast_ref as rr
from tests import shade_ref as sr

OUTPUTS = ("rgb", "normal", "depth", "seg")
_FILL = dict(rgb=(np.uint8, 77, 3), normal=(np.float32, np.nan, 3), depth=(np.float32, np.nan, 0), seg=(np.int32, -7, 0))

NO_LIGHT = appearance.Shading(ambient=(0.7, 0.5, 0.9), background=(0.2, 0.3, 0.4))
HEADLIGHT = appearance.Shading(ambient=(0.1, 0.1, 0.1), background=(0.05, 0.05, 0.1), lights=(appearance.Light(None, (0.8, 0.7, 0.6)),))
# ambient 0.9 and two lights of 0.9 from above: every upward face sums to more than 1 of a colour near 1 and saturates
SATURATING = appearance.Shading(ambient=(0.9, 0.9, 0.9), background=(1.5, 0.0, 0.5),
                                lights=(appearance.Light.along((0, 0, -1), (0.9, 0.9, 0.9)), appearance.Light.along((0.1, 0.2, -1), (0.9, 0.9, 0.9))))


def render_color(sim, cams, H, W, colors, shading, env_index=None, per_env=False, want=OUTPUTS, source=None):
    """one colour render on an ArraySim / TreeArraySim (either backend) -> dict of numpy arrays for the outputs named in `want` ([n, ncam, H, W]
    and [n, ncam, H, W, 3]).  The outputs start as 77 / NaN / -7, so a pixel the kernels do not write fails every check."""
    n = sim.N if env_index is None else len(env_index)
    colors = np.ascontiguousarray(colors, dtype=np.float32)
    bufs = {}
    for name in want:
        dt, fill, last = _FILL[name]
        bufs[name] = np.full((n, len(cams), H, W) + ((last,) if last else ()), fill, dtype=dt)
    idx = None if env_index is None else np.asarray(env_index, dtype=np.int32)
    if sim.backend == "gpu":
        t = sim.torch
        bufs = {k: t.from_numpy(v).to(sim.dev) for k, v in bufs.items()}
        colors = t.from_numpy(colors).to(sim.dev)
        idx = None if idx is None else t.from_numpy(idx).to(sim.dev)
    ptrs = {k: (sim.ptr(bufs[k]) if k in bufs else None) for k in OUTPUTS}
    extra = {} if source is None else dict(source=source)
    sim.sim.render_color([c.spec() for c in cams], H, W, None if idx is None else sim.ptr(idx), n, shading.spec(), sim.ptr(colors), per_env,
                         stream=sim.stream(), **ptrs, **extra)
    return {k: sim._get(v) for k, v in bufs.items()}


def check(ref, key, out, e, qpos, cams, colors, shading, label):
    """shade_ref.assert_image of every camera's image of entry e; returns (worst |n - n64|_inf, unambiguous pixels per feature code)"""
    H, W = out["seg"].shape[-2:]
    worst, counts = 0.0, np.zeros(len(sr.FEATURE_NAMES), dtype=np.int64)
    for k, cam in enumerate(cams):
        img = sr.reference_image(ref, key, qpos, rr.cam_tuple(cam), H, W)
        err, c = sr.assert_image(out["rgb"][e, k], out["normal"][e, k], out["depth"][e, k], out["seg"][e, k], img, ref.ngeom, colors, shading,
                                 f"{label} {cam.name} {H}x{W}")
        worst, counts = max(worst, err), counts + c
    return worst, counts


bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
