"""Shared pieces of the camera tests (test_render_emu.py on the emulated build, test_render_gpu.py on the MI355X): the test
camera, the hull planes of a blob as the product computes them, one so101_render call through tests/simharness.ArraySim."""
from __future__ import annotations

import numpy as np

from so101_sim_amd import cameras
from so101_sim_amd.model import blob as blobfmt, meshes

# looks down the jaw: on arm link 4 (Fixed_Jaw) at the wrist camera's position, x = (1, 0, 0), y = (0, 0, -1), fovy 70
JAW_CAM = cameras.Camera.from_xyaxes("jaw_cam", 4, (0.0, 0.02, 0.04), (1, 0, 0, 0, 0, -1), fovy=70.0)
SCENE_CAMS = [cameras.SO100_CAMERAS[n] for n in ("overhead_cam", "side_cam", "front_cam", "wrist_cam")]
FIVE_CAMS = SCENE_CAMS + [JAW_CAM]


def scene_planes(blob_f32: bytes):
    """(planes [n, 4] float32, plane_adr [ngeom + 1] int32) of a blob's mesh geoms, from meshes.hull_planes"""
    m = blobfmt.unpack(blob_f32)
    verts = np.asarray(m["mesh_vert"], dtype=np.float64).reshape(-1, 3)
    adr, chunks = [0], []
    for t, a, n in zip(m["geom_type"], m["geom_vertadr"], m["geom_vertnum"]):
        k = 0
        if int(t) == 5:
            chunks.append(meshes.hull_planes(verts[a:a + n]))
            k = len(chunks[-1])
        adr.append(adr[-1] + k)
    return np.concatenate(chunks).astype(np.float32), np.asarray(adr, dtype=np.int32)


def render(sim, cams, H, W, env_index=None):
    """so101_render on an ArraySim (either backend) -> numpy depth [n, ncam, H, W] float32, seg int32.  The outputs start as NaN / -7, so a
    pixel the kernel does not write fails every check."""
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
    sim.sim.render([c.spec() for c in cams], H, W, None if idx is None else sim.ptr(idx), n, sim.ptr(depth), sim.ptr(seg), sim.stream())
    return sim._get(depth), sim._get(seg)
