"""Depth / segmentation cameras without a GPU: the hull planes, the camera table, the library's argument and plane checks and one small
render through the emulated build of the kernel source (tests/hostemu), against the fp64 reference of tests/raycast_ref.py."""
import ctypes as C

import numpy as np
import pytest

from so101_sim_amd import cameras, native
from so101_sim_amd.model import blob as blobfmt, meshes
from tests import raycast_ref as rr
from tests.render_cases import JAW_CAM, render, scene_planes
from tests.simharness import ArraySim

# what commit f55d392 (the last one whose two engines each counted and grew their own render buffers) reports for the sequence of
# test_scratch_bytes_count_the_planes_and_the_grown_frames_scratch, measured with that commit's library under the emulator
SCRATCH_BYTES_AFTER_RENDERS = 1043419

def _check_planes(verts, planes):
    assert planes.dtype == np.float64 and planes.shape[1] == 4 and len(planes) >= 4
    np.testing.assert_allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0, atol=1e-12)
    sd = verts @ planes[:, :3].T + planes[:, 3]           # [V, F] signed distances
    assert sd.max() <= 1e-9, "a vertex lies outside a plane"
    assert sd.max(axis=0).min() >= -1e-9, "a plane touches no vertex"


def test_hull_planes_on_a_cube_and_a_scene_hull(blobs):
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-2, 2) for z in (-3, 3)], dtype=np.float64)
    p = meshes.hull_planes(np.vstack([cube, [[0.2, 0.1, -0.3]]]))          # an interior point changes nothing
    _check_planes(cube, p)
    # the twelve triangles of the six faces are merged; merging must not matter, so only the SET of half-spaces is checked
    want = {(1, 0, 0, -1), (-1, 0, 0, -1), (0, 1, 0, -2), (0, -1, 0, -2), (0, 0, 1, -3), (0, 0, -1, -3)}
    assert {tuple(int(v) for v in np.round(r)) for r in p} == want and np.abs(p - np.round(p)).max() < 1e-12
    m = blobfmt.unpack(blobs["f64"])
    g = int(np.flatnonzero(m["geom_type"] == 5)[0])
    v = m["mesh_vert"].reshape(-1, 3)[m["geom_vertadr"][g]: m["geom_vertadr"][g] + m["geom_vertnum"][g]]
    _check_planes(v, meshes.hull_planes(v))


def test_so100_cameras_match_the_reference_scene(golden):
    gold = golden["so100_cameras"]
    assert {c["name"] for c in gold["cameras"]} == set(cameras.SO100_CAMERAS) and len(gold["cameras"]) == 5
    for c in gold["cameras"]:
        cam = cameras.SO100_CAMERAS[c["name"]]
        pos = np.array(c["pos"])
        if c["body"] in cameras.ARM_LINKS:
            assert cam.body == cameras.ARM_LINKS.index(c["body"])
        else:
            # fixed to the world or to a static, unrotated body: composed with that body's position
            assert cam.body == -1 and all(b["quat"] is None for b in c["chain"])
            pos = pos + sum((np.array(b["pos"]) for b in c["chain"]), np.zeros(3))
        np.testing.assert_allclose(cam.pos, pos, atol=1e-12)
        assert cam.fovy == (c["fovy"][0] if c["fovy"] else gold["default_fovy"])
        M = np.array(cam.mat)
        np.testing.assert_allclose(M.T @ M, np.eye(3), atol=1e-12)
        assert abs(np.linalg.det(M) - 1) < 1e-12
        if c["xyaxes"] is None:
            np.testing.assert_array_equal(M, np.eye(3))
        else:
            x, y = np.array(c["xyaxes"][:3]), np.array(c["xyaxes"][3:])
            np.testing.assert_allclose(M[:, 0], x / np.linalg.norm(x), atol=1e-12)          # x keeps its direction
            assert abs(M[:, 1] @ M[:, 0]) < 1e-12 and M[:, 1] @ y > 0                        # y: the part of the given y across x
            np.testing.assert_allclose(np.cross(np.cross(x, y), M[:, 2]), 0, atol=1e-12)     # z: normal of the given plane
    w = cameras.SO100_CAMERAS["wrist_cam"]
    assert w.body == 4 and w.fovy == 70.0


def test_plane_validation_and_render_state_errors(blobs):
    sim = ArraySim(blobs["f32"], 1, backend="emu")
    L, h = sim.sim.L, sim.sim.h
    planes, adr = scene_planes(blobs["f32"])
    gtype = blobfmt.unpack(blobs["f32"])["geom_type"]
    mesh = int(np.flatnonzero(gtype == 5)[0])
    cam = (native.CameraSpec * 1)()
    cam[0].body, cam[0].fovy_deg = -1, 45.0
    cam[0].pos[:], cam[0].mat[:] = [0, -0.2, 1.0], [1, 0, 0, 0, 1, 0, 0, 0, 1]
    depth, seg = np.zeros((1, 1, 4, 4), np.float32), np.zeros((1, 1, 4, 4), np.int32)
    call = lambda ncam=1, H=4, W=4, n=1, d=depth.ctypes.data, s=seg.ctypes.data: L.so101_render(h, cam, ncam, H, W, None, n, d, s, None)
    # mesh geoms and no planes yet
    assert call() == -4 and b"so101_set_hull_planes" in L.so101_last_error(h)

    def rejected(p, a, what):
        p, a = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(a, np.int32)
        assert L.so101_set_hull_planes(h, p.ctypes.data, a.ctypes.data) == -1
        msg = L.so101_last_error(h).decode()
        assert what in msg, msg
        return msg

    k0 = int(adr[mesh])
    # a non-mesh geom with planes: the floor (geom 0) takes the first mesh's first plane
    a = adr.copy(); a[1:mesh + 1] += 1
    assert "geom 0:" in rejected(planes, a, "not a mesh geom")
    # a mesh geom with three planes
    a = adr.copy(); a[mesh + 1:] -= int(adr[mesh + 1] - adr[mesh]) - 3
    rejected(np.delete(planes, np.arange(k0 + 3, int(adr[mesh + 1])), axis=0), a, f"geom {mesh}: a mesh geom needs at least 4 planes")
    p = planes.copy(); p[k0 + 2, :3] *= 1.001
    rejected(p, adr, f"geom {mesh}: plane 2 has no unit normal")
    p = planes.copy(); p[k0 + 1, 3] += 1e-4           # moved inwards: a vertex is left outside
    rejected(p, adr, f"geom {mesh}: plane 1 cuts off a hull vertex")
    p = planes.copy(); p[k0 + 1, 3] -= 1e-4           # moved outwards: it touches nothing
    rejected(p, adr, f"geom {mesh}: plane 1 touches no hull vertex")
    assert L.so101_set_hull_planes(h, None, None) == -1 and L.so101_set_hull_planes(None, None, None) == -1
    assert call() == -4                                # nothing was accepted so far
    sim.sim.set_hull_planes(planes, adr)
    assert call() == 0
    for bad in (dict(ncam=0), dict(ncam=9), dict(H=0), dict(W=4097), dict(n=0), dict(n=2), dict(d=None, s=None)):
        assert call(**bad) == -1, bad
    cam[0].body = 8
    assert call() == -1
    cam[0].body, cam[0].fovy_deg = -1, 180.0
    assert call() == -1
    assert L.so101_render(None, cam, 1, 4, 4, None, 1, None, None, None) == -1


def test_scratch_bytes_count_the_planes_and_the_grown_frames_scratch(blobs):
    """create, set_hull_planes, a render of 2 envs, then one of 5 (the frames scratch is freed and allocated again): SO101_INFO_SCRATCH_BYTES
    counts the planes once and the scratch of 5 envs, not of 2 + 5"""
    sim = ArraySim(blobs["f32"], 5, backend="emu")
    sim.sim.set_hull_planes(*scene_planes(blobs["f32"]))
    sim.set_state(np.tile(rr.STATES["grasp"][:, None], (1, 5)))
    cams = [cameras.SO100_CAMERAS["overhead_cam"]]
    render(sim, cams, 4, 4, env_index=[0, 1])
    render(sim, cams, 4, 4)
    print("scratch_bytes", sim.sim.info()["scratch_bytes"])
    assert sim.sim.info()["scratch_bytes"] == SCRATCH_BYTES_AFTER_RENDERS


def test_emulated_render_matches_fp64_reference(blobs):
    """one env in the grasp state, overhead_cam and the jaw camera at 16 x 24 (ragged: 2 x 3 tiles of 8 x 8) through the emulated kernels"""
    ref = rr.RaycastRef(blobs["f64"])
    sim = ArraySim(blobs["f32"], 1, backend="emu")
    sim.sim.set_hull_planes(*scene_planes(blobs["f32"]))
    q = rr.STATES["grasp"]
    sim.set_state(q[:, None])
    cams = [cameras.SO100_CAMERAS["overhead_cam"], JAW_CAM]
    depth, seg = render(sim, cams, 16, 24)
    q_before = sim.get_state()[0]
    for k, cam in enumerate(cams):
        img = rr.reference_image(ref, "banana", q, rr.cam_tuple(cam), 16, 24)
        rr.assert_image(depth[0, k], seg[0, k], img, ref.ngeom, f"emu grasp {cam.name} 16x24")
        assert np.isfinite(img[0]).any()
    np.testing.assert_array_equal(q_before[:, 0], q.astype(np.float32))      # the render changed no state
