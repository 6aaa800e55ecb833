"""Depth / segmentation cameras of the general-tree engine without a GPU: the ALOHA camera table, the library's plane and state checks and
one small render through the emulated build of the kernel source (tests/hostemu), against the fp64 reference of tests/tree_raycast_ref.py."""
import numpy as np
import pytest

from so101_sim_amd import cameras, native
from so101_sim_amd.model import blob as blobfmt, scenes
from tests import raycast_ref as rr
from tests import tree_render_cases as tc
from tests.simharness import TreeArraySim, build_emu


def _mat_of_quat(q):
    return rr.q2m(np.asarray(q, dtype=np.float64) / np.linalg.norm(q))


def test_aloha_cameras_match_the_reference_scene(golden):
    gold = golden["aloha_cameras"]
    assert {c["name"] for c in gold["cameras"]} == set(cameras.ALOHA_CAMERAS) and len(gold["cameras"]) == 6
    assert gold["angle"] == "radian"
    body_names = tc.blobs("banana")["meta"]["body_names"]
    for c in gold["cameras"]:
        cam = cameras.ALOHA_CAMERAS[c["name"]]
        pos = np.array(c["pos"])
        if c["body"] == "world":
            assert cam.body == cameras.WORLD and c["chain"] == []
        else:
            # fixed to a moving body: by name, in that body's frame as the file states it
            assert cam.body == c["body"] == c["chain"][-1]["name"] and cam.body in body_names
            assert cam.with_body_ids(body_names).body == body_names.index(c["body"])
        if c["name"] == "worms_eye_cam":
            pos = pos + [0.0, 0.0, scenes.ALOHA_TABLE_HEIGHT_OFFSET]          # lifted with the table (aloha2_task.py:504-507)
        if c["name"].startswith("wrist_cam"):
            np.testing.assert_array_equal(pos, cameras.WRIST_CAMERA_POSITION)  # (aloha2_task.py:217-221 sets what the file already states)
        np.testing.assert_allclose(cam.pos, pos, atol=1e-12)
        # field of view: focal / sensorsize where given (fovy = 2 atan(sensorsize_y / (2 focal_y))), MuJoCo's default otherwise
        if c["focal"] is not None:
            assert c["fovy"] is None and c["focal"][0] == c["focal"][1]
            want = np.degrees(2 * np.arctan(c["sensorsize"][1] / (2 * c["focal"][1])))
            assert abs(want - 58.008) < 1e-3
        else:
            want = c["fovy"][0] if c["fovy"] else gold["default_fovy"]
        assert abs(cam.fovy - want) < 1e-12
        M = np.array(cam.mat)
        np.testing.assert_allclose(M.T @ M, np.eye(3), atol=1e-12)
        assert abs(np.linalg.det(M) - 1) < 1e-12
        assert sum(c[k] is not None for k in ("quat", "euler", "xyaxes")) == 1
        if c["quat"] is not None:
            np.testing.assert_allclose(M, _mat_of_quat(c["quat"]), atol=1e-12)
        elif c["euler"] is not None:
            # only the first angle is used in the file: a rotation about x, whatever the sequence
            assert c["euler"][1] == c["euler"][2] == 0.0
            a = c["euler"][0]
            np.testing.assert_allclose(M, [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], atol=1e-12)
        else:
            x, y = np.array(c["xyaxes"][:3]), np.array(c["xyaxes"][3:])
            np.testing.assert_allclose(M[:, 0], x / np.linalg.norm(x), atol=1e-12)
            assert abs(M[:, 1] @ M[:, 0]) < 1e-12 and M[:, 1] @ y > 0
            np.testing.assert_allclose(np.cross(np.cross(x, y), M[:, 2]), 0, atol=1e-12)
    # the general constructors: an euler triple in MuJoCo's default sequence (intrinsic x, y, z) and a quaternion that is not normalised
    e = cameras.Camera.from_euler("e", 0, (0, 0, 0), (0.3, -0.2, 0.5))
    qx, qy, qz = (rr._axis_quat(ax, a) for ax, a in (((1, 0, 0), 0.3), ((0, 1, 0), -0.2), ((0, 0, 1), 0.5)))
    np.testing.assert_allclose(np.array(e.mat), rr.q2m(rr.qmul(rr.qmul(qx, qy), qz)), atol=1e-12)
    q = cameras.Camera.from_quat("q", 0, (0, 0, 0), (2.0, 0.0, 2.0, 0.0))
    np.testing.assert_allclose(np.array(q.mat), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-12)
    with pytest.raises(ValueError):
        cameras.Camera.from_quat("n", "no/such_body", (0, 0, 0)).with_body_ids(body_names)
    with pytest.raises(ValueError):
        cameras.ALOHA_CAMERAS["wrist_cam_left"].spec()          # a body still given by name


def test_tree_entry_points_are_exported():
    assert {"so101_tree_set_hull_planes", "so101_tree_render"} <= set(native.EXPORTS)


def test_plane_validation_and_render_state_errors():
    raw32 = tc.blobs("banana")["f32"]
    sim = TreeArraySim(raw32, 1, backend="emu")
    L, h = sim.sim.L, sim.sim.h
    planes, adr = tc.planes("banana")
    m = blobfmt.unpack(raw32)
    gtype = m["geom_type"]
    mesh, other = int(np.flatnonzero(gtype == 5)[0]), int(np.flatnonzero(gtype != 5)[0])
    cam = (native.CameraSpec * 1)()
    cam[0].body, cam[0].fovy_deg = -1, 45.0
    cam[0].pos[:], cam[0].mat[:] = [0, -0.2, 1.0], [1, 0, 0, 0, 1, 0, 0, 0, 1]
    depth, seg = np.zeros((1, 1, 4, 4), np.float32), np.zeros((1, 1, 4, 4), np.int32)
    call = lambda ncam=1, H=4, W=4, n=1, src=0, d=depth.ctypes.data, s=seg.ctypes.data: L.so101_tree_render(h, cam, ncam, H, W, None, n, src, d, s, None)
    err = lambda: L.so101_tree_last_error(h).decode()
    # mesh geoms and no planes yet
    assert call() == -4 and "so101_tree_set_hull_planes" in err()

    def rejected(p, a, what):
        p, a = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(a, np.int32)
        assert L.so101_tree_set_hull_planes(h, p.ctypes.data, a.ctypes.data) == -1
        msg = err()
        assert msg.startswith("so101_tree_set_hull_planes: geom ") and what in msg, msg
        return msg

    k0 = int(adr[mesh])
    # a non-mesh geom with planes: it takes the first plane of the mesh geom after it
    nxt = int(np.flatnonzero((gtype == 5) & (np.arange(len(gtype)) > other))[0])
    a = adr.copy(); a[other + 1:nxt + 1] += 1
    assert f"geom {other}:" in rejected(planes, a, "not a mesh geom")
    # a mesh geom with three planes
    a = adr.copy(); a[mesh + 1:] -= int(adr[mesh + 1] - adr[mesh]) - 3
    rejected(np.delete(planes, np.arange(k0 + 3, int(adr[mesh + 1])), axis=0), a, f"geom {mesh}: a mesh geom needs at least 4 planes")
    p = planes.copy(); p[k0 + 2, :3] *= 1.001
    rejected(p, adr, f"geom {mesh}: plane 2 has no unit normal")
    p = planes.copy(); p[k0 + 1, 3] += 1e-4           # moved inwards: a vertex is left outside
    rejected(p, adr, f"geom {mesh}: plane 1 cuts off a hull vertex")
    p = planes.copy(); p[k0 + 1, 3] -= 1e-4           # moved outwards: it touches nothing
    rejected(p, adr, f"geom {mesh}: plane 1 touches no hull vertex")
    a = adr.copy(); a[0] = 1
    rejected(planes, a, "plane_adr must start at 0")
    assert L.so101_tree_set_hull_planes(h, None, None) == -1 and L.so101_tree_set_hull_planes(None, None, None) == -1
    assert call() == -4                                # nothing was accepted so far
    sim.sim.set_hull_planes(planes, adr)
    assert call() == 0
    # the delayed source without a bound physics-state line; another source
    assert call(src=1) == -4 and "so101_tree_bind_physics_state" in err()
    assert call(src=2) == -1 and call(src=-1) == -1
    for bad in (dict(ncam=0), dict(ncam=9), dict(H=0), dict(W=4097), dict(n=0), dict(n=2), dict(d=None, s=None)):
        assert call(**bad) == -1, bad
    cam[0].body = sim.sim.nbody
    assert call() == -1 and f"-1 .. {sim.sim.nbody - 1}" in err()
    cam[0].body = -2
    assert call() == -1
    cam[0].body = sim.sim.nbody - 1
    assert call() == 0
    cam[0].body, cam[0].fovy_deg = 0, 180.0
    assert call() == -1
    cam[0].fovy_deg = 45.0
    assert L.so101_tree_render(None, cam, 1, 4, 4, None, 1, 0, None, None, None) == -1
    # with a line bound, source 1 is accepted
    sim.enable_env(physics_state=True, n_substeps=1, settle_max_substeps=0, physics_delay_steps=2)
    assert call(src=1) == 0
    # a handle whose state is not bound
    raw = native.TreeSim(raw32, 1, device=0, lib_path=build_emu())
    raw.set_hull_planes(planes, adr)
    assert raw.L.so101_tree_render(raw.h, cam, 1, 4, 4, None, 1, 0, depth.ctypes.data, seg.ctypes.data, None) == -4
    raw.close()


def test_emulated_render_matches_fp64_reference():
    """one env of the banana scene in the bent state, overhead_cam and wrist_cam_left at 16 x 24 (ragged: 2 x 3 tiles of 8 x 8) through the
    emulated kernels; then the same state through the delayed source"""
    raw32 = tc.blobs("banana")["f32"]
    sim = TreeArraySim(raw32, 1, backend="emu")
    sim.sim.set_hull_planes(*tc.planes("banana"))
    q = tc.STATES["bent"]
    sim.set_state(q[:, None])
    cams = tc.cams_of("banana", ["overhead_cam", "wrist_cam_left"])
    depth, seg = tc.render(sim, cams, 16, 24)
    tc.check("banana", depth[0], seg[0], q, cams, "emu bent")
    ref = tc.reference("banana")
    for cam in cams:
        assert np.isfinite(rr.reference_image(ref, "tree_banana", q, rr.cam_tuple(cam), 16, 24)[0]).any()
    np.testing.assert_array_equal(sim.get_state()[0][:, 0], q.astype(np.float32))      # the render changed no state
    # source 1 reads the first nq entries of the delayed line [n_envs][nq + nv]: begin_episode fills the line with the bound state
    sim.enable_env(physics_state=True, n_substeps=1, settle_max_substeps=0, physics_delay_steps=2)
    sim.begin_episode()
    np.testing.assert_array_equal(sim.delayed_physics_state[0, :sim.sim.nq], q.astype(np.float32))
    sim.set_state(tc.STATES["home"][:, None])
    d1, s1 = tc.render(sim, cams, 16, 24, source=1)
    assert np.array_equal(d1.view(np.int32), depth.view(np.int32)) and np.array_equal(s1, seg)
