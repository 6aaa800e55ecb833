"""Colour cameras without a GPU: one small so101_render_color / so101_tree_render_color through the emulated builds of the kernel source
(tests/hostemu) against the fp64 reference of tests/shade_ref.py, the library's argument checks, and the appearance tables."""
import ctypes as C
import fnmatch

import numpy as np
import pytest

from so101_sim_amd import appearance, cameras, native
from so101_sim_amd.model import scenes
from tests import raycast_ref as rr
from tests import shade_cases as sc
from tests import tree_render_cases as tc
from tests.render_cases import JAW_CAM, render, scene_planes
from tests.simharness import ArraySim, TreeArraySim


def test_emulated_color_render_matches_fp64_reference(blobs):
    """one env in the grasp state, overhead_cam and the jaw camera at 16 x 24 (ragged: 2 x 3 tiles of 8 x 8) through the emulated kernels"""
    ref = rr.RaycastRef(blobs["f64"])
    sim = ArraySim(blobs["f32"], 1, backend="emu")
    sim.sim.set_hull_planes(*scene_planes(blobs["f32"]))
    q = rr.STATES["grasp"]
    sim.set_state(q[:, None])
    cams = [cameras.SO100_CAMERAS["overhead_cam"], JAW_CAM]
    colors = appearance.so100_colors(blobs["meta"])
    out = sc.render_color(sim, cams, 16, 24, colors, appearance.SO100_SHADING)
    worst, counts = sc.check(ref, "banana", out, 0, q, cams, colors, appearance.SO100_SHADING, "emu grasp")
    print(f"worst |n - n64|_inf under the emulator (SO100, 2 images): {worst:.3e}")
    assert counts.sum() > 100
    # depth and seg are so101_render's, bit for bit; the other outputs do not depend on which are asked for
    depth, seg = render(sim, cams, 16, 24)
    assert np.array_equal(sc.bits(out["depth"]), sc.bits(depth)) and np.array_equal(out["seg"], seg)
    alone = sc.render_color(sim, cams, 16, 24, colors, appearance.SO100_SHADING, want=("rgb",))
    assert np.array_equal(alone["rgb"], out["rgb"])
    alone = sc.render_color(sim, cams, 16, 24, colors, appearance.SO100_SHADING, want=("normal", "seg"))
    assert np.array_equal(sc.bits(alone["normal"]), sc.bits(out["normal"])) and np.array_equal(alone["seg"], seg)
    np.testing.assert_array_equal(sim.get_state()[0][:, 0], q.astype(np.float32))      # the render changed no state


def test_emulated_tree_color_render_matches_fp64_reference():
    """the same through the general-tree engine's emulated build: one env of the hand-over scene, bent state, overhead_cam and the finger camera"""
    sim = TreeArraySim(tc.blobs("banana")["f32"], 1, backend="emu")
    sim.sim.set_hull_planes(*tc.planes("banana"))
    q = tc.STATES["bent"]
    sim.set_state(q[:, None])
    cams = tc.cams_of("banana", ["overhead_cam", tc.FINGER_CAM])
    colors = appearance.aloha_colors(tc.blobs("banana")["meta"])
    out = sc.render_color(sim, cams, 16, 24, colors, appearance.ALOHA_SHADING)
    worst, counts = sc.check(tc.reference("banana"), "tree_banana", out, 0, q, cams, colors, appearance.ALOHA_SHADING, "emu bent")
    print(f"worst |n - n64|_inf under the emulator (tree engine, 2 images): {worst:.3e}")
    assert counts.sum() > 100
    depth, seg = tc.render(sim, cams, 16, 24)
    assert np.array_equal(sc.bits(out["depth"]), sc.bits(depth)) and np.array_equal(out["seg"], seg)


def _shading(**kw):
    s = native.shading_struct(appearance.SO100_SHADING.spec())
    for k, v in kw.items():
        getattr(s, k)[:] = v
    return s


@pytest.mark.parametrize("engine", ["so100", "tree"])
def test_argument_errors(blobs, engine):
    if engine == "so100":
        sim = ArraySim(blobs["f32"], 1, backend="emu")
        planes, api, ngeom = scene_planes(blobs["f32"]), "so101_render_color", len(blobs["meta"]["geom_names"])
    else:
        sim = TreeArraySim(tc.blobs("banana")["f32"], 1, backend="emu")
        planes, api, ngeom = tc.planes("banana"), "so101_tree_render_color", sim.sim.ngeom
    L, h = sim.sim.L, sim.sim.h
    fn = getattr(L, api)
    err = (L.so101_last_error if engine == "so100" else L.so101_tree_last_error)
    cam = (native.CameraSpec * 1)()
    cam[0].body, cam[0].fovy_deg = -1, 45.0
    cam[0].pos[:], cam[0].mat[:] = [0, -0.2, 1.0], [1, 0, 0, 0, 1, 0, 0, 0, 1]
    rgb, col = np.zeros((1, 1, 4, 4, 3), np.uint8), np.full((ngeom, 3), 0.5, np.float32)
    good_out = native.ColorOut(rgb.ctypes.data, None, None, None)

    def call(ncam=1, H=4, W=4, n=1, shading=None, colors=col.ctypes.data, out=good_out, source=0):
        sh = C.byref(_shading()) if shading is None else shading
        out = C.byref(out) if out is not None else None
        head = (h, cam, ncam, H, W, None, n) + ((source,) if engine == "tree" else ())
        return fn(*head, sh, colors, 0, out, None)

    def rejected(what, status=-1, **kw):
        assert call(**kw) == status, (what, kw)
        msg = err(h).decode()
        assert msg.startswith(api + ":") and what in msg, msg

    rejected("no hull planes", status=-4)
    sim.sim.set_hull_planes(*planes)
    assert call() == 0
    # the shared arguments: so101_render's checks under the new name
    for bad in (dict(ncam=0), dict(ncam=9), dict(H=0), dict(W=4097), dict(n=0)):
        rejected("bad argument", **bad)
    rejected("n_render exceeds the envs of the handle", n=2)
    if engine == "tree":
        rejected("source must be 0", source=2)
    # the new ones
    rejected("NULL shading", shading=C.POINTER(native.ShadingSpec)())
    rejected("NULL geom_rgb", colors=None)
    rejected("NULL out", out=None)
    rejected("no output pointer at all", out=native.ColorOut(None, None, None, None))
    for nl in (-1, 5):
        s = _shading(); s.nlight = nl
        rejected("nlight must be 0 .. 4", shading=C.byref(s))
    s = _shading(); s.light[0].dir[:] = [0.0, 0.0, -1.001]
    rejected("light 0: dir is no unit vector", shading=C.byref(s))
    s = _shading(); s.light[2].dir[:] = [0.0, 0.0, 0.0]          # a headlight's dir is not read
    assert s.light[2].headlight == 1 and call(shading=C.byref(s)) == 0
    s = _shading(); s.light[1].diffuse[:] = [0.4, -0.1, 0.4]
    rejected("light 1: diffuse must be finite and >= 0", shading=C.byref(s))
    rejected("ambient must be finite and >= 0", shading=C.byref(_shading(ambient=[0.1, float("nan"), 0.1])))
    rejected("background must be finite and >= 0", shading=C.byref(_shading(background=[float("inf"), 0.0, 0.0])))
    s = _shading(); s.nlight = 0; s.light[0].dir[:] = [9.0, 9.0, 9.0]          # lights beyond nlight are not read
    assert call(shading=C.byref(s)) == 0
    cam[0].body = 99
    rejected("camera 0: body must be")
    assert fn(*((None, cam, 1, 4, 4, None, 1) + ((0,) if engine == "tree" else ())), C.byref(_shading()), col.ctypes.data, 0, C.byref(good_out), None) == -1


def test_scratch_bytes_count_the_pixel_scratch(blobs):
    """a colour render whose caller takes neither depth nor seg keeps them in the handle: 8 bytes per pixel of the largest such call,
    counted in SO101_INFO_SCRATCH_BYTES; a call that takes both needs none"""
    sim = ArraySim(blobs["f32"], 2, backend="emu")
    sim.sim.set_hull_planes(*scene_planes(blobs["f32"]))
    sim.set_state(np.tile(rr.STATES["grasp"][:, None], (1, 2)))
    cams = [cameras.SO100_CAMERAS["overhead_cam"]]
    colors = appearance.so100_colors(blobs["meta"])
    render(sim, cams, 4, 4)
    base = sim.sim.info()["scratch_bytes"]
    sc.render_color(sim, cams, 8, 12, colors, appearance.SO100_SHADING)
    assert sim.sim.info()["scratch_bytes"] == base
    sc.render_color(sim, cams, 8, 12, colors, appearance.SO100_SHADING, want=("rgb",))
    assert sim.sim.info()["scratch_bytes"] == base + 8 * 2 * 8 * 12
    sc.render_color(sim, cams, 4, 4, colors, appearance.SO100_SHADING, want=("rgb", "depth"))
    assert sim.sim.info()["scratch_bytes"] == base + 8 * 2 * 8 * 12


def test_appearance_tables():
    metas = dict(so100=scenes.load_blob("banana", "f32")[1], so100_pen=scenes.load_blob("pen", "f32")[1], aloha=scenes.load_aloha_blob("banana", "f32")[1],
                 dining=scenes.load_dining_blob("banana", "f32")[1])
    for key, meta in metas.items():
        fn = appearance.so100_colors if key.startswith("so100") else appearance.aloha_colors
        table = appearance.SO100_COLOR_TABLE if key.startswith("so100") else appearance.ALOHA_COLOR_TABLE
        col = fn(meta)
        names = list(meta["geom_names"])
        assert col.shape == (len(names), 3) and col.dtype == np.float32 and np.all((col >= 0) & (col <= 1)), key
        # every geom gets a colour from the table, none is left at the default by omission
        specs = [s for s, _ in table] + ["object/*"]
        assert all(any(fnmatch.fnmatchcase(n, s) for s in specs) for n in names), key
    for shading in (appearance.SO100_SHADING, appearance.ALOHA_SHADING):
        assert len(shading.lights) <= appearance.MAX_LIGHTS
        for l in shading.lights:
            assert l.dir is None or abs(np.linalg.norm(l.dir) - 1.0) < 1e-12
            assert all(0 <= v <= 1 for v in l.diffuse)
        assert all(0 <= v <= 1 for v in shading.ambient + shading.background)
    # what the scene files give (so100/scene_pbr.xml, aloha/scene_pbr.xml)
    meta, col = metas["so100"], appearance.so100_colors(metas["so100"])
    at = lambda name: col[list(meta["geom_names"]).index(name)].tolist()
    f32 = lambda *v: np.asarray(v, dtype=np.float32).tolist()
    assert at("table_surface") == f32(0.8, 0.6, 0.4) and all(at(f"table_leg_{k}") == f32(0.8, 0.6, 0.4) for k in range(4))
    assert at("floor") == f32(0.3, 0.3, 0.3) and at("banana") == f32(1, 1, 0) and at("bowl") == f32(0, 0.5, 1)
    for link in ("Base", "Rotation_Pitch", "Upper_Arm", "Lower_Arm", "Wrist_Pitch_Roll", "Fixed_Jaw_Collision_1", "Moving_Jaw_Collision_3"):
        assert at(link) == f32(1, 0.331, 0)
    assert at("fixed_jaw_pad_1") == f32(0.1, 0.1, 0.1) and at("moving_jaw_pad_4") == f32(0.1, 0.1, 0.1)
    s = appearance.SO100_SHADING
    assert [l.dir for l in s.lights][0] == (0.0, 0.0, -1.0) and s.lights[2].dir is None and s.ambient == (0.4, 0.4, 0.4)
    np.testing.assert_allclose(s.lights[1].dir, -np.ones(3) / np.sqrt(3), atol=1e-15)
    assert [l.diffuse for l in s.lights] == [(0.7, 0.7, 0.7), (0.4, 0.4, 0.4), (0.4, 0.4, 0.4)]
    a = appearance.ALOHA_SHADING
    assert a.ambient == (0.6, 0.6, 0.6) and len(a.lights) == 1 and a.lights[0].dir is None and a.lights[0].diffuse == (0.6, 0.6, 0.6)
    # a table: later entries override, the default is 0.5 grey, a spec that matches nothing is an error
    t = appearance.color_table(meta, [("table_*", (1, 0, 0)), ("table_leg_2", (0, 1, 0))])
    idx = lambda name: list(meta["geom_names"]).index(name)
    assert t[idx("table_surface")].tolist() == [1, 0, 0] and t[idx("table_leg_2")].tolist() == [0, 1, 0] and t[idx("floor")].tolist() == [0.5, 0.5, 0.5]
    with pytest.raises(ValueError):
        appearance.color_table(meta, {"no_such_geom": (1, 1, 1)})
    assert np.array_equal(appearance.to_bytes([0.0, 0.5, 1.0, 2.0, -1.0]), np.array([0, 128, 255, 255, 0], dtype=np.uint8))
