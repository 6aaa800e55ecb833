"""Appearance of the colour cameras (`so101_render_color` / `so101_tree_render_color`, include/so101.h;
`BatchedEnvironment.render_color`, `AlohaEnvironment.render_color`): one flat colour per geom and the lights.

What is rendered is the COLLISION geometry the kernels step, flat-coloured per geom and Lambert-shaded by directional lights -
not MuJoCo's renderer: no textures, shadows, specular term, visual-only meshes or positional lights (cameras.py says the same
of `render_depth`).  The numbers below restate what the reference's scene files give: the `rgba` of the geoms and materials of
so101_sim/assets/so100/scene_pbr.xml and the `<light>` / `<headlight>` elements of that file and of
so101_sim/assets/aloha/scene_pbr.xml, each light taken as a directional light along its `dir`.  Where a scene file gives a
texture or nothing (the ALOHA arms and table, the props), a flat colour is chosen here.  Numbers only, as cameras.SO100_CAMERAS
does it: the model blobs and their meta are untouched.
"""
from __future__ import annotations

import collections
import dataclasses
import fnmatch

import numpy as np

from . import contacts as _contacts

MAX_LIGHTS = 4               # SO101_MAX_LIGHTS of include/so101.h
DEFAULT_RGB = (0.5, 0.5, 0.5)          # a geom no table entry names (MuJoCo's default geom rgba)

# what render_color returns: tensors on the env's device, rgb uint8 [n, ncam, H, W, 3], normal float32 [n, ncam, H, W, 3] (world frame, unit,
# 0 where the ray hits nothing), depth float32 / seg int32 [n, ncam, H, W] as render_depth gives them; all but rgb None unless asked for
ColorImages = collections.namedtuple("ColorImages", "rgb normal depth seg")


@dataclasses.dataclass(frozen=True)
class Light:
    """A directional light: `dir` the unit world direction it travels, or None for a headlight (the camera's viewing direction)"""
    dir: tuple | None
    diffuse: tuple = (0.7, 0.7, 0.7)          # MuJoCo's default <light diffuse>

    @classmethod
    def along(cls, direction, diffuse=(0.7, 0.7, 0.7)):
        d = np.asarray(direction, dtype=np.float64)
        return cls(tuple(float(x) for x in d / np.linalg.norm(d)), tuple(float(x) for x in diffuse))


@dataclasses.dataclass(frozen=True)
class Shading:
    """rgb = colour * (ambient + sum over the lights of diffuse * max(0, -normal . dir)), clamped to [0, 1]; `background` where a ray hits nothing"""
    ambient: tuple = (0.0, 0.0, 0.0)
    background: tuple = (0.0, 0.0, 0.0)
    lights: tuple = ()

    def __post_init__(self):
        if len(self.lights) > MAX_LIGHTS:
            raise ValueError(f"at most {MAX_LIGHTS} lights, got {len(self.lights)}")

    def spec(self):
        """(ambient, background, [(dir or None, diffuse)]) as native.shading_struct takes it"""
        return tuple(self.ambient), tuple(self.background), [(l.dir, tuple(l.diffuse)) for l in self.lights]

    def background_bytes(self) -> np.ndarray:
        return to_bytes(np.asarray(self.background, dtype=np.float32))


def to_bytes(v) -> np.ndarray:
    """the kernel's conversion of colour values to bytes: (uint8)(255 clamp(v, 0, 1) + 0.5)"""
    return (255.0 * np.clip(np.asarray(v, dtype=np.float64), 0.0, 1.0) + 0.5).astype(np.uint8)


# MuJoCo's default <headlight>: ambient 0.1, diffuse 0.4 (its specular term is not rendered)
_HEADLIGHT_AMBIENT, _HEADLIGHT_DIFFUSE = 0.1, 0.4

# so100/scene_pbr.xml:72-73: light1 straight down with ambient 0.3 (diffuse: the default 0.7), light2 along (-1, -1, -1) / sqrt 3 with diffuse
# 0.4; plus the default headlight.  The ambient terms of all lights add up.
SO100_SHADING = Shading(ambient=(0.3 + _HEADLIGHT_AMBIENT,) * 3, background=(0.0, 0.0, 0.0),
                        lights=(Light.along((0, 0, -1)), Light.along((-0.57735, -0.57735, -0.57735), (0.4, 0.4, 0.4)),
                                Light(None, (_HEADLIGHT_DIFFUSE,) * 3)))
# aloha/scene_pbr.xml:23 <headlight diffuse="0.6 0.6 0.6" ambient="0.6 0.6 0.6">; the scene's two <light> elements are commented out
ALOHA_SHADING = Shading(ambient=(0.6, 0.6, 0.6), background=(0.0, 0.0, 0.0), lights=(Light(None, (0.6, 0.6, 0.6)),))

ORANGE, BLACK = (1.0, 0.331, 0.0), (0.1, 0.1, 0.1)          # so100/scene_pbr.xml:46-47, the arm's two materials
_BANANA, _PEN, _WHITE = (0.95, 0.85, 0.2), (0.1, 0.2, 0.8), (0.85, 0.85, 0.9)

# (geom group spec, rgb) in order, later entries override.  The links carry the orange material (their collision meshes are the
# orange visual meshes; the black motors have no collision geometry), the jaw pads the black one.
SO100_COLOR_TABLE = (
    ("floor", (0.3, 0.3, 0.3)),                        # scene_pbr.xml:69
    ("Base", ORANGE), ("Rotation_Pitch", ORANGE), ("Upper_Arm", ORANGE), ("Lower_Arm", ORANGE), ("Wrist_Pitch_Roll", ORANGE),
    ("Fixed_Jaw_Collision_*", ORANGE), ("Moving_Jaw_Collision_*", ORANGE),
    ("fixed_jaw_pad_*", BLACK), ("moving_jaw_pad_*", BLACK),
    ("table_surface", (0.8, 0.6, 0.4)), ("table_leg_*", (0.8, 0.6, 0.4)),          # scene_pbr.xml:133-137
    ("banana", (1.0, 1.0, 0.0)),                       # scene_pbr.xml:142, the static capsule
    ("bowl", (0.0, 0.5, 1.0)),                         # scene_pbr.xml:145, the static cylinder
    ("container/*", _WHITE),
)
_SO100_OBJECT = {"banana": _BANANA, "pen": _PEN}

_ARM = (0.15, 0.15, 0.15)
ALOHA_COLOR_TABLE = (
    ("vx300s_*", _ARM), ("geom*", BLACK),              # the arms' links; the finger pads and grips (unnamed geoms)
    ("d405_solid", (0.7, 0.7, 0.7)), ("overhead_mount", (0.4, 0.4, 0.4)), ("wormseye_mount", (0.4, 0.4, 0.4)),
    ("tablelegs", (0.4, 0.4, 0.4)), ("table", (0.6, 0.5, 0.4)),
    ("mug/*", (0.8, 0.2, 0.2)), ("pen/*", _PEN), ("banana/*", _BANANA), ("plate/*", (0.9, 0.9, 0.9)), ("bowl/*", (0.3, 0.6, 0.9)),
    ("container/*", _WHITE),
)


def color_table(meta, table, base=None, resolve=None) -> np.ndarray:
    """float32 [ngeom, 3]: `base` (DEFAULT_RGB everywhere when None) with the entries of `table` - (spec, rgb) pairs or a dict -
    applied in order.  `resolve`: spec -> contacts.GeomGroup, an environment's `geom_group`; without one a spec is a geom name, an
    fnmatch pattern over the geom names, geom ids or a GeomGroup.  A spec that matches nothing raises ValueError."""
    ngeom = len(meta["geom_names"])
    out = np.tile(np.asarray(DEFAULT_RGB, dtype=np.float32), (ngeom, 1)) if base is None else np.array(base, dtype=np.float32).reshape(ngeom, 3)
    if resolve is None:
        resolve = lambda spec: _contacts.resolve(spec, {}, meta, limit=max(ngeom, _contacts.TREE_MAX_GEOMS))
    for spec, rgb in (table.items() if isinstance(table, dict) else table):
        rgb = np.asarray(rgb, dtype=np.float32)
        if rgb.shape != (3,):
            raise ValueError(f"colour of {spec!r}: expected 3 values, got shape {rgb.shape}")
        out[list(resolve(spec).geoms)] = rgb
    return out


def _scene_colors(meta, table):
    """a scene table on a scene that may lack some of its props: entries that match no geom name are left out"""
    names = list(meta["geom_names"])
    present = [(spec, rgb) for spec, rgb in table if any(fnmatch.fnmatchcase(n, spec) for n in names)]
    return color_table(meta, present)


def so100_colors(meta) -> np.ndarray:
    """float32 [ngeom, 3] of an SO100 scene (scenes.load_blob's meta): SO100_COLOR_TABLE, and the task's object by its name"""
    obj = _SO100_OBJECT.get(str(meta.get("object_name", "")), _BANANA)
    return _scene_colors(meta, SO100_COLOR_TABLE + (("object/*", obj),))


def aloha_colors(meta) -> np.ndarray:
    """float32 [ngeom, 3] of an ALOHA hand-over or Dining scene (scenes.load_aloha_blob / load_dining_blob's meta)"""
    obj = _SO100_OBJECT.get(str(meta.get("object_name", "")), _BANANA)
    return _scene_colors(meta, ALOHA_COLOR_TABLE + (("object/*", obj),))


class ColorCameras:
    """The colour cameras shared by the batched environments (`BatchedEnvironment` of env.py, `AlohaEnvironment` of aloha.py), on the pattern
    of contacts.ContactSensing: colour and output handling of `render_color`.  An environment supplies `_scene_colors()` (its scene table as
    float32 [ngeom, 3]), `_scene_shading`, `geom_group`, `_ensure_hull_planes`, `_env_index`, and keeps its own public `render_color`."""

    def _color_tensor(self, colors):
        """`colors` of render_color -> (float32 tensor on the device, per_env)"""
        torch = self.torch
        ngeom = len(self.meta["geom_names"])
        if colors is None or isinstance(colors, dict):
            if getattr(self, "_scene_rgb", None) is None:
                self._scene_rgb = self._scene_colors()
                self._scene_rgb_dev = torch.as_tensor(self._scene_rgb, device=self.device)
            if colors is None:
                return self._scene_rgb_dev, False
            return torch.as_tensor(color_table(self.meta, colors, base=self._scene_rgb, resolve=self.geom_group), device=self.device), False
        t = torch.as_tensor(colors, dtype=torch.float32, device=self.device).contiguous()
        if tuple(t.shape) == (ngeom, 3):
            return t, False
        if tuple(t.shape) == (self.n_envs, ngeom, 3):
            return t, True
        raise ValueError(f"colors must be None, a dict, [{ngeom}, 3] or [{self.n_envs}, {ngeom}, 3], got {tuple(t.shape)}")

    def _render_color(self, cams, height, width, env_ids, colors, shading, normals, depth, segmentation, **source) -> ColorImages:
        torch = self.torch
        shading = self._scene_shading if shading is None else shading
        rgb_table, per_env = self._color_tensor(colors)
        self._ensure_hull_planes()
        idx, n = self._env_index(env_ids)
        shape = (n, len(cams), int(height), int(width))
        out = ColorImages(torch.empty(*shape, 3, dtype=torch.uint8, device=self.device),
                          torch.empty(*shape, 3, dtype=torch.float32, device=self.device) if normals else None,
                          torch.empty(*shape, dtype=torch.float32, device=self.device) if depth else None,
                          torch.empty(*shape, dtype=torch.int32, device=self.device) if segmentation else None)
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.sim.render_color([c.spec() for c in cams], height, width, ptr(idx), n, shading.spec() if isinstance(shading, Shading) else shading,
                              rgb_table.data_ptr(), per_env, ptr(out.rgb), ptr(out.normal), ptr(out.depth), ptr(out.seg), self._stream(), **source)
        return out
