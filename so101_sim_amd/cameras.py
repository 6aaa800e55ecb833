"""Cameras of the depth / segmentation renderer (`so101_render`, include/so101.h; `BatchedEnvironment.render_depth`).

What is rendered is the COLLISION geometry the kernels step - depth along the optical axis and the geom index per
pixel - not RGB: the reference's images come from MuJoCo's renderer with its visual meshes, materials and lights
(so100_task.py:107-112 `cameras=('overhead_cam',)`, `image_observation_enabled=True`), which this library does not
reproduce.  The camera frames are the reference's: the five `<camera>` elements of
so101_sim/assets/so100/scene_pbr.xml restated as numbers below (tests/golden/so100_cameras.json holds the values
scripts/make_golden_cameras.py parsed from that file; a test compares the two).
"""
from __future__ import annotations

import dataclasses

import numpy as np

DEFAULT_FOVY = 45.0          # MuJoCo's default <camera fovy>, degrees

# `body` numbering (so101_camera of include/so101.h, the model's geom_dyn): -1 world, 0..5 the arm links in chain
# order, 6..7 the free props (object, container)
WORLD = -1
ARM_LINKS = ("Rotation_Pitch", "Upper_Arm", "Lower_Arm", "Wrist_Pitch_Roll", "Fixed_Jaw", "Moving_Jaw")


def frame_from_xyaxes(xyaxes) -> np.ndarray:
    """3 x 3 matrix with columns x (right), y (up), z of a MuJoCo `xyaxes` attribute, orthonormalised the way MuJoCo's
    compiler does: x normalised, y made orthogonal to x and normalised, z = x cross y.  The camera looks along -z."""
    a = np.asarray(xyaxes, dtype=np.float64).reshape(2, 3)
    x = a[0] / np.linalg.norm(a[0])
    y = a[1] - x * np.dot(x, a[1])
    y = y / np.linalg.norm(y)
    return np.stack([x, y, np.cross(x, y)], axis=1)


@dataclasses.dataclass(frozen=True)
class Camera:
    """A pinhole camera fixed to a body: `pos` and `mat` (3 x 3, columns x right, y up, z; looking along -z) in that
    body's frame, `fovy` the vertical field of view in degrees."""
    name: str
    body: int = WORLD
    pos: tuple = (0.0, 0.0, 0.0)
    mat: tuple = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    fovy: float = DEFAULT_FOVY

    @classmethod
    def from_xyaxes(cls, name, body, pos, xyaxes=None, fovy=DEFAULT_FOVY, parent_pos=(0.0, 0.0, 0.0)):
        """`parent_pos`: world position of a static, unrotated parent body the camera is composed with (body = WORLD)"""
        m = np.eye(3) if xyaxes is None else frame_from_xyaxes(xyaxes)
        p = np.asarray(pos, dtype=np.float64) + np.asarray(parent_pos, dtype=np.float64)
        return cls(name, int(body), tuple(float(v) for v in p), tuple(tuple(float(v) for v in row) for row in m), float(fovy))

    def spec(self):
        """(body, pos[3], mat[9] row-major, fovy_deg) as native.Sim.render takes it"""
        return self.body, tuple(self.pos), tuple(np.asarray(self.mat, dtype=np.float64).reshape(9)), self.fovy


_TABLE_POS = (0.0, 0.0, 0.4)          # scene_pbr.xml:132 <body name="table" pos="0 0 0.4">, static and unrotated

SO100_CAMERAS = {c.name: c for c in (
    Camera.from_xyaxes("overhead_cam", WORLD, (0.0, -0.2, 1.0)),                                              # scene_pbr.xml:70
    Camera.from_xyaxes("worms_eye_cam", WORLD, (0.0, 0.0, 0.1)),                                              # scene_pbr.xml:71
    Camera.from_xyaxes("wrist_cam", ARM_LINKS.index("Fixed_Jaw"), (0.0, 0.02, 0.04), (1, 0, 0, 0, -0.5, 0.87), fovy=70.0),      # scene_pbr.xml:113
    Camera.from_xyaxes("side_cam", WORLD, (0.4, -0.3, 0.2), (0.6, 0.8, 0, -0.32, 0.24, 0.92), parent_pos=_TABLE_POS),           # scene_pbr.xml:138
    Camera.from_xyaxes("front_cam", WORLD, (0.0, -0.45, 0.5), (1, 0, 0, 0, 0.707, 0.707), parent_pos=_TABLE_POS),               # scene_pbr.xml:139
)}


def resolve(camera, known=None) -> list:
    """A name, a Camera, or a sequence of either -> list of Camera (`known`: the name table, SO100_CAMERAS by default)"""
    known = SO100_CAMERAS if known is None else known
    items = [camera] if isinstance(camera, (str, Camera)) else list(camera)
    out = []
    for c in items:
        if isinstance(c, str):
            if c not in known:
                raise ValueError(f"unknown camera {c!r}: the scene has {sorted(known)}")
            c = known[c]
        if not isinstance(c, Camera):
            raise TypeError(f"camera must be a name or a Camera, got {type(c).__name__}")
        out.append(c)
    if not out:
        raise ValueError("no camera given")
    return out
