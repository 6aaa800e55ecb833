"""Cameras of the depth / segmentation renderer (`so101_render` / `so101_tree_render`, include/so101.h;
`BatchedEnvironment.render_depth`, `AlohaEnvironment.render_depth`) and of the colour renderer on top of it (`so101_render_color` /
`so101_tree_render_color`; `render_color` of both environments, appearance.py): the same collision geometry, flat-coloured per geom and
Lambert-shaded by directional lights - not MuJoCo's renderer, no textures, shadows, specular term, visual-only meshes or positional lights.

What is rendered is the COLLISION geometry the kernels step - depth along the optical axis and the geom index per
pixel - not RGB: the reference's images come from MuJoCo's renderer with its visual meshes, materials and lights
(so100_task.py:107-112 `cameras=('overhead_cam',)`, `image_observation_enabled=True`), which this library does not
reproduce.  The camera frames are the reference's: the five `<camera>` elements of
so101_sim/assets/so100/scene_pbr.xml restated as numbers below (tests/golden/so100_cameras.json holds the values
scripts/make_golden_cameras.py parsed from that file; a test compares the two).  The ALOHA and Dining tasks have the six
cameras of so101_sim/assets/aloha/scene_pbr.xml and aloha_pbr.xml (ALOHA_CAMERAS, tests/golden/aloha_cameras.json).
"""
from __future__ import annotations

import dataclasses

import numpy as np

DEFAULT_FOVY = 45.0          # MuJoCo's default <camera fovy>, degrees

# `body` numbering (so101_camera of include/so101.h, the model's geom_dyn): -1 world, 0..5 the arm links in chain
# order, 6..7 the free props (object, container)
WORLD = -1
ARM_LINKS = ("Rotation_Pitch", "Upper_Arm", "Lower_Arm", "Wrist_Pitch_Roll", "Fixed_Jaw", "Moving_Jaw")


def frame_from_quat(quat) -> np.ndarray:
    """3 x 3 matrix (columns x, y, z) of a MuJoCo `quat` attribute (w x y z), normalised as MuJoCo's compiler does"""
    w, x, y, z = np.asarray(quat, dtype=np.float64) / np.linalg.norm(np.asarray(quat, dtype=np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def frame_from_euler(euler) -> np.ndarray:
    """3 x 3 matrix of a MuJoCo `euler` attribute in radians with the default eulerseq "xyz": rotations about the x, y and z
    axes of the rotating frame, in that order - R = Rx(e0) Ry(e1) Rz(e2)"""
    out = np.eye(3)
    for k, a in enumerate(np.asarray(euler, dtype=np.float64)):
        c, s = np.cos(a), np.sin(a)
        i, j = (k + 1) % 3, (k + 2) % 3
        r = np.eye(3)
        r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
        out = out @ r
    return out


def fovy_from_focal(focal_y: float, sensorsize_y: float) -> float:
    """Vertical field of view in degrees of a camera given by `focal` / `sensorsize` (lengths): 2 atan(sensorsize_y / (2 focal_y))"""
    return float(np.degrees(2.0 * np.arctan(sensorsize_y / (2.0 * focal_y))))


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
    body's frame, `fovy` the vertical field of view in degrees.  `body` is the number the render call takes (SO100: WORLD or the
    geom_dyn index; tree engine: the body id) or, for the tree engine, a body NAME that `with_body_ids` resolves."""
    name: str
    body: int | str = WORLD
    pos: tuple = (0.0, 0.0, 0.0)
    mat: tuple = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    fovy: float = DEFAULT_FOVY

    @classmethod
    def from_xyaxes(cls, name, body, pos, xyaxes=None, fovy=DEFAULT_FOVY, parent_pos=(0.0, 0.0, 0.0)):
        """`parent_pos`: world position of a static, unrotated parent body the camera is composed with (body = WORLD)"""
        m = np.eye(3) if xyaxes is None else frame_from_xyaxes(xyaxes)
        p = np.asarray(pos, dtype=np.float64) + np.asarray(parent_pos, dtype=np.float64)
        return cls._make(name, body, p, m, fovy)

    @classmethod
    def _make(cls, name, body, pos, mat, fovy):
        return cls(name, body if isinstance(body, str) else int(body), tuple(float(v) for v in np.asarray(pos, dtype=np.float64)),
                   tuple(tuple(float(v) for v in row) for row in np.asarray(mat, dtype=np.float64).reshape(3, 3)), float(fovy))

    @classmethod
    def from_quat(cls, name, body, pos, quat=(1.0, 0.0, 0.0, 0.0), fovy=DEFAULT_FOVY):
        """orientation as a MuJoCo `quat` attribute (w x y z)"""
        return cls._make(name, body, pos, frame_from_quat(quat), fovy)

    @classmethod
    def from_euler(cls, name, body, pos, euler=(0.0, 0.0, 0.0), fovy=DEFAULT_FOVY):
        """orientation as a MuJoCo `euler` attribute, radians, eulerseq "xyz" """
        return cls._make(name, body, pos, frame_from_euler(euler), fovy)

    def with_body_ids(self, body_names):
        """this camera with a body given by name replaced by its index in `body_names` (a model's meta["body_names"]; "world" is 0)"""
        if not isinstance(self.body, str):
            return self
        names = list(body_names)
        if self.body not in names:
            raise ValueError(f"camera {self.name!r}: the model has no body {self.body!r}")
        return dataclasses.replace(self, body=names.index(self.body))

    def spec(self):
        """(body, pos[3], mat[9] row-major, fovy_deg) as native.Sim.render / native.TreeSim.render take it"""
        if isinstance(self.body, str):
            raise ValueError(f"camera {self.name!r}: body {self.body!r} is a name, resolve it with with_body_ids(meta['body_names'])")
        return self.body, tuple(self.pos), tuple(np.asarray(self.mat, dtype=np.float64).reshape(9)), self.fovy


_TABLE_POS = (0.0, 0.0, 0.4)          # scene_pbr.xml:132 <body name="table" pos="0 0 0.4">, static and unrotated

SO100_CAMERAS = {c.name: c for c in (
    Camera.from_xyaxes("overhead_cam", WORLD, (0.0, -0.2, 1.0)),                                              # scene_pbr.xml:70
    Camera.from_xyaxes("worms_eye_cam", WORLD, (0.0, 0.0, 0.1)),                                              # scene_pbr.xml:71
    Camera.from_xyaxes("wrist_cam", ARM_LINKS.index("Fixed_Jaw"), (0.0, 0.02, 0.04), (1, 0, 0, 0, -0.5, 0.87), fovy=70.0),      # scene_pbr.xml:113
    Camera.from_xyaxes("side_cam", WORLD, (0.4, -0.3, 0.2), (0.6, 0.8, 0, -0.32, 0.24, 0.92), parent_pos=_TABLE_POS),           # scene_pbr.xml:138
    Camera.from_xyaxes("front_cam", WORLD, (0.0, -0.45, 0.5), (1, 0, 0, 0, 0.707, 0.707), parent_pos=_TABLE_POS),               # scene_pbr.xml:139
)}


# ---- ALOHA hand-over and Dining scenes.  The six cameras state `focal` / `sensorsize` (a D405: focal 1.93 mm, sensor 3.896 x 2.140 mm) or
# nothing; this renderer has square pixels and one vertical field of view, fovy = 2 atan(sensorsize_y / (2 focal_y)) = 58.008 degrees
# (DESIGN.md lists the consequence for the horizontal extent as a deviation).  Bodies by name: AlohaEnvironment resolves them.
ALOHA_FOVY = fovy_from_focal(1.93e-3, 2140e-6)
ALOHA_TABLE_HEIGHT_OFFSET = 0.011                              # aloha2_task.py:107; the model blobs are compiled for it
WRIST_CAMERA_POSITION = (-0.011, -0.0814748, -0.0095955)       # aloha2_task.py:72-76, set on both wrist cameras (aloha2_task.py:217-221)

ALOHA_CAMERAS = {c.name: c for c in (
    Camera.from_quat("overhead_cam", WORLD, (0.0, -0.303794, 1.02524), (0.976332, 0.216277, 0, 0), fovy=ALOHA_FOVY),                  # scene_pbr.xml:74-75
    # lifted with the table (aloha2_task.py:504-507)
    Camera.from_quat("worms_eye_cam", WORLD, (0.0, -0.377167, 0.0506055 + ALOHA_TABLE_HEIGHT_OFFSET), (0.672659, 0.739953, 0, 0), fovy=ALOHA_FOVY),      # scene_pbr.xml:76-77
    Camera.from_xyaxes("teleoperator_pov", WORLD, (0.0, -1.354, 0.685), (1, 0, 0, 0, 0.2, 0.8)),                                     # aloha_pbr.xml:122
    Camera.from_xyaxes("collaborator_pov", WORLD, (0.0, 1.5, 0.8), (-1, 0, 0, 0, -0.2, 0.8)),                                        # aloha_pbr.xml:123
    Camera.from_euler("wrist_cam_left", "left/gripper_base", WRIST_CAMERA_POSITION, (2.70525955359, 0, 0), fovy=ALOHA_FOVY),          # aloha_pbr.xml:165-173
    Camera.from_euler("wrist_cam_right", "right/gripper_base", WRIST_CAMERA_POSITION, (2.70525955359, 0, 0), fovy=ALOHA_FOVY),        # aloha_pbr.xml:249-257
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
