"""Tool frames of the Cartesian interface (`so101_tool_pose` / `so101_tool_ik`, include/so101.h;
`BatchedEnvironment.tool_pose`, `solve_ik`, `cartesian_action`; `so101_tree_tool_pose` / `so101_tree_tool_ik` and the same three
methods of `AlohaEnvironment`).

A tool is a frame fixed to an arm link, the way a MuJoCo site is: the kernels give its world pose, its 6 x 6
Jacobian (mj_jacSite) and the joint angles that bring it to a target.  The scene's own tool, `fixed_jaw_pad`, is the
frame of the collision geom `fixed_jaw_pad_3` on `Fixed_Jaw` - the pad the fixed jaw touches a grasped object with -
read from the model blob, so it moves with the model.  The ALOHA and Dining scenes have the six tool sites of
so101_sim/assets/aloha/aloha_pbr.xml restated as numbers below (ALOHA_TOOLS; tests/golden/aloha_sites.json holds the values
scripts/make_golden_sites.py parsed from that file, a test compares the two): there a tool's body is any articulated body of the
tree, given by name.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .cameras import ARM_LINKS, frame_from_quat, frame_from_xyaxes

DEFAULT_TOOL = "fixed_jaw_pad"
_PAD_GEOM, _PAD_BODY = "fixed_jaw_pad_3", "Fixed_Jaw"


@dataclasses.dataclass(frozen=True)
class Tool:
    """A frame fixed to an arm link: `body` 0..5 (the arm links in chain order, cameras.ARM_LINKS), `pos` and `mat`
    (3 x 3, columns x, y, z) in that link's frame.  For the general-tree engine `body` is a body id of the model or a body NAME
    that `with_body_ids` resolves."""
    name: str
    body: int | str = len(ARM_LINKS) - 2
    pos: tuple = (0.0, 0.0, 0.0)
    mat: tuple = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))

    @classmethod
    def _make(cls, name, body, pos, mat):
        return cls(name, body if isinstance(body, str) else int(body), tuple(float(v) for v in np.asarray(pos, dtype=np.float64)),
                   tuple(tuple(float(v) for v in row) for row in np.asarray(mat, dtype=np.float64).reshape(3, 3)))

    @classmethod
    def from_quat(cls, name, body, pos, quat=(1.0, 0.0, 0.0, 0.0)):
        """orientation as a MuJoCo `quat` attribute (w x y z)"""
        return cls._make(name, body, pos, frame_from_quat(quat))

    @classmethod
    def from_xyaxes(cls, name, body, pos, xyaxes=None):
        """orientation as a MuJoCo `xyaxes` attribute (None: the link's own axes)"""
        return cls._make(name, body, pos, np.eye(3) if xyaxes is None else frame_from_xyaxes(xyaxes))

    def with_body_ids(self, body_names):
        """this tool with a body given by name replaced by its index in `body_names` (a model's meta["body_names"]; "world" is 0)"""
        if not isinstance(self.body, str):
            return self
        names = list(body_names)
        if self.body not in names:
            raise ValueError(f"tool {self.name!r}: the model has no body {self.body!r}")
        return dataclasses.replace(self, body=names.index(self.body))

    def spec(self):
        """(body, pos[3], mat[9] row-major) as native.Sim.tool_pose / tool_ik and native.TreeSim.tool_pose / tool_ik take it"""
        if isinstance(self.body, str):
            raise ValueError(f"tool {self.name!r}: body {self.body!r} is a name, resolve it with with_body_ids(meta['body_names'])")
        return self.body, tuple(self.pos), tuple(np.asarray(self.mat, dtype=np.float64).reshape(9))


def so100_tools(meta: dict, model: dict) -> dict:
    """The tools of an SO100 scene from its blob (`scenes.load_blob` gives `meta`, `blob.unpack` the arrays):
    {"fixed_jaw_pad": the frame of geom fixed_jaw_pad_3 on Fixed_Jaw}."""
    names = list(meta["geom_names"])
    if _PAD_GEOM not in names:
        raise ValueError(f"the model has no geom {_PAD_GEOM!r}")
    g = names.index(_PAD_GEOM)
    arm = [int(b) for b in np.asarray(model["arm_body"]).ravel()]
    body = int(np.asarray(model["geom_body"]).ravel()[g])
    if body not in arm or ARM_LINKS[arm.index(body)] != _PAD_BODY:
        raise ValueError(f"geom {_PAD_GEOM!r} is not on arm link {_PAD_BODY!r}")
    pos = np.asarray(model["geom_pos"], dtype=np.float64).reshape(-1, 3)[g]
    quat = np.asarray(model["geom_quat"], dtype=np.float64).reshape(-1, 4)[g]
    return {DEFAULT_TOOL: Tool.from_quat(DEFAULT_TOOL, arm.index(body), pos, quat)}


# ---- ALOHA hand-over and Dining scenes: the six <site> elements of aloha_pbr.xml (none states an orientation: the body's own axes).
# Bodies by name: AlohaEnvironment resolves them.
DEFAULT_ALOHA_TOOL = "left/gripper"
ALOHA_TOOLS = {t.name: t for t in (
    Tool.from_quat("left/gripper", "left/gripper_link", (0.15, 0.0, 0.0)),                     # aloha_pbr.xml:164
    Tool.from_quat("left/left_finger", "left/left_finger_link", (0.015, -0.06, 0.02)),         # aloha_pbr.xml:185
    Tool.from_quat("left/right_finger", "left/right_finger_link", (0.015, 0.06, 0.02)),        # aloha_pbr.xml:198
    Tool.from_quat("right/gripper", "right/gripper_link", (0.15, 0.0, 0.0)),                   # aloha_pbr.xml:248
    Tool.from_quat("right/left_finger", "right/left_finger_link", (0.015, -0.06, 0.02)),       # aloha_pbr.xml:269
    Tool.from_quat("right/right_finger", "right/right_finger_link", (0.015, 0.06, 0.02)),      # aloha_pbr.xml:282
)}


def resolve(tool, known: dict) -> Tool:
    """a name of `known` or a Tool -> Tool"""
    if isinstance(tool, str):
        if tool not in known:
            raise ValueError(f"unknown tool {tool!r}: the scene has {sorted(known)}")
        tool = known[tool]
    if not isinstance(tool, Tool):
        raise TypeError(f"tool must be a name or a Tool, got {type(tool).__name__}")
    return tool
