"""Geom groups and report types of the contact interface (`so101_contacts`, include/so101.h; `BatchedEnvironment.contacts`,
`touch`, `geom_group`; `env.physics.data.contact` / `.ncon` of the single-env facade).

The reference's tasks ask "does any geom of A touch any geom of B" by looping over `physics.data.contact`
(`_touching(geoms_a, geoms_b)`, so100_hand_over.py:291-313).  Here a set of geoms is a `GeomGroup` - a 128-bit mask, one bit per
geom id - and the question is answered per env on the GPU for up to 16 pairs of groups per call.  The scene's own groups come
from the model blob (`so100_groups`), so they move with the model.

The general-tree engine (ALOHA hand-over, Dining; `so101_tree_contacts`, `AlohaEnvironment.contacts` / `touch` / `geom_group`) takes
256-bit masks - `GeomGroup(name, geoms, limit=TREE_MAX_GEOMS).mask(words=8)` - and its scene groups come from `aloha_groups`.

Limits: an SO100 env reports at most `so101_max_contacts()` = 64 contacts (more: one per touching geom pair, `flags` bit 128); an
ALOHA / Dining env at most 64 / 160, the list ending at the first geom pair that does not fit (`flags` bit 2).  Forces are those of a
forward pass at the current state, not the impulses of the last substep.
"""
from __future__ import annotations

import collections
import dataclasses
import fnmatch

import numpy as np

from .cameras import ARM_LINKS

MAX_GEOMS = 128                    # bits of a group mask (so101_geom_pair)
TREE_MAX_GEOMS = 256               # bits of a group mask of the general-tree engine (so101_tree_geom_pair)
MAX_PAIRS = 16                     # SO101_TOUCH_MAX_PAIRS
FLAG_CANDIDATE_OVERFLOW, FLAG_CONTACT_OVERFLOW, FLAG_CONTACTS_REDUCED = 1, 2, 128
FLAG_TREE_ROW_OVERFLOW = 4         # general-tree engine, with forces: the rows of the last contacts did not fit, those contacts report zero force
_PAD_GROUPS = {"fixed_jaw_pads": "fixed_jaw_pad_*", "moving_jaw_pads": "moving_jaw_pad_*"}

ContactReport = collections.namedtuple("ContactReport", "count flags geom dist pos frame force")
ContactReport.__doc__ = """BatchedEnvironment.contacts(): count [n] int32, flags [n] int32, geom [n, C, 2] int32 (-1 beyond count), dist [n, C] (+inf
beyond count), pos [n, C, 3], frame [n, C, 3, 3] (rows: normal geom1 -> geom2, tangent 1, tangent 2), force [n, C, 6] or None; C = 64
(AlohaEnvironment: 64 for the hand-over scenes, 160 for Dining)"""
TouchReport = collections.namedtuple("TouchReport", "count touching dist normal_force force")
TouchReport.__doc__ = """BatchedEnvironment.touch(): count [n, npair] int32, touching [n, npair] bool, dist [n, npair] (minimum, +inf without a contact),
normal_force [n, npair] and force [n, npair, 3] (world frame, ON the pair's first group) or None without forces"""


@dataclasses.dataclass(frozen=True)
class GeomGroup:
    """A named set of geom ids below `limit`: 128 (the default, the SO100 engine's so101_geom_pair) or TREE_MAX_GEOMS = 256 (the
    general-tree engine's so101_tree_geom_pair)."""
    name: str
    geoms: tuple
    limit: int = MAX_GEOMS

    def __post_init__(self):
        g = tuple(sorted({int(x) for x in self.geoms}))
        if not g:
            raise ValueError(f"geom group {self.name!r} is empty")
        if self.limit not in (MAX_GEOMS, TREE_MAX_GEOMS):
            raise ValueError(f"geom group {self.name!r}: limit must be {MAX_GEOMS} or {TREE_MAX_GEOMS}")
        if g[0] < 0 or g[-1] >= self.limit:
            raise ValueError(f"geom group {self.name!r}: geom ids must be 0 .. {self.limit - 1}, got {g[0]} .. {g[-1]}")
        object.__setattr__(self, "geoms", g)

    def mask(self, words: int = 4) -> tuple:
        """`words` 32-bit words, bit (g & 31) of word g >> 5: the four of so101_geom_pair (default) or the eight of so101_tree_geom_pair"""
        if words not in (4, 8):
            raise ValueError("a group mask has 4 or 8 words")
        if self.geoms[-1] >= 32 * words:
            raise ValueError(f"geom group {self.name!r}: geom {self.geoms[-1]} does not fit a mask of {words} words")
        w = [0] * words
        for g in self.geoms:
            w[g >> 5] |= 1 << (g & 31)
        return tuple(w)

    def __or__(self, other):
        return GeomGroup(f"{self.name}|{other.name}", self.geoms + other.geoms, max(self.limit, other.limit))


def so100_groups(meta: dict, model: dict) -> dict:
    """The geom groups of an SO100 scene from its blob (`scenes.load_blob` gives `meta`, `blob.unpack` the arrays): one per body
    name with at least one geom; "fixed_jaw_pads" / "moving_jaw_pads" (the pad geoms, by their names); "gripper" (Fixed_Jaw and
    Moving_Jaw); "arm" (the six links); "props" (object and container)."""
    geom_names, body_names = list(meta["geom_names"]), list(meta["body_names"])
    geom_body = [int(b) for b in np.asarray(model["geom_body"]).ravel()]
    groups = {}
    for b, name in enumerate(body_names):
        gs = [g for g, gb in enumerate(geom_body) if gb == b]
        if gs:
            groups[name] = GeomGroup(name, gs)
    for name, pattern in _PAD_GROUPS.items():
        groups[name] = GeomGroup(name, [g for g, n in enumerate(geom_names) if fnmatch.fnmatchcase(n, pattern)])
    union = lambda name, bodies: GeomGroup(name, [g for b in bodies for g in groups[b].geoms])
    arm = [body_names[int(b)] for b in np.asarray(model["arm_body"]).ravel()]
    if tuple(arm) != tuple(ARM_LINKS):
        raise ValueError(f"the model's arm links are {arm}, expected {list(ARM_LINKS)}")
    groups["gripper"] = union("gripper", ("Fixed_Jaw", "Moving_Jaw"))
    groups["arm"] = union("arm", arm)
    props = [body_names[int(np.asarray(model[k]).ravel()[0])] for k in ("task_object_body", "task_container_body")]
    groups["props"] = union("props", props)
    return groups


def aloha_groups(meta: dict, model: dict) -> dict:
    """The geom groups of an ALOHA hand-over or Dining scene from its blob (`scenes.load_aloha_blob` / `load_dining_blob` give `meta`,
    `blob.unpack` the arrays), 256-bit groups of the general-tree engine:
      one per body name with at least one geom ("world" and "table" among them);
      "left_arm" / "right_arm": the bodies left/* / right/*;  "arms": both;
      "left_gripper" / "right_gripper": the geoms of left/gripper_link / right/gripper_link and of every body below it (the fingers);
      "grippers": both;  "object", "container": the task's two props;  "props": every free body (six in Dining).
    "object", "container", "left_gripper" and "right_gripper" are exactly the geoms with bit 1, 2, 4, 8 of the blob's task_geom_class
    (what the contact rewards of the step test) wherever the blob carries that bit - the hand-over blobs carry all four, the Dining blobs
    1 and 2 only, where the gripper groups come from the body tree alone.  A group that would be empty (the bare-arm blob has no props)
    is left out.  The task groups own their names: Dining has a prop body named "container" (the white cup), which is the task's
    container in the pen task only - in the other Dining tasks that body's group is filed as "container_body"."""
    body_names = list(meta["body_names"])
    geom_body = [int(b) for b in np.asarray(model["geom_body"]).ravel()]
    parent = [int(b) for b in np.asarray(model["body_parent"]).ravel()]
    jnttype = [int(t) for t in np.asarray(model["body_jnttype"]).ravel()]
    of_bodies = lambda bodies: [g for g, gb in enumerate(geom_body) if gb in bodies]
    groups = {}

    def add(name, geoms):
        if geoms:
            groups[name] = GeomGroup(name, geoms, TREE_MAX_GEOMS)

    for b, name in enumerate(body_names):
        add(name, of_bodies({b}))

    def below(root):            # the body `root` and every body under it (bodies are numbered parents first)
        keep = {root}
        for b in range(root + 1, len(parent)):
            if parent[b] in keep:
                keep.add(b)
        return keep

    for side in ("left", "right"):
        add(f"{side}_arm", of_bodies({b for b, n in enumerate(body_names) if n.startswith(side + "/")}))
        link = f"{side}/gripper_link"
        if link in body_names:
            add(f"{side}_gripper", of_bodies(below(body_names.index(link))))
    union = lambda name, parts: add(name, [g for p in parts if p in groups for g in groups[p].geoms])
    union("arms", ("left_arm", "right_arm"))
    union("grippers", ("left_gripper", "right_gripper"))
    for name, key in (("object", "task_object_body"), ("container", "task_container_body")):
        b = int(np.asarray(model[key]).ravel()[0]) if key in model and np.asarray(model[key]).size else 0
        if b > 0:
            if name in groups and body_names[b] != name:          # (Dining has a prop NAMED container, the receptacle of the pen task only)
                groups[name + "_body"] = GeomGroup(name + "_body", groups[name].geoms, TREE_MAX_GEOMS)
            add(name, of_bodies({b}))
    add("props", of_bodies({b for b, t in enumerate(jnttype) if t == 2}))            # (2: a free joint, TJ_FREE of csrc/so101_tree.hpp)
    cls = np.asarray(model["task_geom_class"]).ravel() if "task_geom_class" in model else np.zeros(0, dtype=np.int64)
    for bit, name in ((1, "object"), (2, "container"), (4, "left_gripper"), (8, "right_gripper")):
        marked = tuple(g for g, c in enumerate(cls) if int(c) & bit)
        if marked and (name not in groups or groups[name].geoms != marked):
            raise ValueError(f"group {name!r} from the body tree {groups[name].geoms if name in groups else ()} is not the blob's task_geom_class bit {bit} {marked}")
    return groups


def resolve(spec, groups: dict, meta: dict, limit: int = MAX_GEOMS) -> GeomGroup:
    """spec -> GeomGroup: a GeomGroup, the name of a group (the body names among them), a geom name, an fnmatch pattern over the
    geom names, or an iterable of geom ids.  Geom names need not be unique - the ALOHA model has `vx300s_8_custom_finger_left` once
    per arm: a geom name, like a pattern, resolves to ALL geoms that carry it.  `limit`: the id limit of the groups made here."""
    if isinstance(spec, GeomGroup):
        return spec
    geom_names = list(meta["geom_names"])
    if isinstance(spec, str):
        if spec in groups:
            return groups[spec]
        if spec in geom_names:
            return GeomGroup(spec, [g for g, n in enumerate(geom_names) if n == spec], limit)
        hit = [g for g, n in enumerate(geom_names) if fnmatch.fnmatchcase(n, spec)]
        if hit:
            return GeomGroup(spec, hit, limit)
        raise ValueError(f"unknown geom group {spec!r}: the scene has the groups {sorted(groups)} and the geoms {geom_names}")
    try:
        ids = [int(g) for g in spec]
    except (TypeError, ValueError):
        raise ValueError(f"unknown geom group {spec!r}: give a group, geom or body name, a pattern over geom names, geom ids or a GeomGroup") from None
    if not ids or min(ids) < 0 or max(ids) >= len(geom_names):
        raise ValueError(f"unknown geom group {spec!r}: geom ids must be 0 .. {len(geom_names) - 1} and at least one")
    return GeomGroup("geoms" + "_".join(str(g) for g in sorted(set(ids))), ids, limit)


class ContactRecord:
    """One entry of `physics.data.contact`: geom1, geom2, dist, pos [3], frame [9] (numpy float64), as MuJoCo's mjContact names them"""
    __slots__ = ("geom1", "geom2", "dist", "pos", "frame", "geom")

    def __init__(self, geom1, geom2, dist, pos, frame):
        self.geom1, self.geom2, self.dist, self.pos, self.frame = int(geom1), int(geom2), float(dist), pos, frame
        self.geom = np.array([self.geom1, self.geom2], dtype=np.int32)

    def __repr__(self):
        return f"ContactRecord(geom1={self.geom1}, geom2={self.geom2}, dist={self.dist:.6g})"


def records(report: ContactReport, entry: int = 0) -> list:
    """the contacts of one entry of a ContactReport as a list of ContactRecord (host copy)"""
    n = int(report.count[entry])
    if n <= 0:
        return []
    geom = report.geom[entry, :n].cpu().numpy()
    dist = report.dist[entry, :n].cpu().numpy().astype(np.float64)
    pos = report.pos[entry, :n].cpu().numpy().astype(np.float64)
    frame = report.frame[entry, :n].cpu().numpy().astype(np.float64).reshape(n, 9)
    return [ContactRecord(geom[k, 0], geom[k, 1], dist[k], pos[k], frame[k]) for k in range(n)]


class ContactSensing:
    """Contact sensing shared by the batched environments (`BatchedEnvironment` of env.py on the SO100 engine, `AlohaEnvironment` of aloha.py
    on the general-tree engine), on the pattern of tool_control.ToolControl: output allocation and argument handling of `contacts` and `touch`.

    An environment supplies `_geom_groups()` (the scene's groups: so100_groups / aloha_groups), `_geom_limit` (the id limit of its group
    masks, MAX_GEOMS or TREE_MAX_GEOMS) and `_contact_capacity` (contacts per entry), and keeps its own public `geom_group` / `contacts` /
    `touch` with their documentation; `self.sim` has contacts (native.Sim, native.TreeSim), `_env_index` comes from ToolControl."""

    def _geom_group(self, spec) -> GeomGroup:
        return resolve(spec, self._geom_groups(), self.meta, limit=self._geom_limit)

    def _contacts(self, env_ids, forces) -> ContactReport:
        from . import native
        torch = self.torch
        idx, n = self._env_index(env_ids)
        C = self._contact_capacity
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
        rep = ContactReport(e(n, dt=torch.int32), e(n, dt=torch.int32), e(n, C, 2, dt=torch.int32), e(n, C), e(n, C, 3), e(n, C, 3, 3),
                            e(n, C, 6) if forces else None)
        out = native.ContactOut(**{k: (t.data_ptr() if t is not None else None) for k, t in rep._asdict().items()})
        self.sim.contacts(idx.data_ptr() if idx is not None else None, n, forces, None, out, self._stream())
        return rep

    def _touch(self, pairs, env_ids, forces) -> TouchReport:
        from . import native
        torch = self.torch
        pairs = list(pairs)
        if not 1 <= len(pairs) <= MAX_PAIRS:
            raise ValueError(f"touch takes 1 .. {MAX_PAIRS} pairs, got {len(pairs)}")
        words = self._geom_limit // 32
        masks = [(self.geom_group(a).mask(words), self.geom_group(b).mask(words)) for a, b in pairs]
        idx, n = self._env_index(env_ids)
        P = len(masks)
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
        count, dist = e(n, P, dt=torch.int32), e(n, P)
        normal, force = (e(n, P), e(n, P, 3)) if forces else (None, None)
        out = native.ContactOut(pair_count=count.data_ptr(), pair_dist=dist.data_ptr(), pair_normal=normal.data_ptr() if forces else None,
                                pair_force=force.data_ptr() if forces else None)
        self.sim.contacts(idx.data_ptr() if idx is not None else None, n, forces, masks, out, self._stream())
        return TouchReport(count, count > 0, dist, normal, force)
