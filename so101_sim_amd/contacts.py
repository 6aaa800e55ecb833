"""Geom groups and report types of the contact interface (`so101_contacts`, include/so101.h; `BatchedEnvironment.contacts`,
`touch`, `geom_group`; `env.physics.data.contact` / `.ncon` of the single-env facade).

The reference's tasks ask "does any geom of A touch any geom of B" by looping over `physics.data.contact`
(`_touching(geoms_a, geoms_b)`, so100_hand_over.py:291-313).  Here a set of geoms is a `GeomGroup` - a 128-bit mask, one bit per
geom id - and the question is answered per env on the GPU for up to 16 pairs of groups per call.  The scene's own groups come
from the model blob (`so100_groups`), so they move with the model.

Limits: the SO100 engine only; an env reports at most `so101_max_contacts()` = 64 contacts (more: one per touching geom pair,
`flags` bit 128); forces are those of a forward pass at the current state, not the impulses of the last substep.
"""
from __future__ import annotations

import collections
import dataclasses
import fnmatch

import numpy as np

from .cameras import ARM_LINKS

MAX_GEOMS = 128                    # bits of a group mask (so101_geom_pair)
MAX_PAIRS = 16                     # SO101_TOUCH_MAX_PAIRS
FLAG_CANDIDATE_OVERFLOW, FLAG_CONTACT_OVERFLOW, FLAG_CONTACTS_REDUCED = 1, 2, 128
_PAD_GROUPS = {"fixed_jaw_pads": "fixed_jaw_pad_*", "moving_jaw_pads": "moving_jaw_pad_*"}

ContactReport = collections.namedtuple("ContactReport", "count flags geom dist pos frame force")
ContactReport.__doc__ = """BatchedEnvironment.contacts(): count [n] int32, flags [n] int32, geom [n, C, 2] int32 (-1 beyond count), dist [n, C] (+inf
beyond count), pos [n, C, 3], frame [n, C, 3, 3] (rows: normal geom1 -> geom2, tangent 1, tangent 2), force [n, C, 6] or None; C = 64"""
TouchReport = collections.namedtuple("TouchReport", "count touching dist normal_force force")
TouchReport.__doc__ = """BatchedEnvironment.touch(): count [n, npair] int32, touching [n, npair] bool, dist [n, npair] (minimum, +inf without a contact),
normal_force [n, npair] and force [n, npair, 3] (world frame, ON the pair's first group) or None without forces"""


@dataclasses.dataclass(frozen=True)
class GeomGroup:
    """A named set of geom ids."""
    name: str
    geoms: tuple

    def __post_init__(self):
        g = tuple(sorted({int(x) for x in self.geoms}))
        if not g:
            raise ValueError(f"geom group {self.name!r} is empty")
        if g[0] < 0 or g[-1] >= MAX_GEOMS:
            raise ValueError(f"geom group {self.name!r}: geom ids must be 0 .. {MAX_GEOMS - 1}, got {g[0]} .. {g[-1]}")
        object.__setattr__(self, "geoms", g)

    def mask(self) -> tuple:
        """the four 32-bit words of so101_geom_pair: bit (g & 31) of word g >> 5"""
        w = [0, 0, 0, 0]
        for g in self.geoms:
            w[g >> 5] |= 1 << (g & 31)
        return tuple(w)

    def __or__(self, other):
        return GeomGroup(f"{self.name}|{other.name}", self.geoms + other.geoms)


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


def resolve(spec, groups: dict, meta: dict) -> GeomGroup:
    """spec -> GeomGroup: a GeomGroup, the name of a group (the body names among them), a geom name, an fnmatch pattern over the
    geom names, or an iterable of geom ids"""
    if isinstance(spec, GeomGroup):
        return spec
    geom_names = list(meta["geom_names"])
    if isinstance(spec, str):
        if spec in groups:
            return groups[spec]
        if spec in geom_names:
            return GeomGroup(spec, (geom_names.index(spec),))
        hit = [g for g, n in enumerate(geom_names) if fnmatch.fnmatchcase(n, spec)]
        if hit:
            return GeomGroup(spec, hit)
        raise ValueError(f"unknown geom group {spec!r}: the scene has the groups {sorted(groups)} and the geoms {geom_names}")
    try:
        ids = [int(g) for g in spec]
    except (TypeError, ValueError):
        raise ValueError(f"unknown geom group {spec!r}: give a group, geom or body name, a pattern over geom names, geom ids or a GeomGroup") from None
    if not ids or min(ids) < 0 or max(ids) >= len(geom_names):
        raise ValueError(f"unknown geom group {spec!r}: geom ids must be 0 .. {len(geom_names) - 1} and at least one")
    return GeomGroup("geoms" + "_".join(str(g) for g in sorted(set(ids))), ids)


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
