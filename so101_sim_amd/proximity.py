"""Report type and argument handling of the proximity interface (`so101_proximity`, include/so101.h; `BatchedEnvironment.proximity`).

MuJoCo answers "how far apart are these two things" with `mj_geomDistance` or a `<distance>` sensor, one geom pair at a time on the host.
Here the question is asked per env (or per arm waypoint against an env's props) and pair of geom groups on the GPU: the smallest signed
distance over the geom pairs the model's own pair list admits, with the closest points.  The groups are those of contacts.py.

Both engines answer it: `BatchedEnvironment.proximity` (SO100, `so101_proximity`: 128-bit groups, `q` the six arm joints) and
`AlohaEnvironment.proximity` (the ALOHA hand-over and Dining scenes, `so101_tree_proximity`: 256-bit groups, `q` as columns of named joints -
a tool's chain, what `solve_ik` returns, or any one-dof joints by qpos address).  One distance code runs under both
(csrc/so101_proximity_core.hpp).

Limits: distances are reported below `max_dist` (at most 10 m); a penetrating pair reports the narrowphase's contact distance, the number
`touch` gives at the same state; `q` places arm joints only, never a prop; joint equalities are not enforced on `q`."""
from __future__ import annotations

import collections
import math

import numpy as np

from .contacts import MAX_PAIRS

FLAG_PENETRATING, FLAG_ITERATION_CAP, FLAG_BEYOND, FLAG_OUTSIDE = 1, 2, 4, 8
MAX_DIST_LIMIT = 10.0

ProximityReport = collections.namedtuple("ProximityReport", "dist geom point normal flags")
ProximityReport.__doc__ = """BatchedEnvironment.proximity(): dist [n, P] float32 (signed, max_dist where nothing is nearer), geom [n, P, 2] int32 (the a-side
geom first, -1 with flags bit 4), point [n, P, 2, 3] (closest point on the a-side geom, on the b-side geom, world frame), normal [n, P, 3] (unit,
from the a point to the b point), flags [n, P] int32 (1 penetrating, 2 iteration cap: dist is an upper bound, 4 nothing within max_dist,
8 env id out of range)"""


class ProximityRecord:
    """One pair of one entry of a ProximityReport on the host: geom1, geom2 (a side, b side), dist, point1 [3], point2 [3], normal [3] (numpy
    float64), flags, and `penetrating` / `found` read from the flags"""
    __slots__ = ("geom1", "geom2", "dist", "point1", "point2", "normal", "flags")

    def __init__(self, geom, dist, point, normal, flags):
        self.geom1, self.geom2, self.dist, self.flags = int(geom[0]), int(geom[1]), float(dist), int(flags)
        self.point1, self.point2, self.normal = point[0], point[1], normal

    penetrating = property(lambda self: bool(self.flags & FLAG_PENETRATING))
    found = property(lambda self: not self.flags & FLAG_BEYOND)

    def __repr__(self):
        return f"ProximityRecord(geom1={self.geom1}, geom2={self.geom2}, dist={self.dist:.6g}, flags={self.flags})"


def records(report: ProximityReport, entry: int = 0) -> list:
    """the pairs of one entry of a ProximityReport as a list of ProximityRecord (host copy)"""
    geom = report.geom[entry].cpu().numpy()
    dist = report.dist[entry].cpu().numpy().astype(np.float64)
    point = report.point[entry].cpu().numpy().astype(np.float64)
    normal = report.normal[entry].cpu().numpy().astype(np.float64)
    flags = report.flags[entry].cpu().numpy()
    return [ProximityRecord(geom[p], dist[p], point[p], normal[p], flags[p]) for p in range(len(dist))]


class ProximitySensing:
    """Proximity sensing of a batched environment, on the pattern of contacts.ContactSensing: output allocation and argument handling of
    `proximity`.  The environment supplies `geom_group` and `_geom_limit` (ContactSensing), `_env_index` and `_joint_rows` (ToolControl), and keeps
    its own public `proximity` with its documentation; `self.sim` has proximity (native.Sim, native.TreeSim).  An environment whose `q` is a
    set of joint columns (the general-tree engine) overrides `_proximity_columns`."""

    _q_is_columns = False          # True: sim.proximity takes the qpos addresses of q's columns after q (native.TreeSim)

    def _proximity_columns(self, joints):
        """the qpos addresses of q's columns, or None where q is the engine's fixed arm (SO100: qpos[0:6])"""
        if joints is not None:
            raise ValueError("joints: this engine's q is the six arm joints, qpos[0:6]")
        return None

    def _proximity(self, pairs, env_ids, q, max_dist, queries=False, joints=None):
        from . import native
        pairs = list(pairs)
        if not 1 <= len(pairs) <= MAX_PAIRS:
            raise ValueError(f"proximity takes 1 .. {MAX_PAIRS} pairs, got {len(pairs)}")
        try:
            max_dist = float(max_dist)
        except (TypeError, ValueError):
            raise ValueError(f"max_dist must be a finite number above 0 and at most {MAX_DIST_LIMIT:g}, got {max_dist!r}") from None
        if not (math.isfinite(max_dist) and 0.0 < max_dist <= MAX_DIST_LIMIT):
            raise ValueError(f"max_dist must be a finite number above 0 and at most {MAX_DIST_LIMIT:g}, got {max_dist!r}")
        words = self._geom_limit // 32
        masks = [(self.geom_group(a).mask(words), self.geom_group(b).mask(words)) for a, b in pairs]
        torch = self.torch
        idx, n = self._env_index(env_ids)
        if q is None and joints is not None:
            raise ValueError("joints names the columns of q: it needs q")
        adr = self._proximity_columns(joints) if q is not None else None
        if q is not None:
            ncol = 6 if adr is None else len(adr)
            what = "arm joint angles" if adr is None else "joint values"
            q = self._joint_rows(q, ncol, "q")
            if q.shape[0] != n:
                raise ValueError(f"q must be [{n}, {ncol}]: one row of {what} per entry, got {tuple(q.shape)}")
        P = len(masks)
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=self.device)
        rep = ProximityReport(e(n, P), e(n, P, 2, dt=torch.int32), e(n, P, 2, 3), e(n, P, 3), e(n, P, dt=torch.int32))
        count = e(n, P, dt=torch.int32) if queries else None
        out = native.ProximityOut(queries=count.data_ptr() if queries else None, **{k: t.data_ptr() for k, t in rep._asdict().items()})
        columns = (adr,) if self._q_is_columns else ()          # (the general-tree engine's call takes the addresses after q)
        self.sim.proximity(idx.data_ptr() if idx is not None else None, n, q.data_ptr() if q is not None else None, *columns, masks, max_dist, out, self._stream())
        return (rep, count) if queries else rep
