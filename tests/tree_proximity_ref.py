"""fp64 reference of the proximity interface of the general-tree engine (so101_tree_proximity, include/so101.h): tests/proximity_ref.ProximityRef
- its GJK, its plane form, its exhaustive minimum and its algorithm-free certificate, unchanged - with the body frames of a general-tree blob
(tests/tree_raycast_ref.TreeRaycastRef.body_frames: hinge, slide and free joints) in place of the SO100 chain's.

Exhaustive over the admitted pairs of a group pair, with one exception: a group pair with more than CULL_ABOVE members (arms | props: 1 824 in
the hand-over blob) skips a member whose fp64 bounding-sphere gap (geom_center, geom_rbound) already exceeds the best distance found so far, or
max_dist.  The true distance of two geoms is at least the gap of their bounding spheres, so a skipped member cannot be the minimum; the members
are visited in the order of their gaps, the result carries how many were skipped."""
from __future__ import annotations

import numpy as np

from tests.proximity_ref import ProximityRef, in_mask
from tests.tree_raycast_ref import TreeRaycastRef

CULL_ABOVE = 1000


class TreeProximityRef(ProximityRef):
    def __init__(self, blob_f64: bytes):
        super().__init__(blob_f64)
        self.rc = TreeRaycastRef(blob_f64)              # (poses() asks self.rc for the body frames)
        self.nq = self.rc.nq

    def onedof_addresses(self):
        """qpos addresses of the hinge and slide joints, in qpos order"""
        return sorted(int(self.rc.qadr[b]) for b in range(len(self.rc.par)) if int(self.rc.jtype[b]) in (1, 3))

    def sphere_gap(self, g1, g2, poses):
        c1 = poses[g1][1] + poses[g1][0] @ self.rc.gcenter[g1]
        c2 = poses[g2][1] + poses[g2][0] @ self.rc.gcenter[g2]
        return float(np.linalg.norm(c2 - c1) - self.rc.grbound[g1] - self.rc.grbound[g2])

    def query(self, qpos, mask_a, mask_b, max_dist, cache=None):
        mask_a, mask_b = [int(w) for w in mask_a], [int(w) for w in mask_b]
        members = self.members(mask_a, mask_b)
        if len(members) <= CULL_ABOVE:
            out = super().query(qpos, mask_a, mask_b, max_dist, cache)
            out.update(members=len(members), skipped=0)
            return out
        poses = self.poses(qpos)
        cache = {} if cache is None else cache
        gaps = [self.sphere_gap(g1, g2, poses) for g1, g2, _ in members]
        best, pen, table, skipped = None, [], {}, 0
        for k in np.argsort(gaps, kind="stable"):
            g1, g2, sw = members[int(k)]
            if gaps[int(k)] > (best["dist"] if best is not None else max_dist):
                skipped += 1
                continue
            if (g1, g2) not in cache:
                cache[(g1, g2)] = self.pair(g1, g2, poses)
            r = cache[(g1, g2)]
            key = (g2, g1) if sw else (g1, g2)
            if r is None:
                pen.append(key)
                continue
            d, pa, pb, n = r
            table[key] = d
            order = members.index((g1, g2, sw))
            if d < max_dist and (best is None or d < best["dist"] or (d == best["dist"] and order < best["order"])):
                best = dict(dist=d, geom=key, pa=pb if sw else pa, pb=pa if sw else pb, n=-n if sw else n, order=order)
        out = best if best is not None else dict(dist=None, geom=(-1, -1), pa=None, pb=None, n=None)
        out.update(penetrating=pen, table=table, poses=poses, members=len(members), skipped=skipped)
        return out

    def pair_distance(self, ga, gb, poses):
        """distance of one geom pair given a side first (None: touching), for a winner the culled table does not hold"""
        for g1, g2 in ((ga, gb), (gb, ga)):
            if (g1, g2) in self._pair_set():
                r = self.pair(g1, g2, poses)
                return None if r is None else r[0]
        raise KeyError((ga, gb))

    def _pair_set(self):
        if not hasattr(self, "_pairs"):
            self._pairs = set(self.pairs)
        return self._pairs


__all__ = ["TreeProximityRef", "in_mask", "CULL_ABOVE"]
