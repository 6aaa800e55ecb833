"""fp64 reference of the proximity interface (so101_proximity, include/so101.h), numpy on the f64 blob alone; the kernels never run here.

(a) ProximityRef.query: forward kinematics from the blob (tests/raycast_ref.py's body frames), its own GJK per geom pair with spheres and
    capsules as core plus radius, the plane in closed form, taken exhaustively over the admitted pairs of the model's pair list.  A pair
    whose cores touch or whose surfaces overlap is reported as penetrating without a distance: what the kernel reports there is the
    narrowphase's contact, which the tests compare with so101_contacts.
(b) certificate: depends on no algorithm.  For witnesses (pa, pb, n, d) of a separated geom pair it returns the largest violation of
      pa in A, pb in B (facet planes of the hull / the analytic inside test),
      |(pb - pa) - d n| = 0 and |n| = 1,
      min over B of n.y - max over A of n.x >= d (vertex extremes / analytic supports),
    which together bound d from above and from below."""
from __future__ import annotations

import itertools

import numpy as np

from so101_sim_amd.model import meshes
from tests.raycast_ref import RaycastRef

PLANE, SPHERE, CAPSULE, CYLINDER, BOX, MESH = range(6)


def in_mask(mask, g) -> bool:
    return g >= 0 and bool((int(mask[g >> 5]) >> (g & 31)) & 1)


def _closest_on_simplex(P):
    """closest point of conv(P) to the origin: (weights, point).  Every sub-simplex whose affine projection of the origin has non-negative
    weights lies in the hull; the closest of them is the answer."""
    best = None
    n = len(P)
    for k in range(1, n + 1):
        for idx in itertools.combinations(range(n), k):
            Q = P[list(idx)]
            if k == 1:
                w = np.ones(1)
            else:
                E = (Q[1:] - Q[0]).T                       # [3, k - 1]
                G = E.T @ E
                if abs(np.linalg.det(G)) < 1e-300:
                    continue
                t = np.linalg.solve(G, -E.T @ Q[0])
                w = np.r_[1.0 - t.sum(), t]
            if np.any(w < -1e-14):
                continue
            w = np.clip(w, 0.0, None)
            w = w / w.sum()
            x = w @ Q
            d2 = float(x @ x)
            if best is None or d2 < best[0]:
                full = np.zeros(n)
                full[list(idx)] = w
                best = (d2, full, x)
    return best[1], best[2]


class ProximityRef:
    def __init__(self, blob_f64: bytes):
        self.rc = RaycastRef(blob_f64)
        m = self.rc.m
        self.m = m
        self.ngeom = self.rc.ngeom
        self.gtype = [int(t) for t in m["geom_type"]]
        self.gsize = m["geom_size"].reshape(-1, 3)
        mv = m["mesh_vert"].reshape(-1, 3)
        self.verts, self.planes = {}, {}
        for g in range(self.ngeom):
            if self.gtype[g] == MESH:
                a, n = int(m["geom_vertadr"][g]), int(m["geom_vertnum"][g])
                self.verts[g] = mv[a:a + n]
        self.pairs = [(int(a), int(b)) for a, b in np.asarray(m["pair_geom"]).reshape(-1, 2)]

    def hull_planes(self, g):
        if g not in self.planes:
            self.planes[g] = meshes.hull_planes(self.verts[g])
        return self.planes[g]

    # ---- poses
    def poses(self, qpos):
        """world (R [3, 3], p [3]) of every geom at qpos [20]"""
        from tests.raycast_ref import q2m
        P, R = self.rc.body_frames(np.asarray(qpos, dtype=np.float64))
        out = []
        for g in range(self.ngeom):
            b = int(self.rc.gbody[g])
            out.append((R[b] @ q2m(self.rc.gquat[g]), P[b] + R[b] @ self.rc.gpos[g]))
        return out

    # ---- one geom
    def radius(self, g):
        return float(self.gsize[g][0]) if self.gtype[g] in (SPHERE, CAPSULE) else 0.0

    def support(self, g, pose, d, core=False):
        """world support point of geom g (its core: radius 0 for sphere and capsule) along the world direction d"""
        R, p = pose
        dl = R.T @ np.asarray(d, dtype=np.float64)
        t, s = self.gtype[g], self.gsize[g]
        if t == MESH:
            V = self.verts[g]
            loc = V[int(np.argmax(V @ dl))]
        elif t == BOX:
            loc = np.where(dl >= 0, s, -s)
        elif t in (SPHERE, CAPSULE):
            r = 0.0 if core else s[0]
            nrm = np.linalg.norm(dl)
            loc = r * dl / nrm if nrm > 0 else np.zeros(3)
            if t == CAPSULE:
                loc = loc + np.array([0, 0, s[1] if dl[2] >= 0 else -s[1]])
        elif t == CYLINDER:
            nrm = np.hypot(dl[0], dl[1])
            loc = np.array([s[0] * dl[0] / nrm, s[0] * dl[1] / nrm, 0.0]) if nrm > 0 else np.zeros(3)
            loc[2] = s[1] if dl[2] >= 0 else -s[1]
        else:
            raise ValueError("a plane has no support point")
        return p + R @ loc

    def outside(self, g, pose, x):
        """how far the world point x lies outside geom g (<= 0: inside), by the facet planes or the analytic test"""
        R, p = pose
        l = R.T @ (np.asarray(x, dtype=np.float64) - p)
        t, s = self.gtype[g], self.gsize[g]
        if t == MESH:
            E = self.hull_planes(g)
            return float(np.max(E[:, :3] @ l + E[:, 3]))
        if t == BOX:
            return float(np.max(np.abs(l) - s))
        if t == SPHERE:
            return float(np.linalg.norm(l) - s[0])
        if t == CAPSULE:
            z = np.clip(l[2], -s[1], s[1])
            return float(np.linalg.norm(l - np.array([0, 0, z])) - s[0])
        if t == CYLINDER:
            return float(max(np.hypot(l[0], l[1]) - s[0], abs(l[2]) - s[1]))
        return float(l[2])                                  # plane: the half space below it

    # ---- one pair
    def pair(self, g1, g2, poses, tol=1e-13, maxit=400):
        """(dist, pa, pb, n) of the separated geoms g1, g2 - pa on g1, pb on g2, n the unit vector from pa to pb - or None when they
        touch or overlap"""
        A, B = poses[g1], poses[g2]
        if self.gtype[g1] == PLANE or self.gtype[g2] == PLANE:
            sw = self.gtype[g1] != PLANE
            gp, go, Pp, Po = (g2, g1, B, A) if sw else (g1, g2, A, B)
            n = Pp[0][:, 2]
            s = self.support(go, Po, -n)
            d = float(n @ (s - Pp[1]))
            if d <= 0:
                return None
            pp = s - d * n
            return (d, s, pp, -n) if sw else (d, pp, s, n)
        r1, r2 = self.radius(g1), self.radius(g2)
        sup = lambda d: (self.support(g1, A, d, core=True), self.support(g2, B, -d, core=True))
        c1, c2 = A[1], B[1]
        v = c1 - c2
        if v @ v < 1e-30:
            v = np.array([1.0, 0, 0])
        a, b = sup(-v)
        SV, SA, SB = np.array([a - b]), np.array([a]), np.array([b])
        w = np.ones(1)
        v = SV[0]
        for _ in range(maxit):
            vv = float(v @ v)
            if vv < 1e-24:
                return None
            a, b = sup(-v)
            x = a - b
            if vv - float(v @ x) <= tol * vv or np.any(np.all(SV == x, axis=1)):
                break
            SV, SA, SB = np.vstack([SV, x]), np.vstack([SA, a]), np.vstack([SB, b])
            w, nv = _closest_on_simplex(SV)
            keep = w > 0
            if keep.sum() == 4:
                return None                                 # the origin is inside the tetrahedron
            SV, SA, SB, w = SV[keep], SA[keep], SB[keep], w[keep]
            if not float(nv @ nv) < vv:
                v = nv
                break
            v = nv
        pa, pb = w @ SA, w @ SB
        d = pb - pa
        L = float(np.linalg.norm(d))
        if L - r1 - r2 <= 0 or L < 1e-12:
            return None
        n = d / L
        return L - r1 - r2, pa + r1 * n, pb - r2 * n, n

    def members(self, mask_a, mask_b):
        """the admitted pairs of (a, b) in pair-list order: (g1, g2, swapped) - swapped: g2 is the a-side geom (the second order)"""
        out = []
        for g1, g2 in self.pairs:
            if in_mask(mask_a, g1) and in_mask(mask_b, g2):
                out.append((g1, g2, False))
            elif in_mask(mask_a, g2) and in_mask(mask_b, g1):
                out.append((g1, g2, True))
        return out

    def query(self, qpos, mask_a, mask_b, max_dist, cache=None):
        """exhaustive: dict(dist, geom (a side, b side), pa, pb, n, penetrating [the member pairs that touch], table {(ga, gb): dist})
        - dist None when nothing separated lies below max_dist"""
        poses = self.poses(qpos)
        cache = {} if cache is None else cache
        best, pen, table = None, [], {}
        for g1, g2, sw in self.members(mask_a, mask_b):
            if (g1, g2) not in cache:
                cache[(g1, g2)] = self.pair(g1, g2, poses)
            r = cache[(g1, g2)]
            key = (g2, g1) if sw else (g1, g2)
            if r is None:
                pen.append(key)
                continue
            d, pa, pb, n = r
            table[key] = d
            if d < max_dist and (best is None or d < best["dist"]):
                best = dict(dist=d, geom=key, pa=pb if sw else pa, pb=pa if sw else pb, n=-n if sw else n)
        out = best if best is not None else dict(dist=None, geom=(-1, -1), pa=None, pb=None, n=None)
        out.update(penetrating=pen, table=table, poses=poses)
        return out

    # ---- the certificate
    def certificate(self, ga, gb, poses, pa, pb, n, d):
        """largest violation (metres; <= slack passes) of: pa in ga, pb in gb, (pb - pa) = d n, |n| = 1, the slab along n separates the
        geoms by at least d"""
        pa, pb, n = (np.asarray(x, dtype=np.float64) for x in (pa, pb, n))
        A, B = poses[ga], poses[gb]
        parts = dict(inside_a=self.outside(ga, A, pa), inside_b=self.outside(gb, B, pb), witness=float(np.linalg.norm((pb - pa) - d * n)),
                     unit=abs(float(np.linalg.norm(n)) - 1.0))
        if self.gtype[ga] == PLANE:
            hi = float(n @ A[1]) if np.allclose(n, A[0][:, 2], atol=1e-3) else np.inf
        else:
            hi = float(n @ self.support(ga, A, n))
        if self.gtype[gb] == PLANE:
            lo = float(n @ B[1]) if np.allclose(-n, B[0][:, 2], atol=1e-3) else -np.inf
        else:
            lo = float(n @ self.support(gb, B, -n))
        parts["slab"] = d - (lo - hi)
        return max(parts.values()), parts
