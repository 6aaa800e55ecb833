"""fp64 reference of the depth / segmentation cameras (include/so101.h so101_render), written from the model blob alone.

Everything here is numpy on the f64 blob: forward kinematics of the body tree, MuJoCo's primitive shapes intersected
analytically, mesh geoms as the half-spaces of `scipy.spatial.ConvexHull(...).equations` (unmerged, straight from qhull;
the product's `meshes.hull_planes` is NOT used).  The definition of a pixel is the one of csrc/so101_camera.hpp:

  ray    pixel (r, c) of H x W: camera-frame direction ((c + 0.5 - W/2) s, -(r + 0.5 - H/2) s, -1), s = 2 tan(fovy/2) / H
  depth  ray parameter t of the nearest hit (distance along the optical axis); no hit: +inf and seg -1; equal t: lower geom
  geoms  plane: front side only, clipped to its positive sizes; a hit needs t > 0; a geom that holds the origin is invisible

A pixel is AMBIGUOUS when moving the camera-frame direction by +-1e-4 in x or y (four rays) changes the geom id or the depth
by more than 1e-3 relative: silhouettes, creases seen edge-on, the rim of the floor.  There fp32 and fp64 may legitimately
disagree; everywhere else the image must match (assert_image).
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial import ConvexHull

from so101_sim_amd.model import blob as blobfmt
from so101_sim_amd.pregrasp import GRASP_Q, HOME_Q

PLANE, SPHERE, CAPSULE, CYLINDER, BOX, MESH = range(6)
DEPTH_RTOL = 5e-5            # |z - z64| <= 5e-5 z64 on unambiguous pixels (9 x the error of this reference run in float32)
AMBIGUOUS_CAP = 0.02         # share of ambiguous pixels an image of >= 1024 pixels may have: a condition on the test's inputs
JITTER, JITTER_RTOL = 1e-4, 1e-3


def _axis_quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.r_[np.cos(0.5 * angle), np.sin(0.5 * angle) * a]


_ID = [1.0, 0.0, 0.0, 0.0]
_CONTAINER = [-0.25, 0.0, 0.42262]
# qpos = arm(6) | object pos, quat | container pos, quat
STATES = {
    "home": np.r_[HOME_Q, [0.25, 0.0, 0.42171], _ID, _CONTAINER, _ID],
    "grasp": np.r_[GRASP_Q, [0.2616, -0.008, 0.42171], _ID, _CONTAINER, _ID],
    "tilted": np.r_[[0.4, -0.6, 0.9, 0.5, -0.3, 0.5], [0.15, 0.12, 0.50], _axis_quat((1, 2, 0.5), 0.9),
                    [-0.2, -0.1, 0.47], _axis_quat((0.3, 1, 0), 0.5)],
}


def q2m(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _interval_slab(o, d, h):
    """[t0, t1] of the lines o + t d (arrays) inside |x| <= h"""
    with np.errstate(all="ignore"):
        a, b = (-h - o) / d, (h - o) / d
    t0, t1 = np.minimum(a, b), np.maximum(a, b)
    par = d == 0
    inside = np.abs(o) <= h
    t0 = np.where(par, np.where(inside, -np.inf, np.inf), t0)
    t1 = np.where(par, np.where(inside, np.inf, -np.inf), t1)
    return t0, t1


def _interval_quadric(o, D, r):
    """[t0, t1] of the lines o + t D[i] inside |x| <= r, in as many dimensions as o has"""
    a = np.einsum("ij,ij->i", D, D)
    b = D @ o
    c = o @ o - r * r
    with np.errstate(all="ignore"):
        disc = b * b - a * c
        sq = np.sqrt(np.maximum(disc, 0.0))
        t0, t1 = (-b - sq) / a, (-b + sq) / a
    miss = disc < 0
    t0, t1 = np.where(miss, np.inf, t0), np.where(miss, -np.inf, t1)
    par = a == 0
    t0 = np.where(par, np.inf if c > 0 else -np.inf, t0)
    t1 = np.where(par, -np.inf if c > 0 else np.inf, t1)
    return t0, t1


class RaycastRef:
    def __init__(self, blob_f64: bytes):
        m = blobfmt.unpack(blob_f64)
        assert m["mesh_vert"].dtype == np.float64, "the reference reads the f64 blob"
        self.m = m
        self.ngeom = int(m["ngeom"][0])
        self.bp, self.bq = m["body_pos"].reshape(-1, 3), m["body_quat"].reshape(-1, 4)
        self.par, self.arm, self.free = m["body_parent"], list(m["arm_body"]), list(m["free_body"])
        self.axis = m["jnt_axis"].reshape(-1, 3)
        self.gtype, self.gbody = m["geom_type"], m["geom_body"]
        self.gpos, self.gquat = m["geom_pos"].reshape(-1, 3), m["geom_quat"].reshape(-1, 4)
        self.gsize, self.gcenter, self.grbound = m["geom_size"].reshape(-1, 3), m["geom_center"].reshape(-1, 3), m["geom_rbound"]
        mv = m["mesh_vert"].reshape(-1, 3)
        self.planes = {}
        for g in range(self.ngeom):
            if self.gtype[g] == MESH:
                a, n = int(m["geom_vertadr"][g]), int(m["geom_vertnum"][g])
                self.planes[g] = ConvexHull(mv[a:a + n]).equations.copy()

    # ---- kinematics
    def body_frames(self, qpos):
        nb = len(self.par)
        P, Q = np.zeros((nb, 3)), np.zeros((nb, 4))
        Q[0] = [1, 0, 0, 0]
        for b in range(1, nb):
            if b in self.free:
                f = self.free.index(b)
                P[b] = qpos[6 + 7 * f: 9 + 7 * f]
                q = np.asarray(qpos[9 + 7 * f: 13 + 7 * f], dtype=np.float64)
                Q[b] = q / np.linalg.norm(q)
                continue
            p = self.par[b]
            P[b] = P[p] + q2m(Q[p]) @ self.bp[b]
            Q[b] = qmul(Q[p], self.bq[b])
            if b in self.arm:
                k = self.arm.index(b)
                Q[b] = qmul(Q[b], np.r_[np.cos(0.5 * qpos[k]), np.sin(0.5 * qpos[k]) * self.axis[k]])
            Q[b] /= np.linalg.norm(Q[b])
        return P, [q2m(q) for q in Q]

    def camera_frame(self, qpos, cam):
        """cam = (body, pos, mat [3, 3] columns x y z, fovy_deg); body: -1 world, 0..5 arm link, 6..7 free prop"""
        body, pos, mat, _ = cam
        pos, mat = np.asarray(pos, dtype=np.float64), np.asarray(mat, dtype=np.float64).reshape(3, 3)
        if body < 0:
            return pos, mat
        P, R = self.body_frames(qpos)
        b = self.arm[body] if body < 6 else self.free[body - 6]
        return P[b] + R[b] @ pos, R[b] @ mat

    # ---- one geom against all rays: [t0, t1] of each line inside the solid (plane: t of the surface, inf)
    def _interval(self, g, ol, Dl):
        t, s = self.gtype[g], self.gsize[g]
        if t == PLANE:
            with np.errstate(all="ignore"):
                tt = -ol[2] / Dl[:, 2]
                x, y = ol[0] + tt * Dl[:, 0], ol[1] + tt * Dl[:, 1]
            on = (Dl[:, 2] < 0) & (ol[2] > 0)
            if s[0] > 0:
                on &= np.abs(x) <= s[0]
            if s[1] > 0:
                on &= np.abs(y) <= s[1]
            return np.where(on, tt, np.inf), np.where(on, np.inf, -np.inf)
        if t == SPHERE:
            return _interval_quadric(ol, Dl, s[0])
        if t in (CAPSULE, CYLINDER):
            a0, a1 = _interval_quadric(ol[:2], Dl[:, :2], s[0])
            z0, z1 = _interval_slab(ol[2], Dl[:, 2], s[1])
            t0, t1 = np.maximum(a0, z0), np.minimum(a1, z1)
            if t == CAPSULE:
                parts = [(t0, t1)] + [_interval_quadric(ol - np.array([0, 0, cz]), Dl, s[0]) for cz in (s[1], -s[1])]
                t0 = np.min([np.where(p0 <= p1, p0, np.inf) for p0, p1 in parts], axis=0)
                t1 = np.max([np.where(p0 <= p1, p1, -np.inf) for p0, p1 in parts], axis=0)
            return t0, t1
        if t == BOX:
            iv = [_interval_slab(ol[k], Dl[:, k], s[k]) for k in range(3)]
            return np.max([i[0] for i in iv], axis=0), np.min([i[1] for i in iv], axis=0)
        E = self.planes[g]
        den = Dl @ E[:, :3].T                     # [P, F]
        num = E[:, :3] @ ol + E[:, 3]             # [F]  > 0: the origin is outside that plane
        with np.errstate(all="ignore"):
            tt = -num[None, :] / den
        t0 = np.max(np.where(den < 0, tt, -np.inf), axis=1)
        t1 = np.min(np.where(den > 0, tt, np.inf), axis=1)
        t0 = np.where(np.any((den == 0) & (num[None, :] > 0), axis=1), np.inf, t0)
        return t0, t1

    def cast(self, qpos, o, D):
        """nearest hit of the rays o + t D[i] (world): depth [P], seg [P]"""
        P, R = self.body_frames(qpos)
        depth, seg = np.full(len(D), np.inf), np.full(len(D), -1, dtype=np.int32)
        dd = np.einsum("ij,ij->i", D, D)
        for g in range(self.ngeom):
            b = self.gbody[g]
            Rg, pg = R[b] @ q2m(self.gquat[g]), P[b] + R[b] @ self.gpos[g]
            sel = np.arange(len(D))
            if self.gtype[g] != PLANE:
                # rays that pass the bounding sphere (generously widened: this only saves time)
                oc = pg + Rg @ self.gcenter[g] - o
                bq = D @ oc
                sel = np.flatnonzero((oc @ oc) * dd - bq * bq <= (self.grbound[g] * 1.001 + 1e-9) ** 2 * dd)
                if not len(sel):
                    continue
            t0, t1 = self._interval(g, Rg.T @ (o - pg), D[sel] @ Rg)
            hit = (t0 <= t1) & (t0 > 0) & (t0 < depth[sel])          # strict <: the lower geom index keeps an equal t
            depth[sel[hit]], seg[sel[hit]] = t0[hit], g
        return depth, seg

    def render(self, qpos, cam, H, W, jitter=(0.0, 0.0)):
        o, M = self.camera_frame(qpos, cam)
        s = 2.0 * np.tan(0.5 * np.deg2rad(cam[3])) / H
        r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        dc = np.stack([(c + 0.5 - W / 2) * s + jitter[0], -(r + 0.5 - H / 2) * s + jitter[1], -np.ones((H, W))], axis=-1).reshape(-1, 3)
        depth, seg = self.cast(np.asarray(qpos, dtype=np.float64), o, dc @ M.T)
        return depth.reshape(H, W), seg.reshape(H, W)

    def image(self, qpos, cam, H, W):
        """(depth, seg, ambiguous) of one image"""
        depth, seg = self.render(qpos, cam, H, W)
        amb = np.zeros((H, W), dtype=bool)
        for j in ((JITTER, 0), (-JITTER, 0), (0, JITTER), (0, -JITTER)):
            d2, s2 = self.render(qpos, cam, H, W, jitter=j)
            with np.errstate(all="ignore"):
                amb |= (s2 != seg) | (np.isfinite(depth) & (np.abs(d2 - depth) > JITTER_RTOL * depth))
        return depth, seg, amb


def cam_tuple(cam):
    """a so101_sim_amd.cameras.Camera as the plain tuple this module takes"""
    return (cam.body, tuple(cam.pos), tuple(np.asarray(cam.mat, dtype=np.float64).reshape(9)), cam.fovy)


_refs = {}


@functools.lru_cache(maxsize=None)
def _cached_image(key, qpos, cam, H, W):
    return _refs[key].image(np.asarray(qpos), cam, H, W)


def reference_image(ref: RaycastRef, key: str, qpos, cam, H, W):
    """ref.image(...) computed once per (model key, state, camera, size) and shared between tests; the arrays are read-only"""
    _refs[key] = ref
    out = _cached_image(key, tuple(float(x) for x in qpos), (cam[0], tuple(cam[1]), tuple(np.asarray(cam[2]).reshape(9)), float(cam[3])), int(H), int(W))
    for a in out:
        a.setflags(write=False)
    return out


def assert_image(depth, seg, ref_image, ngeom, label=""):
    """The acceptance rule of one image; prints its figures first.  Returns (ambiguous share, worst relative depth error)."""
    zd, zs, amb = ref_image
    depth, seg = np.asarray(depth), np.asarray(seg)
    assert depth.shape == zd.shape and seg.shape == zs.shape and depth.dtype == np.float32 and seg.dtype == np.int32
    share = float(amb.mean())
    clear = ~amb
    same = seg[clear] == zs[clear]
    fin = clear & np.isfinite(zd) & (seg == zs)
    rel = float(np.max(np.abs(depth[fin].astype(np.float64) - zd[fin]) / zd[fin])) if fin.any() else 0.0
    print(f"render {label}: {depth.size} px, hit {float(np.isfinite(zd).mean()):.3f}, ambiguous {share:.4f}, seg mismatches {int((~same).sum())}, "
          f"worst relative depth error {rel:.3e}")
    if depth.size >= 1024:
        assert share <= AMBIGUOUS_CAP, f"{label}: {share:.4f} of the pixels are ambiguous - the view is no valid test input"
    # every pixel is well formed, ambiguous or not
    assert np.all((seg >= -1) & (seg < ngeom)), label
    assert np.array_equal(seg == -1, np.isposinf(depth)), label
    assert not np.any(np.isnan(depth)) and np.all(depth > 0), label
    assert same.all(), f"{label}: {int((~same).sum())} unambiguous pixels with another geom id"
    miss = clear & (zs == -1)
    assert np.all(np.isposinf(depth[miss])), label
    assert rel <= DEPTH_RTOL, f"{label}: relative depth error {rel:.3e} > {DEPTH_RTOL}"
    return share, rel
