"""fp64 reference of the two broadphases (so101_device.hpp broadphase + obb_filter, so101_tree.hpp broadphase), numpy on the f64 blob alone;
no kernel runs here.  Everything is evaluated at what the device receives, float32 values converted to float64: the body frames of the query,
the geoms' sizes, boxes and vertices of the f32 blob, and the geoms' frames read back from the probe (Scene.set_frames).

  Scene.poses            world frame of every geom from the body frames of one query
  Scene.extent           exact support value of geoms along world directions: hull max(V @ d), sphere / capsule / cylinder / box in closed form
  Scene.separation       exact fp64 gap of geom pairs along the directions of the filter's family (no table, no box): a positive value proves
                         that the pair does not touch
  Scene.designed_margin  the filter as DESIGN.md section 3.1 and the comments above the device functions describe it, in fp64, thresholds
                         included: the pair is dropped iff the value is > 0.  It is the largest of
                           world      the 3 world axes with the world boxes (SO100 plane: its half space when the normal is a world axis;
                                      tree plane: the lowest corner of the other box along the normal),
                           obb        the 15 oriented-box axes with the geom_aabb boxes, `fabs(Rm) + 1e-6` and gap 1e-6 as written (the nine
                                      cross axes are not normalised there either: the sign is the gap's, the size is at most the gap),
                           table      with a hull as second geom and the support-bound tables on: box - its three faces on the hull's side; sphere,
                                      capsule, cylinder, hull - centre to centre, the primitive's axis, the radial direction from it; plane - its
                                      normal.  The hull's extent is bilinear in the float32 table the product built (read back from the probe).
  Scene.inside           the common-point certificate of tests/proximity_ref.py::ProximityRef.outside (hull facet planes / analytic test)
"""
from __future__ import annotations

import numpy as np

from so101_sim_amd.model import blob as blobfmt
from tests.proximity_ref import ProximityRef
from tests.raycast_ref import q2m, qmul

PLANE, SPHERE, CAPSULE, CYLINDER, BOX, MESH = range(6)
TYPE_NAMES = ("plane", "sphere", "capsule", "cylinder", "box", "mesh")
GAP = 1e-6                     # the filters' own `gap` constant (so101_device.hpp obb_filter, so101_tree.hpp broadphase, so101_geom.hpp sbt_separated)
SBT_GRID = 5
NDIR = 21                      # family directions per pair: 3 world, 3 + 3 box axes, 9 cross axes, 3 table directions


def _unit(v, eps=1e-12):
    """rows of v normalised; (unit rows, mask of rows longer than eps)"""
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    ok = n[..., 0] > eps
    return np.where(ok[..., None], v / np.where(n > eps, n, 1.0), 0.0), ok


def sbt_bound(T, dl):
    """so101_geom.hpp sbt_bound in fp64, row by row: T [n, 6, G, G] (float32 tables as float64), dl [n, 3]"""
    a = np.abs(dl)
    ax = np.where(a[:, 0] >= a[:, 1], np.where(a[:, 0] >= a[:, 2], 0, 2), np.where(a[:, 1] >= a[:, 2], 1, 2))
    r = np.arange(len(dl))
    dm, du, dv = dl[r, ax], dl[r, (ax + 1) % 3], dl[r, (ax + 2) % 3]
    mm = np.maximum(np.abs(dm), 1e-20)
    gs = 0.5 * (SBT_GRID - 1)
    gu, gv = np.clip((du / mm + 1.0) * gs, 0.0, SBT_GRID - 1.0), np.clip((dv / mm + 1.0) * gs, 0.0, SBT_GRID - 1.0)
    iu, iv = np.minimum(gu.astype(int), SBT_GRID - 2), np.minimum(gv.astype(int), SBT_GRID - 2)
    fu, fv = gu - iu, gv - iv
    f = 2 * ax + (dm < 0)
    h = (1 - fu) * ((1 - fv) * T[r, f, iu, iv] + fv * T[r, f, iu, iv + 1]) + fu * ((1 - fv) * T[r, f, iu + 1, iv] + fv * T[r, f, iu + 1, iv + 1])
    return h * mm


class Scene:
    """engine 0: the SO100 engine (frames = the NDYN dynamic bodies, static geoms resolved to the world); 32 / 64: the tree builds (frames = the
    blob's bodies, body 0 the world)."""

    def __init__(self, blob_f64: bytes, engine: int, nb: int, blob_f32: bytes = None):
        """blob_f32: the blob the device is built from.  With it the geoms' sizes, boxes and vertices are its float32 values as float64 - what
        the device holds - and the geoms' frames are replaced by the device's own once a probe exists (set_frames); the body tree, needed for
        the static geoms of the SO100 engine only, stays the f64 blob's."""
        m = self.m = blobfmt.unpack(blob_f64)
        assert m["mesh_vert"].dtype == np.float64, "the reference reads the f64 blob"
        self.engine, self.nb = engine, nb
        self.prox = ProximityRef(blob_f64)                          # outside(), hull_planes()
        self.device_frames = False
        if blob_f32 is not None:
            m32 = blobfmt.unpack(blob_f32)
            assert m32["mesh_vert"].dtype == np.float32
            m = dict(m)
            for k in ("geom_size", "geom_aabb", "geom_rbound", "geom_center", "mesh_vert", "geom_pos", "geom_quat"):
                m[k] = np.asarray(m32[k], dtype=np.float64)
            mv = m["mesh_vert"].reshape(-1, 3)
            for g in list(self.prox.verts):
                a, n = int(m["geom_vertadr"][g]), int(m["geom_vertnum"][g])
                self.prox.verts[g] = mv[a:a + n]
            self.prox.gsize = m["geom_size"].reshape(-1, 3)
        ng = self.ngeom = int(m["ngeom"][0])
        self.gtype = np.asarray(m["geom_type"]).astype(int)
        self.gsize = np.asarray(m["geom_size"], dtype=np.float64).reshape(-1, 3)
        ab = np.asarray(m["geom_aabb"], dtype=np.float64).reshape(-1, 6)
        self.bc, self.bh = ab[:, :3], ab[:, 3:]
        self.rbound = np.asarray(m["geom_rbound"], dtype=np.float64)
        self.center = np.asarray(m["geom_center"], dtype=np.float64).reshape(-1, 3)
        self.verts = self.prox.verts
        gbody = np.asarray(m["geom_body"]).astype(int)
        gpos = np.asarray(m["geom_pos"], dtype=np.float64).reshape(-1, 3)
        gR = np.stack([q2m(q) for q in np.asarray(m["geom_quat"], dtype=np.float64).reshape(-1, 4)])
        if engine == 0:
            # build_model() of so101_hip.hip: geoms of the arm links and the free props keep body-local frames, the rest is resolved to the world
            par, jt = np.asarray(m["body_parent"]).astype(int), np.asarray(m["body_jnttype"]).astype(int)
            bp, bq = np.asarray(m["body_pos"], dtype=np.float64).reshape(-1, 3), np.asarray(m["body_quat"], dtype=np.float64).reshape(-1, 4)
            nbody = len(par)
            wp, wq, static = np.zeros((nbody, 3)), np.zeros((nbody, 4)), np.zeros(nbody, bool)
            wq[0, 0], static[0] = 1.0, True
            for i in range(1, nbody):
                if jt[i] != 0 or not static[par[i]]:
                    continue
                static[i] = True
                wp[i] = wp[par[i]] + q2m(wq[par[i]]) @ bp[i]
                wq[i] = qmul(wq[par[i]], bq[i])
            dyn = -np.ones(nbody, int)
            for k, b in enumerate(m["arm_body"]):
                dyn[int(b)] = k
            for f, b in enumerate(m["free_body"]):
                dyn[int(b)] = len(m["arm_body"]) + f
            self.fb = dyn[gbody]
            self.lp, self.lR = gpos.copy(), gR.copy()
            for g in np.nonzero(self.fb < 0)[0]:
                assert static[gbody[g]], "geom on an unsupported body"
                Rb = q2m(wq[gbody[g]])
                self.lp[g], self.lR[g] = wp[gbody[g]] + Rb @ gpos[g], Rb @ gR[g]
        else:
            self.fb, self.lp, self.lR = gbody, gpos, gR
        assert self.fb.max() < nb
        self.movable = self.fb >= (0 if engine == 0 else 1)
        pg = np.asarray(m["pair_geom"]).astype(int).reshape(-1, 2)
        sw = self.gtype[pg[:, 0]] > self.gtype[pg[:, 1]]
        self.pairs = np.where(sw[:, None], pg[:, ::-1], pg)        # as upload_geometry() packs them: geom types ordered
        self.pair_index = {(int(a), int(b)): k for k, (a, b) in enumerate(self.pairs)}
        self.p1, self.p2 = self.pairs[:, 0], self.pairs[:, 1]
        self.sbt = None                                            # [ngeom, 6, G, G] float64 of the product's float32 tables (set_tables)

    def so100_frames(self):
        """geom_dyn, geom_pos, geom_mat of the SO100 probe"""
        return self.fb.astype(np.int32), self.lp.astype(np.float32), self.lR.astype(np.float32)

    def set_frames(self, gdyn, gpos32, gmat32):
        """the geoms' frames as the device holds them (read back from a probe): from here on every reference quantity is evaluated at them"""
        assert np.array_equal(np.asarray(gdyn), self.fb)
        lp, lR = np.asarray(gpos32, dtype=np.float64).reshape(-1, 3), np.asarray(gmat32, dtype=np.float64).reshape(-1, 3, 3)
        assert np.abs(lp - self.lp).max() <= 1e-6 and np.abs(lR - self.lR).max() <= 1e-6, "the probe's geom frames are not the blob's"
        if self.device_frames:
            assert np.array_equal(lp, self.lp) and np.array_equal(lR, self.lR), "two probes of one scene hold different geom frames"
        self.lp, self.lR, self.device_frames = lp, lR, True

    def set_tables(self, sbt32):
        self.sbt = np.asarray(sbt32, dtype=np.float64).reshape(self.ngeom, 6, SBT_GRID, SBT_GRID)

    def type_pair(self, k):
        return TYPE_NAMES[self.gtype[self.p1[k]]] + "|" + TYPE_NAMES[self.gtype[self.p2[k]]]

    # ---- frames
    def rest_frames(self):
        """identity frames: xpos [nb, 3], xmat [nb, 3, 3]"""
        return np.zeros((self.nb, 3)), np.tile(np.eye(3), (self.nb, 1, 1))

    def poses(self, xpos, xmat):
        """world P [ngeom, 3], R [ngeom, 3, 3] at the body frames of one query (float32 values as float64)"""
        xpos, xmat = np.asarray(xpos, dtype=np.float64).reshape(-1, 3), np.asarray(xmat, dtype=np.float64).reshape(-1, 3, 3)
        f = np.maximum(self.fb, 0)
        R = xmat[f] @ self.lR
        P = xpos[f] + np.einsum("gij,gj->gi", xmat[f], self.lp)
        st = self.fb < 0
        R[st], P[st] = self.lR[st], self.lp[st]
        return P, R

    def body_frame_for(self, g, Rw, pw):
        """the frame of g's body that puts geom g at world rotation Rw, origin pw"""
        Rb = Rw @ self.lR[g].T
        return pw - Rb @ self.lp[g], Rb

    # ---- exact extents
    def extent(self, geoms, D, P, R):
        """exact support value max_x x . D[k] of geom geoms[k] (no plane), rows grouped by geom"""
        geoms, D = np.asarray(geoms), np.asarray(D, dtype=np.float64)
        out = np.empty(len(geoms))
        for g in np.unique(geoms):
            r = np.nonzero(geoms == g)[0]
            d = D[r]
            L = d @ R[g]
            t, s = self.gtype[g], self.gsize[g]
            if t == MESH:
                e = (L @ self.verts[g].T).max(axis=1)
            elif t == SPHERE:
                e = s[0] * np.linalg.norm(L, axis=1)
            elif t == CAPSULE:
                e = s[0] * np.linalg.norm(L, axis=1) + s[1] * np.abs(L[:, 2])
            elif t == CYLINDER:
                e = s[0] * np.hypot(L[:, 0], L[:, 1]) + s[1] * np.abs(L[:, 2])
            elif t == BOX:
                e = np.abs(L) @ s
            else:
                raise ValueError("a plane has no support value")
            out[r] = d @ P[g] + e
        return out

    def support_point(self, g, pose, d):
        return self.prox.support(g, pose, d)

    def inside(self, g, pose, x):
        """how far x lies inside geom g (> 0: inside)"""
        return -self.prox.outside(g, pose, x)

    # ---- the direction family of pairs
    def _boxes(self, idx, P, R):
        g1, g2 = self.p1[idx], self.p2[idx]
        A, B = R[g1], R[g2]
        ca, cb = P[g1] + np.einsum("nij,nj->ni", A, self.bc[g1]), P[g2] + np.einsum("nij,nj->ni", B, self.bc[g2])
        return g1, g2, A, B, ca, cb, self.bh[g1], self.bh[g2]

    def table_dirs(self, idx, P, R):
        """the table directions of sbt_separated / sbt_plane_separated for the pairs idx, oriented from geom 1 to geom 2: D [n, 3, 3], valid
        [n, 3] (all invalid unless geom 2 is a hull)"""
        g1, g2, A, B, ca, cb, a, b = self._boxes(idx, P, R)
        n = len(idx)
        D, ok = np.zeros((n, 3, 3)), np.zeros((n, 3), bool)
        t1, mesh2 = self.gtype[g1], self.gtype[g2] == MESH
        t = np.einsum("nji,nj->ni", A, cb - ca)
        box = mesh2 & (t1 == BOX)
        sg = np.where(t >= 0, 1.0, -1.0)
        D[box] = (sg[:, None, :] * A).transpose(0, 2, 1)[box]     # row i: sg_i * column i of A
        ok[box] = True
        pl = mesh2 & (t1 == PLANE)
        D[pl, 0] = A[pl][:, :, 2]
        ok[pl, 0] = True
        oth = mesh2 & ~box & ~pl
        d0, ok0 = _unit(cb - ca, 1e-9)
        D[oth, 0], ok[oth, 0] = d0[oth], ok0[oth]
        ax = oth & ((t1 == CAPSULE) | (t1 == CYLINDER))
        az = A[:, :, 2]
        w = cb - P[g1]
        s = np.einsum("ni,ni->n", w, az)
        D[ax, 1] = (np.where(s >= 0, 1.0, -1.0)[:, None] * az)[ax]
        ok[ax, 1] = True
        rr, okr = _unit(w - s[:, None] * az, 1e-9)
        D[ax, 2], ok[ax, 2] = rr[ax], okr[ax]
        return D, ok

    def family(self, idx, P, R):
        """unit directions of the filter's family for the pairs idx: D [n, NDIR, 3], valid [n, NDIR].  A plane pair has its normal only."""
        g1, g2, A, B, ca, cb, a, b = self._boxes(idx, P, R)
        n = len(idx)
        D, ok = np.zeros((n, NDIR, 3)), np.ones((n, NDIR), bool)
        D[:, 0:3] = np.eye(3)
        D[:, 3:6], D[:, 6:9] = A.transpose(0, 2, 1), B.transpose(0, 2, 1)
        cr = np.cross(D[:, 3:6, None, :], D[:, None, 6:9, :]).reshape(n, 9, 3)
        D[:, 9:18], ok[:, 9:18] = _unit(cr, 1e-6)
        D[:, 18:21], ok[:, 18:21] = self.table_dirs(idx, P, R)
        pl = self.gtype[g1] == PLANE
        ok[pl] = False
        D[pl, 18], ok[pl, 18] = A[pl][:, :, 2], True
        return D, ok

    def separation(self, idx, P, R):
        """exact: per pair of idx the largest fp64 gap over the family's directions (either orientation), and that direction [n, 3]"""
        idx = np.asarray(idx)
        D, ok = self.family(idx, P, R)
        n = len(idx)
        g1, g2 = np.repeat(self.p1[idx], NDIR), np.repeat(self.p2[idx], NDIR)
        Df = D.reshape(-1, 3)
        pl = self.gtype[g1] == PLANE
        v = ok.reshape(-1) & ~pl
        sep = np.full(n * NDIR, -np.inf)
        if v.any():
            fwd = -self.extent(g2[v], -Df[v], P, R) - self.extent(g1[v], Df[v], P, R)
            bwd = -self.extent(g1[v], -Df[v], P, R) - self.extent(g2[v], Df[v], P, R)
            sep[v] = np.maximum(fwd, bwd)
        vp = ok.reshape(-1) & pl                                    # the half space below the plane: the other geom's lowest point along the normal
        if vp.any():
            sep[vp] = -self.extent(g2[vp], -Df[vp], P, R) - np.einsum("ni,ni->n", Df[vp], P[g1[vp]])
        sep = sep.reshape(n, NDIR)
        k = np.argmax(sep, axis=1)
        return sep[np.arange(n), k], D[np.arange(n), k]

    def sphere_gap(self, idx, P, R):
        """gap of the pairs' bounding spheres (planes: the sphere above the plane): > 0 proves separation cheaply"""
        g1, g2 = self.p1[idx], self.p2[idx]
        c1, c2 = P[g1] + np.einsum("nij,nj->ni", R[g1], self.center[g1]), P[g2] + np.einsum("nij,nj->ni", R[g2], self.center[g2])
        gap = np.linalg.norm(c2 - c1, axis=1) - self.rbound[g1] - self.rbound[g2]
        pl = self.gtype[g1] == PLANE
        gap[pl] = np.einsum("ni,ni->n", c2[pl] - P[g1[pl]], R[g1[pl]][:, :, 2]) - self.rbound[g2[pl]]
        return gap

    # ---- the filter as designed
    def world_margin(self, P, R, idx=None):
        """the first pass on the pairs idx (None: all); > 0: the world boxes (or the plane rule) separate the pair"""
        c = P + np.einsum("gij,gj->gi", R, self.bc)
        e = np.einsum("gij,gj->gi", np.abs(R), self.bh)
        lo, hi = c - e, c + e
        pl = np.nonzero(self.gtype == PLANE)[0]
        if self.engine == 0:
            for g in pl:
                nrm = R[g][:, 2]
                axis = np.abs(nrm) == 1.0
                lo[g] = np.where(axis & (nrm < 0), P[g], -3.0e38)
                hi[g] = np.where(axis & (nrm > 0), P[g], 3.0e38)
        g1, g2 = (self.p1, self.p2) if idx is None else (self.p1[idx], self.p2[idx])
        mg = np.maximum(lo[g1] - hi[g2], lo[g2] - hi[g1]).max(axis=1)
        if self.engine != 0:
            k = np.nonzero(self.gtype[g1] == PLANE)[0]
            nrm = R[g1[k]][:, :, 2]
            mg[k] = np.einsum("ni,ni->n", nrm, np.where(nrm >= 0, lo[g2[k]], hi[g2[k]]) - P[g1[k]])
        return mg

    def obb_margin(self, idx, P, R):
        """the 15 axes as obb_filter writes them; -inf for plane pairs (they pass)"""
        g1, g2, A, B, ca, cb, a, b = self._boxes(idx, P, R)
        t = np.einsum("nji,nj->ni", A, cb - ca)
        Rm = np.einsum("nki,nkj->nij", A, B)
        Ab = np.abs(Rm) + 1e-6
        m = [np.abs(t) - (a + np.einsum("nj,nij->ni", b, Ab) + GAP), np.abs(np.einsum("ni,nij->nj", t, Rm)) - (np.einsum("ni,nij->nj", a, Ab) + b + GAP)]
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                ra = a[:, i1] * Ab[:, i2, j] + a[:, i2] * Ab[:, i1, j]
                rb = b[:, j1] * Ab[:, i, j2] + b[:, j2] * Ab[:, i, j1]
                m.append((np.abs(t[:, i2] * Rm[:, i1, j] - t[:, i1] * Rm[:, i2, j]) - (ra + rb + GAP))[:, None])
        out = np.concatenate(m, axis=1).max(axis=1)
        out[self.gtype[g1] == PLANE] = -np.inf
        return out

    def table_margin(self, idx, P, R):
        """sbt_separated / sbt_plane_separated as written, the hulls' extents bilinear in the product's tables; -inf where they do not apply"""
        n = len(idx)
        out = np.full(n, -np.inf)
        if self.sbt is None or n == 0:
            return out
        g1, g2, A, B, ca, cb, a, b = self._boxes(idx, P, R)
        D, ok = self.table_dirs(idx, P, R)
        t1 = self.gtype[g1]
        for q in range(3):
            r = np.nonzero(ok[:, q])[0]
            if len(r) == 0:
                continue
            d = D[r, q]
            # sbt_lowest of the hull: min_x x . d >= p . d - bound(-R' d) - 2e-6
            low2 = np.einsum("ni,ni->n", P[g2[r]], d) - sbt_bound(self.sbt[g2[r]], -np.einsum("nji,nj->ni", B[r], d)) - 2e-6
            tt = t1[r]
            val = np.empty(len(r))
            bx = tt == BOX
            val[bx] = low2[bx] - np.einsum("ni,ni->n", ca[r][bx], d[bx]) - (a[r][bx, q] + GAP)
            pl = tt == PLANE
            val[pl] = low2[pl] - np.einsum("ni,ni->n", P[g1[r]][pl], d[pl]) - 1e-6
            ot = ~bx & ~pl
            if ot.any():
                ro = r[ot]
                do = d[ot]
                pa_d = np.einsum("ni,ni->n", P[g1[ro]], do)
                along = np.abs(np.einsum("ni,ni->n", A[ro][:, :, 2], do))
                s = self.gsize[g1[ro]]
                to = t1[ro]
                top = np.where(to == SPHERE, pa_d + s[:, 0], np.where(to == CAPSULE, pa_d + s[:, 0] + s[:, 1] * along,
                               pa_d + s[:, 0] * np.sqrt(np.maximum(1 - along * along, 0)) + s[:, 1] * along))
                hm = to == MESH
                if hm.any():
                    top[hm] = pa_d[hm] + sbt_bound(self.sbt[g1[ro][hm]], np.einsum("nji,nj->ni", A[ro][hm], do[hm])) + 2e-6
                val[ot] = low2[ot] - top - (GAP + 2e-6)
            out[r] = np.maximum(out[r], val)
        return out

    def designed_margin(self, P, R, tables=True, beyond=None):
        """all pairs -> [npair]; the pair is dropped iff the value is > 0.  The oriented boxes and the tables are evaluated for every pair (the
        device evaluates them on the survivors of the world boxes only; the decision is the same) - or, with `beyond`, for the pairs whose world
        margin is at most `beyond`: the others keep their world margin, a lower bound of the value that already decides them"""
        w = self.world_margin(P, R)
        idx = np.arange(len(self.pairs)) if beyond is None else np.nonzero(w <= beyond)[0]
        out = w.copy()
        if len(idx):
            out[idx] = np.maximum(out[idx], self.obb_margin(idx, P, R))
            if tables:
                out[idx] = np.maximum(out[idx], self.table_margin(idx, P, R))
        return out

    # ---- check 1
    def static_violation(self):
        """per geom: how far it reaches outside its geom_aabb box and its geom_rbound sphere (geom frame), fp64; planes 0"""
        box, sph = np.zeros(self.ngeom), np.zeros(self.ngeom)
        I = np.eye(3)
        for g in range(self.ngeom):
            t, s = self.gtype[g], self.gsize[g]
            if t == PLANE:
                continue
            if t == MESH:
                V = self.verts[g]
                ext = np.abs(V - self.bc[g]).max(axis=0)
                far = np.linalg.norm(V - self.center[g], axis=1).max()
            else:
                assert np.all(self.bc[g] == 0) and np.all(self.center[g] == 0)          # (primitives are symmetric about their origin)
                ext = self.extent(np.full(3, g), I, np.zeros((self.ngeom, 3)), np.tile(I, (self.ngeom, 1, 1)))
                far = {SPHERE: s[0], CAPSULE: s[0] + s[1], CYLINDER: np.hypot(s[0], s[1]), BOX: np.linalg.norm(s)}[t]
            box[g], sph[g] = (ext - self.bh[g]).max(), far - self.rbound[g]
        return box, sph
