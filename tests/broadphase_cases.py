"""Shared cases and checks of the broadphase tests: tests/test_broadphase_emu.py through the emulated probe builds, tests/test_broadphase_gpu.py on
the MI355X.  The probe (tests/devprims/broadphase_probe.hip) runs the product's broadphase() of either engine on body frames given directly;
the reference (tests/broadphase_ref.py) is numpy fp64 on the f64 blob.

Scenes: SO100 banana and pen (so101_device.hpp, MAXCAND 256), ALOHA hand-over (so101_tree.hpp 32-dof build, TCAND 256), Dining (64-dof build,
TCAND 512), and the ALOHA blob on the 64-dof build (the two tree builds must give the same list bit for bit).

The SO100 probe takes geom_dyn / geom_pos / geom_mat from the test (Scene.so100_frames: build_model()'s derivation restated in fp64 and rounded
to float32); the product's own loop is not shared with the probe.  The reference then works with the geom frames read back from the probe and
with the float32 sizes, boxes and vertices of the f32 blob, so a probe has to exist before cases are built.

Families (every body that a case does not place sits alone, far from the scene):
  T  certified touching.  Geom A presents a feature along a unit direction n (hull: facet, vertex, the table's grid points and cube-map cell
     edges, random; box: face, edge, corner; cylinder: cap, side, rim), geom B a facet interior or smooth point along -n (hull: the centroid of a
     facet of meshes.hull_planes, any facet of the hull - tests/golden/hull_facets.json holds the eight largest of some hulls only -; box: face
     centre; cylinder: cap centre or side; sphere, capsule: any point; plane: its surface), B's feature delta in {1e-6, 1e-5, 1e-3} m below A's
     support point; box | box also parallel, edge to edge.  Certificate, at the float32 frames: A's support point (a point of A's surface, held in A's frame) is within 1e-7 m of A by its facet planes and at least
     delta / 4 inside B (plane as A: B's anchor point at least delta / 4 below the plane).  Where B is a sphere too small to hold a point delta / 4 inside at that depth (the 0.6 mm finger spheres of ALOHA and Dining at
     delta = 1e-3) A presents a facet interior or smooth point too and the witness is the middle of the dip, delta / 4 inside both geoms.
     Both role orders; cases that fail the certificate are left out, at most 10 % of a (type pair, delta) cell, and every cell keeps some.
  S  certified near misses: B lifted delta in {1e-4, 1e-3} m clear of A along a designed direction - `table`: a box face normal, the plane's
     normal, centre to centre / axis / radial of a sphere, capsule, cylinder, hull, with a grid point of the hull's table along that direction
     (the table is exact there); `obb`: an oriented-box axis, the two geom_aabb boxes face to face; `world`: a plane's normal, the
     lowest corner of the other geom's box above it.  Kept where the fp64 designed_margin exceeds
     BAND.
  R  real states: tests/golden/contact_rich_states.json and probe_outlier_states.json (SO100), the hand-over and Dining states of
     tests/tree_contact_cases.py (tree), with the fp64 kinematics of tests/raycast_ref.py / tree_raycast_ref.py; each as is and with the free
     bodies moved by up to 5 mm and 0.05 rad.
     The pairs at the ends of the list and of its 64-lane blocks, four-block trips and bursts get a touching case each.
  O  over capacity: every body at one place, so that more pairs pass the world boxes than the candidate list holds.

BAND (check 4).  The largest |designed_margin| at which the device's decision and the fp64 decision differ, over families S and R, measured
first with the full families on both backends: emulator 1.58e-8 m, MI355X 1.58e-8 m (the same case on both: a box | box pair in a query of
family S whose fp64 margin is +1.58e-8 m and which the device keeps - conservative).  Over family R, and over family T, the decisions never
differ.  Asserted on all three families: four times the larger (6.4e-8 m), and never more than 2e-5 m.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from so101_sim_amd.model import scenes
from tests import broadphase_ref as br
from tests.broadphase_ref import BOX, CAPSULE, CYLINDER, MESH, PLANE, SPHERE

MEASURED_BAND = dict(emu=1.59e-8, gpu=1.59e-8)          # m, see the module docstring
BAND = min(4.0 * max(MEASURED_BAND.values()), 2e-5)
T_DELTAS = (1e-6, 1e-5, 1e-3)
S_DELTAS = (1e-4, 1e-3)
SAFETY = -1e-6                                  # check 3: the filters' own gap constant
ENGINE = {"so100_banana": 0, "so100_pen": 0, "aloha": 32, "dining": 64, "aloha@64": 64, "so100_banana@32": 32, "so100_banana@64": 64}      # name@build: a blob on another build
FAR = np.array([50.0, 30.0, 20.0])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------- setups
def _blobs(name):
    name = name.split("@")[0]
    if name.startswith("so100_"):
        return scenes.load_blob(name[6:], "f32")[0], scenes.load_blob(name[6:], "f64")[0]
    load = scenes.load_dining_blob if name == "dining" else scenes.load_aloha_blob
    return load("banana", "f32")[0], load("banana", "f64")[0]


class Setup:
    def __init__(self, name):
        from tests.devprims import broadphase as bp
        self.name, self.engine = name, ENGINE[name]
        self.f32, self.f64 = _blobs(name)
        self.nb = 8 if self.engine == 0 else 32
        self.scene = br.Scene(self.f64, self.engine, self.nb, self.f32)
        self._bp, self._probes = bp, {}

    def probe(self, kind, sbt=True):
        key = (kind, sbt)
        if key not in self._probes:
            S = self.scene
            p = self._bp.Probe(kind, self.engine, self.f32, S.so100_frames() if self.engine == 0 else None, sbt=sbt)
            assert (p.nb, p.ngeom, p.npair) == (self.nb, S.ngeom, len(S.pairs))
            assert np.array_equal(p.packed & 0xff, S.p1) and np.array_equal((p.packed >> 8) & 0xff, S.p2)
            assert np.array_equal((p.packed >> 16) & 1, (S.gtype[S.p1] == PLANE).astype(np.uint32)) and not np.any(p.packed >> 17)
            S.set_frames(p.geom_dyn, p.geom_pos, p.geom_mat)
            if sbt:
                S.set_tables(p.sbt)
            assert all(q.cap == p.cap for q in self._probes.values())
            self._probes[key] = p
        return self._probes[key]

    @property
    def cap(self):
        """the candidate capacity (MAXCAND / TCAND) as the probe build reports it"""
        assert self._probes, "no probe yet"
        return next(iter(self._probes.values())).cap


@functools.lru_cache(maxsize=None)
def setup(name) -> Setup:
    return Setup(name)


# ---------------------------------------------------------------------------------------------------------------- small geometry
def _basis(v):
    v = v / np.linalg.norm(v)
    a = np.eye(3)[int(np.argmin(np.abs(v)))]
    x = np.cross(a, v)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(v, x), v], axis=1)


def rot_map(a, b, angle):
    """a rotation that takes the unit vector a to b, with a spin of `angle` about it"""
    c, s = np.cos(angle), np.sin(angle)
    return _basis(np.asarray(b, dtype=np.float64)) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ _basis(np.asarray(a, dtype=np.float64)).T


def rand_unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def rand_rot(rng):
    return rot_map(rand_unit(rng), rand_unit(rng), rng.uniform(0, 2 * np.pi))


def small_rot(rng, amax):
    return _axis_angle(rand_unit(rng), rng.uniform(0, amax))


def _axis_angle(u, ang):
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def grid_dir(rng):
    """a direction through a grid point of the support-bound table (cube face, 5 x 5 points)"""
    ax, sg = rng.integers(3), rng.choice([-1.0, 1.0])
    d = np.zeros(3)
    d[ax], d[(ax + 1) % 3], d[(ax + 2) % 3] = sg, rng.choice([-1, -0.5, 0, 0.5, 1.0]), rng.choice([-1, -0.5, 0, 0.5, 1.0])
    return d / np.linalg.norm(d)


def cell_edge_dir(rng):
    """a direction on an edge between two cells of the 8 x 8 cube map of the support-vertex lists"""
    ax, sg = rng.integers(3), rng.choice([-1.0, 1.0])
    d = np.zeros(3)
    d[ax], d[(ax + 1) % 3], d[(ax + 2) % 3] = sg, rng.integers(-4, 5) / 4.0, rng.uniform(-1, 1)
    return d / np.linalg.norm(d)


# ---------------------------------------------------------------------------------------------------------------- features
def a_direction(S, g, rng):
    """geom-frame direction along which A presents a feature, with its name"""
    t = S.gtype[g]
    k = rng.integers(5)
    if t == MESH:
        E = S.prox.hull_planes(g)
        return [(E[rng.integers(len(E)), :3], "facet"), (rand_unit(rng), "vertex"), (grid_dir(rng), "grid"), (cell_edge_dir(rng), "cell edge"), (np.eye(3)[rng.integers(3)], "axis")][k]
    if t == BOX:
        sg = rng.choice([-1.0, 1.0], size=3)
        return [(sg * np.eye(3)[rng.integers(3)], "face"), (sg * np.roll([1, 1, 0.0], rng.integers(3)) / np.sqrt(2), "edge"), (sg / np.sqrt(3), "corner"),
                (rand_unit(rng), "corner"), (sg * np.eye(3)[rng.integers(3)], "face")][k]
    if t == CYLINDER:
        c, s = np.cos(rng.uniform(0, 6.28)), np.sin(rng.uniform(0, 6.28))
        rad = np.array([c, s, 0]) / np.hypot(c, s)
        return [(np.array([0, 0, rng.choice([-1.0, 1.0])]), "cap"), (rad, "side"), ((rad + [0, 0, rng.choice([-1.0, 1.0])]) / np.sqrt(2), "rim"), (rand_unit(rng), "rim"), (rad, "side")][k]
    return rand_unit(rng), "smooth"


def b_feature(S, g, rng):
    """(geom-frame outward direction l, geom-frame anchor point on the surface where the outward normal is l) - a facet interior or smooth point"""
    t, s = S.gtype[g], S.gsize[g]
    if t == MESH:
        E, V = S.prox.hull_planes(g), S.verts[g]
        best = None
        for _ in range(40):                                    # a facet whose centroid is interior enough to dip the largest delta below it, if there is one
            e = E[rng.integers(len(E))]
            on = np.abs(V @ e[:3] + e[3]) < 1e-9
            if on.sum() < 3:
                continue
            l, c = e[:3] / np.linalg.norm(e[:3]), V[on].mean(axis=0)
            room = -np.max(E[:, :3] @ (c - T_DELTAS[-1] * l) + E[:, 3])
            if best is None or room > best[0]:
                best = (room, l, c)
            if room >= 0.5 * T_DELTAS[-1]:
                break
        assert best is not None, "no facet with three vertices"
        return best[1], best[2]
    if t == BOX:
        l = rng.choice([-1.0, 1.0]) * np.eye(3)[rng.integers(3)]
        return l, l * s
    if t == SPHERE:
        l = rand_unit(rng)
        return l, s[0] * l
    if t == CAPSULE:
        l = rand_unit(rng)
        return l, s[0] * l + np.array([0, 0, np.sign(l[2]) * s[1]])
    if t == CYLINDER:
        if rng.integers(2):
            sg = rng.choice([-1.0, 1.0])
            return np.array([0, 0, sg]), np.array([0, 0, sg * s[1]])
        a = rng.uniform(0, 2 * np.pi)
        l = np.array([np.cos(a), np.sin(a), 0])
        return l, s[0] * l + np.array([0, 0, rng.uniform(-0.8, 0.8) * s[1]])
    return np.array([0, 0, 1.0]), np.zeros(3)          # plane


def far_frames(S):
    xp, xm = S.rest_frames()
    for b in range(S.nb):
        if S.engine == 0 or b > 0:
            xp[b] = FAR + 7.0 * b
    return xp, xm


def _place(S, xp, xm, g, Rw, pw):
    p, R = S.body_frame_for(g, Rw, pw)
    xp[S.fb[g]], xm[S.fb[g]] = p, R


def _round(xp, xm):
    return xp.astype(np.float32), xm.astype(np.float32)


def _world(S, g):
    """fixed world frame of a geom that cannot be moved"""
    return S.lR[g], S.lp[g]


# ---------------------------------------------------------------------------------------------------------------- family T
def touching_case(S, gA, gB, delta, rng, parallel=False):
    """-> dict(xpos, xmat [float32], cert, feature) or None when the pair cannot be posed (two geoms of one body, both fixed)"""
    mA, mB = S.movable[gA], S.movable[gB]
    if not (mA or mB) or (mA and mB and S.fb[gA] == S.fb[gB]):
        return None
    tA, tB = S.gtype[gA], S.gtype[gB]
    lB, aB = b_feature(S, gB, rng)
    lA, name = a_direction(S, gA, rng) if tA != PLANE else (np.array([0, 0, 1.0]), "plane")
    # A sphere B of radius r holds no point delta below its surface more than r - |delta - r| inside: where that is below delta / 4 (the 0.6 mm
    # spheres of the ALOHA fingers at delta = 1e-3) A's support point cannot be the witness.  There A presents a facet interior or smooth point
    # as well, and the witness is the middle of the dip, which must lie delta / 4 inside BOTH geoms.
    small = bool(tB == SPHERE and tA != PLANE and S.gsize[gB][0] - abs(delta - S.gsize[gB][0]) < delta / 4)
    if small:
        (lA, aA), name = b_feature(S, gA, rng), "interior"
    if parallel:                                                # two boxes with parallel axes, edge against edge
        i = rng.integers(3)
        lA = np.roll([1, 1, 0.0], i) / np.sqrt(2) * rng.choice([-1.0, 1.0])
        lB, name = -lA, "parallel edge"
        aB = lB * np.sqrt(2) * S.gsize[gB] * (np.abs(lB) > 0) + (np.abs(lB) == 0) * rng.uniform(-0.5, 0.5) * S.gsize[gB]
    spin = lambda: rng.uniform(0, 2 * np.pi)
    if mB:
        if mA:
            n = [rand_unit(rng), np.eye(3)[rng.integers(3)] * rng.choice([-1.0, 1.0])][int(rng.integers(3) == 0)]
            RA, pA = rot_map(lA, n, spin()), np.array([0.1, 0.05, 0.6]) + rng.uniform(-0.05, 0.05, 3)
        else:
            RA, pA = _world(S, gA)
            n = RA @ lA if parallel or small or tA in (PLANE, BOX, CYLINDER) or rng.integers(2) else rand_unit(rng)
        RB = RA if parallel else rot_map(lB, -n, spin())
    else:
        RB, pB = _world(S, gB)
        n = -(RB @ lB)
        RA, pA = (RB if parallel else rot_map(lA, n, spin())), np.array([0.1, 0.05, 0.6])
    if tA == PLANE:
        sA = pA + RA @ np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 0.0])
    elif small:
        sA = pA + RA @ aA
    else:
        sA = S.support_point(gA, (RA, pA), n)
    xp, xm = far_frames(S)
    pA0 = pA
    if mB:
        pB = sA - delta * n - RB @ aB
        if tB == PLANE:
            return None
    else:
        anchor = pB + RB @ aB
        if tB == PLANE:                                         # the point of the plane under A's support point
            anchor = sA - ((sA - pB) @ (RB[:, 2])) * RB[:, 2]
        pA = pA + (anchor + delta * n - sA)
    if mA:
        _place(S, xp, xm, gA, RA, pA)
    if mB:
        _place(S, xp, xm, gB, RB, pB)
    xp, xm = _round(xp, xm)
    P, R = S.poses(xp, xm)
    poseA, poseB = (R[gA], P[gA]), (R[gB], P[gB])
    if tA == PLANE:
        x = P[gB] + R[gB] @ aB
        deep, own = S.inside(gA, poseA, x), S.inside(gB, poseB, x)
    elif small:
        x = P[gA] + R[gA] @ (aA - 0.5 * delta * lA)
        deep, own = S.inside(gB, poseB, x), S.inside(gA, poseA, x)
        return dict(xpos=xp, xmat=xm, cert=bool(deep >= delta / 4 and own >= delta / 4), deep=deep, own=own, feature=name, n=n)
    else:
        x = P[gA] + R[gA] @ (RA.T @ (sA - pA0))                # the same point of A (where a face or an edge is presented, rounding moves the support point)
        deep, own = S.inside(gB, poseB, x), S.inside(gA, poseA, x)
    return dict(xpos=xp, xmat=xm, cert=bool(deep >= delta / 4 and own >= -1e-7), deep=deep, own=own, feature=name, n=n)


def _featured_hulls(S):
    """the smallest, the largest and a middle hull of the scene"""
    hs = sorted(S.verts, key=lambda g: (len(S.verts[g]), g))
    return {hs[0], hs[-1], hs[len(hs) // 2]}


def _pairs_by_type(S):
    out = {}
    for k in range(len(S.pairs)):
        out.setdefault(S.type_pair(k), []).append(k)
    return out


def _pick_pairs(S, ks, n, rng):
    """n pairs of ks: those with a featured hull first (smallest, largest, middle), then at random"""
    feat = _featured_hulls(S)
    first = [k for k in ks if S.p1[k] in feat or S.p2[k] in feat]
    rng.shuffle(first)
    seen = set()
    lead = []
    for k in first:                                             # one pair per featured hull in front
        h = [g for g in (S.p1[k], S.p2[k]) if g in feat and g not in seen]
        if h:
            seen.update(h)
            lead.append(k)
    rest = [ks[i] for i in rng.permutation(len(ks))]
    return (lead + rest)[:n] if n <= len(lead) + len(rest) else [(lead + rest)[i % len(lead + rest)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def family_t(name, per_cell, seed=1):
    """-> list of dict(k, role, delta, type, xpos, xmat, cert, ...), `per_cell` cases per (type pair, delta, role order)"""
    S = setup(name).scene
    assert S.device_frames, "build a probe first: the cases are posed with the geom frames the device holds"
    rng = np.random.default_rng(seed)
    out = []
    for tp, ks in sorted(_pairs_by_type(S).items()):
        for delta in T_DELTAS:
            for role in (0, 1):
                made = 0
                for k in _pick_pairs(S, ks, 8 * per_cell, rng):
                    gA, gB = (S.p1[k], S.p2[k]) if role == 0 else (S.p2[k], S.p1[k])
                    par = tp == "box|box" and made % 2 == 1
                    c = touching_case(S, gA, gB, delta, rng, parallel=par)
                    if c is None:
                        continue
                    c.update(k=k, role=role, delta=delta, type=tp, A=gA, B=gB)
                    out.append(c)
                    made += 1
                    if made == per_cell:
                        break
    # the ends of the pair list and of its blocks: the first and the last pair, the pairs on either side of a 64-lane block, of the tree's
    # four-block trip and of the SO100 engine's PAIR_CHUNK x 64 burst
    for k in sorted({0, 63, 64, 255, 256, 2047, 2048, len(S.pairs) - 2, len(S.pairs) - 1} & set(range(len(S.pairs)))):
        for role in (0, 1):
            gA, gB = (S.p1[k], S.p2[k]) if role == 0 else (S.p2[k], S.p1[k])
            c = touching_case(S, gA, gB, 1e-5, rng)
            if c is not None and (c["cert"] or role == 1):
                c.update(k=k, role=("list position", k), delta=1e-5, type=S.type_pair(k), A=gA, B=gB)
                out.append(c)
                break
        else:
            raise AssertionError(f"pair {k} of the list cannot be posed")
    return out


def one_per_cell(cases, keys=("type", "delta", "role")):
    """the emulator's share: the first case of every cell (family T: a certified one where the cell has any)"""
    out = {}
    for c in cases:
        k = tuple(c[x] for x in keys)
        if k not in out or (not out[k].get("cert", True) and c.get("cert", True)):
            out[k] = c
    return list(out.values())


def check_family_t(name, per_cell):
    """reference alone: every (type pair of the list, delta) cell has certified cases, at most 10 % of a cell fail their certificate; prints the counts"""
    S = setup(name).scene
    cases = family_t(name, per_cell)
    types = set(_pairs_by_type(S))
    stats = {}
    for c in cases:
        s = stats.setdefault((c["type"], c["delta"]), [0, 0])
        s[0] += 1
        s[1] += not c["cert"]
    for (tp, d), (n, bad) in sorted(stats.items()):
        print(f"{name} T {tp} delta {d:g}: {n - bad} certified, {bad} left out ({100.0 * bad / n:.0f} %)")
        assert bad <= 0.1 * n and n - bad >= 1, (name, tp, d, n, bad)
    assert set(stats) == {(tp, d) for tp in types for d in T_DELTAS}, (types, set(stats))
    hulls = {g for c in cases if c["cert"] for g in (c["A"], c["B"]) if S.gtype[g] == MESH}
    assert _featured_hulls(S) <= hulls, (_featured_hulls(S), "not all covered")
    return stats


# ---------------------------------------------------------------------------------------------------------------- family S
def near_miss_case(S, k, delta, kind, rng):
    """pair k lifted delta clear along a designed direction; kind: "table" (geom 2 a hull) or "obb".  -> dict(xpos, xmat) or None"""
    g1, g2 = S.p1[k], S.p2[k]
    m1, m2 = S.movable[g1], S.movable[g2]
    t1, t2 = S.gtype[g1], S.gtype[g2]
    if not (m1 or m2) or (m1 and m2 and S.fb[g1] == S.fb[g2]) or (kind == "table" and t2 != MESH) or (kind == "obb" and t1 == PLANE) or (kind == "world" and t1 != PLANE):
        return None
    R1, p1 = (rand_rot(rng), np.array([0.1, 0.05, 0.6])) if m1 else _world(S, g1)
    R2, p2 = (rand_rot(rng), np.zeros(3)) if m2 else _world(S, g2)
    if kind == "world":                                         # the lowest corner of the other geom's box delta above the plane
        n = R1[:, 2]
        q2 = p1 + R1 @ np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 0.0])
        low = (q2 + R2 @ S.bc[g2]) @ n - np.abs(R2.T @ n) @ S.bh[g2]
        shift = q2 + (p1 @ n - low + delta) * n - p2
    elif kind == "obb":
        i, j = rng.integers(3), rng.integers(3)
        if m2:
            n = R1[:, i] * rng.choice([-1.0, 1.0])
            R2 = rot_map(np.eye(3)[j], -n, rng.uniform(0, 2 * np.pi))
        else:
            n = -R2[:, j] * rng.choice([-1.0, 1.0])
            R1 = rot_map(np.eye(3)[i], n, rng.uniform(0, 2 * np.pi))
        ca = p1 + R1 @ S.bc[g1]
        cb = ca + (S.bh[g1][i] + S.bh[g2][j] + delta) * n
        shift = cb - (p2 + R2 @ S.bc[g2])
    else:
        gd = grid_dir(rng)                                      # the hull's table is exact along this geom-frame direction
        l1 = {BOX: np.eye(3)[rng.integers(3)] * rng.choice([-1.0, 1.0]), PLANE: np.array([0, 0, 1.0]), SPHERE: rand_unit(rng), MESH: grid_dir(rng)}.get(t1)
        if l1 is None:                                          # capsule, cylinder: along the axis, radial, or any direction (centre to centre)
            a = rng.uniform(0, 2 * np.pi)
            l1 = [np.array([0, 0, rng.choice([-1.0, 1.0])]), np.array([np.cos(a), np.sin(a), 0]), rand_unit(rng)][rng.integers(3)]
        if m2:
            n = R1 @ l1
            R2 = rot_map(gd, -n, rng.uniform(0, 2 * np.pi))
        else:
            n = -(R2 @ gd)
            R1 = rot_map(l1, n, rng.uniform(0, 2 * np.pi))
        if t1 == PLANE:                                         # the hull's lowest point delta above the plane
            q2 = p1 + R1 @ np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 0.0])
            low = -S.extent([g2], [-n], {g2: q2}, {g2: R2})[0]
            shift = q2 + (p1 @ n - low + delta) * n - p2
        else:
            shift = p1 + R1 @ S.bc[g1] - (p2 + R2 @ S.bc[g2])   # box centres on one line along n ...
            Pq, Rq = {g1: p1, g2: p2 + shift}, {g1: R1, g2: R2}
            gap = -S.extent([g2], [-n], Pq, Rq)[0] - S.extent([g1], [n], Pq, Rq)[0]
            shift = shift + (delta - gap) * n                   # ... and the exact gap along n is delta
    xp, xm = far_frames(S)
    if m2:
        if m1:
            _place(S, xp, xm, g1, R1, p1)
        _place(S, xp, xm, g2, R2, p2 + shift)
    else:
        _place(S, xp, xm, g1, R1, p1 - shift)
    xp, xm = _round(xp, xm)
    return dict(xpos=xp, xmat=xm, n=n)


S_STATS = {}                                    # (name, per_cell) -> {(type, delta, kind): [made, kept, within BAND]}


@functools.lru_cache(maxsize=None)
def family_s(name, per_cell, seed=2):
    """-> list of dict(k, delta, kind, type, xpos, xmat, margin, margin_nosbt) of the near misses whose fp64 designed_margin (tables on) exceeds
    BAND; needs the tables (setup(name).probe(kind) must have run)"""
    S = setup(name).scene
    assert S.sbt is not None and S.device_frames
    rng = np.random.default_rng(seed)
    out = []
    stats = S_STATS[(name, per_cell)] = {}
    for tp, ks in sorted(_pairs_by_type(S).items()):
        for delta in S_DELTAS:
            for kind in ("table", "obb", "world"):
                made = 0
                st = stats.setdefault((tp, delta, kind), [0, 0, 0])
                kinds = 1 + (tp.endswith("|mesh") and tp != "plane|mesh" or tp == "plane|mesh")
                want = per_cell if kinds == 1 else (per_cell + 1) // 2          # the same number per pair type, whether it has one kind of near miss or two
                for k in _pick_pairs(S, ks, 8 * per_cell, rng):
                    c = near_miss_case(S, k, delta, kind, rng)
                    if c is None:
                        continue
                    P, R = S.poses(c["xpos"], c["xmat"])
                    idx = np.array([k])
                    w = S.world_margin(P, R, idx)[0]
                    o = S.obb_margin(idx, P, R)[0]
                    c.update(k=k, delta=delta, kind=kind, type=tp, margin=max(w, o, S.table_margin(idx, P, R)[0]), margin_nosbt=max(w, o))
                    made += 1
                    st[0] += 1
                    st[2] += abs(c["margin"]) <= BAND
                    if c["margin"] > BAND:
                        st[1] += 1
                        out.append(c)
                    if made == want:
                        break
    return out


def check_family_s(name, per_cell, need=50):
    """reference alone: at least `need` near misses per pair type, at most 5 % of a cell within BAND of the decision; prints the counts"""
    cases = family_s(name, per_cell)
    per_type = {}
    for (tp, d, kind), (made, kept, band) in sorted(S_STATS[(name, per_cell)].items()):
        if made:
            print(f"{name} S {tp} delta {d:g} {kind}: {made} built, {kept} with designed_margin > BAND, {band} within BAND")
            assert band <= 0.05 * made, (name, tp, d, kind, made, band)
        per_type[tp] = per_type.get(tp, 0) + kept
    assert set(per_type) == set(_pairs_by_type(setup(name).scene)) and min(per_type.values()) >= need, per_type
    return per_type, len(cases)


# ---------------------------------------------------------------------------------------------------------------- family R
def _jitter(S, xp, xm, free, rng):
    xp, xm = xp.copy(), xm.copy()
    for b in free:
        xp[b] += rng.uniform(-5e-3, 5e-3, 3)
        xm[b] = small_rot(rng, 0.05) @ xm[b]
    return xp, xm


@functools.lru_cache(maxsize=None)
def family_r(name, limit=None, seed=3):
    """-> xpos [n, nb, 3], xmat [n, nb, 3, 3] float32: the real states, each followed by its jittered copy"""
    S = setup(name).scene
    rng = np.random.default_rng(seed)
    frames = []
    if name.startswith("so100_"):
        from tests.raycast_ref import RaycastRef
        rc = RaycastRef(setup(name).f64)
        ids = list(rc.arm) + list(rc.free) if S.engine == 0 else list(range(len(rc.par)))      # (on a tree build: every body of the blob, the static ones too)
        free = [ids.index(b) for b in rc.free]
        qs = []
        for f in ("contact_rich_states", "probe_outlier_states"):
            with open(os.path.join(GOLDEN, f + ".json")) as fh:
                qs += [s["qpos"] for s in json.load(fh)["states"]]
        for q in qs[:limit]:
            Pb, Rb = rc.body_frames(np.asarray(q, dtype=np.float32).astype(np.float64))
            xp, xm = S.rest_frames()
            xp[:len(ids)], xm[:len(ids)] = np.stack([Pb[b] for b in ids]), np.stack([Rb[b] for b in ids])
            frames.append((xp, xm))
    else:
        from tests import tree_contact_cases as tc
        from tests.tree_raycast_ref import TJ_FREE, TreeRaycastRef
        rc = TreeRaycastRef(setup(name).f64)
        free = [b for b in range(len(rc.par)) if rc.jtype[b] == TJ_FREE]
        Q = tc.states("dining" if name == "dining" else "handover")[0]
        for e in range(Q.shape[1])[:limit]:
            Pb, Rb = rc.body_frames(Q[:, e].astype(np.float32).astype(np.float64))
            xp, xm = S.rest_frames()
            xp[:len(Pb)], xm[:len(Pb)] = Pb, np.stack(Rb)
            frames.append((xp, xm))
    out = []
    for xp, xm in frames:
        out += [(xp, xm), _jitter(S, xp, xm, free, rng)]
    return np.array([f[0] for f in out], np.float32), np.array([f[1] for f in out], np.float32)


# ---------------------------------------------------------------------------------------------------------------- family O
@functools.lru_cache(maxsize=None)
def family_o(name, n, seed=4):
    """the geoms of every body gathered about one point (the middle of the static geoms), each body with a random rotation: -> xpos, xmat float32, `n` queries in each of which more pairs than the candidate
    list holds pass the world boxes, none of the first (capacity + 1) of them within BAND of the decision"""
    su = setup(name)
    S = su.scene
    rng = np.random.default_rng(seed)
    XP, XM = [], []
    st = np.nonzero(~S.movable & (S.gtype != PLANE))[0]
    target = (S.lp[st] + np.einsum("gij,gj->gi", S.lR[st], S.bc[st])).mean(axis=0) if len(st) else np.array([0.0, 0.0, 0.6])
    for _ in range(20 * n):
        xp, xm = S.rest_frames()
        for b in range(S.nb):
            if S.engine == 0 or b > 0:
                on = np.nonzero(S.fb == b)[0]
                if len(on) == 0:
                    continue
                c = (S.lp[on] + np.einsum("gij,gj->gi", S.lR[on], S.bc[on])).mean(axis=0)      # the body's geoms gathered about the target point
                xm[b] = rand_rot(rng)
                xp[b] = target + rng.uniform(-0.01, 0.01, 3) - xm[b] @ c
        xp, xm = _round(xp, xm)
        P, R = S.poses(xp, xm)
        w = S.world_margin(P, R)
        passing = np.nonzero(w <= 0)[0]
        if len(passing) <= su.cap:
            continue
        upto = passing[su.cap]
        if np.any(np.abs(w[:upto + 1]) <= max(BAND, 1e-7)):
            continue
        XP.append(xp); XM.append(xm)
        if len(XP) == n:
            break
    assert len(XP) == n, (name, len(XP))
    return np.array(XP), np.array(XM)


# ---------------------------------------------------------------------------------------------------------------- running and checking
def run(su, kind, xpos, xmat, sbt=True):
    """the probe on a batch -> kept [nq, npair] bool, overflow [nq], after check 5's list mechanics: every one of the ncand words
    decodes to a pair of the list in the list's geom order, strictly increasing list position (so no duplicates)"""
    S = su.scene
    ncand, cand, over = su.probe(kind, sbt).run(xpos, xmat)
    nq = len(ncand)
    kept = np.zeros((nq, len(S.pairs)), bool)
    lut = -np.ones((256, 256), int)
    lut[S.p1, S.p2] = np.arange(len(S.pairs))
    for q in range(nq):
        n = int(ncand[q])
        assert 0 <= n <= su.cap, (q, n)
        w = cand[q, :n]
        assert np.all((w & 0xff00ff00) == 0), (q, "ncand counts a slot that holds no candidate word")
        pos = lut[w & 0xffff, w >> 16]
        assert np.all(pos >= 0), (q, "a candidate that is no pair of the list, or in the other geom order")
        assert np.all(np.diff(pos) > 0), (q, "candidates out of pair-list order, or twice")
        kept[q, pos] = True
        # the rest of the store (filled with 0xffffffff before the call): untouched, or what the world-box pass left there before the list was
        # compacted in place - pairs of the list that pass the world boxes, no more of them than the pass can have written
        t = cand[q, n:]
        t = t[t != 0xffffffff]
        assert np.all((t & 0xff00ff00) == 0) and np.all(lut[t & 0xffff, t >> 16] >= 0), (q, "a foreign word beyond ncand")
        P, R = S.poses(xpos[q], xmat[q])
        wm = S.world_margin(P, R)
        assert n + len(t) <= min(int((wm <= BAND).sum()), su.cap), (q, n, len(t), "more slots written than pairs pass the world boxes")
        assert np.all(wm[lut[t & 0xffff, t >> 16]] <= BAND), (q, "a left-over word of a pair the world boxes separate")
    assert np.all((over == 0) | (over == 1))
    return kept, over, (ncand, cand)


def check_certified(su, cases, kept):
    """check 2: every certified pair of family T is a candidate"""
    miss = [(c["type"], c["delta"], c["role"], int(c["A"]), int(c["B"]), c["feature"]) for c, kq in zip(cases, kept) if c["cert"] and not kq[c["k"]]]
    assert not miss, (su.name, len(miss), miss[:5])
    return sum(c["cert"] for c in cases)


def check_dropped(su, xpos, xmat, kept, worst=None):
    """check 3: every pair the device dropped has a direction of the designed family with an exact fp64 separation >= -1e-6 m.  Pairs whose
    bounding spheres are apart are proven separated by those.  -> the worst (smallest) separation seen"""
    S = su.scene
    worst = dict(sep=np.inf) if worst is None else worst
    for q in range(len(kept)):
        P, R = S.poses(xpos[q], xmat[q])
        drop = np.nonzero(~kept[q])[0]
        near = drop[S.sphere_gap(drop, P, R) <= 0]
        if len(near) == 0:
            continue
        sep, d = S.separation(near, P, R)
        j = int(np.argmin(sep))
        if sep[j] < worst["sep"]:
            worst.update(sep=float(sep[j]), pair=(int(S.p1[near[j]]), int(S.p2[near[j]])), type=S.type_pair(near[j]), dir=d[j], query=q)
        assert sep[j] >= SAFETY, (su.name, "dropped a pair no designed direction separates", worst)
    return worst


def check_tight(su, xpos, xmat, kept, tables=True, band=None, stat=None):
    """check 4: the device keeps a pair iff designed_margin <= 0, for every pair whose |designed_margin| exceeds the band.
    -> dict(inside: pairs within the band, disagree: largest |margin| at which the decisions differ (0: none), kept/ref counts)"""
    S = su.scene
    band = BAND if band is None else band
    stat = dict(inside=0, disagree=0.0, conservative=0, pairs=0, kept=0) if stat is None else stat
    for q in range(len(kept)):
        P, R = S.poses(xpos[q], xmat[q])
        mg = S.designed_margin(P, R, tables, beyond=min(band, 2e-5))
        dis = (mg <= 0) != kept[q]
        if dis.any():
            k = np.nonzero(dis)[0][int(np.argmax(np.abs(mg[dis])))]
            if abs(mg[k]) > stat["disagree"]:
                stat.update(disagree=float(abs(mg[k])), at=(q, int(S.p1[k]), int(S.p2[k]), S.type_pair(k), float(mg[k])))
        bind = np.abs(mg) > band
        stat["inside"] += int((~bind).sum()); stat["pairs"] += len(mg); stat["kept"] += int(kept[q].sum())
        bad = np.nonzero(dis & bind)[0]
        stat["conservative"] += int((kept[q][bad] & (mg[bad] > 0)).sum())
        assert len(bad) == 0, (su.name, "tables" if tables else "no tables", q,
                               [(int(S.p1[k]), int(S.p2[k]), S.type_pair(k), float(mg[k]), bool(kept[q][k])) for k in bad[:5]])
    return stat


def check_capacity(su, xpos, xmat, kept, over, tables=True):
    """check 6 on family O: overflow set, ncand <= capacity, the list = the oriented-box and table filter on the first `capacity` survivors of
    the world boxes in pair order (pairs within BAND of a decision are not compared)"""
    S = su.scene
    idx = np.arange(len(S.pairs))
    for q in range(len(kept)):
        assert over[q] == 1 and kept[q].sum() <= su.cap, (q, over[q], kept[q].sum())
        P, R = S.poses(xpos[q], xmat[q])
        w = S.world_margin(P, R)
        first = np.nonzero(w <= 0)[0][:su.cap]
        o = np.maximum(S.obb_margin(idx, P, R), S.table_margin(idx, P, R) if tables else -np.inf)
        want = np.zeros(len(idx), bool)
        want[first] = o[first] <= 0
        bind = np.ones(len(idx), bool)
        bind[first] = np.abs(o[first]) > BAND
        assert np.array_equal(want[bind], kept[q][bind]), (su.name, q, np.nonzero(want != kept[q])[0][:8])
    return int(kept.sum())


def check_batch(su, kind, xpos, xmat, label):
    """checks 3, 4, 5 and the clear overflow bit on one batch, with the tables and with SO101_NO_SBT.  -> {tables: dict(kept, raw, worst, stat)};
    prints the worst separation of check 3, the largest |designed_margin| at which device and fp64 differ, and the candidate counts"""
    out = {}
    for sbt in (True, False):
        kept, over, raw = run(su, kind, xpos, xmat, sbt)
        assert not over.any(), (su.name, label, "overflow bit outside family O")
        worst = check_dropped(su, xpos, xmat, kept)
        stat = check_tight(su, xpos, xmat, kept, tables=sbt)
        print(f"{su.name} {kind} {label} {'tables' if sbt else 'SO101_NO_SBT'}: {len(kept)} queries, {int(kept.sum())} candidates, worst separation of a dropped pair "
              f"{worst['sep']:.3e} m ({worst.get('type')}), largest |designed_margin| with device != fp64 {stat['disagree']:.3e} m {stat.get('at', '')}, "
              f"{stat['inside']} of {stat['pairs']} pairs within BAND {BAND:.1e}")
        out[sbt] = dict(kept=kept, raw=raw, worst=worst, stat=stat)
    assert np.all(out[False]["kept"] | ~out[True]["kept"]), "the tables added a candidate"
    return out


def check_touching(name, kind, cases):
    """family T on one backend: checks 2 - 5"""
    su = setup(name)
    xp, xm = np.array([c["xpos"] for c in cases]), np.array([c["xmat"] for c in cases])
    out = check_batch(su, kind, xp, xm, "T")
    for sbt in (True, False):
        n = check_certified(su, cases, out[sbt]["kept"])
    print(f"{name} {kind} T: {n} certified touching pairs of {len(cases)} cases kept, with and without the tables")
    cells = {(c["type"], c["delta"]) for c in cases}
    assert cells == {(c["type"], c["delta"]) for c in cases if c["cert"]}, "a (type pair, delta) cell without a certified case"
    return out


def check_near_misses(name, kind, cases):
    """family S on one backend: checks 3 - 5; the pair of every case is dropped with the tables, and without them iff a box axis separates it"""
    su = setup(name)
    xp, xm = np.array([c["xpos"] for c in cases]), np.array([c["xmat"] for c in cases])
    out = check_batch(su, kind, xp, xm, "S")
    for q, c in enumerate(cases):
        assert not out[True]["kept"][q][c["k"]], (name, "a near miss along a designed direction is kept", c["type"], c["kind"], c["delta"], c["margin"])
        if abs(c["margin_nosbt"]) > BAND:
            assert out[False]["kept"][q][c["k"]] == (c["margin_nosbt"] <= 0), (name, "SO101_NO_SBT", c["type"], c["kind"], c["delta"], c["margin_nosbt"])
    tab = [c for c in cases if c["kind"] == "table"]
    only = sum(c["margin_nosbt"] <= 0 for c in tab)
    print(f"{name} {kind} S: {len(cases)} near misses dropped with the tables; of the {len(tab)} along a table direction {only} are kept under SO101_NO_SBT")
    assert not tab or only > 0, "no near miss that only the tables separate: the table filter is not exercised"
    return out


def check_over_capacity(name, kind, n):
    su = setup(name)
    su.probe(kind)
    xp, xm = family_o(name, n)
    for sbt in (True, False):
        kept, over, raw = run(su, kind, xp, xm, sbt)
        total = check_capacity(su, xp, xm, kept, over, tables=sbt)
        print(f"{name} {kind} O {'tables' if sbt else 'SO101_NO_SBT'}: {n} queries over capacity {su.cap}, {total} candidates kept")


def check_same_decisions(name_a, name_b, kind, xa, ma, xb, mb):
    """two builds on the same frames (each in its own body numbering): the decisions agree wherever check 4 binds them; -> (kept a, kept b)"""
    a, b = setup(name_a), setup(name_b)
    ka, kb = run(a, kind, xa, ma)[0], run(b, kind, xb, mb)[0]
    assert np.array_equal(a.scene.pairs, b.scene.pairs)
    for q in range(len(ka)):
        P, R = a.scene.poses(xa[q], ma[q])
        bind = np.abs(a.scene.designed_margin(P, R, beyond=BAND)) > BAND
        assert np.array_equal(ka[q][bind], kb[q][bind]), (name_a, name_b, q, np.nonzero(ka[q] != kb[q])[0][:8])
    return ka, kb
