"""Hull support queries and the per-hull tables built on them, against an fp64 brute force.

The support point of a hull in a direction is the vertex with the largest dot product, the smallest index winning ties.  The device
functions of so101_geom.hpp run in the probe kernels of tests/devprims (one query per 64-lane workgroup, the hull at the origin with the
identity rotation, so a support point is a vertex float for float); the tables come from so101_tables.hpp, the builder both engines call.
  paths agree       every support() / support_patch() path (NoCache, HullCache, HullLDS with 256 / 512 / 0 slots, HullLDS under G16, HullSub)
                    returns the NoCache point bit for bit
  matches fp64      the point scores within 1e-6 sum|v||d| of the fp64 maximum and is the fp64 argmax wherever the runner-up is further behind;
                    on exact-tie shapes (dyadic coordinates and directions) the smallest index wins on every path
  bound table       hull_sbt equals the fp64 maxima rounded up to float, bit for bit; sbt_bound() >= h - 2e-6 (the slack sbt_lowest takes)
                    and stays within 20 % of the hull's largest vertex norm above it
  lists             every cell's list is non-empty, sorted, duplicate-free and holds the vertices' own floats; in the cell widened by up to
                    3.9e-3 rad (the builder guarantees 4e-3) the fp64 argmax is in the list and support<HullSub> equals support<NoCache>
  cells             hl_cell() agrees with the fp64 cell away from boundaries and returns a cell whose closed region holds the direction on them;
                    light_first_cell() picks the box face the first way scan_faces() does (ties of lb0 / lb1: the lower axis)
The `gpu` tests run everything on the MI355X; the CPU suite runs the emulated build on a subset (two scene hulls, 24 cells, synthetic hulls
up to 513 vertices) and feeds non-finite directions, which never go to the GPU."""
import itertools
import json
import os

import numpy as np
import pytest

from so101_sim_amd.model import blob as blobfmt
from so101_sim_amd.model import scenes
from tests import devprims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_PLANE, G_BOX, G_MESH = 0, 4, 5
SIZES = [4, 8, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1080, 5676]
CPU_SIZES = [s for s in SIZES if s <= 513]
F64 = np.float64


# ------------------------------------------------------------------ hulls
def _mesh_hulls(raw):
    m = blobfmt.unpack(raw)
    mv = m["mesh_vert"].reshape(-1, 3).astype(np.float32)
    return [mv[a:a + n] for t, a, n in zip(m["geom_type"], m["geom_vertadr"], m["geom_vertnum"]) if t == G_MESH]


_SCENES = None


def scene_hulls():
    """every distinct mesh of the SO100 banana / pen, ALOHA banana / pen and Dining scenes"""
    global _SCENES
    if _SCENES is None:
        raws = [("so100_banana", scenes.load_blob("banana", "f32")[0]), ("so100_pen", scenes.load_blob("pen", "f32")[0]),
                ("aloha_banana", scenes.load_aloha_blob("banana", "f32")[0]), ("aloha_pen", scenes.load_aloha_blob("pen", "f32")[0]),
                ("dining", scenes.load_dining_blob("banana", "f32")[0])]
        out, seen = {}, set()
        for name, raw in raws:
            for k, V in enumerate(_mesh_hulls(raw)):
                if V.tobytes() not in seen:
                    seen.add(V.tobytes())
                    out[f"{name}[{k}]:{len(V)}"] = V
        _SCENES = out
    return _SCENES


def ellipsoid(n, seed):
    rng = np.random.RandomState(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return (p * [0.06, 0.04, 0.03] + [0.01, -0.02, 0.005]).astype(np.float32)


def surface_grid(k, a=2.0 ** -5):
    """the points of a k x k x k grid over [-a, a]^3 that lie on the cube's surface: dyadic, with exact ties in every axis direction"""
    t = np.linspace(-a, a, k)
    pts = [p for p in itertools.product(t, t, t) if np.max(np.abs(p)) == a]
    return np.array(pts, np.float32)


def prism():
    """a triangular prism with edge midpoints, dyadic coordinates"""
    tri = [(0, 0), (2 ** -4, 0), (0, 2 ** -4), (2 ** -5, 0), (0, 2 ** -5), (2 ** -5, 2 ** -5)]
    return np.array([(x, y, z) for z in (-2 ** -5, 0.0, 2 ** -5) for x, y in tri], np.float32)


def tie_hulls():
    cube = np.array(list(itertools.product([-2 ** -5, 2 ** -5], repeat=3)), np.float32)
    g5 = surface_grid(5)
    return {"cube:8": cube, "cube_twice:16": np.concatenate([cube, cube]), "prism:18": prism(), "grid5:98": g5,
            "grid5_dup64:128": np.concatenate([g5[:64], g5[:64]]), "grid9:386": surface_grid(9), "grid13:866": surface_grid(13)}


def synthetic_hulls(sizes):
    out = {f"ellipsoid:{n}": ellipsoid(n, n) for n in sizes}
    e = ellipsoid(65, 7)
    e[64] = e[0]
    out["ellipsoid_dup:65"] = e
    return out


def cpu_hulls():
    sc = scene_hulls()
    names = list(sc)
    big = max((k for k in names if len(sc[k]) <= 1080), key=lambda k: len(sc[k]))      # (the largest hull whose lists the product mostly uses)
    picked = {names[0]: sc[names[0]], big: sc[big]}
    return {**picked, **synthetic_hulls(CPU_SIZES), **tie_hulls()}


def gpu_hulls():
    return {**scene_hulls(), **synthetic_hulls(SIZES), **tie_hulls()}


# ------------------------------------------------------------------ directions
def unit(a):
    a = np.asarray(a, F64)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def random_dirs(n, seed):
    return unit(np.random.RandomState(seed).normal(size=(n, 3)))


def dyadic_dirs():
    """components in {0, +-1/2, +-1}, with both signs of zero: every dot product with a dyadic hull is exact in float"""
    v = [-1.0, -0.5, 0.0, -0.0, 0.5, 1.0]
    d = np.array([p for p in itertools.product(v, repeat=3) if np.any(np.array(p) != 0)], np.float32)
    return d


def adversarial_dirs():
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    diag = np.array([p for p in itertools.product([-1, 0, 1], repeat=3) if any(p)], F64)
    return np.concatenate([axes.astype(np.float32), unit(diag), dyadic_dirs()])


def patch_frames(dirs):
    """f = -d (the first patch direction is d), u, v an orthonormal pair across it"""
    f = -np.asarray(dirs, F64)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    a = np.where(np.abs(f[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])
    u = np.cross(f, a)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(f, u)
    return np.concatenate([f, u, v], axis=1).astype(np.float32)


def patch_dirs64(frames):
    """the NCPP directions support_patch() queries, in fp64 (so101_geom.hpp support_patch)"""
    fr = frames.astype(F64)
    f, u, v = fr[:, 0:3], fr[:, 3:6], fr[:, 6:9]
    out = []
    for k in range(devprims.NCPP):
        su = 1.0 if k in (1, 4) else -1.0
        sv = 1.0 if k in (1, 2) else -1.0
        e = 0.0 if k == 0 else 1e-3 * 0.70710678
        d = -f + e * (su * u + sv * v)
        out.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    return np.stack(out, axis=1)


# ------------------------------------------------------------------ fp64 references
def check_fp64(V, D64, P, exact=False, what=""):
    """P: points returned for the directions D64.  Near-optimal in fp64; the fp64 argmax wherever the gap to the runner-up point exceeds
    the tolerance; exact=True: the first fp64 argmax for every direction (dyadic data, no rounding anywhere)"""
    V64 = V.astype(F64)
    for s in range(0, len(D64), 256):
        D, Q = D64[s:s + 256], P[s:s + 256].astype(F64)
        S = D @ V64.T
        best, first = S.max(1), S.argmax(1)
        tol = 1e-6 * (np.abs(D) @ np.abs(V64).T).max(1)
        got = (Q * D).sum(1)
        bad = got < best - tol
        assert not bad.any(), f"{what}: support point {np.abs(best - got)[bad].max():.3g} below the fp64 maximum"
        same = np.all(V64[None, :, :] == V64[first][:, None, :], axis=2)
        runner = np.where(same, -np.inf, S).max(1)
        decided = (best - runner > tol) | exact
        wrong = decided & ~np.all(Q == V64[first], axis=1)
        assert not wrong.any(), f"{what}: {wrong.sum()} directions return another vertex than the fp64 argmax, e.g. {D[wrong][0]}: {Q[wrong][0]} != {V64[first][wrong][0]}"


def sbt_ref(V):
    """the support-bound table by its definition: fp64 maximum over the vertices, summed as (x c0 + y c1) + z c2, rounded up to float"""
    V64 = V.astype(F64)
    out = np.empty(6 * 25, np.float32)
    for face in range(6):
        ax, sg = face // 2, (-1.0 if face & 1 else 1.0)
        for iu in range(5):
            for iv in range(5):
                c = np.zeros(3)
                c[ax], c[(ax + 1) % 3], c[(ax + 2) % 3] = sg, -1.0 + 0.5 * iu, -1.0 + 0.5 * iv
                best = ((V64[:, 0] * c[0] + V64[:, 1] * c[1]) + V64[:, 2] * c[2]).max()
                f = np.float32(best)
                if F64(f) < best:
                    f = np.nextafter(f, np.float32(np.inf))
                out[(face * 5 + iu) * 5 + iv] = f
    return out


def cell_ref(D):
    """fp64 cube-map cell of directions and the distance of each from the nearest cell boundary (face coordinates)"""
    D = np.asarray(D, F64)
    a = np.abs(D)
    ax = np.argmax(a, axis=1)
    r = np.arange(len(D))
    dm = D[r, ax]
    u, v = D[r, (ax + 1) % 3] / np.abs(dm), D[r, (ax + 2) % 3] / np.abs(dm)
    gu, gv = (u + 1) * 4, (v + 1) * 4
    iu, iv = np.clip(np.floor(gu), 0, 7).astype(int), np.clip(np.floor(gv), 0, 7).astype(int)
    second = np.sort(a, axis=1)[:, 1]
    margin = np.minimum.reduce([np.abs(gu - np.round(gu)) / 4, np.abs(gv - np.round(gv)) / 4, (np.abs(dm) - second) / np.abs(dm)])
    return ((2 * ax + (dm < 0)) * 8 + iu) * 8 + iv, margin


def cell_contains(cell, D, tol=1e-6):
    """the closed region of `cell` holds the directions D"""
    D = np.asarray(D, F64)
    face, iu, iv = cell // 64, (cell // 8) % 8, cell % 8
    ax, neg = face // 2, face % 2
    r = np.arange(len(D))
    dm = D[r, ax]
    mx = np.abs(D).max(1)
    ok = (np.abs(dm) >= mx * (1 - tol)) & ((dm < 0) == (neg == 1)) | (np.abs(dm) == 0)
    gu = (D[r, (ax + 1) % 3] / np.abs(dm) + 1) * 4
    gv = (D[r, (ax + 2) % 3] / np.abs(dm) + 1) * 4
    return ok & (gu >= iu - tol * 8) & (gu <= iu + 1 + tol * 8) & (gv >= iv - tol * 8) & (gv <= iv + 1 + tol * 8)


def cell_samples(cell, tilts):
    """directions of the cell widened by at most max(tilts) rad: corners, edge midpoints, a 3 x 3 interior grid, and the boundary
    points tilted outward by each angle across their edge (corners: along the outward diagonal)"""
    face, iu, iv = cell // 64, (cell // 8) % 8, cell % 8
    ax, sg = face // 2, (-1.0 if face % 2 else 1.0)
    eu, ev, em = np.eye(3)[(ax + 1) % 3], np.eye(3)[(ax + 2) % 3], np.eye(3)[ax]
    u0, u1, v0, v1 = -1 + iu / 4, -1 + (iu + 1) / 4, -1 + iv / 4, -1 + (iv + 1) / 4

    def pt(u, v):
        d = sg * em + u * eu + v * ev
        return d / np.linalg.norm(d)

    out = [pt(u0 + (u1 - u0) * a, v0 + (v1 - v0) * b) for a in (0.25, 0.5, 0.75) for b in (0.25, 0.5, 0.75)]
    n_u0, n_u1 = -(eu - u0 * sg * em), eu - u1 * sg * em           # outward normals of the four edges' great circles
    n_v0, n_v1 = -(ev - v0 * sg * em), ev - v1 * sg * em
    bnd = [(pt(u0, (v0 + v1) / 2), [n_u0]), (pt(u1, (v0 + v1) / 2), [n_u1]), (pt((u0 + u1) / 2, v0), [n_v0]), (pt((u0 + u1) / 2, v1), [n_v1]),
           (pt(u0, v0), [n_u0, n_v0]), (pt(u0, v1), [n_u0, n_v1]), (pt(u1, v0), [n_u1, n_v0]), (pt(u1, v1), [n_u1, n_v1])]
    for p, ns in bnd:
        out.append(p)
        o = sum(n / np.linalg.norm(n) for n in ns)
        o = o - (o @ p) * p
        o /= np.linalg.norm(o)
        for t in tilts:
            out.append(np.cos(t) * p + np.sin(t) * o)
    return np.array(out)


# ------------------------------------------------------------------ checks
PATHS = [p for p in devprims.PATHS if p not in ("nocache", "sub")]


def check_paths(probes, V, D, exact, what, npatch=None):
    """npatch: patch frames on the first npatch directions only (the emulated build: five reductions per query)"""
    H = probes.hull(V)
    try:
        D = np.asarray(D, np.float32)
        ref = H.support("nocache", D)
        check_fp64(V, D.astype(F64), ref, exact=exact, what=f"{what} nocache")
        for p in PATHS:
            got = H.support(p, D)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{what}: support<{p}> differs from NoCache"
        cells = probes.hl_cell(D)
        got = H.support("sub", D, cells)
        use = sub_compared(H, cells, got[:, 0], what)
        assert np.array_equal(got[use].view(np.uint32), ref[use].view(np.uint32)), f"{what}: support<HullSub> differs from NoCache"
        frames = patch_frames(D[:npatch])
        pref = H.support_patch("nocache", frames)
        check_fp64(V, patch_dirs64(frames).reshape(-1, 3), pref.reshape(-1, 3), what=f"{what} patch")
        for p in PATHS:
            got = H.support_patch(p, frames)
            assert np.array_equal(got.view(np.uint32), pref.view(np.uint32)), f"{what}: support_patch<{p}> differs from NoCache"
        pcells = probes.hl_cell(-frames[:, :3])
        got = H.support_patch("sub", frames, pcells)
        use = sub_compared(H, pcells, got[:, 0, 0], what)
        assert np.array_equal(got[use].view(np.uint32), pref[use].view(np.uint32)), f"{what}: support_patch<HullSub> differs from NoCache"
    finally:
        H.close()


def sub_compared(H, cells, first, what):
    """the HullSub queries that were compared: exactly those whose cell list the product uses (1 .. HL_MAX entries; the probe returns NaN
    for the others), and on every hull whose lists the product uses at all, most of the queries"""
    cnt = np.diff(H.off.astype(np.int64))
    usable = cnt[cells] <= devprims.HL_MAX
    assert np.array_equal(np.isfinite(first), usable), f"{what}: HullSub answered other queries than those with a usable list"
    if np.mean(cnt <= devprims.HL_MAX) >= 0.5:
        assert usable.mean() >= 0.25, f"{what}: only {usable.mean():.0%} of the HullSub queries compared"
    return usable


def check_tables(probes, V, ncells, what, rng):
    H = probes.hull(V)
    try:
        # bound table: bit for bit
        ref = sbt_ref(V)
        assert np.array_equal(H.sbt.view(np.uint32), ref.view(np.uint32)), f"{what}: support-bound table differs from the fp64 maxima rounded up"
        # lists: structure
        n = len(V)
        cnt = np.diff(H.off.astype(np.int64))
        assert H.off[0] == 0 and np.all(cnt >= 1), f"{what}: empty support-vertex list"
        # useful, not just safe: every scene hull's lists average under 8 % of its vertices (the most, 18 %, on an 8-vertex box; the synthetic
        # 4-vertex hull 32 %) - a list that keeps every vertex passes every membership test below
        assert cnt.mean() <= max(8.0, 0.1 * n), f"{what}: support-vertex lists average {cnt.mean():.1f} of {n} vertices"
        for c in range(devprims.HL_CELLS):
            idx, xyz = H.list_of(c)
            assert np.all((idx >= 0) & (idx < n)) and np.all(np.diff(idx) > 0), f"{what}: cell {c} list not sorted / duplicated / out of range"
            assert np.array_equal(xyz.view(np.uint32), V[idx].view(np.uint32)), f"{what}: cell {c} list entries are not the vertices' floats"
        # lists: contract in the widened cell (device: HullSub = NoCache wherever the product would use the list)
        cells = np.arange(devprims.HL_CELLS) if ncells >= devprims.HL_CELLS else np.sort(rng.choice(devprims.HL_CELLS, ncells, replace=False))
        V64 = V.astype(F64)
        dirs, dcell, frames, fcell = [], [], [], []
        for c in cells:
            idx, _ = H.list_of(c)
            D = cell_samples(c, (1e-3, 3.9e-3)).astype(np.float32)
            S = D.astype(F64) @ V64.T
            missing = ~np.isin(S.argmax(1), idx)
            assert not missing.any(), f"{what}: cell {c}: the fp64 support vertex of {D[missing][0]} is not in the cell's list"
            dirs.append(D); dcell += [c] * len(D)
            if len(idx) <= devprims.HL_MAX:
                Fd = cell_samples(c, (1e-3, 2.9e-3))               # (the patch samples lie 1e-3 rad further out)
                frames.append(patch_frames(Fd)); fcell += [c] * len(Fd)
        D = np.concatenate(dirs)
        ref, sub = H.support("nocache", D), H.support("sub", D, np.array(dcell))
        use = sub_compared(H, np.array(dcell), sub[:, 0], what)
        assert np.array_equal(sub[use].view(np.uint32), ref[use].view(np.uint32)), f"{what}: support<HullSub> differs from NoCache in a widened cell"
        if frames:
            Fr = np.concatenate(frames)
            pref, psub = H.support_patch("nocache", Fr), H.support_patch("sub", Fr, np.array(fcell))
            assert np.array_equal(psub.view(np.uint32), pref.view(np.uint32)), f"{what}: support_patch<HullSub> differs from NoCache in a widened cell"
    finally:
        H.close()


def bound_dirs(nrand, seed):
    g = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    grid = []
    for ax in range(3):
        for sg in (1.0, -1.0):
            for a, b in itertools.product(g, g):
                d = np.zeros(3)
                d[ax], d[(ax + 1) % 3], d[(ax + 2) % 3] = sg, a, b
                grid.append(d)
            t = np.linspace(-1, 1, 17)
            for a, s in itertools.product(g, t):                 # grid lines, both families
                for d3 in ((a, s), (s, a)):
                    d = np.zeros(3)
                    d[ax], d[(ax + 1) % 3], d[(ax + 2) % 3] = sg, d3[0], d3[1]
                    grid.append(d)
    edges = [p for p in itertools.product([-1.0, 1.0, 0.3, -0.7], repeat=3) if sum(abs(x) == 1 for x in p) >= 2]
    # just inside a cube edge: the face coordinate rounds to the face's far grid line (u * 1/|dm| + 1 == 2 in float)
    e = float(np.float32(1 - 2.0 ** -24))
    for ax, other in itertools.permutations(range(3), 2):
        for s1, s2, w in itertools.product((-1.0, 1.0), (-1.0, 1.0), (0.0, 0.5, e)):
            d = [w * s1] * 3
            d[ax], d[other] = s1, s2 * e
            edges.append(tuple(d))
    zeros = [p for p in itertools.product([-0.0, 0.0, 1.0, -1.0], repeat=3) if any(x != 0 for x in p)]
    base = np.concatenate([np.asarray(grid, F64), np.asarray(edges, F64), np.asarray(zeros, F64)])
    units = np.concatenate([unit(base), random_dirs(nrand, seed), np.asarray(zeros, np.float32)])
    return np.concatenate([units, base.astype(np.float32), 0.5 * units, 2.0 * units]).astype(np.float32)


def check_bound(probes, V, D, what):
    H = probes.hull(V)
    try:
        b = H.sbt_bound(D).astype(F64)
        bn = H.sbt_bound(D, pad=np.nan)                          # (NaN around the table: a read outside it shows)
        assert np.array_equal(b.astype(np.float32).view(np.uint32), bn.view(np.uint32)), f"{what}: sbt_bound read outside its table"
        D64 = D.astype(F64)
        h = np.concatenate([(D64[s:s + 4096] @ V.astype(F64).T).max(1) for s in range(0, len(D), 4096)])
        L = np.linalg.norm(D64, axis=1)
        # the 2e-6 that sbt_lowest subtracts is stated for unit directions; sbt_bound is positively homogeneous (bilinear value times |d|_inf),
        # so for the directions of length 2 the same relative rounding is 2 x 2e-6 - the slack scales with |d|, it is not widened
        low = b < h - 2e-6 * np.maximum(L, 1.0)
        assert not low.any(), f"{what}: sbt_bound below the support function by {(h - b)[low].max():.3g} at {D[low][0]}"
        rel = (b - h) / (np.linalg.norm(V.astype(F64), axis=1).max() * L)
        assert rel.max() < 0.2, f"{what}: sbt_bound {rel.max():.1%} of the hull's size above the support function at {D[np.argmax(rel)]}"
    finally:
        H.close()


def light_pairs(probes, rng, n):
    """box / plane faces against a hull: (g1, g2, expected first-query direction of the hull (geom frame, fp64), exact)"""
    def pack(t, size, R, p, c):
        return np.concatenate([[t], size, np.asarray(R, F64).ravel(), p, c])

    def rot(rng):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])

    G1, G2, dl, exact = [], [], [], []
    eye = np.eye(3)
    for k in range(n):
        R2 = rot(rng)
        c2 = rng.uniform(-0.1, 0.1, 3)
        kind = k % 4
        if kind == 0:                                              # plane, random normal
            R1 = rot(rng)
            G1.append(pack(G_PLANE, [0, 0, 0], R1, [0, 0, 0], [0, 0, 0]))
            f = R1[:, 2]
            ex = False
        elif kind == 1:                                            # box, near-tie of lb0 / lb1 (1e-4 m apart) and clear picks
            R1 = rot(rng)
            s = np.array([0.05, 0.05, 0.3])
            loc = np.array([0.01, 0.01 + rng.choice([-1e-4, 1e-4, 2e-2]), 0.0]) * rng.choice([-1, 1], 3)
            c1 = rng.uniform(-0.1, 0.1, 3)
            c2 = c1 + R1 @ loc
            G1.append(pack(G_BOX, s, R1, c1, c1))
            lb = s - np.abs(R1.T @ (c2 - c1))
            a = int(np.argmin(lb))
            f = (1.0 if (R1.T @ (c2 - c1))[a] >= 0 else -1.0) * R1[:, a]
            ex = False
        else:                                                      # box, exact tie lb0 == lb1: square face, identity rotation, centre on its diagonal
            R2 = eye if kind == 2 else R2
            t = [2 ** -6, 3 * 2 ** -7][k % 2] * rng.choice([-1, 1])
            c1 = np.zeros(3)
            c2 = np.array([t, t * rng.choice([-1, 1]), 0.0])
            G1.append(pack(G_BOX, [2 ** -4, 2 ** -4, 0.5], eye, c1, c1))
            f = np.array([1.0 if t >= 0 else -1.0, 0, 0])
            ex = True
        G2.append(pack(G_MESH, [0, 0, 0], R2, c2, c2))
        dl.append(R2.T @ -f)
        exact.append(ex)
    return np.array(G1), np.array(G2), np.array(dl), np.array(exact)


def check_cells(probes, nrand, seed):
    rng = np.random.RandomState(seed)
    D = np.concatenate([random_dirs(nrand, seed), bound_dirs(0, seed)])
    got = probes.hl_cell(D)
    assert np.all((got >= 0) & (got < devprims.HL_CELLS))
    ref, margin = cell_ref(D)
    away = margin > 1e-5
    assert np.array_equal(got[away], ref[away]), "hl_cell differs from the fp64 cell away from the boundaries"
    assert np.all(cell_contains(got, D)), "hl_cell returned a cell that does not hold the direction"
    # light_first_cell: the cell of the first query direction, the box face chosen as scan_faces() does
    g1, g2, dl, exact = light_pairs(probes, rng, 400)
    got = probes.first_cell(g1, g2)
    ref, margin = cell_ref(dl)
    ok = (margin > 1e-5) | exact
    expect = np.where(exact, probes.hl_cell(dl.astype(np.float32)), ref)
    bad = ok & (got != expect)
    assert not bad.any(), f"light_first_cell: {bad.sum()} pairs in another cell than the first face's, e.g. pair {np.flatnonzero(bad)[0]} (exact tie: {exact[bad][0]})"
    assert np.all(cell_contains(got[~ok], dl[~ok], tol=1e-5))


# ------------------------------------------------------------------ the fast path: a flat face against a hull
def facet_normals():
    with open(os.path.join(ROOT, "tests", "golden", "hull_facets.json")) as f:
        return json.load(f)["normals"]


def rot_to(a, b):
    """a rotation taking the unit vector a to the unit vector b"""
    a, b = np.asarray(a, F64) / np.linalg.norm(a), np.asarray(b, F64) / np.linalg.norm(b)
    v, c = np.cross(a, b), float(a @ b)
    if c < -1 + 1e-12:                                           # (antiparallel: half a turn about any axis across a)
        p = np.cross(a, [1.0, 0, 0] if abs(a[0]) < 0.9 else [0, 1.0, 0])
        p /= np.linalg.norm(p)
        return 2 * np.outer(p, p) - np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K / (1 + c)


def rot_axis(axis, t):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def pack_geom(t, size, R, p, c):
    return np.concatenate([[t], size, np.asarray(R, F64).ravel(), p, c]).astype(np.float32)


def edge_dirs(rng, k):
    """geom-frame directions on cube-map cell edges (one face coordinate on the grid) and corners (both)"""
    out = []
    for j in range(k):
        ax, sg = rng.randint(3), rng.choice([-1.0, 1.0])
        u = -1 + rng.randint(9) / 4
        v = -1 + rng.randint(9) / 4 if j % 2 else rng.uniform(-1, 1)
        d = np.zeros(3)
        d[ax], d[(ax + 1) % 3], d[(ax + 2) % 3] = sg, u, v
        out.append(d / np.linalg.norm(d))
    return out


def fast_poses(V, normals, rng, nmax):
    """(g1, g2, rb, kind) of adversarial flat-face poses against the hull V (geom frame = vertex frame):
    plane: resting on each facet (depth 2e-3 and 5e-4 apart), tilted +-1e-3 rad, and -f on cube-map cell edges and corners;
    box: the hull resting on a face of a rotated box, near-ties of lb0 / lb1 (1e-6 .. 1e-4 m) and exact ties (square face, identity rotation,
    the hull's centre on the face diagonal)"""
    V64 = V.astype(F64)
    ctr, rb2 = V64.mean(0), float(np.linalg.norm(V64, axis=1).max())
    ez = np.array([0, 0, 1.0])
    G1, G2, RB, kind = [], [], [], []

    def hull_at(R2, p2, c2=None):
        return pack_geom(G_MESH, [0, 0, 0], R2, p2, R2 @ ctr + p2 if c2 is None else c2)

    def plane(R2, depth):
        p2 = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), -depth - (V64 @ R2.T)[:, 2].min()])
        G1.append(pack_geom(G_PLANE, [0, 0, 0], np.eye(3), [0, 0, 0], [0, 0, 0])); G2.append(hull_at(R2, p2)); RB.append([0.0, rb2])

    for nf in normals:
        R2 = rot_axis(ez, rng.uniform(0, 2 * np.pi)) @ rot_to(nf, -ez)
        for t in (0.0, 1e-3, -1e-3):
            for depth in (2e-3, -5e-4):
                plane(rot_axis([np.cos(t * 1e3), np.sin(t * 1e3), 0], t) @ R2, depth); kind.append("plane facet" if t == 0 else "plane tilted")
    for d in edge_dirs(rng, len(normals)):
        plane(rot_axis(ez, rng.uniform(0, 2 * np.pi)) @ rot_to(d, -ez), 2e-3); kind.append("plane cell edge")
    s = np.array([2.0 ** -4, 2.0 ** -4, 2.0 ** -3])
    rb1 = float(np.linalg.norm(s))
    for j, nf in enumerate(normals):
        # resting on face a of a rotated box
        R1 = rot_axis(rng.normal(size=3), rng.uniform(0, np.pi))
        a, sg = j % 3, (1.0 if j % 2 else -1.0)
        f = sg * R1[:, a]
        R2 = rot_axis(f, rng.uniform(0, 2 * np.pi)) @ rot_to(nf, -f)
        c1 = rng.uniform(-0.1, 0.1, 3)
        p2 = c1 + f * (s[a] - 2e-3 - (V64 @ R2.T @ f).min()) + 0.2 * s[a] * (R1[:, (a + 1) % 3] * rng.uniform(-1, 1))
        G1.append(pack_geom(G_BOX, s, R1, c1, c1)); G2.append(hull_at(R2, p2)); RB.append([rb1, rb2]); kind.append("box face")
        # the hull's centre next to the box edge where faces 0 and 1 meet: exact ties (identity box, centre on the diagonal) and near-ties
        R2 = rot_axis(rng.normal(size=3), rng.uniform(0, np.pi))
        for reach, delta in itertools.product((0.25, 0.5), (0.0, 1e-6, -1e-5, 1e-4)):
            L = float(np.float32(s[0] + reach * rb2))          # (0.25: the hull reaches over the edge into the box; 0.5: it stays clear)
            exact = delta == 0.0
            R1 = np.eye(3) if exact or j % 2 else rot_axis(rng.normal(size=3), rng.uniform(0, np.pi))
            c1 = np.zeros(3) if exact else rng.uniform(-0.1, 0.1, 3)
            c2 = (c1 + R1 @ np.array([L, (L + delta) * rng.choice([-1, 1]), 0.0])).astype(np.float32).astype(F64)
            G1.append(pack_geom(G_BOX, s, R1, c1, c1)); G2.append(hull_at(R2, c2 - R2 @ ctr, c2)); RB.append([rb1, rb2])
            kind.append("box exact tie" if exact else "box near tie")
    G1, G2, RB, kind = np.array(G1), np.array(G2), np.array(RB), np.array(kind)
    if len(G1) > nmax:
        pick = np.sort(rng.choice(len(G1), nmax, replace=False))
        G1, G2, RB, kind = G1[pick], G2[pick], RB[pick], kind[pick]
    return G1, G2, RB, kind


def check_fast_path(probes, V, normals, what, rng, nmax=400):
    """wherever k_narrow's fast path or its row pass reports the pair settled, its contacts are the fused step's bit for bit"""
    H = probes.hull(V)
    try:
        g1, g2, rb, kind = fast_poses(V, normals, rng, nmax)
        ref = H.pairs("fused", g1, g2, rb)
        counts = {}
        for mode in ("fast", "rows"):
            got = H.pairs(mode, g1, g2, rb)
            settled = got[0] == 1
            counts[mode] = int(settled.sum())
            if mode == "fast":
                # the fast path takes a pair exactly when light_first_cell's cell has a list of 1 .. HL_MAX entries (publish_candidates)
                cells = probes.first_cell(g1, g2)
                cnt = np.where(cells >= 0, np.diff(H.off.astype(np.int64))[np.maximum(cells, 0)], 0)
                assert np.array_equal(got[0] >= 0, (cnt >= 1) & (cnt <= devprims.HL_MAX)), f"{what}: the fast path took other pairs than the lists allow"
            # a plane is always settled by the closed form
            plane = (kind != "box face") & np.char.startswith(kind.astype(str), "plane") & (got[0] >= 0)
            assert np.all(settled[plane]), f"{what}: {mode} did not settle a plane pair"
            for i in np.flatnonzero(settled):
                v = int(got[1][i])
                assert v == int(ref[1][i]), f"{what} {kind[i]} pair {i}: {mode} contact mask {v:#x} != fused {int(ref[1][i]):#x}"
                on = [(v >> q) & 1 == 1 for q in range(devprims.NCPP)]
                same = (np.array_equal(got[2][i].view(np.uint32), ref[2][i].view(np.uint32)) and
                        np.array_equal(got[3][i][on].view(np.uint32), ref[3][i][on].view(np.uint32)) and
                        np.array_equal(got[4][i][on].view(np.uint32), ref[4][i][on].view(np.uint32)))
                assert same, f"{what} {kind[i]} pair {i}: {mode} contacts differ from the fused step's"
        return len(g1), counts
    finally:
        H.close()


# ------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def emu():
    return devprims.Probes("emu")


@pytest.fixture(scope="module")
def gpu():
    return devprims.Probes("gpu")


def test_support_paths_agree_and_match_fp64_emulated(emu):
    rng = np.random.RandomState(5)
    A = adversarial_dirs()
    for name, V in cpu_hulls().items():
        D = np.concatenate([random_dirs(32, len(V)), A[rng.choice(len(A), 64, replace=False)]])
        check_paths(emu, V, D, False, name, npatch=32)
    for name, V in tie_hulls().items():
        check_paths(emu, V, dyadic_dirs(), True, name, npatch=16)


def test_support_tables_emulated(emu):
    rng = np.random.RandomState(1)
    for name, V in cpu_hulls().items():
        check_tables(emu, V, 24, name, rng)


def test_support_bound_emulated(emu):
    for name, V in cpu_hulls().items():
        check_bound(emu, V, bound_dirs(2000, 2), name)


def test_cells_emulated(emu):
    check_cells(emu, 4000, 3)


def test_non_finite_directions_stay_in_range_emulated(emu):
    """(emulated build only: never fed to the GPU)"""
    nan, inf = np.nan, np.inf
    D = np.array([[nan, 0, 0], [nan, nan, nan], [inf, 0, 0], [-inf, inf, 0], [inf, inf, inf], [1, nan, 0], [0, -inf, 1], [1e38, 1e38, -1e38]], np.float32)
    cells = emu.hl_cell(D)
    assert np.all((cells >= 0) & (cells < devprims.HL_CELLS))
    for name, V in list(tie_hulls().items())[:2] + [("ellipsoid:513", ellipsoid(513, 513))]:
        H = emu.hull(V)
        try:
            # sbt_bound indexes its table with the direction: the same bits whether the floats around the table are NaN or zero
            b0, bn = H.sbt_bound(D, pad=0.0), H.sbt_bound(D, pad=np.nan)
            assert np.array_equal(b0.view(np.uint32), bn.view(np.uint32)), f"{name}: sbt_bound read outside its table for {D[b0.view(np.uint32) != bn.view(np.uint32)]}"
            for p in ("nocache", "hullcache", "lds256", "lds512", "lds0", "g16_256", "sub"):
                P = H.support(p, D, cells)
                P = P[np.isfinite(P[:, 0])]
                ok = np.all(P == 0, axis=1) | np.any(np.all(P[:, None, :] == V[None], axis=2), axis=1)
                assert ok.all(), f"{name} {p}: a non-finite direction returned {P[~ok][0]}, neither a vertex nor the geom origin"
        finally:
            H.close()


def test_fast_path_matches_fused_emulated(emu):
    normals, rng = facet_normals(), np.random.RandomState(6)
    for name, V in list(cpu_hulls().items())[:2]:
        n, counts = check_fast_path(emu, V, normals[name][:4], name, rng, nmax=48)
        assert counts["fast"] >= n // 3 and counts["rows"] >= n // 3, (name, n, counts)


@pytest.mark.gpu
def test_support_paths_agree_and_match_fp64(gpu):
    for name, V in gpu_hulls().items():
        D = np.concatenate([random_dirs(2048, len(V)), adversarial_dirs()])
        check_paths(gpu, V, D, False, name)
    for name, V in tie_hulls().items():
        check_paths(gpu, V, dyadic_dirs(), True, name)


@pytest.mark.gpu
def test_support_tables(gpu):
    rng = np.random.RandomState(1)
    for name, V in gpu_hulls().items():
        check_tables(gpu, V, devprims.HL_CELLS, name, rng)


@pytest.mark.gpu
def test_support_bound(gpu):
    for name, V in gpu_hulls().items():
        check_bound(gpu, V, bound_dirs(100000, 2), name)


@pytest.mark.gpu
def test_cells(gpu):
    check_cells(gpu, 100000, 3)


@pytest.mark.gpu
def test_fast_path_matches_fused(gpu):
    normals, rng = facet_normals(), np.random.RandomState(6)
    total, counts = 0, {"fast": 0, "rows": 0}
    for name, V in gpu_hulls().items():
        n, c = check_fast_path(gpu, V, normals[name], name, rng)
        total += n
        for k in c:
            counts[k] += c[k]
    assert counts["fast"] >= total // 3 and counts["rows"] >= total // 3, (total, counts)
