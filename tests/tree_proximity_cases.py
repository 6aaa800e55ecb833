"""Shared cases of the proximity-interface tests of the general-tree engine (so101_tree_proximity, include/so101.h): the raw call on a
TreeArraySim of either backend, the states, the pairs, ONE pass of every launch the tests read (`run_handover`, `run_dining`), the fp64 side
(`reference`, once per session) and the checks both backends share - tests/test_tree_proximity_emu.py through the emulated build,
tests/test_tree_proximity_gpu.py on the MI355X.  Checks that do not depend on the engine (the reference's own certificate, swap, beyond and
outside) are those of tests/proximity_cases.py.

States (tests/tree_contact_cases.py).  Hand-over, a 3-env batch: env 0 = state 0 (resting props, closed fingers touching), env 1 = state 6 (the
banana on the right gripper), env 2 = FREE = state 8 (props lifted, fingers open: no contact at all).  Dining: state 0 (settled, 48 contacts).

Pairs.  Hand-over: the six group pairs GROUP_SPECS on all three envs; arms | props (1 824 members: the reference culls, tree_proximity_ref.py)
on FREE; SINGLE: one single-geom pair per type combination the pair list admits (sphere | mesh, sphere | sphere, sphere | box, box | mesh,
mesh | mesh) and one with a d405_solid hull (5 676 vertices), picked from the pair list by type; MEMBER_SPEC: left_gripper | object against its 40
single-geom pairs in calls of at most 16.  Dining: DINING_SPECS (the emulator: one entry, the first two).

Waypoints.  The left gripper's chain (6 columns, tool "left/gripper") moves from FREE's own angles to NEAR_Q in eight steps, against FREE in one
call.  NEAR_Q was chosen on the CPU with the fp64 reference: along the straight line in joint space from FREE's angles towards
NEAR_TARGET, the point where left_gripper | table is NEAR_DIST = 3.0 mm (bisection on the reference's distance, then rounded to float32;
the reference gives 3.0000024 mm at the rounded pose: within 5 mm, still separated).  right_arm | table must keep its bits over all eight,
left_gripper | object and left_gripper | table change and are compared with the reference at each waypoint.

Tolerance.  Worst deviation from the fp64 reference over all cases, measured first (profiles/README.md, "Proximity sensing, general-tree
engine"): emulator 1.006e-7 m (dist) and 1.258e-7 m (certificate on the kernel's witnesses), MI355X 1.304e-7 m and 1.693e-7 m - MEASURED below.
Asserted: four times the larger, rounded up to one digit (TOL 6e-7, SLACK 7e-7) - below the 1e-5 m the interface allows itself.

The fp64 side takes 4.5 s (REFERENCE_SECONDS: measured on the CPU the emulator tests run on; once per session, shared by both backends);
the whole emulator file runs in 25 s."""
from __future__ import annotations

import time

import numpy as np

from so101_sim_amd import native
from tests import contact_cases as cc, contact_ref as cr, proximity_cases as px, tree_contact_cases as tc
from tests.tree_proximity_ref import TreeProximityRef

HANDOVER_STATES = (0, 6, 8)
FREE = 2                                  # env of the free state in the 3-env batch
DINING_STATES = (0,)
GROUP_SPECS = (("grippers", "object"), ("arms", "table"), ("left_arm", "right_arm"), ("object", "container"), ("props", "table"), ("arms", "arms"))
GROUP_MEMBERS = (80, 60, 255, 212, 114, 423)
BIG_SPEC, BIG_MEMBERS = ("arms", "props"), 1824
MEMBER_SPEC = ("left_gripper", "object")
WAY_SPECS = (("right_arm", "table"), ("left_gripper", "object"), ("left_gripper", "table"))
WAY_TOOL = "left/gripper"
NEAR_TARGET = (0.0, 0.35, 0.45, 0.0, 0.6, 0.0)       # the line's far end: shoulder and elbow lowered, wrist pitched down (find_near_pose)
NEAR_DIST = 3.0e-3
NEAR_Q = (0.0, 0.16113542020320892, 0.5556141138076782, 0.0, 0.47389790415763855, 0.0)      # find_near_pose(), float32 values
DINING_SPECS = (("grippers", "object"), ("object", "container"), ("props", "table"))
MEASURED = dict(emu=dict(dist=1.006e-7, cert=1.258e-7), gpu=dict(dist=1.304e-7, cert=1.693e-7))      # metres; the Dining pairs stay below both
TOL = 6e-7                            # 4 x 1.304e-7 (worst |dist - reference|, MI355X: the sphere | mesh single pair) = 5.2e-7, one digit up
SLACK = 7e-7                          # 4 x 1.693e-7 (worst certificate violation on the kernel's witnesses, MI355X, the same pair) = 6.8e-7, one digit up
REFERENCE_SECONDS = 4.5               # hand-over 2.8 s + Dining 1.7 s
FIELDS = px.FIELDS
GROUP_MAX_DIST, BIG_MAX_DIST = 1.0, 10.0      # (the free state holds its props 0.5 m up: with the default 0.1 m most pairs would report "beyond")
SPHERE, BOX, MESH = 1, 4, 5
D405_VERTS = 5676


def w8(*bits):
    return tuple(sum(1 << (int(g) & 31) for g in bits if int(g) >> 5 == k) for k in range(8))


def masks_of(b, specs):
    return tc.pair_masks(b, specs)


def single_pairs(b):
    """-> [(label, g1, g2)]: the first pair of the model's pair list per type combination, a prop on one side where the list has one, and the
    first pair of the left gripper's d405_solid hull with a prop"""
    from so101_sim_amd.model import blob as blobfmt
    m = blobfmt.unpack(b["f32"])
    gt, vn = [int(t) for t in m["geom_type"]], [int(v) for v in m["geom_vertnum"]]
    pairs = [(int(x), int(y)) for x, y in np.asarray(m["pair_geom"]).reshape(-1, 2)]
    props = set(b["groups"]["props"].geoms)
    left = set(b["groups"]["left_gripper"].geoms)
    out = []
    for label, ta, tb_ in (("sphere|mesh", SPHERE, MESH), ("sphere|sphere", SPHERE, SPHERE), ("sphere|box", SPHERE, BOX), ("box|mesh", BOX, MESH), ("mesh|mesh", MESH, MESH)):
        hits = [(x, y) for x, y in pairs if gt[x] == ta and gt[y] == tb_ and vn[x] < D405_VERTS and vn[y] < D405_VERTS]
        pick = [p for p in hits if (p[0] in props) != (p[1] in props)] or hits
        out.append((label, *pick[0]))
    hits = [(x, y) for x, y in pairs if (vn[x] == D405_VERTS and x in left and y in props) or (vn[y] == D405_VERTS and y in left and x in props)]
    out.append(("d405_solid", *hits[0]))
    return out


def raw_proximity(sim, pairs, n=None, env_index=None, q=None, q_adr=None, max_dist=0.1, want=FIELDS):
    """so101_tree_proximity on a TreeArraySim -> dict of numpy arrays [n, P, ...].  The outputs start as 7e7 / -7, so an element the kernel does
    not write fails every check."""
    n = sim.N if n is None else n
    P = len(pairs)
    gpu = sim.backend == "gpu"
    arrs = {}
    for k in want:
        shape = (n, P) + px._SHAPE[k]
        if gpu:
            arrs[k] = sim.torch.full(shape, -7 if k in px._INT else 7e7, dtype=sim.torch.int32 if k in px._INT else sim.torch.float32, device=sim.dev)
        else:
            arrs[k] = np.full(shape, -7 if k in px._INT else 7e7, dtype=np.int32 if k in px._INT else np.float32)
    dev = lambda a, dt: None if a is None else (sim.torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(sim.dev) if gpu else np.ascontiguousarray(a, dtype=dt))
    idx, qd = dev(env_index, np.int32), dev(q, np.float32)
    out = native.ProximityOut(**{k: sim.ptr(a) for k, a in arrs.items()})
    sim.sim.proximity(sim.ptr(idx) if idx is not None else None, n, sim.ptr(qd) if qd is not None else None, q_adr, list(pairs), max_dist, out, sim.stream())
    return {k: sim._get(a) for k, a in arrs.items()}


def way_columns(sim):
    """qpos addresses of the left gripper's chain, from the library (so101_tree_tool_chain)"""
    names = _blobs["handover"]["meta"]["body_names"]
    return sim.sim.tool_chain(names.index("left/gripper_link"))[1]


def waypoints(Q, adr, near=None):
    near = np.asarray(NEAR_Q if near is None else near, dtype=np.float64)
    own = Q[adr, FREE].astype(np.float32).astype(np.float64)
    t = np.linspace(0.0, 1.0, 8)[:, None]
    return ((1 - t) * own + t * near).astype(np.float32)


_blobs, _refs, _cache = {}, {}, {}


def blobs(kind):
    if kind not in _blobs:
        _blobs[kind] = tc.blobs(kind)
    return _blobs[kind]


def _ref_of(kind, b=None):
    if kind not in _refs:
        _refs[kind] = TreeProximityRef((b or blobs(kind))["f64"])
    return _refs[kind]


def run_handover(sim):
    """every hand-over launch the tests read, once: -> dict"""
    b = blobs("handover")
    Q, V, CT, W = tc.states("handover", HANDOVER_STATES)
    tc.load(sim, Q, V, CT, W)
    adr16 = _ref_of("handover").onedof_addresses()
    own = np.ascontiguousarray(Q[adr16].T, dtype=np.float32)                      # [3, 16] the envs' own one-dof joint values
    gm = masks_of(b, GROUP_SPECS)
    singles = single_pairs(b)
    sm = [(w8(g1), w8(g2)) for _, g1, g2 in singles]
    g = b["groups"]
    members = [(ga, gb) for ga in g[MEMBER_SPEC[0]].geoms for gb in g[MEMBER_SPEC[1]].geoms]
    member_masks = [(w8(ga), w8(gb)) for ga, gb in members]
    state = lambda: [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    before = state()
    wadr = way_columns(sim)
    out = dict(Q=Q, own=own, adr16=adr16, group_masks=gm, singles=singles, single_masks=sm, members=members, way_adr=wadr, before=before)
    out["group"] = raw_proximity(sim, gm, n=3, max_dist=GROUP_MAX_DIST)
    out["swapped"] = raw_proximity(sim, [(y, x) for x, y in gm], n=2, env_index=[0, FREE], max_dist=GROUP_MAX_DIST)
    out["own_q"] = raw_proximity(sim, gm, n=2, env_index=[FREE, 0], q=own[[FREE, 0]], q_adr=adr16, max_dist=GROUP_MAX_DIST)        # permuted, q = the envs' own values
    out["big"] = raw_proximity(sim, masks_of(b, [BIG_SPEC]), n=1, env_index=[FREE], max_dist=BIG_MAX_DIST)
    out["single"] = raw_proximity(sim, sm, n=1, env_index=[FREE], max_dist=10.0)
    wm = masks_of(b, WAY_SPECS)
    out["way"] = raw_proximity(sim, wm, n=8, env_index=[FREE] * 8, q=waypoints(Q, wadr), q_adr=wadr, max_dist=GROUP_MAX_DIST)
    out["way_base"] = raw_proximity(sim, wm, n=1, env_index=[FREE], max_dist=GROUP_MAX_DIST)
    out["way_tool"] = wm
    parts = [raw_proximity(sim, member_masks[k:k + 16], n=2, env_index=[FREE, 0], max_dist=10.0) for k in range(0, len(member_masks), 16)]
    out["member_single"] = {f: np.concatenate([p[f] for p in parts], axis=1) for f in FIELDS}
    out["member_group"] = raw_proximity(sim, masks_of(b, [MEMBER_SPEC]), n=2, env_index=[FREE, 0], max_dist=10.0)
    nan = np.full((1, 16), np.nan, dtype=np.float32)                                                 # (non-finite joints: no bound is below max_dist, nothing loops)
    out["beyond"] = raw_proximity(sim, gm[0:1], n=3, env_index=[FREE, 5, FREE], q=np.concatenate([own[[FREE]], own[[FREE]], nan]), q_adr=adr16, max_dist=1e-3)
    out["after"] = state()
    out["touch"] = tc.raw_contacts(sim, n=3, forces=False, pairs=gm)
    return out


def run_dining(sim, nspec):
    b = blobs("dining")
    tc.load(sim, *tc.states("dining", DINING_STATES))
    dm = masks_of(b, DINING_SPECS[:nspec])
    return dict(masks=dm, group=raw_proximity(sim, dm, n=1, max_dist=GROUP_MAX_DIST), touch=tc.raw_contacts(sim, n=1, forces=False, pairs=dm))


def reference(kind, sim_adr=None):
    """the fp64 side of the runs, computed once per session and shared by the emulator and the GPU tests"""
    if kind in _cache:
        return _cache[kind]
    t0 = time.time()
    b = blobs(kind)
    ref = _ref_of(kind)
    out = dict(ref=ref)
    q32 = lambda col: col.astype(np.float32).astype(np.float64)
    if kind == "handover":
        Q = tc.states("handover", HANDOVER_STATES)[0]
        gm = masks_of(b, GROUP_SPECS)
        caches = [{} for _ in range(3)]
        out["group"] = [[ref.query(q32(Q[:, e]), x, y, GROUP_MAX_DIST, caches[e]) for x, y in gm] for e in range(3)]
        out["big"] = [[ref.query(q32(Q[:, FREE]), *masks_of(b, [BIG_SPEC])[0], BIG_MAX_DIST, caches[FREE])]]
        out["single"] = [[ref.query(q32(Q[:, FREE]), w8(g1), w8(g2), 10.0, caches[FREE]) for _, g1, g2 in single_pairs(b)]]
        wm = masks_of(b, WAY_SPECS)
        way = []
        for w in waypoints(Q, sim_adr):
            qq = q32(Q[:, FREE]); qq[sim_adr] = w.astype(np.float64)
            c = {}
            way.append([ref.query(qq, x, y, GROUP_MAX_DIST, c) for x, y in wm])
        out["way"] = way
        out["beyond"] = [[ref.query(q32(Q[:, FREE]), *gm[0], 1e-3, caches[FREE])]]
    else:
        Q = tc.states("dining", DINING_STATES)[0]
        c = {}
        out["group"] = [[ref.query(q32(Q[:, 0]), x, y, GROUP_MAX_DIST, c) for x, y in masks_of(b, DINING_SPECS)]]
    out["seconds"] = time.time() - t0
    print(f"fp64 reference ({kind}): {out['seconds']:.1f} s")
    _cache[kind] = out
    return out


def find_near_pose(dist=NEAR_DIST):
    """how NEAR_Q was found (CPU, fp64 reference): bisection along the line from FREE's angles to NEAR_TARGET on left_gripper | table"""
    b = blobs("handover")
    ref = _ref_of("handover")
    Q = tc.states("handover", HANDOVER_STATES)[0]
    names = b["meta"]["body_names"]
    body, adr = names.index("left/gripper_link"), []
    while body:
        if int(ref.rc.jtype[body]) in (1, 3):
            adr.insert(0, int(ref.rc.qadr[body]))
        body = int(ref.rc.par[body])
    own = Q[adr, FREE].astype(np.float32).astype(np.float64)
    x, y = masks_of(b, [("left_gripper", "table")])[0]

    def d(t):
        qq = Q[:, FREE].astype(np.float32).astype(np.float64)
        qq[adr] = (1 - t) * own + t * np.asarray(NEAR_TARGET)
        r = ref.query(qq, x, y, 10.0)
        return -1.0 if r["penetrating"] else r["dist"]
    lo, hi = 0.0, 1.0
    assert d(lo) > dist > d(hi), (d(lo), d(hi))
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if d(mid) > dist else (lo, mid)
    q = ((1 - lo) * own + lo * np.asarray(NEAR_TARGET)).astype(np.float32)
    return adr, q, d(lo)


# ---------------------------------------------------------------------------------------------------------------- checks
def check_separated(rep, refs, ref, label, worst):
    """every entry and pair of `rep` against the reference rows `refs`: no iteration cap, the winning pair (or one the reference puts within TOL
    of the best), |dist - reference| <= TOL, the certificate on the kernel's own witnesses against the fp64 poses <= SLACK.  Penetrating results
    are left to check_penetrating.  -> (separated results checked, penetrating results seen)"""
    nsep = npen = 0
    for e, row in enumerate(refs):
        for p, r in enumerate(row):
            fl, d = int(rep["flags"][e, p]), float(rep["dist"][e, p])
            assert not fl & 2, (label, e, p, "iteration cap")
            if fl & 1:
                npen += 1
                continue
            if fl & 4:
                assert r["dist"] is None and not r["penetrating"], (label, e, p, r["dist"], r["penetrating"])
                assert np.all(rep["geom"][e, p] == -1) and np.all(cc.bits(rep["point"][e, p]) == 0) and np.all(cc.bits(rep["normal"][e, p]) == 0), (label, e, p)
                continue
            nsep += 1
            ga, gb = (int(x) for x in rep["geom"][e, p])
            assert r["dist"] is not None, (label, e, p, d)
            if (ga, gb) != tuple(r["geom"]):
                other = r["table"][(ga, gb)] if (ga, gb) in r["table"] else ref.pair_distance(ga, gb, r["poses"])
                assert other is not None and abs(other - r["dist"]) <= TOL, (label, e, p, (ga, gb), r["geom"], other, r["dist"])
            err = abs(d - r["dist"])
            viol, parts = ref.certificate(ga, gb, r["poses"], rep["point"][e, p, 0], rep["point"][e, p, 1], rep["normal"][e, p], d)
            worst["dist"], worst["cert"] = max(worst["dist"], err), max(worst["cert"], viol)
            print(f"{label} entry {e} pair {p}: geoms {(ga, gb)} dist {d:.9g} reference {r['dist']:.12g} |diff| {err:.2e} certificate {viol:.2e}")
            assert err <= TOL, (label, e, p, d, r["dist"])
            assert viol <= SLACK, (label, e, p, parts)
    return nsep, npen


def check_penetrating(rep, touch, masks, n):
    """flags bit 1 exactly where so101_tree_contacts counts a contact of the pair, dist the bits of its pair_dist, the geoms members of (a, b),
    the witnesses the contact position offset along the unit normal"""
    seen = 0
    for e in range(n):
        for p, (a, b) in enumerate(masks):
            fl = int(rep["flags"][e, p])
            assert bool(fl & 1) == bool(touch["pair_count"][e, p] > 0), (e, p, fl, touch["pair_count"][e, p])
            if not fl & 1:
                continue
            seen += 1
            ga, gb = (int(x) for x in rep["geom"][e, p])
            assert cr.in_mask(a, ga) and cr.in_mask(b, gb), (e, p, ga, gb)
            assert rep["dist"][e, p] < 0 and cc.same_bits(rep["dist"][e, p], touch["pair_dist"][e, p]), (e, p, rep["dist"][e, p], touch["pair_dist"][e, p])
            nrm = rep["normal"][e, p].astype(np.float64)
            assert abs(np.linalg.norm(nrm) - 1) <= 1e-6
            gap = (rep["point"][e, p, 1].astype(np.float64) - rep["point"][e, p, 0]) - float(rep["dist"][e, p]) * nrm
            assert np.abs(gap).max() <= 1e-6, (e, p, gap)
    print(f"penetrating results: {seen}")
    return seen


def check_handover_separated(res, ref):
    worst = dict(dist=0.0, cert=0.0)
    R = ref["ref"]
    ns, npn = check_separated(res["group"], ref["group"], R, "group", worst)
    assert ns >= 8 and npn >= 4, (ns, npn)
    assert not any(int(f) & 1 for f in res["group"]["flags"][FREE])                  # the free state: every pair separated
    bs, bp = check_separated(res["big"], ref["big"], R, "arms|props", worst)
    assert (bs, bp) == (1, 0) and ref["big"][0][0]["members"] == BIG_MEMBERS and ref["big"][0][0]["skipped"] > 0
    ss, sp = check_separated(res["single"], ref["single"], R, "single", worst)
    assert (ss, sp) == (len(res["singles"]), 0), (ss, sp)
    ws, wp = check_separated(res["way"], ref["way"], R, "waypoints", worst)
    assert wp == 0 and ws == 8 * len(WAY_SPECS), (ws, wp)
    print(f"worst |dist - reference| {worst['dist']:.3e} m, worst certificate violation on the kernel's witnesses {worst['cert']:.3e} m (asserted: {TOL:g}, {SLACK:g})")
    return worst


def check_reference(ref, keys):
    worst = 0.0
    for k in keys:
        worst = max(worst, px.check_reference_certificate(ref[k], ref["ref"]))
    return worst


def check_invariants(res):
    """q = the envs' own joint values and a permutation of the entries: the rows' bits; (a, b) swapped; the bound state untouched"""
    for f in FIELDS:
        assert cc.same_bits(res["own_q"][f], res["group"][f][[FREE, 0]]), f
    px.check_swap(res["group"], (0, FREE), res["swapped"], res["group_masks"])
    for a, b in zip(res["before"], res["after"]):
        assert cc.same_bits(a, b)                                               # qpos, qvel, ctrl and the warmstart


def check_waypoints(res, ref):
    """q moves what it names and nothing else: right_arm | table keeps the bits it has without q over all eight waypoints; left_gripper | object
    and left_gripper | table move (and are the reference's: check_handover_separated); waypoint 0 is the env's own pose; the last is NEAR_Q"""
    way, base = res["way"], res["way_base"]
    for f in ("dist", "geom", "point", "normal", "flags"):
        for k in range(8):
            assert cc.same_bits(way[f][k, 0], base[f][0, 0]), (f, k)
        assert cc.same_bits(way[f][0], base[f][0]), f
    for p in (1, 2):
        assert len({float(x) for x in way["dist"][:, p]}) == 8, way["dist"][:, p]
    near = ref["way"][7][2]
    assert near["dist"] is not None and not near["penetrating"] and 0 < near["dist"] < 5e-3, near["dist"]
    assert not way["flags"][7, 2] and 0 < way["dist"][7, 2] < 5e-3


def check_members(res):
    """a group pair's result is the minimum of the kernel's own single-geom-pair results over its members, bit for bit, with the first minimum's
    geoms (the members in pair-list order: ties go to the earlier pair)"""
    single, group, members = res["member_single"], res["member_group"], res["members"]
    assert len(members) == 40 and single["dist"].shape == (2, 40)
    pairs = _ref_of("handover").pairs
    order = [pairs.index((ga, gb)) if (ga, gb) in pairs else pairs.index((gb, ga)) for ga, gb in members]
    for e in range(2):
        d = single["dist"][e]
        ties = sorted((j for j in range(40) if d[j] == d.min()), key=lambda j: order[j])
        assert cc.same_bits(group["dist"][e, 0], d.min()), (e, group["dist"][e, 0], d.min())
        assert tuple(group["geom"][e, 0]) == tuple(single["geom"][e, ties[0]]) == members[ties[0]], (e, group["geom"][e, 0], members[ties[0]])
        for f in ("point", "normal", "flags"):
            assert cc.same_bits(group[f][e, 0], single[f][e, ties[0]]), (e, f)
        assert 1 <= int(group["queries"][e, 0]) <= 40
    print(f"members: group dist {group['dist'][:, 0]}, exact queries of the group {group['queries'][:, 0]} of 40 members")


def check_culling(res):
    q = int(res["big"]["queries"][0, 0])
    print(f"arms | props on the free state: {q} exact queries of {BIG_MEMBERS} members")
    assert 1 <= q < BIG_MEMBERS


def check_argument_errors(kind, backend):
    """the argument and state errors of so101_tree_proximity, one assertion per message"""
    import ctypes as C
    from tests.simharness import TreeArraySim
    b = blobs(kind)
    sim = TreeArraySim(b["f32"], 2, backend=backend)
    L, h = sim.sim.L, sim.sim.h
    err = lambda: L.so101_tree_last_error(h).decode()
    ngeom = len(b["meta"]["geom_names"])
    assert ngeom == sim.sim.ngeom and sim.sim.build == (32 if kind == "handover" else 64)
    gpu = backend == "gpu"
    mk = lambda shape, dt: (sim.torch.zeros(shape, dtype=sim.torch.int32 if dt == np.int32 else sim.torch.float32, device=sim.dev) if gpu else np.zeros(shape, dt))
    dist, idx, qq = mk((4, 16), np.float32), mk((4,), np.int32), mk((4, 16), np.float32)
    one = native.geom_pair_array([(w8(0), w8(1))], 8)
    P = lambda a: None if a is None else sim.ptr(a)
    adr = _ref_of(kind).onedof_addresses()
    A = lambda a: None if a is None else (C.c_int32 * len(a))(*a)
    free_adr = next(int(_ref_of(kind).rc.qadr[bd]) for bd in range(len(_ref_of(kind).rc.par)) if int(_ref_of(kind).rc.jtype[bd]) == 2)

    def call(hh=h, idx=None, n=2, q=None, q_adr=None, ncol=0, pairs=one, npair=1, max_dist=0.1, out="default"):
        o = native.ProximityOut(dist=P(dist)) if out == "default" else out
        return L.so101_tree_proximity(hh, P(idx), n, P(q), A(q_adr), ncol, pairs, npair, max_dist, C.byref(o) if o is not None else None, sim.stream() if gpu else None)

    name = "so101_tree_proximity: "
    assert call() == 0 and call(idx=idx, n=4, q=qq, q_adr=adr, ncol=16) == 0 and call(q=qq, q_adr=adr[3:4], ncol=1) == 0
    assert call(hh=None) == -1
    assert call(out=None) == -1 and err() == name + "NULL out"
    assert call(out=native.ProximityOut()) == -1 and err() == name + "no output (every pointer of out is NULL)"
    for n in (0, -1, (1 << 26) + 1):
        assert call(n=n, idx=idx) == -1 and err() == name + "n must be 1 .. 2^26"
    assert call(n=3) == -1 and err() == name + "n exceeds the envs of the handle"
    for npair in (0, -1, 17):
        assert call(npair=npair) == -1 and err() == name + "npair must be 1 .. 16"
    assert call(pairs=None) == -1 and err() == name + "NULL pairs"
    for side in (0, 1):
        empty = native.geom_pair_array([(w8(0), w8(1)), (w8(), w8(2))[::1 if side == 0 else -1]], 8)
        assert call(pairs=empty, npair=2) == -1 and err() == name + f"pair 1, group {'ab'[side]} is empty"
        beyond = native.geom_pair_array([(w8(0), w8(ngeom))[::1 if side == 1 else -1]], 8)
        assert call(pairs=beyond) == -1 and err() == name + f"pair 0, group {'ab'[side]}: bit {ngeom} is at or beyond ngeom = {ngeom}"
    assert call(pairs=native.geom_pair_array([(w8(ngeom - 1), w8(0))], 8)) == 0          # the last geom is a member like any other
    assert call(pairs=native.geom_pair_array([(w8(0), w8(255))], 8)) == -1 and "bit 255" in err()      # the eighth word is read
    for md in (0.0, -1.0, 10.5, float("inf"), float("nan")):
        assert call(max_dist=md) == -1 and err() == name + "max_dist must be a finite number above 0 and at most 10", md
    assert call(max_dist=10.0) == 0
    assert call(q=qq, ncol=16) == -1 and err() == name + "q without q_adr"
    assert call(q_adr=adr, ncol=16) == -1 and err() == name + "q_adr without q"
    for ncol in (0, -1, 17):
        assert call(q=qq, q_adr=adr, ncol=ncol) == -1 and err() == name + "ncol must be 1 .. 16", ncol
    for bad in (free_adr, free_adr + 3, -1, sim.sim.nq, 1 << 20):
        assert call(q=qq, q_adr=[adr[0], bad], ncol=2) == -1 and err() == name + f"q_adr[1] = {bad} is not the qpos address of a hinge or slide joint", bad
    assert call(q=qq, q_adr=[adr[2], adr[5], adr[2]], ncol=3) == -1 and err() == name + f"q_adr[2] repeats address {adr[2]} of q_adr[0]"
    un = native.TreeSim(b["f32"], 2, lib_path=sim.sim.L._name)
    assert call(hh=un.h) == -4 and L.so101_tree_last_error(un.h).decode() == name + "state buffers not bound (call so101_tree_bind_state)"
    assert call(hh=un.h, max_dist=0.0) == -1 and call(hh=un.h, q=qq, ncol=16) == -1          # the arguments are checked first
    un.close()
    assert "so101_tree_proximity" in native.EXPORTS
    if gpu:
        sim.torch.cuda.synchronize()


def check_python_arguments():
    """ProximitySensing's own argument checks on AlohaEnvironment's methods, on a stand-in that has the scene's groups and nothing to launch on"""
    import pytest
    import torch
    from so101_sim_amd import aloha, contacts as ct, proximity as pr
    from so101_sim_amd.tool_control import ToolControl
    b = blobs("handover")

    class Stub(ToolControl, ct.ContactSensing, pr.ProximitySensing):
        _geom_limit = ct.TREE_MAX_GEOMS
        _q_is_columns = True
        meta = b["meta"]
        n_envs = 3
        device = torch.device("cpu")
        geom_group = ct.ContactSensing._geom_group
        _proximity_columns = aloha.AlohaEnvironment._proximity_columns
        proximity = aloha.AlohaEnvironment.proximity

        def _geom_groups(self):
            return b["groups"]

    s = Stub()
    s.torch = torch
    s._onedof_qadr = list(range(16))
    for md in (0.0, -0.1, float("nan"), float("inf"), 10.5, "far", None):
        with pytest.raises(ValueError, match="max_dist must be"):
            s.proximity([("grippers", "object")], max_dist=md)
    with pytest.raises(ValueError, match="1 .. 16 pairs"):
        s.proximity([("grippers", "object")] * 17)
    with pytest.raises(ValueError, match="1 .. 16 pairs"):
        s.proximity([])
    with pytest.raises(ValueError, match="unknown geom group"):
        s.proximity([("grippers", "no_such_thing")])
    with pytest.raises(ValueError, match=r"q must be \[3, 16\]: one row of joint values per entry"):
        s.proximity([("grippers", "object")], q=np.zeros((2, 16)))
    with pytest.raises(ValueError, match=r"q must be \[n, 2\]"):
        s.proximity([("grippers", "object")], q=np.zeros((3, 16)), joints=[0, 1])
    with pytest.raises(ValueError, match="needs q"):
        s.proximity([("grippers", "object")], joints=[0, 1])
    with pytest.raises(ValueError, match="distinct qpos addresses"):
        s.proximity([("grippers", "object")], q=np.zeros((3, 2)), joints=[1, 1])
    with pytest.raises(ValueError, match="distinct qpos addresses"):
        s.proximity([("grippers", "object")], q=np.zeros((3, 17)), joints=list(range(17)))
