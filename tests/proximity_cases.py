"""Shared cases of the proximity-interface tests (so101_proximity, include/so101.h): the raw call on an ArraySim of either backend, the
states, the pairs, ONE pass of every launch the tests read (`run`), and the checks both backends share - tests/test_proximity_emu.py
through the emulated build, tests/test_proximity_gpu.py on the MI355X.

The batch has five envs: 0 .. 3 are four of the contact-rich states (contact_cases.EMU_STATES: the penetrating branch, groups in resting
contact), env 4 holds the props of a state where both rest on the table; its arm is placed by `q`: LIFTED clear of everything (every
cross-body pair separated), eight WAYPOINTS from there down towards the table, and PARALLEL_Q, which holds fixed_jaw_pad_3 with its large
face parallel to the table top to 5e-9 rad, 19 mm above it (found with the fp64 kinematics of tests/proximity_ref.py): the closest points are
not unique there, so only dist, normal and the certificate are checked.  (The issue's "post-reset rest state" would cost a settle of a
thousand substeps under the emulator; the resting props of a recorded state serve the same purpose on both backends.)

Tolerance.  Worst deviation from the fp64 reference over all cases, measured first (profiles/README.md): emulator 3.24e-7 m (dist: the
cylinder post, whose iteration ends on the relative gap) and 3.94e-7 m (certificate on the kernel's witnesses); MI355X: 2.94e-7 m and 3.33e-7 m.
Asserted: four times the larger, rounded up to one digit - below the 1e-5 m the interface allows itself."""
from __future__ import annotations

import numpy as np

from so101_sim_amd import contacts as ct, native
from tests import contact_cases as cc, contact_ref as cr
from tests.proximity_ref import ProximityRef

N_ENVS = 5
REST = 4                              # the env whose props rest on the table
REST_STATE = 3                        # ... from this state of the fixture
LIFTED = (0.0, -1.2, 1.0, 0.3, 0.0, 0.5)
LOWERED = (0.0, -0.45, 1.33, -0.88, 0.0, 0.3)
PARALLEL_Q = (0.0, -0.5814465284347534, 2.5814366340637207, -2.0, 5.656852408719715e-06, 0.30000001192092896)
GROUP_SPECS = (("gripper", "object"), ("arm", "table"), ("object", "container"), ("arm", "props"), ("gripper", "arm"))      # the last: groups that share geoms
SINGLE_SPECS = (("object/coacd_part_001", "container/coacd_part_*"),           # a 1080-vertex hull against the bowl pieces: mesh | mesh beyond HULL_LDS_MAX
                ("object/coacd_part_001", "container/coacd_part_030"),         # ... and against one piece
                ("fixed_jaw_pad_3", "object/coacd_part_002"),                  # box | mesh
                ("banana", "object/coacd_part_000"),                           # the static capsule post: core plus radius
                ("floor", "Wrist_Pitch_Roll"),                                 # plane | mesh
                ("table_surface", "Lower_Arm"),                                # box | mesh
                ("bowl", "Fixed_Jaw_Collision_2"))                             # the static cylinder post: its support function
MEMBER_SPEC = ("fixed_jaw_pads", "object")                                     # 4 x 4 single-geom pairs: a group's result is the minimum over them
TOL = 2e-6                            # 4 x 3.24e-7 (worst |dist - reference|) = 1.3e-6, one digit up
SLACK = 2e-6                          # 4 x 3.94e-7 (worst certificate violation on the kernel's witnesses) = 1.6e-6, one digit up
FIELDS = ("dist", "geom", "point", "normal", "flags", "queries")
_SHAPE = dict(dist=(), geom=(2,), point=(2, 3), normal=(3,), flags=(), queries=())
_INT = ("geom", "flags", "queries")


def masks_of(blobs, specs):
    g = cc.groups(blobs)
    return [(ct.resolve(a, g, blobs["meta"]).mask(), ct.resolve(b, g, blobs["meta"]).mask()) for a, b in specs]


def states(golden):
    Q, V, A, W = cc.rich_states(golden, cc.EMU_STATES + (REST_STATE,))
    return Q, V, A, W


def raw_proximity(sim, pairs, n=None, env_index=None, q=None, max_dist=0.1, want=FIELDS):
    """so101_proximity on an ArraySim -> dict of numpy arrays [n, P, ...].  The outputs start as 7e7 / -7, so an element the kernel does not
    write fails every check."""
    n = sim.N if n is None else n
    P = len(pairs)
    gpu = sim.backend == "gpu"
    arrs = {}
    for k in want:
        shape = (n, P) + _SHAPE[k]
        if gpu:
            arrs[k] = sim.torch.full(shape, -7 if k in _INT else 7e7, dtype=sim.torch.int32 if k in _INT else sim.torch.float32, device=sim.dev)
        else:
            arrs[k] = np.full(shape, -7 if k in _INT else 7e7, dtype=np.int32 if k in _INT else np.float32)
    dev = lambda a, dt: None if a is None else (sim.torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(sim.dev) if gpu else np.ascontiguousarray(a, dtype=dt))
    idx, qd = dev(env_index, np.int32), dev(q, np.float32)
    out = native.ProximityOut(**{k: sim.ptr(a) for k, a in arrs.items()})
    sim.sim.proximity(sim.ptr(idx) if idx is not None else None, n, sim.ptr(qd) if qd is not None else None, list(pairs), max_dist, out, sim.stream())
    return {k: sim._get(a) for k, a in arrs.items()}


def waypoints():
    t = np.linspace(0.0, 1.0, 8)[:, None]
    return ((1 - t) * np.array(LIFTED) + t * np.array(LOWERED)).astype(np.float32)


def run(sim, blobs, golden):
    """every launch the tests read, once: -> dict"""
    Q, V, A, W = states(golden)
    cc.load(sim, Q, V, A, W)
    own = np.ascontiguousarray(Q[:6].T, dtype=np.float32)                       # [5, 6] the envs' own arm angles
    gm, sm, mm = masks_of(blobs, GROUP_SPECS), masks_of(blobs, SINGLE_SPECS), masks_of(blobs, [MEMBER_SPEC])
    g = cc.groups(blobs)
    members = [((a,), (b,)) for a in ct.resolve(MEMBER_SPEC[0], g, blobs["meta"]).geoms for b in ct.resolve(MEMBER_SPEC[1], g, blobs["meta"]).geoms]
    member_masks = [(ct.GeomGroup("a", a).mask(), ct.GeomGroup("b", b).mask()) for a, b in members]
    state = lambda: [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    before = state()
    lifted = np.array([LIFTED], dtype=np.float32)
    out = dict(Q=Q, own=own, group_masks=gm, single_masks=sm, member_masks=member_masks, members=members, member_mask=mm)
    out["rich"] = raw_proximity(sim, gm, n=4)                                                         # envs 0 .. 3, the bound arm
    out["rich_swapped"] = raw_proximity(sim, [(b, a) for a, b in gm], n=2, env_index=[0, 2])
    out["rich_q"] = raw_proximity(sim, gm, n=2, env_index=[2, 0], q=own[[2, 0]])                      # permuted, q = the envs' own angles
    out["way"] = raw_proximity(sim, gm[:2] + gm[3:4], n=8, env_index=[REST] * 8, q=waypoints())
    out["single"] = raw_proximity(sim, sm, n=1, env_index=[REST], q=lifted, max_dist=10.0)
    out["parallel"] = raw_proximity(sim, masks_of(blobs, [("fixed_jaw_pad_3", "table_surface")]), n=1, env_index=[REST], q=np.array([PARALLEL_Q], dtype=np.float32))
    mq = np.stack([np.array(LIFTED, dtype=np.float32), own[2]])
    out["member_single"] = raw_proximity(sim, member_masks, n=2, env_index=[REST, 2], q=mq, max_dist=10.0)
    out["member_group"] = raw_proximity(sim, mm, n=2, env_index=[REST, 2], q=mq, max_dist=10.0)
    nan = np.full((1, 6), np.nan, dtype=np.float32)                                                   # (a non-finite arm: no bound is below max_dist, nothing loops)
    out["beyond"] = raw_proximity(sim, gm[1:2], n=3, env_index=[REST, N_ENVS + 2, REST], q=np.concatenate([lifted, lifted, nan]), max_dist=1e-3)
    out["after"] = state()
    out["before"] = before
    out["touch"] = cc.raw_contacts(sim, n=4, forces=False, pairs=gm)
    return out


_ref = {}


def reference(blobs, golden):
    """the fp64 side of `run`, computed once per session and shared by the emulator and the GPU tests"""
    if "r" in _ref:
        return _ref["r"]
    ref = ProximityRef(blobs["f64"])
    Q = states(golden)[0]
    q32 = lambda e, arm=None: np.r_[np.asarray(arm, dtype=np.float32) if arm is not None else Q[:6, e].astype(np.float32), Q[6:, e].astype(np.float32)].astype(np.float64)
    gm, sm = masks_of(blobs, GROUP_SPECS), masks_of(blobs, SINGLE_SPECS)
    out = dict(ref=ref)
    caches = {}

    def ask(key, qpos, masks, max_dist):
        c = caches.setdefault(key, {})
        return [ref.query(qpos, a, b, max_dist, c) for a, b in masks]

    out["rich"] = [ask(("rich", e), q32(e), gm, 0.1) for e in range(4)]
    out["way"] = [ask(("way", k), q32(REST, w), gm[:2] + gm[3:4], 0.1) for k, w in enumerate(waypoints())]
    out["single"] = [ask("lifted", q32(REST, LIFTED), sm, 10.0)]
    out["parallel"] = [ask("parallel", q32(REST, PARALLEL_Q), masks_of(blobs, [("fixed_jaw_pad_3", "table_surface")]), 0.1)]
    out["beyond"] = [ask("lifted", q32(REST, LIFTED), gm[1:2], 1e-3)]
    _ref["r"] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- checks
def check_separated(rep, refs, ref, label, worst=None):
    """every entry and pair of `rep` against the reference rows `refs`: flags, the winning pair, |dist - reference| <= TOL, and the
    certificate on the kernel's own witnesses against the fp64 poses <= SLACK (the points are never compared with the reference's: where
    two flat features face each other they are not unique).  Penetrating results are left to check_penetrating.
    -> (separated results checked, penetrating results seen)"""
    worst = worst if worst is not None else dict(dist=0.0, cert=0.0)
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
                assert (ga, gb) in r["table"] and abs(r["table"][(ga, gb)] - r["dist"]) <= TOL, (label, e, p, (ga, gb), r["geom"])
            err = abs(d - r["dist"])
            viol, parts = ref.certificate(ga, gb, r["poses"], rep["point"][e, p, 0], rep["point"][e, p, 1], rep["normal"][e, p], d)
            worst["dist"], worst["cert"] = max(worst["dist"], err), max(worst["cert"], viol)
            print(f"{label} entry {e} pair {p}: geoms {(ga, gb)} dist {d:.9g} reference {r['dist']:.12g} |diff| {err:.2e} certificate {viol:.2e}")
            assert err <= TOL, (label, e, p, d, r["dist"])
            assert viol <= SLACK, (label, e, p, parts)
    return nsep, npen


def check_reference_certificate(refs, ref):
    """the reference passes its own certificate with a slack of 1e-10 wherever it reports a distance"""
    worst = 0.0
    for row in refs:
        for r in row:
            if r["dist"] is not None:
                v, parts = ref.certificate(r["geom"][0], r["geom"][1], r["poses"], r["pa"], r["pb"], r["n"], r["dist"])
                worst = max(worst, v)
                assert v <= 1e-10, (r["geom"], parts)
    return worst


def check_penetrating(rep, touch, masks, n):
    """bit 1 results: geom is a pair of (a, b), dist < 0 and equal to touch's pair_dist at the same state to 1e-6 (expected: the same bits);
    and where touch counts a contact, proximity reports a penetration"""
    seen, worst = 0, 0.0
    for e in range(n):
        for p, (a, b) in enumerate(masks):
            fl = int(rep["flags"][e, p])
            if touch["pair_count"][e, p] > 0:
                assert fl & 1, (e, p, "touch counts contacts, proximity reports none")
            if not fl & 1:
                continue
            seen += 1
            ga, gb = (int(x) for x in rep["geom"][e, p])
            assert cr.in_mask(a, ga) and cr.in_mask(b, gb), (e, p, ga, gb)
            assert touch["pair_count"][e, p] > 0, (e, p, "proximity reports a penetration touch does not count")
            diff = abs(float(rep["dist"][e, p]) - float(touch["pair_dist"][e, p]))
            worst = max(worst, diff)
            assert rep["dist"][e, p] < 0 and diff <= 1e-6, (e, p, rep["dist"][e, p], touch["pair_dist"][e, p])
            nrm = rep["normal"][e, p].astype(np.float64)
            assert abs(np.linalg.norm(nrm) - 1) <= 1e-6
            gap = (rep["point"][e, p, 1].astype(np.float64) - rep["point"][e, p, 0]) - float(rep["dist"][e, p]) * nrm
            assert np.abs(gap).max() <= 1e-6, (e, p, gap)
    print(f"penetrating results: {seen}, worst |dist - touch dist| {worst:.3e}")
    return seen


def check_swap(rep, rows, swapped, masks):
    """(a, b) exchanged: dist and flags keep their bits, geom and point swap, the normal is negated - on the pairs whose winner does not
    hold both orders (groups that share geoms keep the first order's orientation)"""
    done = 0
    for k, e in enumerate(rows):
        for p, (a, b) in enumerate(masks):
            assert cc.same_bits(rep["dist"][e, p], swapped["dist"][k, p]) and rep["flags"][e, p] == swapped["flags"][k, p], (e, p)
            ga, gb = (int(x) for x in rep["geom"][e, p])
            if ga >= 0 and cr.both_orders(a, b, ga, gb):
                continue
            assert np.array_equal(swapped["geom"][k, p], rep["geom"][e, p][::-1]), (e, p)
            assert cc.same_bits(swapped["point"][k, p], rep["point"][e, p][::-1]), (e, p)
            assert np.array_equal(swapped["normal"][k, p], -rep["normal"][e, p]), (e, p)
            done += int(ga >= 0)
    assert done > 0
    return done


def check_all_separated(res, ref):
    """every separated result of `run` against the reference; prints and returns the worst deviations"""
    worst = dict(dist=0.0, cert=0.0)
    R = ref["ref"]
    ns, npn = check_separated(res["rich"], ref["rich"], R, "rich", worst=worst)
    assert ns >= 3 and npn >= 3, (ns, npn)                                       # both branches are exercised
    ws, wp = check_separated(res["way"], ref["way"], R, "waypoints", worst=worst)
    assert wp == 0 or ws > 0
    assert not any(int(f) & 1 for f in res["way"]["flags"][0])                   # the lifted arm: every cross-body pair is separated
    ss, sp = check_separated(res["single"], ref["single"], R, "single", worst=worst)
    assert (ss, sp) == (len(SINGLE_SPECS), 0), (ss, sp)
    ps, pp = check_separated(res["parallel"], ref["parallel"], R, "parallel", worst=worst)
    assert (ps, pp) == (1, 0)
    n = res["parallel"]["normal"][0, 0].astype(np.float64)
    assert np.abs(n - ref["parallel"][0][0]["n"]).max() <= 1e-6, n
    print(f"worst |dist - reference| {worst['dist']:.3e} m, worst certificate violation on the kernel's witnesses {worst['cert']:.3e} m "
          f"(asserted: {TOL:g}, {SLACK:g})")
    return worst


def check_invariants(res):
    """q = the env's own arm angles and a permutation of env_ids: the rows' bits; (a, b) swapped; the bound state untouched"""
    for f in FIELDS:
        assert cc.same_bits(res["rich_q"][f], res["rich"][f][[2, 0]]), f
    check_swap(res["rich"], (0, 2), res["rich_swapped"], res["group_masks"])
    for a, b in zip(res["before"], res["after"]):
        assert cc.same_bits(a, b)                                               # qpos, qvel, ctrl and the warmstart


def check_members(res):
    """a group pair's result is the minimum of the kernel's own single-geom-pair results over its members, bit for bit, with the first
    minimum's geoms - a culling bound that is no lower bound would lose the winner"""
    single, group = res["member_single"], res["member_group"]
    for e in range(2):
        d = single["dist"][e]
        k = int(np.argmin(d))                                                    # (first minimum: the members are in pair-list order per a-side geom)
        assert cc.same_bits(group["dist"][e, 0], d.min()), (e, group["dist"][e, 0], d.min())
        ties = [j for j in range(len(d)) if d[j] == d.min()]
        assert tuple(group["geom"][e, 0]) in [tuple(single["geom"][e, j]) for j in ties], (e, group["geom"][e, 0], single["geom"][e, k])
        j = [tuple(single["geom"][e, j]) for j in ties].index(tuple(group["geom"][e, 0]))
        for f in ("point", "normal", "flags"):
            assert cc.same_bits(group[f][e, 0], single[f][e, ties[j]]), (e, f)
        assert int(group["queries"][e, 0]) <= len(d)
    print(f"members: group dist {group['dist'][:, 0]}, exact queries of the group {group['queries'][:, 0]} of {single['dist'].shape[1]} members")


def check_beyond(res):
    b = res["beyond"]
    assert b["flags"][0, 0] == 4 and b["dist"][0, 0] == np.float32(1e-3) and np.all(b["geom"][0, 0] == -1)
    assert np.all(cc.bits(b["point"][0, 0]) == 0) and np.all(cc.bits(b["normal"][0, 0]) == 0)
    assert b["flags"][1, 0] & 8 and b["flags"][1, 0] & 4 and b["dist"][1, 0] == np.float32(1e-3) and np.all(b["geom"][1, 0] == -1)
    assert np.all(cc.bits(b["point"][1, 0]) == 0) and np.all(cc.bits(b["normal"][1, 0]) == 0) and b["queries"][1, 0] == 0
    assert b["flags"][2, 0] == 4 and b["dist"][2, 0] == np.float32(1e-3) and np.all(b["geom"][2, 0] == -1) and b["queries"][2, 0] == 0


def check_argument_errors(sim, blobs):
    """the argument and state errors of so101_proximity, one assertion per message"""
    import ctypes as C
    L, h = sim.sim.L, sim.sim.h
    err = lambda: L.so101_last_error(h).decode()
    ngeom = len(blobs["meta"]["geom_names"])
    gpu = sim.backend == "gpu"
    mk = lambda shape, dt: (sim.torch.zeros(shape, dtype=sim.torch.int32 if dt == np.int32 else sim.torch.float32, device=sim.dev) if gpu else np.zeros(shape, dt))
    dist, idx, qq = mk((4, 16), np.float32), mk((4,), np.int32), mk((4, 6), np.float32)
    one = native.geom_pair_array([((2, 0, 0, 0), (1 << 19, 0, 0, 0))])
    P = lambda a: None if a is None else sim.ptr(a)

    def call(hh=h, idx=None, n=2, q=None, pairs=one, npair=1, max_dist=0.1, out="default"):
        o = native.ProximityOut(dist=P(dist)) if out == "default" else out
        return L.so101_proximity(hh, P(idx), n, P(q), pairs, npair, max_dist, C.byref(o) if o is not None else None, sim.stream() if gpu else None)

    assert call() == 0 and call(idx=idx, n=4, q=qq) == 0
    assert call(hh=None) == -1
    assert call(out=None) == -1 and "NULL out" in err()
    assert call(out=native.ProximityOut()) == -1 and "no output" in err()
    for n in (0, -1, (1 << 26) + 1):
        assert call(n=n, idx=idx) == -1 and "n must be 1 .. 2^26" in err()
    assert call(n=3) == -1 and "exceeds" in err()
    for npair in (0, -1, 17):
        assert call(npair=npair) == -1 and "npair must be 1 .. 16" in err()
    assert call(pairs=None) == -1 and "NULL pairs" in err()
    for side in (0, 1):
        empty = native.geom_pair_array([((1, 0, 0, 0), (2, 0, 0, 0)), ((0, 0, 0, 0), (4, 0, 0, 0))[::1 if side == 0 else -1]])
        assert call(pairs=empty, npair=2) == -1 and f"pair 1, group {'ab'[side]} is empty" in err()
        words = [0, 0, 0, 0]; words[ngeom >> 5] = 1 << (ngeom & 31)
        beyond = native.geom_pair_array([((1, 0, 0, 0), tuple(words))[::1 if side == 1 else -1]])
        assert call(pairs=beyond, npair=1) == -1 and f"bit {ngeom} is at or beyond ngeom" in err()
    for md in (0.0, -1.0, 10.5, float("inf"), float("nan")):
        assert call(max_dist=md) == -1 and "max_dist must be" in err(), md
    assert call(max_dist=10.0) == 0
    un = native.Sim(blobs["f32"], 2, lib_path=sim.sim.L._name)
    assert call(hh=un.h) == -4 and b"not bound" in L.so101_last_error(un.h)
    assert call(hh=un.h, max_dist=0.0) == -1                                     # the arguments are checked first
    un.close()
    if gpu:
        sim.torch.cuda.synchronize()


def check_python_arguments(blobs):
    """ProximitySensing's own argument checks, on a stand-in that has the scene's groups and nothing to launch on"""
    import pytest
    from so101_sim_amd import proximity as px

    class Stub(ct.ContactSensing, px.ProximitySensing):
        _geom_limit = ct.MAX_GEOMS
        meta = blobs["meta"]
        geom_group = ct.ContactSensing._geom_group

        def _geom_groups(self):
            return cc.groups(blobs)

    s = Stub()
    for md in (0.0, -0.1, float("nan"), float("inf"), 10.5, "far", None):
        with pytest.raises(ValueError, match="max_dist must be"):
            s._proximity([("gripper", "object")], None, None, md)
    with pytest.raises(ValueError, match="1 .. 16 pairs"):
        s._proximity([("gripper", "object")] * 17, None, None, 0.1)
    with pytest.raises(ValueError, match="1 .. 16 pairs"):
        s._proximity([], None, None, 0.1)
    with pytest.raises(ValueError, match="unknown geom group"):
        s._proximity([("gripper", "no_such_thing")], None, None, 0.1)
