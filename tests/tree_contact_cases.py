"""Shared cases of the contact-interface tests of the general-tree engine (so101_tree_contacts, include/so101.h): the raw call on a
TreeArraySim of either backend, the states, the group pairs and the checks both backends run - tests/test_tree_contacts_emu.py through
the emulated build, tests/test_tree_contacts_gpu.py on the MI355X.  Checks that do not depend on the engine (frames, swap, the outside
convention, row equality) are those of tests/contact_cases.py.

The states, chosen on the CPU with the fp64 oracle (their contact counts and touching pairs are asserted by the tests, so a state cannot
silently go empty):

  hand-over (banana blob, 32-dof build, 64 contacts), 9 envs
    0-5  post-reset states of tests/test_tree_parity.py::_scene_states(raw64, 6, 0): props at rest on the table, random arm targets.
         14 contacts each: 10 props | table, 4 finger on finger (the grippers are closed at home: arms | arms, both orders hold).
    6-7  _scripted_states(raw64, "on_right", 2): the banana dropped onto the right gripper, advanced with the oracle's substeps until its
         list holds a right_gripper | object contact, at most SCRIPT_MAX_SUBSTEPS (the scripted placement already overlaps the fingers: the
         oracle finds the contact after 0 substeps; 16 contacts, 4 of them right_gripper | object).
    8    "nobody touches": scene state 0 with both props lifted 0.5 m and all four fingers opened to 0.03 m.  The bare-arm blob is another
         model and cannot share the batch, and at home its fingers touch each other as well (4 contacts); with the fingers open the oracle
         reports no contact.

  Dining (banana blob, 64-dof build, 160 contacts), 2 envs, tests/test_dining.py::_dining_states
    No SETTLED state exceeds 64 contacts: seeds 0-3, two envs each, settle 1000, give 32-48 (the props rest on ~34 contacts).  The
    six props landing do: 42-50 substeps into the settle the oracle reports 110-140 contacts (654-834 rows, below the 960).  So
    0    _dining_states(2, 1, settle=1000) env 0: settled, 48 contacts - the first lane pass only;
    1    _dining_states(2, 1, settle=45) env 0: the props landing, 140 contacts, 834 rows - the second lane pass full, twelve contacts in
         the third, the rows far beyond what the 32-dof build keeps in LDS.

The pairs: grippers | object, right_gripper | object, arms | table, object | container, props | table, arms | arms (overlapping groups: a
finger-on-finger contact holds both orders and counts once) and left_gripper | container, which no state touches.  No state has an arm on
the table or the object on the container: those pairs and the last are the "nobody touches" case (count 0, dist +inf, zero sums).

The force-sum bound: k * sum |f_j| + 1e-7 with k = 1e-5 in the 32-dof build (64 terms, the bound of tests/contact_cases.py) and 2e-5 in
the 64-dof build: 160 terms plus the rotation give (159 + 4) * 2^-24 ~ 9.7e-6 in the worst case, doubled."""
from __future__ import annotations

import functools

import numpy as np

from oracle.oracle import Oracle
from so101_sim_amd import contacts as ct, native
from so101_sim_amd.model import blob as blobfmt
from so101_sim_amd.model import scenes
from tests import contact_cases as cc, contact_ref as cr
from tests.contact_cases import bound4, check_touch, force_errors, raw_contacts          # (one copy for both engines)

PAIR_SPECS = (("grippers", "object"), ("right_gripper", "object"), ("arms", "table"), ("object", "container"), ("props", "table"), ("arms", "arms"),
              ("left_gripper", "container"))
SEEN = dict(handover=[True, True, False, False, True, True, False], dining=[False, False, False, False, True, True, False])
SUM_BOUND_K = {32: 1e-5, 64: 2e-5}
SCRIPT_MAX_SUBSTEPS = 200
HANDOVER_COUNTS = [14, 14, 14, 14, 14, 14, 16, 16, 0]          # the oracle's; the kernel's lists are compared with them contact by contact
HANDOVER_FREE, HANDOVER_SCRIPTED = 8, (6, 7)
EMU_HANDOVER = (0, 6)                                           # a resting and a gripper-on-object state
DINING_SEED, DINING_LANDING_SUBSTEPS = 1, 45
DINING_COUNTS = [48, 140]
FIELDS = native.CONTACT_OUT_FIELDS
GEOMETRY = cc.GEOMETRY
PAIR_GEOMETRY, PAIR_FORCES = cc.PAIR_GEOMETRY, cc.PAIR_FORCES
same_bits = cc.same_bits


def blobs(kind):
    """-> dict(f64, f32, meta, groups) of the banana hand-over blob or the banana Dining blob"""
    load = scenes.load_dining_blob if kind == "dining" else scenes.load_aloha_blob
    (raw64, _), (raw32, meta) = load("banana", "f64"), load("banana", "f32")
    return dict(f64=raw64, f32=raw32, meta=meta, groups=ct.aloha_groups(meta, blobfmt.unpack(raw32)))


def pair_masks(b, specs=PAIR_SPECS):
    return [(b["groups"][x].mask(8), b["groups"][y].mask(8)) for x, y in specs]


def _pair_counts(b, contacts):
    geom = np.array([[c["geom1"], c["geom2"]] for c in contacts], dtype=np.int64).reshape(-1, 2)
    return cr.reduce_pairs(pair_masks(b), geom, [c["dist"] for c in contacts])[0]


@functools.lru_cache(maxsize=None)
def handover_states():
    """-> Q [30, 9], V [28, 9], CT [14, 9], W [28, 9] (float64), computed once per process with the oracle"""
    from tests.test_tree_parity import _scene_states, _scripted_states
    b = blobs("handover")
    Q, V, W, CT = (x.copy() for x in _scene_states(b["f64"], 6, 0))
    home = np.concatenate([scenes.ALOHA_HOME_CTRL] * 2)
    o = Oracle(b["f64"])
    cols = []
    Qs, Vs = _scripted_states(b["f64"], "on_right", 2)
    for e in range(2):
        o.set_state(Qs[:, e], Vs[:, e], np.zeros(o.nv)); o.set_ctrl(home)
        for k in range(SCRIPT_MAX_SUBSTEPS + 1):
            o.forward()
            if _pair_counts(b, o.contacts())[1] > 0:
                break
            o.substeps(1, False)
        else:
            raise AssertionError(f"scripted state {e}: no right_gripper | object contact within {SCRIPT_MAX_SUBSTEPS} substeps")
        cols.append(o.get_state() + (home,))
    q = Q[:, 0].copy()
    q[18] += 0.5; q[25] += 0.5                      # z of the object and of the container
    q[[6, 7, 14, 15]] = 0.03                        # the four fingers, open
    o.set_state(q, np.zeros(o.nv), np.zeros(o.nv)); o.set_ctrl(home); o.forward()
    assert len(o.contacts()) == 0, "the free state has a contact"
    cols.append((q, np.zeros(o.nv), np.zeros(o.nv), home))
    add = lambda A, k: np.concatenate([A, np.stack([c[k] for c in cols], axis=1)], axis=1)
    return add(Q, 0), add(V, 1), add(CT, 3), add(W, 2)


@functools.lru_cache(maxsize=None)
def dining_states():
    """-> Q [58, 2], V [52, 2], CT [14, 2], W [52, 2]: a settled state and the same reset 45 substeps into its settle"""
    from tests.test_dining import _dining_states
    parts = [_dining_states(2, DINING_SEED, settle) for settle in (1000, DINING_LANDING_SUBSTEPS)]
    Q, V, W, CT = (np.stack([p[k][:, 0] for p in parts], axis=1) for k in range(4))
    return Q, V, CT, W


def states(kind, which=None):
    S = handover_states() if kind == "handover" else dining_states()
    return S if which is None else tuple(x[:, list(which)] for x in S)


def oracle_lists(kind, which=None):
    """per state: (contacts of the oracle's own forward pass, its row count)"""
    return [_oracle_lists(kind)[e] for e in (range(states(kind)[0].shape[1]) if which is None else which)]


@functools.lru_cache(maxsize=None)
def _oracle_lists(kind):
    b = blobs(kind)
    Q, V, CT, W = states(kind)
    o = Oracle(b["f64"])
    out = []
    for e in range(Q.shape[1]):
        o.inject_contacts([])
        o.set_state(Q[:, e], V[:, e], W[:, e]); o.set_ctrl(CT[:, e]); o.forward()
        out.append((o.contacts(), o.nefc))
    return out


def load(sim, Q, V, CT, W):
    sim.set_state(Q, V, CT, W)
    return sim


def run_batch(sim, masks):
    """ONE pass of what most tests read: the report with and without forces, the state before and after, the stage dump"""
    before = [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    rep = raw_contacts(sim, forces=True, pairs=masks)
    geo = raw_contacts(sim, forces=False, pairs=masks)
    after = [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    return dict(sim=sim, masks=masks, rep=rep, geo=geo, before=before, after=after, dbg=sim.debug_forward())


# ---------------------------------------------------------------------------------------------------------------- checks
def check_equals_dump(rep, geo, dbg):
    """count, geom, dist, pos, frame row 0 and force[:, 0] are the bits of so101_tree_debug_forward's dump, flags its flag word (no state
    here drops contacts for rows: flag 4 would lower the dump's count below the report's); slots at or beyond count are filled; the
    geometry without forces is the geometry with forces, bit for bit"""
    for e, d in enumerate(dbg):
        k = int(rep["count"][e])
        assert not d["flags"] & 4
        assert k == d["ncon"] == len(d["contacts"]) and int(rep["flags"][e]) == d["flags"], (e, k, d["ncon"], rep["flags"][e], d["flags"])
        for i, c in enumerate(d["contacts"]):
            assert (int(rep["geom"][e, i, 0]), int(rep["geom"][e, i, 1])) == (c["geom1"], c["geom2"]), (e, i)
            # (the dump is float32 widened to float64 by the harness: widening this side the same way compares the float32 bits)
            assert float(rep["dist"][e, i]) == c["dist"], (e, i)
            assert np.array_equal(rep["pos"][e, i].astype(np.float64), c["pos"]), (e, i)
            assert np.array_equal(rep["frame"][e, i, 0:3].astype(np.float64), c["normal"]), (e, i)
            assert float(rep["force"][e, i, 0]) == c["fn"], (e, i, rep["force"][e, i], c["fn"])
            assert np.all(rep["force"][e, i, c["dim"]:] == 0), (e, i)
        assert np.all(rep["geom"][e, k:] == -1) and np.all(np.isposinf(rep["dist"][e, k:]))
        assert np.all(cc.bits(rep["pos"][e, k:]) == 0) and np.all(cc.bits(rep["frame"][e, k:]) == 0) and np.all(cc.bits(rep["force"][e, k:]) == 0)
    for f in ("count", "geom", "dist", "pos", "frame"):
        assert same_bits(rep[f], geo[f]), f
    assert np.all((rep["flags"] & geo["flags"]) == geo["flags"])          # (the solve may add flag 4 to the collision's bits)


def check_geometry(rep, lists):
    """the kernel's lists against the oracle's, contact by contact, with the tolerances and shares of tests/test_tree_parity.py::check_forward
    (default narrowphase): depth 2e-6 + 1e-4 relative, normal 1e-6, position 2e-5; `loose` (depth or normal beyond that, within 1e-4 m /
    cos 0.999) at most 2 % + 1, `witness` (the point elsewhere on a flat facet) at most 5 % + 1"""
    total = loose = witness = 0
    for e, (oc, _) in enumerate(lists):
        mine = cc.as_list(rep, e)
        assert rep["flags"][e] == 0 and len(mine) == len(oc), (e, len(mine), len(oc), rep["flags"][e])
        assert [(c["geom1"], c["geom2"]) for c in mine] == [(c["geom1"], c["geom2"]) for c in oc], e
        for a, b in zip(mine, oc):
            face = abs(a["dist"] - b["dist"]) < 2e-6 + 1e-4 * abs(b["dist"]) and a["normal"] @ b["normal"] > 1 - 1e-6
            if not face:
                assert abs(a["dist"] - b["dist"]) < 1e-4 and np.abs(a["pos"] - b["pos"]).max() < 1.5e-2 and a["normal"] @ b["normal"] > 0.999, (e, a, b)
                loose += 1
            elif np.abs(a["pos"] - b["pos"]).max() >= 2e-5:
                assert np.abs(a["pos"] - b["pos"]).max() < 1.5e-2, (e, a, b)
                witness += 1
        total += len(oc)
    print(f"{len(lists)} states: {total} contacts, {loose} loose, {witness} witness points elsewhere on a facet")
    assert loose <= 0.02 * max(total, 1) + 1 and witness <= 0.05 * max(total, 1) + 1, (loose, witness, total)
    return total


def check_quiet(rep, seen):
    quiet = ~np.asarray(seen)
    assert np.all(rep["pair_count"][:, quiet] == 0) and np.all(np.isposinf(rep["pair_dist"][:, quiet]))
    assert np.all(rep["pair_normal"][:, quiet] == 0) and np.all(rep["pair_force"][:, quiet] == 0)


def oracle_forces(kind, rep, which=None):
    """per entry of `rep`: the oracle's forces on the kernel's own contact list, [count, 6] fp64"""
    b = blobs(kind)
    Q, V, CT, W = states(kind, which)
    o = Oracle(b["f64"])
    out = []
    for e in range(Q.shape[1]):
        o.set_state(Q[:, e], V[:, e], W[:, e]); o.set_ctrl(CT[:, e])
        o.inject_contacts(cc.as_list(rep, e)); o.forward()
        out.append(cr.oracle_contact_forces(o) if int(rep["count"][e]) else np.zeros((0, 6)))
    o.inject_contacts([])
    return out
