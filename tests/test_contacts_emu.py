"""Contact sensing without a GPU: the library's argument checks, the per-contact report, the touch reduction and env_index through
the emulated build of the kernel source (tests/hostemu), on 4 of the contact-rich states (tests/contact_cases.py), and the Python
layer's geom groups.  The checks themselves are shared with tests/test_contacts_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from so101_sim_amd import contacts as ct, native
from so101_sim_amd.model import blob as blobfmt
from tests import contact_cases as cc, contact_ref as cr
from tests.simharness import ArraySim


@pytest.fixture(scope="module")
def emu(blobs, golden):
    """ONE pass of everything the tests below read: the 4-env batch, its stage dump, the report with and without forces, the report of
    the swapped pairs (the emulator runs a wavefront as 64 OS threads: each launch costs seconds)"""
    sim = cc.load(ArraySim(blobs["f32"], 4, backend="emu"), *cc.rich_states(golden, cc.EMU_STATES))
    masks = cc.pair_masks(blobs)
    before = [a.copy() for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    rep = cc.raw_contacts(sim, forces=True, pairs=masks)
    geo = cc.raw_contacts(sim, forces=False, pairs=masks)
    swapped = cc.raw_contacts(sim, forces=True, pairs=[(b, a) for a, b in masks], want=cc.PAIR_GEOMETRY + cc.PAIR_FORCES)
    after = [a.copy() for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    return dict(sim=sim, masks=masks, rep=rep, geo=geo, swapped=swapped, before=before, after=after, dbg=sim.debug_forward())


def test_argument_and_state_errors(blobs):
    sim = ArraySim(blobs["f32"], 2, backend="emu")
    L, h = sim.sim.L, sim.sim.h
    err = lambda: L.so101_last_error(h).decode()
    ngeom = len(blobs["meta"]["geom_names"])
    cnt, pc, pn = np.zeros(4, np.int32), np.zeros((4, 16), np.int32), np.zeros((4, 16), np.float32)
    force, pf = np.zeros((4, 64, 6), np.float32), np.zeros((4, 16, 3), np.float32)
    idx = np.zeros(4, np.int32)
    one = native.geom_pair_array([((1, 0, 0, 0), (2, 0, 0, 0))])
    P = lambda a: None if a is None else a.ctypes.data

    def call(hh=h, idx=None, n=2, forces=0, pairs=None, npair=0, out="default", **fields):
        o = native.ContactOut(**{k: P(v) for k, v in (fields or dict(count=cnt)).items()}) if out == "default" else out
        return L.so101_contacts(hh, P(idx), n, forces, pairs, npair, C.byref(o) if o is not None else None, None)

    assert call() == 0 and call(idx=idx, n=4) == 0 and call(pairs=one, npair=1, pair_count=pc) == 0
    assert call(forces=1, pairs=one, npair=1, force=force, pair_normal=pn, pair_force=pf) == 0
    assert call(hh=None) == -1
    assert call(out=None) == -1 and "NULL out" in err()
    assert call(out=native.ContactOut()) == -1 and "no output" in err()
    for n in (0, -1, (1 << 26) + 1):
        assert call(n=n, idx=idx) == -1 and "n must be 1 .. 2^26" in err()
    assert call(n=3) == -1 and "exceeds" in err()
    for npair in (-1, 17):
        assert call(pairs=one, npair=npair) == -1 and "npair must be 0 .. 16" in err()
    assert call(npair=1, pair_count=pc) == -1 and "NULL pairs" in err()
    for f in ("pair_count", "pair_dist", "pair_normal", "pair_force"):
        assert call(forces=1, **{f: pn}) == -1 and "npair == 0" in err(), f
    for side in (0, 1):
        empty = native.geom_pair_array([((1, 0, 0, 0), (2, 0, 0, 0)), ((0, 0, 0, 0), (4, 0, 0, 0))[::1 if side == 0 else -1]])
        assert call(pairs=empty, npair=2, pair_count=pc) == -1 and f"pair 1, group {'ab'[side]} is empty" in err()
        words = [0, 0, 0, 0]; words[ngeom >> 5] = 1 << (ngeom & 31)
        beyond = native.geom_pair_array([((1, 0, 0, 0), tuple(words))[::1 if side == 1 else -1]])
        assert call(pairs=beyond, npair=1, pair_count=pc) == -1 and f"bit {ngeom} is at or beyond ngeom" in err()
    last = [0, 0, 0, 0]; last[(ngeom - 1) >> 5] = 1 << ((ngeom - 1) & 31)
    assert call(pairs=native.geom_pair_array([(tuple(last), (1, 0, 0, 0))]), npair=1, pair_count=pc) == 0          # the last geom is a member like any other
    assert call(force=force) == -1 and "need forces" in err()
    assert call(pairs=one, npair=1, pair_normal=pn) == -1 and "need forces" in err()
    assert call(pairs=one, npair=1, pair_force=pf) == -1 and "need forces" in err()
    # nothing bound: an error of call order, after the arguments have been checked
    un = native.Sim(blobs["f32"], 2, lib_path=sim.sim.L._name)
    assert call(hh=un.h) == -4 and b"not bound" in L.so101_last_error(un.h)
    assert call(hh=un.h, out=None) == -1
    un.close()
    # (a model with more than 128 geoms cannot be made for this engine: so101_create refuses more than 96, so that SO101_ERR_STATE is unreachable here)


def test_report_is_bit_identical_to_the_stage_dump_and_changes_no_state(emu):
    cc.check_equals_dump(emu["rep"], emu["geo"], emu["dbg"])
    assert [int(k) for k in emu["rep"]["count"]] == [d["ncon"] for d in emu["dbg"]] and min(emu["rep"]["count"]) >= 6
    for a, b in zip(emu["before"], emu["after"]):
        assert cc.same_bits(a, b)                                   # qpos, qvel, ctrl and the warmstart: untouched
    for f in cc.PAIR_GEOMETRY:
        assert cc.same_bits(emu["rep"][f], emu["geo"][f]), f        # counts and distances of the pairs need no forces


def test_frames_are_orthonormal_completions_of_their_normal(emu):
    cc.check_frames(emu["rep"])
    for n in ([0, 0, 1.0], [0, 1.0, 0], [0.6, 0.8, 0], [0.5, 0.5, np.sqrt(0.5)], [-0.3, -0.49, np.sqrt(1 - 0.09 - 0.49 ** 2)]):
        R = cr.make_frame(n)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and np.linalg.det(R) > 0 and np.array_equal(R[0], n)
    assert np.array_equal(cr.make_frame([0, 0, 1.0])[1], [0, 1, 0]) and np.array_equal(cr.make_frame([0, 1.0, 0])[1], [0, 0, 1])


def test_touch_reduction_against_the_kernels_own_list(emu):
    seen = cc.check_touch(emu["rep"], emu["masks"])
    assert seen.tolist() == [True, True, False, False, True, True, True], seen          # (no state has a pad on the object, or the object on the container)
    quiet = ~seen
    assert np.all(emu["rep"]["pair_count"][:, quiet] == 0) and np.all(np.isposinf(emu["rep"]["pair_dist"][:, quiet]))
    assert np.all(emu["rep"]["pair_normal"][:, quiet] == 0) and np.all(emu["rep"]["pair_force"][:, quiet] == 0)
    cc.check_swap(emu["rep"], emu["swapped"], emu["masks"])


def test_env_index_and_independence_of_the_other_entries(blobs, golden, emu):
    sim = cc.load(ArraySim(blobs["f32"], 3, backend="emu"), *cc.rich_states(golden, cc.EMU_STATES[:3]))
    rep = cc.raw_contacts(sim, n=4, env_index=[2, 3, -1, 0], forces=True, pairs=emu["masks"])
    cc.check_outside(rep, (1, 2), len(emu["masks"]))
    cc.check_rows_equal(rep, (0, 3), emu["rep"], (2, 0))            # the bits of the 4-env call without env_index: not a matter of n or neighbours
    alone = cc.raw_contacts(sim, n=1, env_index=[2], forces=False, pairs=emu["masks"][:2])
    assert cc.same_bits(alone["pair_count"], emu["geo"]["pair_count"][2:3, :2]) and cc.same_bits(alone["pair_dist"], emu["geo"]["pair_dist"][2:3, :2])
    cc.check_rows_equal({k: alone[k] for k in cc.GEOMETRY}, (0,), emu["geo"], (2,))


def test_geom_groups_come_from_the_blob(blobs):
    meta, m = blobs["meta"], blobfmt.unpack(blobs["f32"])
    g = ct.so100_groups(meta, m)
    geom_body = np.asarray(m["geom_body"]).ravel()
    arm_bodies = [int(b) for b in np.asarray(m["arm_body"]).ravel()]
    assert set(g["arm"].geoms) == {i for i, b in enumerate(geom_body) if int(b) in arm_bodies} and len(arm_bodies) == 6
    bodies = [n for n in meta["body_names"] if n in g]
    assert {"Fixed_Jaw", "Moving_Jaw", "table", "object", "container"} <= set(bodies)
    for i, a in enumerate(bodies):
        assert set(g[a].geoms) == {k for k, b in enumerate(geom_body) if meta["body_names"][int(b)] == a}
        for b in bodies[i + 1:]:
            assert not set(g[a].geoms) & set(g[b].geoms), (a, b)
    assert sorted(k for b in bodies for k in g[b].geoms) == list(range(len(geom_body)))          # every geom is in exactly one body group
    for pads, jaw in (("fixed_jaw_pads", "Fixed_Jaw"), ("moving_jaw_pads", "Moving_Jaw")):
        assert g[pads].geoms and set(g[pads].geoms) < set(g[jaw].geoms)
        assert all(meta["geom_names"][k].startswith(pads[:-1]) for k in g[pads].geoms)
    assert set(g["gripper"].geoms) == set(g["Fixed_Jaw"].geoms) | set(g["Moving_Jaw"].geoms)
    assert set(g["props"].geoms) == set(g["object"].geoms) | set(g["container"].geoms)
    # masks: bit (g & 31) of word g >> 5
    assert ct.GeomGroup("t", (0, 33, 64, 127)).mask() == (1, 2, 1, 1 << 31)
    assert all(cr.in_mask(g["arm"].mask(), k) == (k in g["arm"].geoms) for k in range(128))


def test_resolve_accepts_names_patterns_ids_and_rejects_the_rest(blobs):
    meta = blobs["meta"]
    g = ct.so100_groups(meta, blobfmt.unpack(blobs["f32"]))
    names = meta["geom_names"]
    assert ct.resolve("gripper", g, meta) is g["gripper"] and ct.resolve(g["arm"], g, meta) is g["arm"]
    assert ct.resolve("table", g, meta) is g["table"]                                              # a body name
    assert ct.resolve("table_surface", g, meta).geoms == (names.index("table_surface"),)           # a geom name
    assert ct.resolve("table_leg_*", g, meta).geoms == tuple(i for i, n in enumerate(names) if n.startswith("table_leg_"))
    assert ct.resolve([3, 1, 3], g, meta).geoms == (1, 3) and ct.resolve(np.array([5]), g, meta).geoms == (5,)
    for bad in ("no_such_thing", "zz*", 3.5, [], [-1], [len(names)], ["a"], None):
        with pytest.raises(ValueError, match="unknown geom group"):
            ct.resolve(bad, g, meta)
    with pytest.raises(ValueError, match="empty"):
        ct.GeomGroup("e", ())
