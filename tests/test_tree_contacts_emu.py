"""Contact sensing of the general-tree engine without a GPU: the library's argument checks for both builds, the per-contact report, the
touch reduction, the swap and env_index through the emulated build of the kernel source (tests/hostemu) on 2 hand-over states and the
140-contact Dining state (tests/tree_contact_cases.py; half a minute emulated), and the Python layer's geom groups.  The checks themselves are shared with tests/test_tree_contacts_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from so101_sim_amd import contacts as ct, native
from so101_sim_amd.model import blob as blobfmt
from so101_sim_amd.model import scenes
from tests import contact_cases as cc, contact_ref as cr, tree_contact_cases as tc
from tests.simharness import TreeArraySim


@pytest.fixture(scope="module")
def emu():
    """ONE pass of everything the hand-over tests below read: the 2-env batch, its stage dump, the report with and without forces, the
    report of the swapped pairs (each emulated launch costs seconds)"""
    b = tc.blobs("handover")
    sim = tc.load(TreeArraySim(b["f32"], 2, backend="emu"), *tc.states("handover", tc.EMU_HANDOVER))
    out = tc.run_batch(sim, tc.pair_masks(b))
    out["swapped"] = tc.raw_contacts(sim, forces=True, pairs=[(y, x) for x, y in out["masks"]], want=tc.PAIR_GEOMETRY + tc.PAIR_FORCES)
    return out


@pytest.mark.parametrize("kind,build,capacity", [("handover", 32, 64), ("dining", 64, 160)])
def test_argument_and_state_errors(kind, build, capacity):
    """the error matrix of tests/test_contacts_emu.py, message for message, under the name so101_tree_contacts and with the handle's ngeom"""
    b = tc.blobs(kind)
    sim = TreeArraySim(b["f32"], 2, backend="emu")
    assert (sim.sim.build, sim.sim.max_contacts) == (build, capacity)
    L, h = sim.sim.L, sim.sim.h
    err = lambda: L.so101_tree_last_error(h).decode()
    ngeom = len(b["meta"]["geom_names"])
    assert ngeom == sim.sim.ngeom
    cnt, pc, pn = np.zeros(4, np.int32), np.zeros((4, 16), np.int32), np.zeros((4, 16), np.float32)
    force, pf = np.zeros((4, capacity, 6), np.float32), np.zeros((4, 16, 3), np.float32)
    idx = np.zeros(4, np.int32)
    w8 = lambda *bits: tuple(sum(1 << (g & 31) for g in bits if g >> 5 == k) for k in range(8))
    one = native.geom_pair_array([(w8(0), w8(1))], 8)
    P = lambda a: None if a is None else a.ctypes.data

    def call(hh=h, idx=None, n=2, forces=0, pairs=None, npair=0, out="default", **fields):
        o = native.ContactOut(**{k: P(v) for k, v in (fields or dict(count=cnt)).items()}) if out == "default" else out
        return L.so101_tree_contacts(hh, P(idx), n, forces, pairs, npair, C.byref(o) if o is not None else None, None)

    assert call() == 0 and call(idx=idx, n=4) == 0 and call(pairs=one, npair=1, pair_count=pc) == 0
    assert call(hh=None) == -1
    assert call(out=None) == -1 and err() == "so101_tree_contacts: NULL out"
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
        empty = native.geom_pair_array([(w8(0), w8(1)), (w8(), w8(2))[::1 if side == 0 else -1]], 8)
        assert call(pairs=empty, npair=2, pair_count=pc) == -1 and f"pair 1, group {'ab'[side]} is empty" in err()
        beyond = native.geom_pair_array([(w8(0), w8(ngeom))[::1 if side == 1 else -1]], 8)
        assert call(pairs=beyond, npair=1, pair_count=pc) == -1 and f"bit {ngeom} is at or beyond ngeom = {ngeom}" in err() and err().startswith("so101_tree_contacts: pair 0")
    assert call(pairs=native.geom_pair_array([(w8(ngeom - 1), w8(0))], 8), npair=1, pair_count=pc) == 0          # the last geom is a member like any other
    assert call(pairs=native.geom_pair_array([(w8(0), w8(255))], 8), npair=1, pair_count=pc) == -1 and "bit 255" in err()      # the eighth word is read
    assert call(force=force) == -1 and "need forces" in err()
    assert call(pairs=one, npair=1, pair_normal=pn) == -1 and "need forces" in err()
    assert call(pairs=one, npair=1, pair_force=pf) == -1 and "need forces" in err()
    # nothing bound: an error of call order, after the arguments have been checked
    un = native.TreeSim(b["f32"], 2, lib_path=sim.sim.L._name)
    assert call(hh=un.h) == -4 and b"so101_tree_contacts: state buffers not bound" in L.so101_tree_last_error(un.h)
    assert call(hh=un.h, out=None) == -1
    un.close()
    assert "so101_tree_contacts" in native.EXPORTS


def test_report_is_bit_identical_to_the_stage_dump_and_changes_no_state(emu):
    tc.check_equals_dump(emu["rep"], emu["geo"], emu["dbg"])
    counts = [int(k) for k in emu["rep"]["count"]]
    print(f"emulated hand-over states {tc.EMU_HANDOVER}: contacts {counts}, flags {emu['rep']['flags'].tolist()}")
    assert counts == [tc.HANDOVER_COUNTS[e] for e in tc.EMU_HANDOVER]
    for x, y in zip(emu["before"], emu["after"]):
        assert tc.same_bits(x, y)                                   # qpos, qvel, ctrl and the warmstart: untouched
    for f in tc.PAIR_GEOMETRY:
        assert tc.same_bits(emu["rep"][f], emu["geo"][f]), f        # counts and distances of the pairs need no forces
    cc.check_frames(emu["rep"])


def test_geometry_and_forces_against_the_oracle(emu):
    """the shares of check_geometry are conditions on the chosen states: the emulated build (the kernels' fp32 arithmetic) keeps within them"""
    tc.check_geometry(emu["geo"], tc.oracle_lists("handover", tc.EMU_HANDOVER))
    f_ref = tc.oracle_forces("handover", emu["rep"], tc.EMU_HANDOVER)
    for e in range(2):
        err = tc.force_errors(emu["rep"], e, f_ref[e])
        print(f"state {tc.EMU_HANDOVER[e]}: force error per contact {err[0]:.3e}, per geom pair {err[1]:.3e}")
        assert max(err) <= 1e-2          # (a sanity bound of the CPU run - the real ones are measured and asserted on the GPU)


def test_touch_reduction_and_swap(emu):
    seen = tc.check_touch(emu["rep"], emu["masks"], tc.SUM_BOUND_K[32])
    assert seen.tolist() == tc.SEEN["handover"], seen
    tc.check_quiet(emu["rep"], seen)
    cc.check_swap(emu["rep"], emu["swapped"], emu["masks"])


def test_env_index_repeats_chunks_and_outside(emu):
    """forces with n = 5 > n_envs = 2: three launches, an env named three times (each entry in its own scratch slice), two entries outside"""
    sim, masks = emu["sim"], emu["masks"]
    rep = tc.raw_contacts(sim, n=5, env_index=[1, 2, 1, -1, 1], forces=True, pairs=masks)
    cc.check_outside(rep, (1, 3), len(masks))
    cc.check_rows_equal(rep, (0, 2, 4), emu["rep"], (1, 1, 1))
    alone = tc.raw_contacts(sim, n=1, env_index=[0], forces=False, pairs=masks[:2])
    assert tc.same_bits(alone["pair_count"], emu["geo"]["pair_count"][0:1, :2]) and tc.same_bits(alone["pair_dist"], emu["geo"]["pair_dist"][0:1, :2])
    cc.check_rows_equal({k: alone[k] for k in tc.GEOMETRY}, (0,), emu["geo"], (0,))


def test_dining_state_emulated():
    """the Dining state with the props landing through the 64-dof build: 140 contacts, all three lane passes carry some"""
    b = tc.blobs("dining")
    sim = tc.load(TreeArraySim(b["f32"], 1, backend="emu"), *tc.states("dining", (1,)))
    out = tc.run_batch(sim, tc.pair_masks(b))
    tc.check_equals_dump(out["rep"], out["geo"], out["dbg"])
    assert int(out["rep"]["count"][0]) == tc.DINING_COUNTS[1] > 128
    cc.check_frames(out["rep"])
    tc.check_geometry(out["geo"], tc.oracle_lists("dining", (1,)))
    seen = tc.check_touch(out["rep"], out["masks"], tc.SUM_BOUND_K[64])
    assert seen.tolist() == tc.SEEN["dining"], seen


@pytest.mark.parametrize("name", ["banana", "pen", "dining"])
def test_aloha_groups_are_the_task_geom_classes(name):
    raw, meta = scenes.load_dining_blob("mug", "f32") if name == "dining" else scenes.load_aloha_blob(name, "f32")
    m = blobfmt.unpack(raw)
    g = ct.aloha_groups(meta, m)
    cls, geom_body, names = np.asarray(m["task_geom_class"]).ravel(), np.asarray(m["geom_body"]).ravel(), meta["body_names"]
    bits = dict(object=1, container=2) if name == "dining" else dict(object=1, container=2, left_gripper=4, right_gripper=8)
    for group, bit in bits.items():
        assert set(g[group].geoms) == {k for k, c in enumerate(cls) if int(c) & bit} and g[group].geoms, group
    assert not any(int(c) & 12 for c in cls) or name != "dining"                     # Dining carries bits 1 and 2 only: the grippers come from the body tree
    for side in ("left", "right"):
        below = {k for k, bd in enumerate(geom_body) if names[int(bd)] in (f"{side}/gripper_link", f"{side}/gripper_base", f"{side}/left_finger_link", f"{side}/right_finger_link")}
        assert set(g[f"{side}_gripper"].geoms) == below and len(below) == 10
        assert set(g[f"{side}_arm"].geoms) == {k for k, bd in enumerate(geom_body) if names[int(bd)].startswith(side + "/")}
    assert set(g["arms"].geoms) == set(g["left_arm"].geoms) | set(g["right_arm"].geoms) and set(g["grippers"].geoms) == set(g["left_gripper"].geoms) | set(g["right_gripper"].geoms)
    free = {b for b, t in enumerate(np.asarray(m["body_jnttype"]).ravel()) if int(t) == 2}
    assert set(g["props"].geoms) == {k for k, bd in enumerate(geom_body) if int(bd) in free} and len(free) == (6 if name == "dining" else 2)
    # one group per body with geoms, world and table among them; every geom in exactly one of them
    bodies = [n for b, n in enumerate(names) if (geom_body == b).any()]
    key = lambda n: n if (n in g and set(g[n].geoms) == {k for k, bd in enumerate(geom_body) if names[int(bd)] == n}) else n + "_body"
    assert {"world", "table"} <= set(bodies)
    assert sorted(k for n in bodies for k in g[key(n)].geoms) == list(range(len(geom_body)))
    if name == "dining":          # the prop NAMED container is not the mug task's container (the plate)
        assert key("container") == "container_body" and set(g["container"].geoms) == set(g["plate"].geoms) and set(g["object"].geoms) == set(g["mug"].geoms)
        assert max(g["props"].geoms) >= 128 and len(g["props"].mask(8)) == 8
        with pytest.raises(ValueError, match="does not fit"):
            g["props"].mask()
    # geom names are not unique: a name resolves to all its geoms
    dup = "vx300s_8_custom_finger_left"
    hits = [k for k, n in enumerate(meta["geom_names"]) if n == dup]
    assert len(hits) == 2 and ct.resolve(dup, g, meta, limit=ct.TREE_MAX_GEOMS).geoms == tuple(hits)
    assert ct.resolve("grippers", g, meta) is g["grippers"]


def test_geom_group_with_eight_words_and_four_unchanged():
    g4 = ct.GeomGroup("t", (0, 33, 64, 127))
    assert g4.mask() == (1, 2, 1, 1 << 31) and g4.limit == 128 and g4.mask(8) == (1, 2, 1, 1 << 31, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="0 .. 127"):
        ct.GeomGroup("t", (128,))
    g8 = ct.GeomGroup("t", (0, 128, 255), ct.TREE_MAX_GEOMS)
    assert g8.mask(8) == (1, 0, 0, 0, 1, 0, 0, 1 << 31) and all(cr.in_mask(g8.mask(8), k) == (k in g8.geoms) for k in range(256))
    with pytest.raises(ValueError, match="0 .. 255"):
        ct.GeomGroup("t", (256,), ct.TREE_MAX_GEOMS)
    with pytest.raises(ValueError, match="does not fit"):
        g8.mask()
    with pytest.raises(ValueError):
        g8.mask(5)
    with pytest.raises(ValueError, match="limit"):
        ct.GeomGroup("t", (1,), 64)
    u = g4 | g8
    assert u.limit == 256 and u.geoms == (0, 33, 64, 127, 128, 255) and (g4 | g4).limit == 128
    assert ct.GeomGroup("t", (1, 2), ct.TREE_MAX_GEOMS).mask() == (6, 0, 0, 0)          # a small group of the wide kind still fits four words
