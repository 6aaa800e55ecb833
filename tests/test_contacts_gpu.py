"""Contact sensing on the MI355X (so101_contacts, include/so101.h; BatchedEnvironment.contacts / touch; physics.data.contact) against
the stage dump of so101_debug_forward (bits), the fp64 oracle (geometry, capacity rule, forces) and the fp64 reduction of
tests/contact_ref.py.  All 24 contact-rich states of tests/golden/contact_rich_states.json run as ONE 24-env batch per solver; the state
with more contacts than the capacity is a 1-env batch, the resting and the free-space state a 2-env batch.

The force bounds.  Per state the kernel's own contact list goes into the oracle (inject_contacts), which solves it in fp64; two
figures per env, both over max_k f_ref[k][0], the largest normal force of the state:
  per contact    max over contacts and the six entries of |f - f_ref|
  per geom pair  max over the touching geom pairs of |net - net_ref|, net = sum over the pair's contacts of R^T f[0:3] (world frame)
FORCE_MEASURED holds the worst of each over the 24 states as measured on the MI355X (profiles/README.md, "Contact sensing"); the
tests assert 4 x that, rounded up to one significant digit - the margin for fp32 reassociation across compilers and for a solver
that stops at its tolerance on ill-conditioned multi-contact patches."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from so101_sim_amd import native
from tests import contact_cases as cc, contact_ref as cr
from tests.parity_cases import KAT_PROPS, MANY_CONTACTS_QPOS, _compare_contact_lists
from tests.simharness import ArraySim

pytestmark = pytest.mark.gpu
FORCE_MEASURED = dict(contact=1.878e-4, pair=2.028e-4)  # worst figures of the 24 states on the MI355X (states 8 and 7): bounds 8e-4 and 9e-4


def _batch(blobs, golden, solver):
    sim = cc.load(ArraySim(blobs["f32"], 24, backend="gpu", solver=solver), *cc.rich_states(golden))
    masks = cc.pair_masks(blobs)
    before = [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    rep = cc.raw_contacts(sim, forces=True, pairs=masks)
    geo = cc.raw_contacts(sim, forces=False, pairs=masks)
    after = [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
    return dict(sim=sim, masks=masks, rep=rep, geo=geo, before=before, after=after)


@pytest.fixture(scope="module")
def newton(blobs, golden):
    return _batch(blobs, golden, native.SOLVER_NEWTON)


@pytest.fixture(scope="module")
def oracle_forces(blobs, golden, newton):
    """per state: the oracle's forces on the kernel's own contact list, [count, 6] fp64 (computed once, read by two tests)"""
    Q, V, A, W = cc.rich_states(golden)
    out = []
    for e in range(24):
        o = Oracle(blobs["f64"])
        o.set_state(Q[:, e], V[:, e], W[:, e]); o.set_ctrl(A[:, e])
        o.inject_contacts(cc.as_list(newton["rep"], e)); o.forward()
        out.append(cr.oracle_contact_forces(o))
    return out


@pytest.mark.parametrize("solver", ["newton", "pgs"])
def test_report_is_bit_identical_to_the_stage_dump_and_changes_no_state(blobs, golden, newton, solver):
    b = newton if solver == "newton" else _batch(blobs, golden, native.SOLVER_PGS)
    cc.check_equals_dump(b["rep"], b["geo"], b["sim"].debug_forward())
    for x, y in zip(b["before"], b["after"]):
        assert cc.same_bits(x, y)
    for f in cc.PAIR_GEOMETRY:
        assert cc.same_bits(b["rep"][f], b["geo"][f]), f
    cc.check_frames(b["rep"])
    counts = b["rep"]["count"]
    print(f"{solver}: contacts per state {counts.tolist()}, flags {b['rep']['flags'].tolist()}")
    assert counts.max() >= 30 and counts[cc.FREE_STATE] == 0
    if solver == "pgs":          # the PGS kernels solve 32 contacts at most and say so in the flags of a pass with forces - not of one without
        assert np.array_equal((b["rep"]["flags"] & 2) != 0, counts > 32) and np.all(b["geo"]["flags"] == 0)


def test_geometry_matches_the_oracle_on_every_state(blobs, golden, newton):
    Q, V, A, W = cc.rich_states(golden)
    total = loose = witness = 0
    for e in range(24):
        o = Oracle(blobs["f64"])
        o.set_state(Q[:, e], V[:, e], W[:, e]); o.set_ctrl(A[:, e]); o.forward()
        problems, t, l, w = _compare_contact_lists(cc.as_list(newton["geo"], e), o.contacts())
        assert not problems, (e, problems)
        assert newton["geo"]["flags"][e] == 0
        total, loose, witness = total + t, loose + l, witness + w
    print(f"24 states: {total} contacts, {loose} loose normals, {witness} witness points elsewhere on a facet")
    assert total == int(newton["geo"]["count"].sum()) and loose <= 0.02 * total and witness <= 0.05 * total, (total, loose, witness)


def test_capacity_rule_is_the_oracles(blobs):
    q = MANY_CONTACTS_QPOS
    sim = cc.load(ArraySim(blobs["f32"], 1, backend="gpu"), q[:, None], np.zeros((18, 1)), np.zeros((6, 1)), np.zeros((18, 1)))
    rep = cc.raw_contacts(sim, forces=False)
    assert rep["flags"][0] & 128 and not rep["flags"][0] & 2, rep["flags"]
    o = Oracle(blobs["f64"])
    o.set_state(q, np.zeros(18), np.zeros(18)); o.set_ctrl(np.zeros(6))
    o.forward()
    assert len(o.contacts()) > native.MAXCON
    o.set_contact_capacity(native.MAXCON); o.forward()
    ref = o.contacts()
    assert o.contacts_reduced() == 1 and int(rep["count"][0]) == len(ref) <= native.MAXCON
    problems, total, loose, witness = _compare_contact_lists(cc.as_list(rep, 0), ref)
    assert not problems, problems
    assert loose <= max(1, 0.05 * total) and witness <= max(2, 0.1 * total), (loose, witness, total)          # (the shares check_contact_capacity_mirrored asserts on this state)


def test_forces_match_the_oracle_on_the_kernels_list(newton, oracle_forces):
    worst = np.zeros(2)
    for e in range(24):
        err = cc.force_errors(newton["rep"], e, oracle_forces[e])
        print(f"state {e:2d}: {int(newton['rep']['count'][e]):2d} contacts, force error per contact {err[0]:.3e}, per geom pair {err[1]:.3e}")
        worst = np.maximum(worst, err)
    print(f"worst of the 24 states: per contact {worst[0]:.3e}, per geom pair {worst[1]:.3e}")
    assert worst[0] <= cc.bound4(FORCE_MEASURED["contact"]) and worst[1] <= cc.bound4(FORCE_MEASURED["pair"]), worst


def test_resting_and_free_space_states(blobs, golden):
    """the props at rest on the table under the home pose: object | table carries the object; the fixture's state without contacts: nobody
    touches anybody.  Read through a 2-env BatchedEnvironment, whose touch() is compared with the oracle here."""
    import torch
    from so101_sim_amd import task_suite
    Q, V, A, W = cc.rich_states(golden, [cc.FREE_STATE, cc.FREE_STATE])
    Q[:, 0], V[:, 0], A[:, 0], W[:, 0] = np.concatenate([np.zeros(6), KAT_PROPS]), 0.0, 0.0, 0.0
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=3, n_envs=2, prefetch_resets=False)
    for t, a in ((env.qpos, Q), (env.qvel, V), (env.ctrl, A), (env.warm, W)):
        t.copy_(torch.as_tensor(a, dtype=torch.float32, device=env.device))
    pairs = [("object", "table"), ("container", "table")] + list(cc.PAIR_SPECS)
    touch, rep = env.touch(pairs, forces=True), env.contacts(forces=True)
    assert touch.count.shape == (2, len(pairs)) and touch.force.shape == (2, len(pairs), 3) and touch.touching.dtype == torch.bool
    # free space
    assert int(rep.count[1]) == 0 and not bool(touch.touching[1].any()) and bool(torch.isposinf(touch.dist[1]).all())
    assert bool((touch.normal_force[1] == 0).all()) and bool((touch.force[1] == 0).all())
    assert bool((rep.geom[1] == -1).all()) and bool(torch.isposinf(rep.dist[1]).all())
    # at rest
    k = int(rep.count[0])
    raw = {f: getattr(rep, f).cpu().numpy().reshape((2, native.MAXCON, -1) if f in ("pos", "frame", "force") else getattr(rep, f).shape) for f in rep._fields}
    o = Oracle(blobs["f64"])
    o.set_state(Q[:, 0], V[:, 0], W[:, 0]); o.set_ctrl(A[:, 0])
    o.inject_contacts(cc.as_list(raw, 0)); o.forward()
    f_ref = cr.oracle_contact_forces(o)
    g = cc.groups(blobs)
    masks = [(g[a].mask(), g[b].mask()) for a, b in pairs[:2]]
    _, _, normal_ref, net_ref, _ = cr.reduce_pairs(masks, raw["geom"][0, :k], raw["dist"][0, :k], [cr.make_frame(r[:3]) for r in raw["frame"][0, :k]], f_ref)
    scale = f_ref[:, 0].max()
    err_n = np.abs(touch.normal_force[0, :2].cpu().numpy() - normal_ref).max() / scale
    err_f = np.abs(touch.force[0, :2].cpu().numpy() - net_ref).max() / scale
    print(f"resting props: {k} contacts, object | table normal force {float(touch.normal_force[0, 0]):.5f} N (oracle {normal_ref[0]:.5f}), error {err_n:.3e}, net force error {err_f:.3e}")
    assert bool(touch.touching[0, 0]) and bool(touch.touching[0, 1]) and k >= int(touch.count[0, :2].sum())
    assert err_n <= cc.bound4(FORCE_MEASURED["pair"]) and err_f <= cc.bound4(FORCE_MEASURED["pair"])
    assert net_ref[0, 2] > 0 and abs(float(touch.force[0, 0, 2]) - float(touch.normal_force[0, 0])) <= 1e-3 * float(touch.normal_force[0, 0])      # the table pushes the object up


def test_touch_reduction_swap_and_env_index(blobs, golden, newton):
    rep, masks, sim = newton["rep"], newton["masks"], newton["sim"]
    seen = cc.check_touch(rep, masks)
    assert seen.tolist() == [True, True, False, False, True, True, True], seen
    swapped = cc.raw_contacts(sim, forces=True, pairs=[(b, a) for a, b in masks], want=cc.PAIR_GEOMETRY + cc.PAIR_FORCES)
    cc.check_swap(rep, swapped, masks)
    # env_index: a permutation with repeats and two entries outside the batch, 70 entries - more than one launch row of 64
    rs = np.random.RandomState(4)
    idx = np.concatenate([rs.permutation(24), rs.randint(0, 24, size=46)]).astype(np.int32)
    idx[[5, 66]] = [24, -1]
    inside = [i for i in range(70) if i not in (5, 66)]
    picked = cc.raw_contacts(sim, n=70, env_index=idx, forces=True, pairs=masks)
    cc.check_outside(picked, (5, 66), len(masks))
    cc.check_rows_equal(picked, inside, rep, idx[inside])
    # the 3-env batch of the emulated test: entries 1 and 2 of [2, 3, -1, 0] lie outside it; n = 1 alone
    small = cc.load(ArraySim(blobs["f32"], 3, backend="gpu"), *cc.rich_states(golden, cc.EMU_STATES[:3]))
    four = cc.raw_contacts(small, n=4, env_index=[2, 3, -1, 0], forces=True, pairs=masks)
    cc.check_outside(four, (1, 2), len(masks))
    cc.check_rows_equal(four, (0, 3), rep, (cc.EMU_STATES[2], cc.EMU_STATES[0]))
    alone = cc.raw_contacts(small, n=1, env_index=[1], forces=True, pairs=masks)
    cc.check_rows_equal(alone, (0,), rep, (cc.EMU_STATES[1],))


def test_batched_environment_returns_the_raw_calls_tensors(blobs, golden, newton):
    import torch
    from so101_sim_amd import contacts as ct, task_suite
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=3, n_envs=24, prefetch_resets=False)
    for t, a in zip((env.qpos, env.qvel, env.ctrl, env.warm), cc.rich_states(golden)):
        t.copy_(torch.as_tensor(a, dtype=torch.float32, device=env.device))
    raw = newton["rep"]
    touch = env.touch(cc.PAIR_SPECS, forces=True)
    assert isinstance(touch, ct.TouchReport) and touch.count.device == env.qpos.device
    for mine, f in ((touch.count, "pair_count"), (touch.dist, "pair_dist"), (touch.normal_force, "pair_normal"), (touch.force, "pair_force")):
        assert cc.same_bits(mine.cpu().numpy(), raw[f]), f
    assert torch.equal(touch.touching, touch.count > 0)
    quiet = env.touch(cc.PAIR_SPECS[:2], env_ids=[23, 0])
    assert quiet.normal_force is None and quiet.force is None
    assert cc.same_bits(quiet.count.cpu().numpy(), raw["pair_count"][[23, 0], :2]) and cc.same_bits(quiet.dist.cpu().numpy(), raw["pair_dist"][[23, 0], :2])
    rep = env.contacts(forces=True)
    assert isinstance(rep, ct.ContactReport) and rep.frame.shape == (24, native.MAXCON, 3, 3) and rep.geom.dtype == torch.int32
    for f in ("count", "flags", "geom", "dist", "pos", "frame", "force"):
        assert cc.same_bits(getattr(rep, f).cpu().numpy().reshape(raw[f].shape), raw[f]), f
    part = env.contacts(env_ids=torch.tensor([7, 7, 2]))
    assert part.force is None and cc.same_bits(part.pos.cpu().numpy(), raw["pos"][[7, 7, 2]])
    assert env.geom_group("gripper") is env.geom_group(env.geom_group("gripper")) and env.geom_group([3, 4]).geoms == (3, 4)
    with pytest.raises(ValueError, match="unknown geom group"):
        env.touch([("gripper", "no_such_thing")])
    with pytest.raises(ValueError, match="pairs"):
        env.touch([])
    with pytest.raises(ValueError):
        env.contacts(env_ids=[24])
    with pytest.raises(AttributeError):
        env.physics.data.ncon                      # a batch has no single contact list


def test_single_environment_physics_data_contact(blobs):
    """the reference's own loop (so100_hand_over.py _touching) over physics.data.contact, unchanged"""
    from so101_sim_amd import task_suite
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=5)
    env.reset()
    rs = np.random.RandomState(0)
    for _ in range(3):
        env.step(rs.uniform(-0.3, 0.3, size=6))
    physics = env.physics
    count = int(env.contacts().count[0])
    assert physics.data.ncon == len(physics.data.contact) == count and count > 0          # the props lie on something
    geom_names = blobs["meta"]["geom_names"]
    object_geoms = {i for i, n in enumerate(geom_names) if n.startswith("object/")}
    table_geoms = {i for i, n in enumerate(geom_names) if n.startswith("table_")}

    def _touching(geoms_a, geoms_b):
        for contact in physics.data.contact:
            if (contact.geom1 in geoms_a and contact.geom2 in geoms_b) or (contact.geom1 in geoms_b and contact.geom2 in geoms_a):
                return True
        return False

    container_geoms = {i for i, n in enumerate(geom_names) if n.startswith("container/")}
    touch = env.touch([("object", "table"), ("container", "table"), ("object", "Moving_Jaw"), ("props", "world")])
    got = [bool(x) for x in touch.touching[0]]
    want = [_touching(object_geoms, table_geoms), _touching(container_geoms, table_geoms), _touching(object_geoms, set(env.geom_group("Moving_Jaw").geoms)),
            _touching(object_geoms | container_geoms, {geom_names.index("floor")})]
    print(f"single env after 3 steps: {count} contacts, touching {got}")
    assert got == want
    c = physics.data.contact[0]
    assert c.pos.dtype == np.float64 and c.pos.shape == (3,) and c.frame.shape == (9,) and c.frame.dtype == np.float64 and isinstance(c.dist, float)
    assert np.abs(c.frame.reshape(3, 3) @ c.frame.reshape(3, 3).T - np.eye(3)).max() <= 1e-6 and c.dist < 1e-3
