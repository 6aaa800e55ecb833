"""Contact sensing of the general-tree engine on the MI355X (so101_tree_contacts, include/so101.h; AlohaEnvironment.contacts / touch /
geom_group) against the stage dump of so101_tree_debug_forward (bits), the fp64 oracle (geometry, forces) and the fp64 reduction of
tests/contact_ref.py, for both builds of the engine: the 9 hand-over states as one 9-env batch (32-dof build, 64 contacts), the 2 Dining
states as one 2-env batch (64-dof build, 160 contacts, one state with 140).  States, pairs and checks: tests/tree_contact_cases.py.

The force bounds.  Per state the kernel's own contact list goes into the oracle (inject_contacts), which solves it in fp64; two figures
per state, both over max_k f_ref[k][0], the largest normal force of the state:
  per contact    max over contacts and the six entries of |f - f_ref|
  per geom pair  max over the touching geom pairs of |net - net_ref|, net = sum over the pair's contacts of R^T f[0:3] (world frame)
FORCE_MEASURED holds the worst of each per build as measured on the MI355X (profiles/README.md, "Contact sensing, general-tree engine");
the tests assert 4 x that, rounded up to one significant digit - the margin tests/test_contacts_gpu.py gives for fp32 reassociation
across compilers and for a solve that stops at its tolerance.  Hand-over state 3 is 12 x the median of its batch: a finger-on-finger
contact whose friction force is ~1e-5 N beside a normal force of 1.4 N; the kernel and the oracle differ by 4e-5 N there (2e-5 N on the same
contact in the other states, whose largest normal force - the scale - is twice as large), with the solve run to convergence as well."""
import numpy as np
import pytest

from tests import contact_cases as cc, tree_contact_cases as tc
from tests.simharness import TreeArraySim

pytestmark = pytest.mark.gpu
KINDS = dict(handover=dict(build=32, capacity=64, n=9, counts=tc.HANDOVER_COUNTS), dining=dict(build=64, capacity=160, n=2, counts=tc.DINING_COUNTS))
# worst figures on the MI355X: hand-over state 3 (bounds 2e-4, 2e-4), Dining state 1, the 140 contacts (bounds 8e-6, 2e-5)
FORCE_MEASURED = {32: dict(contact=2.706e-5, pair=2.706e-5), 64: dict(contact=1.980e-6, pair=3.508e-6)}


@pytest.fixture(scope="module", params=["handover", "dining"])
def batch(request):
    """ONE pass per build of what the tests below read (the oracle's states and lists are cached by tests/tree_contact_cases.py)"""
    kind = request.param
    b = tc.blobs(kind)
    sim = tc.load(TreeArraySim(b["f32"], KINDS[kind]["n"], backend="gpu"), *tc.states(kind))
    assert (sim.sim.build, sim.sim.max_contacts) == (KINDS[kind]["build"], KINDS[kind]["capacity"])
    out = tc.run_batch(sim, tc.pair_masks(b))
    out.update(kind=kind, blobs=b, **KINDS[kind])
    return out


def test_report_is_bit_identical_to_the_stage_dump_and_changes_no_state(batch):
    tc.check_equals_dump(batch["rep"], batch["geo"], batch["dbg"])
    for x, y in zip(batch["before"], batch["after"]):
        assert tc.same_bits(x, y)                                   # qpos, qvel, ctrl and the warmstart keep their bits across the calls
    for f in tc.PAIR_GEOMETRY:
        assert tc.same_bits(batch["rep"][f], batch["geo"][f]), f
    counts = batch["rep"]["count"]
    print(f"{batch['kind']} (build {batch['build']}): contacts per state {counts.tolist()}, flags {batch['rep']['flags'].tolist()}, rows {[d['nrow'] for d in batch['dbg']]}")
    assert counts.tolist() == batch["counts"]
    if batch["kind"] == "dining":
        assert counts.max() > 128 and counts.max() <= 160           # the second and the third lane pass carry contacts
    else:
        assert counts[tc.HANDOVER_FREE] == 0 and np.all(batch["rep"]["geom"][tc.HANDOVER_FREE] == -1)


def test_frames_are_orthonormal_completions_of_their_normal(batch):
    cc.check_frames(batch["rep"])


def test_geometry_matches_the_oracle_on_every_state(batch):
    total = tc.check_geometry(batch["geo"], tc.oracle_lists(batch["kind"]))
    assert total == int(batch["geo"]["count"].sum()) == sum(batch["counts"])
    assert [d["nrow"] for d in batch["dbg"]] == [rows for _, rows in tc.oracle_lists(batch["kind"])]


def test_forces_match_the_oracle_on_the_kernels_list(batch):
    f_ref = tc.oracle_forces(batch["kind"], batch["rep"])
    errs = np.array([tc.force_errors(batch["rep"], e, f_ref[e]) for e in range(batch["n"])])
    for e, err in enumerate(errs):
        print(f"{batch['kind']} state {e}: {int(batch['rep']['count'][e]):3d} contacts, largest normal force {f_ref[e][:, 0].max() if len(f_ref[e]) else 0.0:9.3f} N, "
              f"force error per contact {err[0]:.3e}, per geom pair {err[1]:.3e}")
    worst = errs.max(axis=0)
    print(f"{batch['kind']} (build {batch['build']}): worst per contact {worst[0]:.3e}, per geom pair {worst[1]:.3e}")
    m = FORCE_MEASURED[batch["build"]]
    assert worst[0] <= tc.bound4(m["contact"]) and worst[1] <= tc.bound4(m["pair"]), worst


def test_touch_reduction_and_swap(batch):
    rep, masks, sim = batch["rep"], batch["masks"], batch["sim"]
    seen = tc.check_touch(rep, masks, tc.SUM_BOUND_K[batch["build"]])
    assert seen.tolist() == tc.SEEN[batch["kind"]], seen
    tc.check_quiet(rep, seen)
    swapped = tc.raw_contacts(sim, forces=True, pairs=[(y, x) for x, y in masks], want=tc.PAIR_GEOMETRY + tc.PAIR_FORCES)
    cc.check_swap(rep, swapped, masks)


def test_repeats_chunks_and_outside(batch):
    """a 3-env batch, n = 8 with forces: three launches (entry i works in scratch slice i mod 3), one env named three times, -1 and n_envs"""
    kind, masks = batch["kind"], batch["masks"]
    pick = (0, 6, 8) if kind == "handover" else (0, 1, 1)
    sim = tc.load(TreeArraySim(batch["blobs"]["f32"], 3, backend="gpu"), *tc.states(kind, pick))
    idx = [1, 0, 1, -1, 2, 3, 1, 0]
    rep = tc.raw_contacts(sim, n=8, env_index=idx, forces=True, pairs=masks)
    cc.check_outside(rep, (3, 5), len(masks))
    inside = [i for i in range(8) if i not in (3, 5)]
    cc.check_rows_equal(rep, inside, batch["rep"], [pick[idx[i]] for i in inside])
    plain = tc.raw_contacts(sim, n=8, env_index=idx, forces=False, pairs=masks)
    cc.check_outside(plain, (3, 5), len(masks))
    cc.check_rows_equal(plain, inside, batch["geo"], [pick[idx[i]] for i in inside])
    alone = tc.raw_contacts(sim, n=1, env_index=[1], forces=True, pairs=masks)
    cc.check_rows_equal(alone, (0,), batch["rep"], (pick[1],))
    first = tc.raw_contacts(sim, n=1, forces=True, pairs=masks)
    cc.check_rows_equal(first, (0,), batch["rep"], (pick[0],))


def test_aloha_environment_returns_the_raw_calls_tensors(batch):
    import torch
    from so101_sim_amd import contacts as ct, task_suite
    kind, raw, C, n = batch["kind"], batch["rep"], batch["capacity"], batch["n"]
    env = task_suite.create_task_env("HandOverBanana" if kind == "handover" else "DiningPlaceBananaInBowl", time_limit=10.0, random_state=3, n_envs=n, prefetch_resets=False)
    assert env.sim.max_contacts == C
    Q, V, CT, W = tc.states(kind)
    for t, a in zip((env.qpos, env.qvel, env.ctrl, env.warm), (Q, V, CT, W)):
        t.copy_(torch.as_tensor(a, dtype=torch.float32, device=env.device))
    touch = env.touch(tc.PAIR_SPECS, forces=True)
    assert isinstance(touch, ct.TouchReport) and touch.count.device == env.qpos.device and touch.force.shape == (n, len(tc.PAIR_SPECS), 3)
    for mine, f in ((touch.count, "pair_count"), (touch.dist, "pair_dist"), (touch.normal_force, "pair_normal"), (touch.force, "pair_force")):
        assert tc.same_bits(mine.cpu().numpy(), raw[f]), f
    assert torch.equal(touch.touching, touch.count > 0) and touch.touching.dtype == torch.bool
    ids = [n - 1, 0]
    quiet = env.touch(tc.PAIR_SPECS[:2], env_ids=ids)
    assert quiet.normal_force is None and quiet.force is None
    assert tc.same_bits(quiet.count.cpu().numpy(), raw["pair_count"][ids, :2]) and tc.same_bits(quiet.dist.cpu().numpy(), raw["pair_dist"][ids, :2])
    rep = env.contacts(forces=True)
    assert isinstance(rep, ct.ContactReport) and rep.frame.shape == (n, C, 3, 3) and rep.geom.dtype == torch.int32 and rep.pos.device == env.qpos.device
    for f in ("count", "flags", "geom", "dist", "pos", "frame", "force"):
        assert tc.same_bits(getattr(rep, f).cpu().numpy().reshape(raw[f].shape), raw[f]), f
    part = env.contacts(env_ids=torch.tensor([1, 1, 0]))
    assert part.force is None and tc.same_bits(part.pos.cpu().numpy(), raw["pos"][[1, 1, 0]])
    recs = ct.records(rep, 0)
    assert len(recs) == int(raw["count"][0]) and recs[0].geom1 == int(raw["geom"][0, 0, 0]) and recs[0].frame.shape == (9,)
    assert env.geom_group("grippers") is env.geom_group(env.geom_group("grippers")) and env.geom_group([3, 4]).geoms == (3, 4)
    assert len(env.geom_group("vx300s_8_custom_finger_left").geoms) == 2          # a geom name that occurs once per arm: all matches
    with pytest.raises(ValueError, match="unknown geom group"):
        env.touch([("grippers", "no_such_thing")])
    with pytest.raises(ValueError, match="pairs"):
        env.touch([])
    with pytest.raises(ValueError):
        env.contacts(env_ids=[n])
    env.close()
