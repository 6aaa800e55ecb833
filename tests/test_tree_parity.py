"""General-tree engine (csrc/so101_tree.hpp, so101_tree_* of include/so101.h) on the ALOHA scenes against the fp64 oracle:
the same stages in the same order, fp32 wave-parallel against fp64 serial.  The `emu` tests run the kernel source compiled for
the host (tests/hostemu) on tiny batches; the `gpu` tests are the parity tests proper, through the C ABI on the MI355X.
Tolerances: kinematics 1e-6 m, mass matrix and bias forces 1e-5 relative, accelerations 1e-4 of the largest, identical contact
lists (pairs and counts), 50 substeps of state within 1e-5 (positions) / 1e-4 (velocities)."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from so101_sim_amd.model import scenes
from tests.simharness import TreeArraySim


def _blobs(name):
    return scenes.load_aloha_blob(name, "f64")[0], scenes.load_aloha_blob(name, "f32")[0]


def _bare_states(n, seed=0):
    rng = np.random.RandomState(seed)
    home = np.concatenate([scenes.ALOHA_HOME_QPOS] * 2)
    sq, sv = np.array([1] * 6 + [0.02] * 2 + [1] * 6 + [0.02] * 2), np.array([1] * 6 + [0.05] * 2 + [1] * 6 + [0.05] * 2)
    Q = np.stack([home + 0.1 * rng.normal(size=16) * sq for _ in range(n)], axis=1)
    V = np.stack([rng.normal(size=16) * sv for _ in range(n)], axis=1)
    CT = np.stack([np.concatenate([scenes.ALOHA_HOME_CTRL] * 2) + np.concatenate([0.2 * rng.normal(size=6), [0.01 * rng.rand()]] * 2) for _ in range(n)], axis=1)
    return Q, V, CT


def _scene_states(raw64, n, seed):
    """post-reset states of a hand-over scene (oracle placement + settle), random arm targets"""
    o = Oracle(raw64)
    rng = np.random.RandomState(seed)
    Q, V, W, CT = [], [], [], []
    for e in range(n):
        o.env_config(seed=seed, env_id=e)
        o.env_reset()
        q, v, w = o.get_state()
        a = np.concatenate([scenes.ALOHA_HOME_CTRL] * 2)
        a[:6] += 0.3 * rng.normal(size=6); a[7:13] += 0.3 * rng.normal(size=6)
        a[6], a[13] = rng.uniform(0.002, 0.037, size=2)
        Q.append(q); V.append(v); W.append(w); CT.append(a)
    return [np.array(x).T for x in (Q, V, W, CT)]


def check_forward(name, backend, n, seed=0, mpr=False):
    """Forward dynamics of the general-tree engine against the fp64 oracle, contact by contact.  Default narrowphase (EPA: an exact face
    of the Minkowski difference) - depth 2e-6 + 1e-4 relative, normal 1e-6, position 2e-5 for every contact, except: `loose` (depth or
    normal beyond that; at most 2 % of the contacts, and then within 1e-4 m / cos 0.999) and `witness` (depth and normal tight, the
    witness point elsewhere on a flat facet - not unique there; at most 5 %, inside the patch).  Accelerations: 1e-4 against the
    oracle's own solve when every contact is tight, else 1e-4 against the oracle solving on the KERNEL's contact list - there is no
    looser fallback.  mpr=True (the -DSO101_MPR option): fp32 and fp64 MPR end on neighbouring portals for centimetre-deep hull pairs;
    only the counts are bounded there (<= 20 %) and the solver is compared on the kernel's list."""
    raw64, raw32 = _blobs(name)
    sim = TreeArraySim(raw32, n, backend=backend, mpr=mpr)
    nv = sim.sim.nv
    if name is None:
        Q, V, CT = _bare_states(n, seed); W = np.zeros((nv, n))
    else:
        Q, V, W, CT = _scene_states(raw64, n, seed)
    sim.set_state(Q, V, CT, W)
    dbg = sim.debug_forward()
    o = Oracle(raw64)
    o.set_narrowphase(not mpr)
    with_contacts = loose = witness = total = 0
    for e in range(n):
        o.inject_contacts([])
        o.set_state(Q[:, e], V[:, e], W[:, e]); o.set_ctrl(CT[:, e]); o.forward()
        d = dbg[e]
        qa, qs = o.qacc()
        assert d["flags"] == 0
        xp = np.array([o.body_pose(b)[0] for b in range(sim.sim.nbody)])
        assert np.abs(d["xpos"] - xp).max() < 1e-6
        M = o.M()
        assert np.abs(d["M"] - M).max() <= 1e-5 * np.abs(M).max()
        assert np.abs(d["bias"] - o.bias()).max() <= 1e-5 * max(1.0, np.abs(o.bias()).max())
        assert np.abs(d["qacc_smooth"] - qs).max() <= 1e-4 * max(1.0, np.abs(qs).max())
        oc = o.contacts()
        assert d["ncon"] == len(oc) and d["nrow"] == o.nefc
        assert [(c["geom1"], c["geom2"]) for c in d["contacts"]] == [(c["geom1"], c["geom2"]) for c in oc]
        off_here = 0
        for a, b in zip(d["contacts"], oc):
            face = abs(a["dist"] - b["dist"]) < 2e-6 + 1e-4 * abs(b["dist"]) and a["normal"] @ b["normal"] > 1 - 1e-6
            if not face:
                if mpr:
                    assert abs(a["dist"] - b["dist"]) < 1e-3 and np.abs(a["pos"] - b["pos"]).max() < 1e-3 and a["normal"] @ b["normal"] > 0.9, (a, b)
                else:
                    assert abs(a["dist"] - b["dist"]) < 1e-4 and np.abs(a["pos"] - b["pos"]).max() < 1.5e-2 and a["normal"] @ b["normal"] > 0.999, (a, b)
                loose += 1; off_here += 1
            elif np.abs(a["pos"] - b["pos"]).max() >= 2e-5:
                assert np.abs(a["pos"] - b["pos"]).max() < 1.5e-2, (a, b)
                witness += 1; off_here += 1
        total += len(oc)
        if off_here:
            o.inject_contacts(d["contacts"])
            o.forward()
            qa = o.qacc()[0]
        assert np.abs(d["qacc"] - qa).max() <= 1e-4 * max(1.0, np.abs(qa).max()), (e, off_here, np.abs(d["qacc"] - qa).max(), np.abs(qa).max())
        with_contacts += d["ncon"] > 0
    o.inject_contacts([])
    if mpr:
        assert loose + witness <= 0.2 * max(total, 1) + 1, (loose, witness, total)
    else:
        assert loose <= 0.02 * max(total, 1) + 1 and witness <= 0.05 * max(total, 1) + 1, (loose, witness, total)
    return with_contacts


def check_rollout(name, backend, n, steps, seed=1):
    raw64, raw32 = _blobs(name)
    sim = TreeArraySim(raw32, n, backend=backend)
    Q, V, W, CT = _scene_states(raw64, n, seed)
    sim.set_state(Q, V, CT, W)
    for _ in range(steps):
        sim.physics(10)
    q1, v1, _ = sim.get_state()
    assert np.all(sim.get_diag()[:, 4] == 0)
    o = Oracle(raw64)
    for e in range(n):
        o.set_state(Q[:, e], V[:, e], W[:, e]); o.set_ctrl(CT[:, e])
        for _ in range(steps):
            o.substeps(10, False)
        q, v, _ = o.get_state()
        assert np.abs(q1[:, e] - q).max() < 1e-5, np.abs(q1[:, e] - q).max()
        assert np.abs(v1[:, e] - v).max() < 1e-4 * max(1.0, np.abs(v).max()), np.abs(v1[:, e] - v).max()
        assert np.abs(q[:6] - Q[:6, e]).max() > 0.02            # (the arms really moved)


def test_emulated_forward_bare_arms():
    assert check_forward(None, "emu", 3) >= 1                   # one of the three states has the arms in contact


def test_emulated_forward_hand_over_scene():
    assert check_forward("banana", "emu", 1) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", [None, "banana", "pen"])
def test_forward_against_the_oracle(name):
    # (bare arms at random poses around home: the contacts are link-on-link and link-on-table hull pairs, a few of them centimetres
    # deep - where MPR and EPA differ most.  With exact faces fp32 and fp64 disagreed in depth or normal on 1 of the 164 contacts in
    # round 3 (the MPR option: 22) and in the witness point alone on 4.)
    assert check_forward(name, "gpu", 32) >= (4 if name is None else 32)


@pytest.mark.gpu
def test_forward_against_the_oracle_with_the_mpr_option():
    """The -DSO101_MPR library (narrowphase="mpr" on the ALOHA envs) runs the general-tree engine with the same switch."""
    assert check_forward(None, "gpu", 32, mpr=True) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["banana", "pen"])
def test_rollout_against_the_oracle(name):
    check_rollout(name, "gpu", 16, 5)


# ---------------------------------------------------------------------------------------------- env layer (hand-over tasks)
def check_env(name, backend, n, steps, settle, seed=7, n_substeps=10):
    """so101_tree_step against oracle/aloha_env.py: FIRST after the in-call reset, observations (delay lines included), reward,
    discount and step type step by step, the time limit's LAST, then the auto-reset's FIRST."""
    from oracle.aloha_env import AlohaOracleEnv
    raw64, raw32 = _blobs(name)
    sim = TreeArraySim(raw32, n, backend=backend)
    sim.enable_env(seed=seed, env_id_base=3, last_step=steps, settle_max_substeps=settle, n_substeps=n_substeps)
    obs, r, d, st = sim.step(np.zeros((n, 14)))
    assert np.all(st == 0) and np.all(r == 0) and np.all(d == 1)
    q, v, w = sim.get_state()
    flags = sim.get_diag()[:, 4]
    assert np.all((flags & ~32) == 0)                      # (32: settle budget used up - expected with the short budgets of the CPU runs)
    envs = []
    for e in range(n):
        oe = AlohaOracleEnv(raw64, seed=seed, env_id=3 + e, last_step=steps, settle_max_substeps=settle, n_substeps=n_substeps)
        o0 = oe.reset()
        qo, vo, _ = oe.o.get_state()
        # placement draws are the same counter-RNG values; the settle is `settle` substeps of contact dynamics in fp32 / fp64
        assert np.abs(q[:16, e] - qo[:16]).max() < 1e-6 and np.abs(q[16:, e] - qo[16:]).max() < (1e-4 if settle <= 300 else 2e-3)
        assert np.abs(obs[e] - o0).max() < 1e-5
        assert np.all(obs[e][:14] == obs[e][30:44]) and np.all(obs[e][14:30] == obs[e][44:60])     # delay lines padded with the reset value
        oe.begin(q[:, e], v[:, e], w[:, e], np.concatenate([scenes.ALOHA_HOME_CTRL] * 2))
        envs.append(oe)
    rng = np.random.RandomState(seed)
    first_pos = obs[:, 30:44].copy()
    for k in range(steps):
        a = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (n, 1)) + 0.3 * rng.normal(size=(n, 14))
        a[:, 6], a[:, 13] = rng.uniform(-0.06, 1.5, size=n), rng.uniform(-0.06, 1.5, size=n)
        obs, r, d, st = sim.step(a)
        for e in range(n):
            o1, r1, d1, s1 = envs[e].step(a[e])
            assert np.abs(obs[e] - o1).max() < 2e-4 * max(1.0, np.abs(o1).max()), (k, e, np.abs(obs[e] - o1).max())
            assert (r[e], d[e], st[e]) == (r1, d1, s1)
        if k < 5:
            assert np.abs(obs[:, :14] - first_pos).max() < 1e-6          # joints_pos lags five control steps behind
        np.testing.assert_allclose(obs[:, 60:66], a[:, :6], rtol=1e-6)   # commanded_joints_pos: the joint targets as given ...
        np.testing.assert_allclose(obs[:, 66], a[:, 6], rtol=1e-4, atol=1e-5)   # ... and the gripper back in follower units
    assert np.all(st == 2) and np.all(d == 1)               # time limit: LAST with discount 1
    obs, r, d, st = sim.step(np.zeros((n, 14)))
    assert np.all(st == 0)                                   # the call after LAST resets and reports FIRST
    ep = sim._get(sim.episode)
    assert np.all(ep == 2)


def test_emulated_env_step():
    check_env("banana", "emu", 1, 1, 2, n_substeps=3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["banana", "pen"])
def test_env_against_the_oracle(name):
    check_env(name, "gpu", 16, 8, 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("n_envs", [1, 8])
def test_python_dropin_api_of_the_aloha_hand_over(n_envs):
    """create_task_env('HandOverBanana') as a caller of the reference uses it (run_eval.py:70-124): FIRST without reward, the
    observation keys and shapes of AlohaTask, the action spec, the instruction, the time limit's LAST and the auto-reset."""
    from so101_sim_amd import task_suite
    env = task_suite.create_task_env("HandOverBanana", time_limit=0.1, random_state=3, n_envs=n_envs, physics_state=True)
    assert env.task.get_instruction() == "hand over the banana and put it in the bowl"
    spec = env.action_spec()
    assert spec.shape == (14,) and spec.dtype == np.float32
    ospec = env.observation_spec()
    assert list(ospec.keys()) == ["commanded_joints_pos", "joints_pos", "joints_vel", "physics_state", "undelayed_joints_pos", "undelayed_joints_vel",
                                  "delayed_joints_pos", "delayed_joints_vel", "delayed_physics_state"]
    ts = env.reset()
    assert ts.reward is None and ts.discount is None
    lead = () if n_envs == 1 else (n_envs,)
    get = (lambda v: np.asarray(v)) if n_envs == 1 else (lambda v: v.double().cpu().numpy())
    for k, sp in ospec.items():
        assert get(ts.observation[k]).shape == lead + sp.shape, k
    home = np.concatenate([scenes.ALOHA_HOME_QPOS[:6], [0.0], scenes.ALOHA_HOME_QPOS[:6], [0.0]])
    jp = get(ts.observation["joints_pos"]).reshape(-1, 14)
    assert np.abs(np.delete(jp, [6, 13], axis=1) - np.delete(home, [6, 13])).max() < 1e-6      # arms at HOME_QPOS; the fingers in follower units
    assert np.abs(jp[:, 6] + 0.03975).max() < 1e-3                                              # 0.0082 m on the rail -> follower units (aloha2_task.py:304-314)
    state0 = get(ts.observation["physics_state"]).reshape(-1, 58)
    assert np.abs(state0[:, 18] - 0.0316).max() < 2e-3                                          # the banana rests on the table top
    a = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (n_envs, 1)).astype(np.float32)
    a[:, 6] = a[:, 13] = 1.0
    act = a[0] if n_envs == 1 else a
    types = []
    for k in range(7):
        ts = env.step(act)
        types.append(int(np.asarray(get(ts.step_type)).reshape(-1)[0]) if n_envs > 1 else int(ts.step_type))
        if k == 0:
            np.testing.assert_allclose(get(ts.observation["delayed_physics_state"]).reshape(-1, 58), state0, atol=1e-6)
            assert np.abs(get(ts.observation["commanded_joints_pos"]).reshape(-1, 14)[:, 6] - 1.0).max() < 1e-4
    # time_limit 0.1 s: control step 5 is the first with physics.time() >= 0.1 (fp64 accumulation of fifty 0.002 s: 0.10000000000000007),
    # the call after it resets and reports FIRST, then the new episode runs
    assert scenes.time_limit_last_step(0.1) == 5
    assert types == [1, 1, 1, 1, 2, 0, 1], types
    env.close()


def check_delay_lines(backend, n, steps, jd, pd, last_step, settle=2, n_substeps=10):
    """Observation delays as configure-time parameters (so101_tree_config.joints_delay_steps / physics_delay_steps) and the
    device-side physics_state line (so101_tree_bind_physics_state): joints_pos / joints_vel of control step k are the undelayed
    values of step k - jd, delayed_physics_state the physics_state of step k - pd, both padded with the reset state and refilled
    by the auto-reset inside a step call - replayed on the host, bit for bit."""
    raw64, raw32 = _blobs("banana")
    sim = TreeArraySim(raw32, n, backend=backend)
    sim.enable_env(seed=5, last_step=last_step, settle_max_substeps=settle, n_substeps=n_substeps, joints_delay_steps=jd, physics_delay_steps=pd, physics_state=True)
    rng = np.random.RandomState(1)
    hist_j, hist_p = [[] for _ in range(n)], [[] for _ in range(n)]
    resets = 0
    for k in range(steps):
        a = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (n, 1)) + 0.2 * rng.normal(size=(n, 14))
        obs, r, d, st = sim.step(a)
        q, v, _ = sim.get_state()
        ps, dps = sim._get(sim.physics_state), sim._get(sim.delayed_physics_state)
        np.testing.assert_array_equal(ps, np.concatenate([q, v]).T.astype(np.float32))          # physics_state = qpos | qvel of this step
        for e in range(n):
            if st[e] == 0:                                                                       # FIRST: the lines restart, padded with the reset state
                hist_j[e], hist_p[e] = [], []
                resets += 1
            und = np.concatenate([obs[e, 30:44], obs[e, 44:60]])
            hist_j[e].append(und); hist_p[e].append(ps[e].copy())
            want_j = hist_j[e][max(len(hist_j[e]) - 1 - jd, 0)]
            want_p = hist_p[e][max(len(hist_p[e]) - 1 - pd, 0)]
            np.testing.assert_array_equal(np.concatenate([obs[e, 0:14], obs[e, 14:30]]), want_j, err_msg=f"joints line, step {k} env {e}")
            np.testing.assert_array_equal(dps[e], want_p, err_msg=f"physics-state line, step {k} env {e}")
    assert resets >= 2 * n                                                                      # the first call and at least one auto-reset per env


def test_emulated_delay_lines():
    check_delay_lines("emu", 1, 5, jd=1, pd=2, last_step=2, n_substeps=1)


@pytest.mark.gpu
@pytest.mark.parametrize("jd,pd", [(5, 15), (1, 1), (0, 0), (2, 3)])
def test_observation_delays_are_configure_time_parameters(jd, pd):
    check_delay_lines("gpu", 8, 40, jd=jd, pd=pd, last_step=17, settle=50)


@pytest.mark.gpu
def test_environment_with_delay():
    """aloha2_task_test.py:136-173 through the Python surface: a task built with image_observation_delay_secs = 0.02 (one control
    step at 50 Hz) - after reset() the first step's delayed_physics_state equals the reset's physics_state, the second step's equals
    the first step's physics_state, bit for bit (the camera half of that test needs a renderer and is out of scope)."""
    from so101_sim_amd import aloha
    task = aloha.HandOverTask("banana", control_timestep=0.02, cameras=("overhead_cam",), image_observation_enabled=True, image_observation_delay_secs=0.02)
    assert (task.joints_delay_steps, task.physics_delay_steps) == (5, 1)
    env = aloha.AlohaEnvironment(task, n_envs=1, random_state=np.random.RandomState(seed=123), settle_max_substeps=100)
    ts = env.reset()
    assert "physics_state" in ts.observation
    initial = ts.observation["physics_state"].copy()
    action = np.zeros(env.action_spec().shape)
    ts = env.step(action)
    first = ts.observation["physics_state"].copy()
    np.testing.assert_array_equal(ts.observation["delayed_physics_state"], initial)
    ts1 = env.step(action)
    np.testing.assert_array_equal(ts1.observation["delayed_physics_state"], first)
    assert not np.array_equal(first, initial)
    env.close()
    # no delay at all: the reference then creates no undelayed_* / delayed_* copies (aloha2_task.py:236-251), and joints_pos is the current value
    task0 = aloha.HandOverTask("banana", joints_observation_delay_secs=0.0, image_observation_delay_secs=0.0)
    env0 = aloha.AlohaEnvironment(task0, n_envs=4, random_state=1, settle_max_substeps=100, physics_state=True)
    assert list(env0.observation_spec().keys()) == ["commanded_joints_pos", "joints_pos", "joints_vel", "physics_state"]
    env0.reset()
    a = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (4, 1)).astype(np.float32); a[:, 1] += 0.3
    ts = env0.step(a)
    assert list(ts.observation.keys()) == ["commanded_joints_pos", "joints_pos", "joints_vel", "physics_state"]
    np.testing.assert_array_equal(ts.observation["joints_pos"].cpu().numpy(), env0.obs[:, 30:44].cpu().numpy())
    env0.close()
    with pytest.raises(ValueError):
        aloha.HandOverTask("banana", joints_observation_delay_secs=0.03)          # not a whole number of control steps


@pytest.mark.gpu
def test_aloha_episode_properties_over_a_full_time_limit():
    """512 ALOHA hand-over envs under uniform random actions over the whole action spec for one 10 s episode and the start of the
    next: finite state throughout, every env reports LAST exactly on control step 500 (or earlier with discount 0 after a physics
    error - bounded), FIRST on the call after, observations inside the joint ranges, the delay line five steps behind."""
    import torch
    from so101_sim_amd import task_suite
    n = 512
    env = task_suite.create_task_env("HandOverBanana", time_limit=10.0, random_state=11, n_envs=n)
    spec = env.action_spec()
    lo, hi = torch.tensor(spec.minimum, device=env.device), torch.tensor(spec.maximum, device=env.device)
    g = torch.Generator(device=env.device); g.manual_seed(5)
    env.reset()
    hist, early, flagged = [], 0, 0
    alive = torch.ones(n, dtype=torch.bool, device=env.device)
    for k in range(1, 504):
        a = lo + (hi - lo) * torch.rand(n, 14, generator=g, device=env.device)
        obs, r, d, st = env.step_tensor(a)
        assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(env.qpos).all()) and bool(torch.isfinite(env.qvel).all())
        hist.append(obs[:, 30:44].clone())
        if k > 5:
            lag = hist[-6]
            same_episode = (env.step_count > 5)
            assert float(((obs[:, 0:14] - lag).abs().max(dim=1).values * same_episode).max()) < 1e-6     # joints_pos = undelayed value of five steps ago
        if k < 500:
            ended = (st == 2)
            early += int(ended.sum()); flagged += int((ended & (d == 0)).sum())
            alive &= ~ended
        elif k == 500:
            assert bool((st[alive] == 2).all()) and bool((d[alive] == 1).all())       # the time limit: LAST with discount 1
        elif k == 501:
            assert bool((st[alive] == 0).all())                                         # auto-reset: FIRST
        qlim = float(env.qpos[:6].abs().max())
        assert qlim < 3.3                                                               # arm joints stay inside (soft) limits
    assert early == flagged                       # nothing but a physics error (or a success, which random actions do not reach) ends an episode early
    assert early <= 0.002 * n * 500, early        # physics errors: fewer than 2 per 1000 env-steps
    env.close()


# ---------------------------------------------------------------------------------------------- contact-sequence reward (hand_over.py:286-338)
def _scripted_states(raw64, which, n):
    """start states for the contact-sequence reward: arms at home, the container where a reset left it, the object
    'in_bowl'    dropped from 6 cm above the container's centre region  (state 2 -> reward 1 once it rests there)
    'on_right'   dropped onto the right arm's gripper                     (state 0 -> 1: the right gripper touches the object)"""
    o = Oracle(raw64)
    Q, V = [], []
    for e in range(n):
        o.env_config(seed=21, env_id=e)
        o.env_reset()
        q, v, _ = o.get_state()
        q, v = q.copy(), np.zeros_like(v)
        if which == "in_bowl":
            q[16:19] = q[23:26] + np.array([-0.025 + 0.004 * e, -0.07, 0.09])
            q[19:23] = [1, 0, 0, 0]
        else:
            p, _ = o.body_pose(18)                            # right/gripper_base
            q[16:19] = np.asarray(p) + np.array([0.0, 0.0, 0.08])
            q[19:23] = [np.cos(0.4), 0, 0, np.sin(0.4)]
        Q.append(q); V.append(v)
    return np.array(Q).T, np.array(V).T


MAX_END_GAP = 0          # control steps between the kernel's and the oracle's episode end: the SAME step since hull pairs carry patches (round 5; measured 0 on all eight drops; 3 until round 4)
END_GAPS = []            # ... as measured by the last calls (printed by the GPU test)


def check_contact_reward(backend, which, requires_handover, n, steps, n_substeps=10):
    from oracle.aloha_env import AlohaOracleEnv
    from so101_sim_amd.model import blob as blobfmt
    raw64, raw32 = _blobs("banana")
    m = blobfmt.unpack(raw64)
    cls, bodies, thr = np.asarray(m["task_geom_class"]), (int(m["task_object_body"][0]), int(m["task_container_body"][0])), float(m["task_dist_threshold"][0])
    Q, V = _scripted_states(raw64, which, n)
    home = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2)[:, None], (1, n))
    sim = TreeArraySim(raw32, n, backend=backend)
    sim.enable_env(seed=21, reward_mode=1, reward_requires_handover=int(requires_handover), last_step=10_000, n_substeps=n_substeps)
    sim.set_state(Q, V, home, np.zeros_like(V))
    sim.begin_episode()
    envs = []
    for e in range(n):
        oe = AlohaOracleEnv(raw64, reward_based_on_overlap=False, reward_requires_handover=requires_handover, geom_class=cls, bodies=bodies, dist_threshold=thr,
                            n_substeps=n_substeps)
        oe.begin(Q[:, e], V[:, e], np.zeros(28), home[:, e])
        envs.append(oe)
    a = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (n, 1))
    a[:, 6] = a[:, 13] = -0.06135                            # grippers closed (FOLLOWER_GRIPPER_CLOSE)
    # Step by step (reward, discount, step type) and the state of the sequence must be EQUAL while both episodes run.  The success itself
    # is gated by "linear velocity < 1e-3" and by the object touching the container.  Until round 4 (one contact point per hull pair: a touch that
    # came and went while the object finished settling) fp32 and fp64 passed that gate up to three control steps apart; with the hull pairs'
    # patches the episode ends on the same control step on both sides, with the same reward, discount and step type (MAX_END_GAP).
    k_last, o_last = np.full(n, -1), np.full(n, -1)
    k_out, o_out = [None] * n, [None] * n
    seen_states, rewards = set(), np.zeros(n)
    for k in range(steps):
        obs, r, d, st = sim.step(a)
        fsm = sim.get_diag()[:, 5]
        for e in range(n):
            both = k_last[e] < 0 and o_last[e] < 0
            if o_last[e] < 0:
                o1, r1, d1, s1 = envs[e].step(a[e])
                if s1 == 2:
                    o_last[e], o_out[e] = k, (r1, d1, s1)
            if k_last[e] < 0:
                seen_states.add(int(fsm[e])); rewards[e] += r[e]
                if st[e] == 2:
                    k_last[e], k_out[e] = k, (float(r[e]), float(d[e]), int(st[e]))
            if both and k_last[e] < 0 and o_last[e] < 0:
                assert (r[e], d[e], st[e]) == (r1, d1, s1), (k, e, r[e], r1, st[e], s1)
                assert fsm[e] == envs[e].success_state
        if np.all(k_last >= 0) and np.all(o_last >= 0):
            break
    for e in range(n):
        assert (k_last[e] >= 0) == (o_last[e] >= 0) or steps - 1 - max(k_last[e], o_last[e]) < 3, (e, k_last[e], o_last[e])
        if k_last[e] >= 0 and o_last[e] >= 0:
            assert abs(k_last[e] - o_last[e]) <= MAX_END_GAP and k_out[e] == o_out[e], (e, k_last[e], o_last[e], k_out[e], o_out[e])
    done = k_last >= 0
    END_GAPS.extend(int(abs(k_last[e] - o_last[e])) for e in range(n) if k_last[e] >= 0 and o_last[e] >= 0)
    return seen_states, rewards, done


@pytest.mark.skipif(not __import__("os").environ.get("SO101_SLOW_TESTS"), reason="emulated run of a path the GPU tests cover; set SO101_SLOW_TESTS=1")
def test_emulated_contact_sequence_reward_counts_states():
    seen, rewards, done = check_contact_reward("emu", "on_right", True, 1, 1, n_substeps=3)
    assert seen <= {0, 1} and rewards.sum() == 0


@pytest.mark.gpu
def test_contact_sequence_reward_against_the_oracle():
    # the object dropped into the bowl: the default sequence (starting in its last state) pays once the object rests there
    seen, rewards, done = check_contact_reward("gpu", "in_bowl", False, 8, 120)
    assert seen == {2} and done.sum() >= 6 and np.all(rewards[done] == 1.0), (seen, rewards, done)
    print("contact-sequence reward, episode ends kernel vs oracle (control steps apart):", END_GAPS)
    # the same with reward_requires_handover: no gripper ever touches the object, the sequence stays in state 0 and nothing is paid
    seen, rewards, done = check_contact_reward("gpu", "in_bowl", True, 4, 60)
    assert seen == {0} and rewards.sum() == 0 and not done.any()
    # the object dropped onto the right gripper: 0 -> 1 (and no further: the left gripper never touches it)
    seen, rewards, done = check_contact_reward("gpu", "on_right", True, 4, 30)
    assert seen <= {0, 1} and 1 in seen and rewards.sum() == 0


@pytest.mark.gpu
def test_single_aloha_env_reset_is_seed_compatible_with_the_reference():
    """N = 1: the placements are numpy RandomState draws in dm_control's PropPlacer order (hand_over.py:208-236): object position,
    object yaw, container position (re-drawn while it collides), so an int seed reproduces what the reference would place."""
    from so101_sim_amd import task_suite
    for seed in (0, 7):
        env = task_suite.create_task_env("HandOverBanana", time_limit=1.0, random_state=seed)
        ts = env.reset()
        rs = np.random.RandomState(seed)
        opos = rs.uniform([0.12, -0.1, 0.1], [0.18, 0.1, 0.1])
        yaw = rs.uniform(-0.1 * np.pi - 0.5 * np.pi, 0.1 * np.pi - 0.5 * np.pi)
        cpos = rs.uniform([-0.18, -0.1, 0.1], [-0.12, 0.1, 0.1])            # (the bowl region is clear of everything: first draw accepted)
        P = env.placements
        np.testing.assert_allclose(P["object_position"], opos, rtol=0, atol=0)
        assert P["object_yaw"] == yaw
        np.testing.assert_allclose(P["container_position"], cpos, rtol=0, atol=0)
        st = ts.observation["physics_state"]
        assert np.abs(st[16:18] - opos[:2]).max() < 0.03 and np.abs(st[23:25] - cpos[:2]).max() < 0.01     # settled near where they were dropped
        assert abs(st[18] - 0.0316) < 3e-3 and abs(st[25] - 0.0325) < 3e-3                                   # resting on the table top
        np.testing.assert_allclose(st[:16], np.concatenate([scenes.ALOHA_HOME_QPOS] * 2), atol=1e-6)
        # a second episode continues the same generator
        for _ in range(60):
            ts = env.step(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2))
            if ts.last():
                break
        ts = env.step(np.zeros(14))
        assert ts.first()
        opos2 = rs.uniform([0.12, -0.1, 0.1], [0.18, 0.1, 0.1])
        np.testing.assert_allclose(env.placements["object_position"], opos2, rtol=0, atol=0)
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["banana", "dining"])
def test_reset_prefetch_of_the_tree_engine_is_bit_identical(scene):
    """so101_tree_config.prefetch_resets: the next episode's settled state computed on a low-priority stream beside the stepping kernels
    changes WHEN a reset state is computed, never its value - rollouts across several auto-resets (short time limit, some envs ended early
    by scripted successes are not needed: the time limit alone resets every env three times) are bit-identical with the prefetch off and on,
    and with the prefetch on the later resets are served from the cache (the step calls that reset get short)."""
    import time
    import torch
    raw32 = scenes.load_dining_blob("banana", "f32")[0] if scene == "dining" else _blobs("banana")[1]
    n, steps = (16, 10) if scene == "dining" else (64, 13)
    out = []
    for prefetch in (0, 1):
        sim = TreeArraySim(raw32, n, backend="gpu")
        sim.enable_env(seed=5, last_step=3, settle_max_substeps=300, prefetch_resets=prefetch)
        rng = np.random.RandomState(2)
        trace = []
        for k in range(steps):
            a = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (n, 1)) + 0.2 * rng.normal(size=(n, 14))
            obs, r, d, st = sim.step(a)
            if prefetch:
                torch.cuda.synchronize(); time.sleep(0.05)          # (let the background settle finish: the next reset then finds its entry)
            trace.append(np.concatenate([obs.ravel(), r, d, st.astype(np.float64)] + [x.ravel() for x in sim.get_state()]))
        out.append(trace)
        assert np.all(sim._get(sim.episode) >= 3)
    for k, (a, b) in enumerate(zip(*out)):
        np.testing.assert_array_equal(a, b, err_msg=f"step {k}")


def _launch_chain_identity(scene, backend, n, steps, n_substeps, settle, last_step=3, reward_mode=0):
    """so101_tree_config.pipeline: the control step as a launch chain (narrowphase in a launch of its own, one wavefront per candidate pair of
    the whole batch) against the single kernel - observations, rewards, step types, states and the per-env diagnostics (contacts, rows, solver
    iterations, candidates, flags) of a rollout across auto-resets, bit for bit."""
    raw32 = scenes.load_dining_blob("mug" if reward_mode == 2 else "banana", "f32")[0] if scene == "dining" else _blobs("banana")[1]
    out = []
    for pipeline in (0, 1):
        sim = TreeArraySim(raw32, n, backend=backend)
        sim.enable_env(seed=5, last_step=last_step, settle_max_substeps=settle, pipeline=pipeline, n_substeps=n_substeps, reward_mode=reward_mode)
        rng = np.random.RandomState(2)
        trace = []
        for k in range(steps):
            a = np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (n, 1)) + 0.2 * rng.normal(size=(n, 14))
            obs, r, d, st = sim.step(a)
            trace.append(np.concatenate([obs.ravel(), r, d, st.astype(np.float64)] + [x.ravel() for x in sim.get_state()] + [sim.get_diag().ravel().astype(np.float64)]))
        out.append(trace)
        assert np.all(sim._get(sim.episode) >= 2)
    for k, (a, b) in enumerate(zip(*out)):
        np.testing.assert_array_equal(a, b, err_msg=f"step {k}")


def test_launch_chain_of_the_tree_engine_is_bit_identical_emulated():
    _launch_chain_identity("banana", "emu", n=1, steps=4, n_substeps=2, settle=2, last_step=2)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,reward_mode", [("banana", 0), ("dining", 0), ("banana", 1), ("dining", 2)])
def test_launch_chain_of_the_tree_engine_is_bit_identical(scene, reward_mode):
    """(reward modes 1 and 2 - contact sequence, object touches receptacle - end the chain with one more narrowphase launch on the post-step state
    and k_tree_pipe_finish)"""
    n, steps = (16, 8) if scene == "dining" else (64, 9)
    _launch_chain_identity(scene, "gpu", n=n, steps=steps, n_substeps=10, settle=300, reward_mode=reward_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,n", [("banana", 512), ("dining", 128)])
def test_launch_chain_slices_are_bit_identical(scene, n):
    """From 128 envs on the chain is cut into two env slices, from 512 into four, each on its own stream (counters and work lists per slice):
    the same rollout across auto-resets as the single kernel, bit for bit."""
    _launch_chain_identity(scene, "gpu", n=n, steps=6, n_substeps=10, settle=300)


@pytest.mark.gpu
@pytest.mark.parametrize("n,reward_mode,plan", [(128, 0, (2, 42, 2, 2)), (64, 0, (1, 21, 1, 2)), (128, 1, (2, 46, 2, 2))])
def test_launch_chain_plan_is_counted_as_enqueued(n, reward_mode, plan):
    """so101_tree_last_plan after one pipelined step on the hand-over blob: slices, kernel launches and memsets as the step function counted
    them while it enqueued them - the values of the closed form the library held before it counted (tests/test_step_plan.py has the table);
    a contact reward ends every slice's chain with one more narrowphase launch and k_tree_pipe_finish."""
    sim = TreeArraySim(_blobs("banana")[1], n, backend="gpu")
    assert sim.sim.last_plan() == (0, 0, 0, 0)
    sim.enable_env(seed=5, last_step=3, settle_max_substeps=20, pipeline=1, n_substeps=10, reward_mode=reward_mode)
    sim.step(np.tile(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), (n, 1)))
    assert sim.sim.last_plan() == plan


@pytest.mark.gpu
def test_settled_store_of_the_tree_engine_is_bit_identical():
    """compute_settled(): the settle results of the first episodes of every env, computed ahead of time; the resets that find them copy -
    the rollout across two auto-resets is bit-identical to the one that settles inside the step calls."""
    import torch
    from so101_sim_amd import task_suite
    n = 64
    traces = []
    for store in (False, True):
        env = task_suite.create_task_env("HandOverBanana", time_limit=0.1, random_state=5, n_envs=n, settle_max_substeps=200)
        if store:
            env.compute_settled(3)
        g = torch.Generator(device=env.device); g.manual_seed(2)
        home = torch.tensor(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), dtype=torch.float32, device=env.device)
        env.reset()
        tr = [env.qpos.clone(), env.qvel.clone()]
        for k in range(13):                     # LAST on steps 5 and 11 (time limit 0.1 s), FIRST on 6 and 12: episodes 0, 1, 2
            obs, r, d, st = env.step_tensor(home + 0.3 * (torch.rand(n, 14, generator=g, device=env.device) - 0.5))
            tr += [obs.clone(), st.clone().float(), env.qpos.clone(), env.qvel.clone()]
        assert int(env.episode[0]) == 3
        traces.append(tr)
        env.close()
    for a, b in zip(*traces):
        assert torch.equal(a, b)
