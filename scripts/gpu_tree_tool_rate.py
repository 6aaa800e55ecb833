"""Time of the Cartesian tool calls of the general-tree engine (so101_tree_tool_pose / so101_tree_tool_ik) on the MI355X.

    python scripts/gpu_tree_tool_rate.py [--aloha 4096 32768] [--dining 1024] [--out FILE]

Per task and env count one child process under `timeout` (the run stops at the first one that fails): an AlohaEnvironment of that many
HandOverBanana or DiningPlaceBananaInBowl envs, reset once; the tool "left/gripper"; the input distribution of the tests' IK cases drawn from
RandomState(1) within the default limits (ik_limits) - q_target = lo + (0.05 + 0.9 u)(hi - lo), the target is the tool pose at q_target
(computed by tool_pose itself), q_init = clamp(q_target + 0.3 (2 u - 1), lo, hi).  Each call: after a device-wide synchronise (the reset
leaves its prefetch running on a stream of its own) two warm-up calls, then three windows of 100 calls between device events; the figure is
the median window, the spread (largest minus smallest window, per call) is printed beside it.  Prints one JSON line per child: ms per call
of tool_pose without and with the Jacobian (reading the bound qpos) and of solve_ik in modes 0, 1 and 2 from q_init (default settings: 60
iterations at most, 1e-4 m, 1e-3 rad), the share of converged solves and their iteration counts, and - for scale - ms per control step of the same batch (step_tensor with random joint targets around the home pose).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, TIMED, WINDOWS = 2, 100, 3
TASKS = dict(aloha="HandOverBanana", dining="DiningPlaceBananaInBowl")


def child(scene, n_envs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from so101_sim_amd import task_suite
    from so101_sim_amd.model import scenes
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    env = task_suite.create_task_env(TASKS[scene], time_limit=10.0, random_state=0, n_envs=n_envs)
    env.reset()
    tool = "left/gripper"
    lo, hi = env.ik_limits(tool)
    ncol = len(lo)
    u = np.random.RandomState(1).uniform(size=(n_envs, 2, ncol))
    q_target = lo + (0.05 + 0.9 * u[:, 0]) * (hi - lo)
    q_init = torch.as_tensor(np.clip(q_target + 0.3 * (2.0 * u[:, 1] - 1.0), lo, hi), dtype=torch.float32, device=env.device)
    target_pos, target_mat = env.tool_pose(tool, q=q_target)

    def timed(fn, calls=TIMED):
        """-> ([median, spread] ms per call over WINDOWS windows of `calls` calls, the last result)"""
        torch.cuda.synchronize()
        for _ in range(WARMUP):
            out = fn()
        ms = []
        for _ in range(WINDOWS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                out = fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / calls)
        ms.sort()
        return [round(ms[len(ms) // 2], 4), round(ms[-1] - ms[0], 4)], out

    row = dict(task=TASKS[scene], build=env.sim.build, envs=n_envs, tool=tool, columns=ncol, warmup_calls=WARMUP, timed_calls=TIMED, windows=WINDOWS)
    row["tool_pose_ms"], _ = timed(lambda: env.tool_pose(tool))
    row["tool_pose_jacobian_ms"], _ = timed(lambda: env.tool_pose(tool, jacobian=True))
    for mode in (0, 1, 2):
        ms, (q, conv, res, iters) = timed(lambda: env.solve_ik(target_pos, target_mat, tool=tool, mode=mode, q_init=q_init))
        row[f"tool_ik_mode{mode}_ms"] = ms
        row[f"tool_ik_mode{mode}_converged"] = float(conv.float().mean())
        row[f"tool_ik_mode{mode}_iters_mean_max"] = [float(iters[conv].float().mean()), int(iters.max())]
        row[f"tool_ik_mode{mode}_residual_max"] = [float(res[conv, 0].max()), float(res[conv, 1].max())]
    # the control step of the same batch
    home = torch.tensor(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), dtype=torch.float32, device=env.device)
    g = torch.Generator(device=env.device); g.manual_seed(1)
    spec = env.action_spec()
    alo, ahi = torch.tensor(spec.minimum, device=env.device), torch.tensor(spec.maximum, device=env.device)
    steps = 10          # per window: a control step is milliseconds of device work
    acts = [torch.clamp(home + 0.5 * (torch.rand(n_envs, 14, generator=g, device=env.device) - 0.5), alo, ahi) for _ in range(WARMUP + WINDOWS * steps)]
    k = iter(acts)
    row["control_step_ms"], _ = timed(lambda: env.step_tensor(next(k)), calls=steps)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aloha", type=int, nargs="*", default=[4096, 32768])
    ap.add_argument("--dining", type=int, nargs="*", default=[1024])
    ap.add_argument("--out", default="")
    ap.add_argument("--child", nargs=2, default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]))
    lines = []
    for scene, n in [("aloha", n) for n in args.aloha] + [("dining", n) for n in args.dining]:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", scene, str(n)], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"{scene} {n} envs: exit status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode)
        lines += [x for x in r.stdout.splitlines() if x.startswith("{")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
