"""Time of the Cartesian tool calls (so101_tool_pose / so101_tool_ik) on the MI355X.

    python scripts/gpu_tool_rate.py [--envs 4096 32768] [--out FILE]

Per env count one child process under `timeout` (the run stops at the first one that fails): a BatchedEnvironment of that many
SO100HandOverBanana envs (no reset: the calls read joint angles only), the input distribution of the tests' IK cases drawn from
RandomState(1) - q_target = lo + (0.05 + 0.9 u)(hi - lo), the target is the tool pose at q_target (computed by tool_pose itself),
q_init = clamp(q_target + 0.3 (2 u - 1), lo, hi) - with q_init written into the bound qpos.  Each call: two warm-up calls, ten timed ones
between device events.  Prints one JSON line per env count: ms per call of tool_pose without and with the Jacobian and of solve_ik in modes
0, 1 and 2 (default settings: 60 iterations at most, 1e-4 m, 1e-3 rad), the share of converged solves and their iteration counts.
The control step of the same number of envs is what `python bench.py --gpus 1 --envs N` reports.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, TIMED = 2, 10


def child(n_envs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from so101_sim_amd import task_suite
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=0, n_envs=n_envs, prefetch_resets=False)
    cfg = env.sim.ik_config()
    lo, hi = np.array(cfg.q_lo[:], dtype=np.float64), np.array(cfg.q_hi[:], dtype=np.float64)
    u = np.random.RandomState(1).uniform(size=(n_envs, 2, 6))
    q_target = lo + (0.05 + 0.9 * u[:, 0]) * (hi - lo)
    q_init = np.clip(q_target + 0.3 * (2.0 * u[:, 1] - 1.0), lo, hi)
    target_pos, target_mat = env.tool_pose(q=q_target)
    env.qpos[:6].copy_(torch.as_tensor(q_init.T, dtype=torch.float32, device=env.device))
    env.qpos[9].fill_(1.0); env.qpos[16].fill_(1.0)

    def timed(fn):
        for _ in range(WARMUP):
            out = fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(TIMED):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / TIMED, out

    row = dict(envs=n_envs, warmup_calls=WARMUP, timed_calls=TIMED)
    row["tool_pose_ms"], _ = timed(lambda: env.tool_pose())
    row["tool_pose_jacobian_ms"], _ = timed(lambda: env.tool_pose(jacobian=True))
    for mode in (0, 1, 2):
        ms, (q, conv, res, iters) = timed(lambda: env.solve_ik(target_pos, target_mat, mode=mode))
        row[f"tool_ik_mode{mode}_ms"] = ms
        row[f"tool_ik_mode{mode}_converged"] = float(conv.float().mean())
        row[f"tool_ik_mode{mode}_iters_mean_max"] = [float(iters[conv].float().mean()), int(iters.max())]
        row[f"tool_ik_mode{mode}_residual_max"] = [float(res[conv, 0].max()), float(res[conv, 1].max())]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    lines = []
    for n in args.envs:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", str(n)], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"{n} envs: exit status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode)
        lines += [x for x in r.stdout.splitlines() if x.startswith("{")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
