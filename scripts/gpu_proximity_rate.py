"""Time of the proximity call (so101_proximity) on the MI355X, beside env.touch with the same pairs on the same state.

    python scripts/gpu_proximity_rate.py [--envs 4096] [--out FILE]

One child process under `timeout`: 4096 SO100HandOverBanana envs, reset (placement + settle) and stepped 100 control steps under uniform
random actions within action_spec, generator seed 0 (the headline workload's actions) - so that the timed state is one the benchmark passes
through.  Then, on that state, per call: three warm-up calls, then five windows of twenty calls, each window between device events; the
figure is the median window's time per call, with the fastest and the slowest window beside it.  Per pair list -
  gripper_object   [("gripper", "object")]
  arm_props        [("arm", "props")]
  three_pairs      [("gripper", "object"), ("object", "container"), ("arm", "table")]
- `proximity` with q=None, `proximity_q` with q given (the envs' own arm angles: the same geometry, the extra read), and `touch`, the
yardstick: kinematics and the whole collision stage per env.  `queries` is the mean number of exact pair queries per (entry, pair) of the
timed state, `found` the share of (entry, pair) with something within max_dist = 0.1 m, `penetrating` the share that touches.
Prints one JSON line.  The numbers are recorded in profiles/README.md; nothing here asserts them.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, WINDOWS, CALLS = 100, 3, 5, 20
LISTS = dict(gripper_object=[("gripper", "object")], arm_props=[("arm", "props")],
             three_pairs=[("gripper", "object"), ("object", "container"), ("arm", "table")])


def child(n_envs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from so101_sim_amd import task_suite
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=0, n_envs=n_envs)
    spec = env.action_spec()
    dev = env.device
    lo, hi = (torch.as_tensor(np.array(x, dtype=np.float32), device=dev) for x in (spec.minimum, spec.maximum))
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    act = lambda: lo + (hi - lo) * torch.rand(n_envs, lo.numel(), device=dev, generator=gen)
    env.reset_all()
    for _ in range(STEPS):
        env.step_tensor(act())
    torch.cuda.synchronize()          # (the background reset prefetch as well: nothing else runs while the calls are timed)

    def windows(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(WINDOWS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / CALLS)
        ms.sort()
        return dict(ms=round(ms[len(ms) // 2], 4), fastest=round(ms[0], 4), slowest=round(ms[-1], 4))

    q = env.qpos[:6].t().contiguous()
    row = dict(envs=n_envs, steps_before=STEPS, warmup_calls=WARMUP, windows=WINDOWS, calls_per_window=CALLS, max_dist=0.1)
    for name, pairs in LISTS.items():
        rep, count = env._proximity(pairs, None, None, 0.1, queries=True)
        r = dict(queries=round(float(count.float().mean()), 3), found=round(float(((rep.flags & 4) == 0).float().mean()), 4),
                 penetrating=round(float(((rep.flags & 1) != 0).float().mean()), 4), capped=int(((rep.flags & 2) != 0).sum()))
        r["proximity"] = windows(lambda: env.proximity(pairs))
        r["proximity_q"] = windows(lambda: env.proximity(pairs, q=q))
        r["touch"] = windows(lambda: env.touch(pairs))
        row[name] = r
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", str(args.envs)], stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        print(f"exit status {r.returncode}", file=sys.stderr)
        sys.exit(r.returncode)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(x for x in r.stdout.splitlines() if x.startswith("{")) + "\n")


if __name__ == "__main__":
    main()
