"""Time of the proximity call of the general-tree engine (so101_tree_proximity) on the MI355X, beside env.touch with the same pairs on the
same state.

    python scripts/gpu_tree_proximity_rate.py [--cases HandOverBanana:4096 DiningPlaceBananaInBowl:1024] [--out FILE]

One child process per case under `timeout`, one after the other (a case that fails ends the run): the envs reset (placement + settle) and
stepped 100 control steps under uniform random actions within action_spec, generator seed 0 - so that the timed state is one the
benchmark passes through.  Then, on that state, per call: three warm-up calls, then five windows of twenty calls, each window between
device events; the figure is the median window's time per call, with the fastest and the slowest window beside it.  Per pair list -
  grippers_object  [("grippers", "object")]
  three_pairs      [("grippers", "object"), ("object", "container"), ("arms", "table")]
  arms_props       [("arms", "props")]                  1 824 member pairs in the hand-over blob, 6 464 in Dining
- `proximity` with q=None, `proximity_q` with q given for the left gripper's chain (the envs' own values: the same geometry, the extra read),
and `touch`, the yardstick: kinematics and the whole collision stage per env.  `queries` is the mean number of exact pair queries per
(entry, pair) of the timed state, `found` the share of (entry, pair) with something within max_dist = 0.1 m, `penetrating` the share that
touches, `capped` the number that hit the iteration cap.  Prints one JSON line per case.  The numbers are recorded in profiles/README.md;
nothing here asserts them.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, WINDOWS, CALLS = 100, 3, 5, 20
LISTS = dict(grippers_object=[("grippers", "object")], three_pairs=[("grippers", "object"), ("object", "container"), ("arms", "table")],
             arms_props=[("arms", "props")])
TOOL = "left/gripper"


def child(task, n_envs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from so101_sim_amd import task_suite
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    env = task_suite.create_task_env(task, time_limit=10.0, random_state=0, n_envs=n_envs)
    spec = env.action_spec()
    dev = env.device
    lo, hi = (torch.as_tensor(np.array(x, dtype=np.float32), device=dev) for x in (spec.minimum, spec.maximum))
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    act = lambda: lo + (hi - lo) * torch.rand(n_envs, lo.numel(), device=dev, generator=gen)
    env.reset()
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

    q = env.qpos[env.tool_chain(TOOL)[1]].t().contiguous()
    row = dict(task=task, envs=n_envs, build=env.sim.build, steps_before=STEPS, warmup_calls=WARMUP, windows=WINDOWS, calls_per_window=CALLS, max_dist=0.1)
    for name, pairs in LISTS.items():
        rep, count = env._proximity(pairs, None, None, 0.1, queries=True)
        r = dict(queries=round(float(count.float().mean()), 3), found=round(float(((rep.flags & 4) == 0).float().mean()), 4),
                 penetrating=round(float(((rep.flags & 1) != 0).float().mean()), 4), capped=int(((rep.flags & 2) != 0).sum()))
        r["proximity"] = windows(lambda: env.proximity(pairs))
        r["proximity_q"] = windows(lambda: env.proximity(pairs, q=q, joints=TOOL))
        r["touch"] = windows(lambda: env.touch(pairs))
        row[name] = r
    print(json.dumps(row), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["HandOverBanana:4096", "DiningPlaceBananaInBowl:1024"])
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        task, n = args.child.split(":")
        return child(task, int(n))
    lines = []
    for case in args.cases:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", case], stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"{case}: exit status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode)
        lines += [x for x in r.stdout.splitlines() if x.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
