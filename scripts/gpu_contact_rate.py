"""Time of the contact-sensing calls (so101_contacts, so101_tree_contacts) on the MI355X, beside the only way there was before them.

    python scripts/gpu_contact_rate.py [--cases SO100HandOverBanana:4096 HandOverBanana:4096 DiningPlaceBananaInBowl:1024] [--out FILE]

Per case TASK:ENVS - a task of either engine - one child process under `timeout` (the run stops at the first one that fails): a batched
environment of that many envs, reset (placement + settle) and stepped 100 control steps under uniform random actions within action_spec,
generator seed 0 (the headline workload's actions) - so that the timed state is one the benchmark passes through.  Then, on that state,
per call: three warm-up calls, then five windows of twenty calls, each window between device events; the figure is the median window's
time per call, with the fastest and the slowest window beside it.
  touch_4pairs           env.touch() of four pairs without forces - SO100: gripper | object, arm | table, fixed_jaw_pads | object,
                         object | container; ALOHA and Dining: grippers | object, arms | table, object | container, props | table
  touch_4pairs_forces    the same with forces (constraint rows + solve; the general-tree engine: the mass matrix as well)
  contacts_full          env.contacts(forces=True): the whole per-contact report
  debug_forward_to_host  the engine's debug_forward and the copy of its dump (2048 floats per env; the general-tree engine: dims[5], the
                         mass matrix among them) to pinned host memory (a host clock around the call, the copy and its synchronise): what
                         reading a contact list cost before
  control_step           general-tree engine only: env.step_tensor() under the same random actions (ten windows of ten): what a touch
                         query is a share of
Prints one JSON line per case, with the contacts per env of the timed state.  The numbers are recorded in profiles/README.md; nothing
here asserts them.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, WINDOWS, CALLS = 100, 3, 5, 20
PAIRS = (("gripper", "object"), ("arm", "table"), ("fixed_jaw_pads", "object"), ("object", "container"))
TREE_PAIRS = (("grippers", "object"), ("arms", "table"), ("object", "container"), ("props", "table"))


def child(task, n_envs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from so101_sim_amd import native, task_suite
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    env = task_suite.create_task_env(task, time_limit=10.0, random_state=0, n_envs=n_envs)
    tree = isinstance(env.sim, native.TreeSim)
    pairs = TREE_PAIRS if tree else PAIRS
    spec = env.action_spec()
    dev = env.device
    lo, hi = (torch.as_tensor(np.array(x, dtype=np.float32), device=dev) for x in (spec.minimum, spec.maximum))
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    act = lambda: lo + (hi - lo) * torch.rand(n_envs, lo.numel(), device=dev, generator=gen)
    env.reset() if tree else env.reset_all()
    for _ in range(STEPS):
        env.step_tensor(act())
    torch.cuda.synchronize()          # (the background reset prefetch as well: nothing else runs while the calls are timed)

    def windows(fn, host=False, windows=WINDOWS, calls=CALLS):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(windows):
            if host:
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                ms.append((time.perf_counter() - t0) * 1e3 / calls)
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b) / calls)
        ms.sort()
        return dict(ms=round(ms[len(ms) // 2], 4), fastest=round(ms[0], 4), slowest=round(ms[-1], 4))

    rep = env.contacts()
    row = dict(task=task, envs=n_envs, build=env.sim.build, capacity=env.sim.max_contacts) if tree else dict(envs=n_envs)
    row.update(steps_before=STEPS, warmup_calls=WARMUP, windows=WINDOWS, calls_per_window=CALLS,
               contacts_per_env_mean_max=[round(float(rep.count.float().mean()), 2), int(rep.count.max())], flagged_envs=int((rep.flags != 0).sum()))
    row["touch_4pairs"] = windows(lambda: env.touch(pairs))
    row["touch_4pairs_forces"] = windows(lambda: env.touch(pairs, forces=True))
    row["contacts_full"] = windows(lambda: env.contacts(forces=True))
    dump = env.sim.debug_dim if tree else native.DEBUG_DIM
    dbg = torch.empty(n_envs, dump, dtype=torch.float32, device=dev)
    host = torch.empty(n_envs, dump, dtype=torch.float32).pin_memory()
    if tree:
        row["dump_floats_per_env"] = dump

    def old_way():
        env.sim.debug_forward(dbg.data_ptr(), env._stream())
        host.copy_(dbg, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()

    row["debug_forward_to_host"] = windows(old_way, host=True)
    if tree:
        row["control_step"] = windows(lambda: env.step_tensor(act()), windows=10, calls=10)      # (last: it moves the state on)
    print(json.dumps(row), flush=True)
    if tree:
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["SO100HandOverBanana:4096", "HandOverBanana:4096", "DiningPlaceBananaInBowl:1024"])
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
