"""Time of the contact-sensing calls (so101_contacts) on the MI355X, beside the only way there was before them.

    python scripts/gpu_contact_rate.py [--envs 4096] [--out FILE]

Per env count one child process under `timeout` (the run stops at the first one that fails): a BatchedEnvironment of that many
SO100HandOverBanana envs, reset (the reference's placement + settle) and stepped 100 control steps under the headline workload's
actions - uniform within action_spec, generator seed 0 - so that the timed state is one the benchmark passes through.  Then, on that
state, per call: three warm-up calls, then five windows of twenty calls, each window between device events; the figure is the median
window's time per call, with the fastest and the slowest window beside it.
  touch_4pairs           env.touch() of gripper | object, arm | table, fixed_jaw_pads | object, object | container, without forces
  touch_4pairs_forces    the same with forces (constraint rows + solve)
  contacts_full          env.contacts(forces=True): the whole per-contact report
  debug_forward_to_host  so101_debug_forward and the copy of its 2048-float dump per env to the host (a host clock around the call, the
                         copy and its synchronise): what reading a contact list cost before
Prints one JSON line per env count, with the contacts per env of the timed state.  The numbers are recorded in profiles/README.md;
nothing here asserts them.
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


def child(n_envs):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from so101_sim_amd import native, task_suite
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=0, n_envs=n_envs)
    spec = env.action_spec()
    dev = env.device
    lo, hi = (torch.as_tensor(np.array(x, dtype=np.float32), device=dev) for x in (spec.minimum, spec.maximum))
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    env.reset_all()
    for _ in range(STEPS):
        env.step_tensor(lo + (hi - lo) * torch.rand(n_envs, 6, device=dev, generator=gen))
    torch.cuda.synchronize()          # (the background reset prefetch as well: nothing else runs while the calls are timed)

    def windows(fn, host=False):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(WINDOWS):
            if host:
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn()
                ms.append((time.perf_counter() - t0) * 1e3 / CALLS)
            else:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(CALLS):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b) / CALLS)
        ms.sort()
        return dict(ms=round(ms[len(ms) // 2], 4), fastest=round(ms[0], 4), slowest=round(ms[-1], 4))

    rep = env.contacts()
    row = dict(envs=n_envs, steps_before=STEPS, warmup_calls=WARMUP, windows=WINDOWS, calls_per_window=CALLS,
               contacts_per_env_mean_max=[round(float(rep.count.float().mean()), 2), int(rep.count.max())], flagged_envs=int((rep.flags != 0).sum()))
    row["touch_4pairs"] = windows(lambda: env.touch(PAIRS))
    row["touch_4pairs_forces"] = windows(lambda: env.touch(PAIRS, forces=True))
    row["contacts_full"] = windows(lambda: env.contacts(forces=True))
    dbg = torch.empty(n_envs, native.DEBUG_DIM, dtype=torch.float32, device=dev)
    host = torch.empty(n_envs, native.DEBUG_DIM, dtype=torch.float32).pin_memory()

    def old_way():
        env.sim.debug_forward(dbg.data_ptr(), env._stream())
        host.copy_(dbg, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()

    row["debug_forward_to_host"] = windows(old_way, host=True)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096])
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
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
