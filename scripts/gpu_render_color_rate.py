"""Rate of the colour cameras (so101_render_color / so101_tree_render_color) on the MI355X, beside the depth / segmentation render of the same
images (so101_render / so101_tree_render) in the same process.  Modelled on scripts/gpu_render_rate.py.

    python scripts/gpu_render_color_rate.py [--workload so100|aloha|dining] [--envs N] [--sizes 64 128] [--out FILE]

Per image size one child process under `timeout` (the run stops at the first one that fails): 4096 SO100HandOverBanana envs, reset, 100
control steps of the headline workload (uniform random actions, bench.py's), then overhead_cam + front_cam of every env, for each of
render_depth (depth + seg), render_color (rgb only) and render_color (rgb + normal): two warm-up calls, ten timed ones between device
events.  Prints one JSON line per size: ms per call and images per second of the three.

--workload aloha: 4096 HandOverBanana envs of the general-tree engine, bench.py's actions of that workload (uniform around the home pose),
overhead_cam + wrist_cam_left; --workload dining: 1024 DiningPlaceBananaInBowl envs, the same cameras.  The default (so100) is the run above.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = ("overhead_cam", "front_cam")
WORKLOADS = {          # task, default envs, cameras
    "so100": ("SO100HandOverBanana", 4096, CAMS),
    "aloha": ("HandOverBanana", 4096, ("overhead_cam", "wrist_cam_left")),
    "dining": ("DiningPlaceBananaInBowl", 1024, ("overhead_cam", "wrist_cam_left")),
}


def child(n_envs, size, workload="so100"):
    sys.path.insert(0, ROOT)
    import torch
    from so101_sim_amd import task_suite
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    task, _, CAMS = WORKLOADS[workload]
    env = task_suite.create_task_env(task, time_limit=10.0, random_state=0, n_envs=n_envs)
    spec = env.action_spec()
    lo, hi = (torch.tensor(a, device=env.device) for a in (spec.minimum, spec.maximum))
    gen = torch.Generator(device=env.device).manual_seed(0)
    if workload == "so100":
        tape = lo + (hi - lo) * torch.rand(100, n_envs, 6, device=env.device, generator=gen)
        env.reset_all()
    else:
        import numpy as np
        from so101_sim_amd.model import scenes
        home = torch.tensor(np.concatenate([scenes.ALOHA_HOME_CTRL] * 2), dtype=torch.float32, device=env.device)
        tape = torch.clamp(home + 0.5 * (torch.rand(100, n_envs, 14, device=env.device, generator=gen) - 0.5), lo, hi)
        env.reset()
        env.render_depth(CAMS, 8, 8)          # (the hull planes are computed and uploaded here, outside everything timed)
    for i in range(100):
        env.step_tensor(tape[i])
    calls = dict(depth_seg=lambda: env.render_depth(CAMS, size, size), rgb=lambda: env.render_color(CAMS, size, size),
                 rgb_normal=lambda: env.render_color(CAMS, size, size, normals=True))
    env.render_color(CAMS, 8, 8)          # (the colour table is built and uploaded here, outside everything timed)
    ms = {}
    for name, call in calls.items():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(2):
            out = call()
        ev[0].record()
        for _ in range(10):
            out = call()
        ev[1].record()
        torch.cuda.synchronize()
        ms[name] = ev[0].elapsed_time(ev[1]) / 10
    rate = lambda t: round(n_envs * len(CAMS) / (t * 1e-3))
    print(json.dumps(dict(workload=workload, envs=n_envs, cameras=list(CAMS), height=size, width=size,
                          **{k + "_ms_per_call": round(v, 3) for k, v in ms.items()}, **{k + "_images_per_s": rate(v) for k, v in ms.items()},
                          color_over_depth=round(ms["rgb"] / ms["depth_seg"], 3), mean_byte=round(float(out.rgb.float().mean()), 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="so100")
    ap.add_argument("--envs", type=int, default=0, help="0: the workload's default (4096; dining 1024)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    args.envs = args.envs or WORKLOADS[args.workload][1]
    if args.child:
        return child(args.envs, args.child, args.workload)
    lines = []
    for size in args.sizes:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--workload", args.workload, "--envs", str(args.envs), "--child", str(size)],
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            print(f"size {size}: exit status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode)
        lines += [x for x in r.stdout.splitlines() if x.startswith("{")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
