#!/usr/bin/env python3
"""What recording a sampler's trajectory costs, and that calls without a trace cost what they did (one GPU):

    python tools/bench_trajectory.py ab   [--reps 3] [--out profiles/trajectory_ab.jsonl]
    python tools/bench_trajectory.py cost [--out profiles/trajectory_cost.jsonl]

`ab`: every library under beso_amd/lib/variants/ (tools/variants.py build parent=@<rev>) and the tree's own, alternating,
each run in a process of its own (BESO_HIP_LIB): BASELINE configs 1 / 4 / 5 as tools/bench_configs.py runs them and the
headline forward (kitchen, B = 4096).  The spread of a library over its runs is the margin its neighbour is read against.
`cost`: kitchen B = 1000 DDIM-10 (the visualize_ode default for one observation) without a trace, with trace=('x',), with
both outputs, and the same trajectory obtained as ten calls on two-entry schedules.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
VDIR = os.path.join(ROOT, "beso_amd", "lib", "variants")


def _timed(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _setup(shape, B, lam=None, smax=1.0):
    import torch
    from bench import build_model
    from beso_amd import synthetic as O
    from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel
    cfg = O.SHAPES[shape]
    model = build_model(cfg, O.make_weights(cfg, seed=0, std=0.02), "bf16", "cuda:0")
    s, g, a = (torch.from_numpy(v).to("cuda:0") for v in O.make_inputs(cfg, B, seed=1))
    x_t = torch.randn_like(a) * smax
    return cfg, model, (model if lam is None else ClassifierFreeSampleModel(model, lam)), s, g, a, x_t


def one():
    """One library (the process's): ms per call of the four workloads."""
    import torch
    res = {}
    with torch.no_grad():
        cfg, model, call, s, g, a, x_t = _setup("kitchen", 4096)
        sig = torch.full((4096,), 0.3, device="cuda:0")
        rt, packed = model.inner_model.runtime(cfg.sigma_data), model.inner_model.packed_weights()
        res["forward_B4096_ms"] = _timed(lambda: rt.denoise(packed, s, a, g, sig, precondition=True), 300, warm=300)
    # BASELINE configs 1 / 4 / 5 as tools/bench_configs.py defines and times them (one definition of the workloads)
    import contextlib
    import io
    from bench_configs import run
    from beso_amd import synthetic as O
    with contextlib.redirect_stdout(io.StringIO()):
        r1 = run("1", O.SHAPES["kitchen"], 64, "ddim", 10, 0.005, 1.0, reps=50)
        r4 = run("4", O.SHAPES["block_push"], 2048, "heun", 50, 0.05, 1.0, lam=2.0, reps=4)
        r5 = run("5", O.SHAPES["long_horizon"], 256, "euler", 100, 0.005, 1.0, reps=3)
    res.update(config1_ms=r1["seconds_per_call"] * 1e3, config4_ms=r4["seconds_per_call"] * 1e3, config5_ms=r5["seconds_per_call"] * 1e3)
    print(json.dumps(res), flush=True)


def ab(reps, out):
    libs = {"tree": None}
    if os.path.isdir(VDIR):
        libs.update({f[len("libbeso_hip_"):-3]: os.path.join(VDIR, f) for f in sorted(os.listdir(VDIR)) if f.endswith(".so")})
    rows = []
    for rep in range(reps):
        for name, path in libs.items():
            env = dict(os.environ)
            env.pop("BESO_HIP_LIB", None)
            if path:
                env["BESO_HIP_LIB"] = path
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "one"], env=env, capture_output=True, text=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode or not line:
                raise SystemExit(f"{name}: run failed ({r.returncode})\n{r.stderr[-2000:]}")
            rows.append({"library": name, "run": rep, **json.loads(line[-1])})
            print(json.dumps(rows[-1]), flush=True)
    if out:
        with open(out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


def cost(out):
    import torch
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    rows = []
    with torch.no_grad():
        cfg, model, call, s, g, a, x_t = _setup("kitchen", 1000)
        sg = ks.get_sigmas_exponential(10, 0.005, 1.0)

        def chain():
            x = x_t
            for i in range(10):
                x = ks.sample_ddim(model, s, x, g, sg[i:i + 2], disable=True)
            return x
        runs = {"no trace (sample_ddim)": lambda: ks.sample_ddim(model, s, x_t, g, sg, disable=True),
                "trace=('x',)": lambda: ks.sample_trajectory("ddim", model, s, x_t, g, sg, trace=("x",)),
                "trace=('x', 'denoised')": lambda: ks.sample_trajectory("ddim", model, s, x_t, g, sg),
                "ten calls on two-entry schedules": chain}
        for rep in range(3):
            for name, fn in runs.items():
                rows.append({"workload": "kitchen B=1000 DDIM-10", "form": name, "run": rep, "ms_per_call": _timed(fn, 30, warm=5)})
                print(json.dumps(rows[-1]), flush=True)
    if out:
        with open(out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab", "cost", "one"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"ab": lambda: ab(a.reps, a.out), "cost": lambda: cost(a.out), "one": one}[a.mode]()
