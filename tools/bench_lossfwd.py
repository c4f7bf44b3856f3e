#!/usr/bin/env python3
"""The held-out denoising loss on the inference path against the training step's forward + backward on the same samples, in
the same process.  Kitchen shape, bf16, EMA image.

    python tools/bench_lossfwd.py [--batches 1024,8192] [--iters 20] [--reps 7] [--out profiles/lossfwd_bench.jsonl]

Per batch size, every repetition times `iters` consecutive calls of each form with device events on the stream, alternating the
forms (the forms then see the same clocks and the same neighbours):
  loss_fwd    the call ``BesoAgent.validation_loss`` makes: ``GCDenoiser.loss`` under ``torch.no_grad()`` in eval mode inside the
              agent's EMA scope -- ``beso_loss_fwd``: prep launch, the forward, two reduction launches
  train_step  ``HipTrainStep.run`` on the same samples with the module in eval mode (no dropout, no goal masking) --
              ``beso_loss_grad``: forward with kept activations, backward, the flat gradient buffer -- what a validation pass
              had to go through before
  forward     the bare network forward (``beso_score_fwd``) on the same samples
event_ms is the time from the first launch to the end of the last kernel divided by `iters` (idle time between launches
included, not a sum of kernel times); the record holds the median over the repetitions and the extremes.  One JSON line per
batch size is appended to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from beso_amd import synthetic as O  # noqa: E402
from _agent import build_agent  # noqa: E402

DEV = "cuda:0"


def timed(fn, iters):
    """event ms per call of `iters` calls of fn()."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lossfwd_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lossfwd.py measures on the GPU; none found")
    cfg = O.SHAPES["kitchen"]
    w = O.make_weights(cfg, seed=0, std=0.02)
    agent = build_agent(cfg, lambda: build_model(cfg, w, "bf16", DEV), device=DEV)
    den = agent._hip_denoiser()
    inner = den.inner_model
    box = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    gen = torch.Generator(DEV).manual_seed(0)
    for B in [int(v) for v in a.batches.split(",")]:
        r = lambda *s: torch.randn(*s, device=DEV, generator=gen)        # noqa: E731
        state, action = r(B, cfg.obs_seq_len, cfg.obs_dim), r(B, cfg.obs_seq_len, cfg.act_dim)
        goal, noise = r(B, cfg.goal_seq_len, cfg.obs_dim), r(B, cfg.obs_seq_len, cfg.act_dim)
        sigma = torch.rand(B, device=DEV, generator=gen) * 0.9 + 0.05
        agent.model.eval()
        step = den.hip_train_step(state, action, goal, noise, sigma)
        if step is None:
            raise SystemExit("the HIP training step does not take these inputs")
        rt = inner.runtime(den.sigma_data)

        def loss_fwd():
            with torch.no_grad(), agent._ema_scope():
                return den.loss(state, action, goal, noise, sigma)

        def train_step():
            return step.run(state, action, goal, noise, sigma)[0]

        def forward():
            with torch.no_grad(), agent._ema_scope():
                return rt.denoise(inner.packed_weights(), state, action, goal, sigma, precondition=False)

        forms = {"loss_fwd": loss_fwd, "train_step": train_step, "forward": forward}
        for fn in forms.values():
            for _ in range(3):
                fn()
        lf, ts = float(loss_fwd()), float(train_step())
        t = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, fn in forms.items():
                t[k].append(timed(fn, a.iters))
        rec = {"bench": "lossfwd", "config": "kitchen", "precision": "bf16", "batch": B, "iters_per_rep": a.iters, "reps": a.reps,
               "loss_fwd_event_ms": stats(t["loss_fwd"]), "train_step_event_ms": stats(t["train_step"]),
               "forward_event_ms": stats(t["forward"]), "loss_fwd_value": round(lf, 6), "train_step_loss_value": round(ts, 6)}
        rec["loss_fwd_over_train_step"] = round(rec["loss_fwd_event_ms"]["median"] / rec["train_step_event_ms"]["median"], 4)
        rec["loss_fwd_over_forward"] = round(rec["loss_fwd_event_ms"]["median"] / rec["forward_event_ms"]["median"], 4)
        rec.update(box)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
