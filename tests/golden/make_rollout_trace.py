#!/usr/bin/env python3
"""Generate tests/golden/rollout_step_trace.npz: what ``VectorRollout.step`` computes across its branch combinations (scaler
tail, sampler, candidates and selection, keyed or explicit noise), recorded from the package's own kernels on the MI355X.  The
file pins the bits of the host path in front of those kernels: tests/test_rollout_trace.py replays ``run_scenarios()`` and
compares every array bit for bit, so regenerate it only for a change that is MEANT to move a result.

    python tests/golden/make_rollout_trace.py

Every scenario: ``O.TINY`` in fp32, tests/test_rollout.py's agent (seeded weights, the EMA shadow equal to them), N = 3
environments, a window of 2, five steps with environment 1 reset in front of step 3 -- lengths 1, 2, the shifted full window, and
1 beside full windows.  Observations, goals, explicit noise and the scalers' data come from seeded numpy generators on the CPU.
Only the rollout's public surface is used: ``agent.vector_rollout``, ``set_goal``, ``reset``, ``seed``, ``step``."""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
N, W, STEPS, RESET_AT = 3, 2, 5, 3
PATH = os.path.join(HERE, "rollout_step_trace.npz")
AFTER = ("index", "scores", "noise_episode", "noise_step")           # of ``last``, where the scenario has them


def _scenarios():
    """name -> (make the scaler from (x, y), step arguments, seed or None, the steps that get an explicit noise)."""
    from beso_amd.networks.scaler.scaler_class import MinMaxScaler, Scaler

    class Declined(MinMaxScaler):                # one overridden method: _scaler_plan declines it, the torch-op tail runs
        def clip_action(self, y):
            return super().clip_action(y)

    def unscaled_tight(x, y):
        sc = MinMaxScaler(x, y, False, DEV)
        sc.y_bounds_tensor = sc.y_bounds_tensor * 0.05           # the clip acts
        return sc

    every = tuple(range(STEPS))
    return {
        "scaler_ddim_explicit": (lambda x, y: Scaler(x, y, True, DEV), dict(new_sampler_type="ddim"), None, every),
        "minmax_ddim_seeded_kde4": (lambda x, y: MinMaxScaler(x, y, True, DEV),
                                    dict(new_sampler_type="ddim", candidates=4, select="kde"), 11, ()),
        "scaler_ancestral_seeded_mean2": (lambda x, y: Scaler(x, y, True, DEV),
                                          dict(new_sampler_type="euler_ancestral", candidates=2, select="mean"), 5, ()),
        "declined_minmax_ddim_explicit": (lambda x, y: Declined(x, y, True, DEV), dict(new_sampler_type="ddim"), None, every),
        "unscaled_minmax_ddim_explicit": (unscaled_tight, dict(new_sampler_type="ddim"), None, every),
        "scaler_ddim_seeded_explicit_at_2": (lambda x, y: Scaler(x, y, True, DEV), dict(new_sampler_type="ddim"), 3, (2,)),
    }


def make_agent():
    from oracle import beso_oracle as O
    from support import build_agent, make_denoiser
    cfg = O.TINY
    w = O.make_weights(cfg, seed=3, std=0.05)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, "fp32"), device=DEV, sampler="ddim")
    agent.ema_helper.load_shadow_params(agent.model.get_params())
    agent.window_size = W
    return cfg, agent


def run_scenarios():
    """{"<scenario>::<array>": numpy array}: ``pred`` [5, N, act] of the five steps; ``lengths``, ``obs_ctx``, ``act_ctx`` and
    ``x0`` (``last["x0"]``) after the last one, and the entries of AFTER that ``last`` then holds."""
    cfg, agent = make_agent()
    out = {}
    for number, (name, (make_scaler, step_args, seed, explicit)) in enumerate(_scenarios().items()):
        rng = np.random.default_rng(100 + number)
        sc = make_scaler((rng.standard_normal((64, cfg.obs_dim)) * 2 + 0.5).astype(np.float32),
                         (rng.standard_normal((64, cfg.act_dim)) * 1.5 - 0.25).astype(np.float32))
        agent.get_scaler(sc)
        agent.set_bounds(sc)
        roll = agent.vector_rollout(N)
        assert roll.window == W
        roll.set_goal(torch.from_numpy(rng.standard_normal((N, cfg.goal_seq_len, cfg.obs_dim)).astype(np.float32)).to(DEV))
        if seed is not None:
            roll.seed(seed)
        preds = []
        for step in range(STEPS):
            if step == RESET_AT:
                roll.reset([1])
            obs = (rng.standard_normal((N, cfg.obs_dim)) * 2 + 0.5).astype(np.float32)
            noise = rng.standard_normal((N, 1, cfg.act_dim)).astype(np.float32)       # drawn every step: one stream per scenario
            noise = torch.from_numpy(noise).to(DEV) if step in explicit else None
            preds.append(roll.step(torch.from_numpy(obs).to(DEV), noise=noise, **step_args))
        got = {"pred": torch.stack(preds), "lengths": roll.lengths, "obs_ctx": roll.obs_ctx, "act_ctx": roll.act_ctx,
               "x0": roll.last["x0"], **{k: roll.last[k] for k in AFTER if k in roll.last}}
        torch.cuda.synchronize()
        for key, v in got.items():
            out[f"{name}::{key}"] = v.detach().cpu().numpy().copy()
    return out


def main():
    out = run_scenarios()
    # members with a fixed date, so that equal arrays give an equal file
    with zipfile.ZipFile(PATH, "w", zipfile.ZIP_DEFLATED) as z:
        for key, v in out.items():
            buf = io.BytesIO()
            np.save(buf, np.ascontiguousarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print(f"wrote {os.path.basename(PATH)}: {os.path.getsize(PATH) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
