#!/usr/bin/env python3
"""Generate tests/golden/tiny_trajectory.npz by RUNNING THE REFERENCE ITSELF (see make_fixtures.py, whose stand-ins and
model construction this script imports): per-step trajectories of the reference's sampler loops on the TINY config.

    python tests/golden/make_trajectory_fixtures.py

Stored per sampler run `<name>`: the schedule, what the loop handed its callback at every step (`::x` [n, B, t, act], the
action at the start of step i; `::denoised` [n, B, t, act]) and the loop's result (`::out`).  euler_ancestral also stores the
draws it made (`::noise`, zero where a step draws nothing).  `ode::*` is the list the reference agent's visualize_ode builds:
sample_ddim called once per step on a two-entry schedule, 2 observations x get_mean 4, 3 steps.
Weights follow oracle.beso_oracle.make_weights(seed, std); only data is written -- no reference source in any form.
"""
import numpy as np
import torch

import make_fixtures as F
from make_fixtures import O, T, build_ref, ref_samp, save

SEED, STD, BATCH = 4, 0.05, 5
SIGMA_MIN, SIGMA_MAX = 0.005, 1.0


def record(fn, *args, **kw):
    xs, dens = [], []

    def callback(info):
        xs.append(info["x" if "x" in info else "action"].clone().numpy())
        dens.append(info["denoised"].clone().numpy())
    out = fn(*args, callback=callback, disable=True, **kw)
    return np.stack(xs), np.stack(dens), out.numpy()


def main():
    cfg = O.TINY
    m = build_ref(cfg, O.make_weights(cfg, seed=SEED, std=STD))
    state, goal, x_t = O.make_inputs(cfg, BATCH, seed=SEED)
    fx = {"seed": SEED, "std": STD, "state": state, "goal": goal, "x_t": x_t}
    args = (m, T(state), T(x_t), T(goal))
    for name, fn, n in (("euler", ref_samp.sample_euler, 5), ("heun", ref_samp.sample_heun, 5),
                        ("dpmpp_2m", ref_samp.sample_dpmpp_2m, 5)):
        sig = ref_samp.get_sigmas_exponential(n, SIGMA_MIN, SIGMA_MAX)
        torch.manual_seed(1234)
        fx[name + "::x"], fx[name + "::denoised"], fx[name + "::out"] = record(fn, *args, sig)
        fx[name + "::sigmas"] = sig.numpy()
    # euler_ancestral: one randn_like per step whose sigma_down > 0; replay the stream to record the draws
    n = 4
    sig = ref_samp.get_sigmas_exponential(n, SIGMA_MIN, SIGMA_MAX)
    torch.manual_seed(4321)
    name = "euler_ancestral"
    fx[name + "::x"], fx[name + "::denoised"], fx[name + "::out"] = record(ref_samp.sample_euler_ancestral, *args, sig)
    torch.manual_seed(4321)
    draws = []
    for i in range(n):
        down, _ = ref_samp.get_ancestral_step(sig[i], sig[i + 1])
        draws.append(torch.randn(x_t.shape).numpy() if down > 0 else np.zeros_like(x_t))
    fx[name + "::noise"], fx[name + "::sigmas"] = np.stack(draws), sig.numpy()
    # the list of the reference agent's visualize_ode: x_T, then sample_ddim on sigmas[i : i + 2] step after step
    n, n_obs, get_mean = 3, 2, 4
    s2, g2, x2 = O.make_inputs(cfg, n_obs * get_mean, seed=SEED + 1)
    s_rpt = torch.repeat_interleave(T(s2[:n_obs]), repeats=get_mean, dim=0)
    g_rpt = torch.repeat_interleave(T(g2[:n_obs]), repeats=get_mean, dim=0)
    sig = ref_samp.get_sigmas_exponential(n, SIGMA_MIN, SIGMA_MAX)
    x = T(x2) * SIGMA_MAX
    actions = [x]
    for i in range(n):
        x = ref_samp.sample_ddim(m, s_rpt, x, g_rpt, sig[i:(i + 2)], disable=True)
        actions.append(x)
    fx.update({"ode::state": s2[:n_obs], "ode::goal": g2[:n_obs], "ode::get_mean": get_mean, "ode::sigmas": sig.numpy(),
               "ode::actions": np.stack([a.numpy() for a in actions])})
    save("tiny_trajectory.npz", **fx)


if __name__ == "__main__":
    assert F.REF
    main()
