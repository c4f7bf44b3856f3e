#!/usr/bin/env python3
"""Generate tests/golden/fit_trace.npz: what four ``GuideTrainer.train_step`` and four ``CriticTrainer.train_step`` calls compute
across the branches of their host side (a per-sample, a shared or no goal; ``use_sigma`` with explicit sigma and generator-drawn
noise; weights with a zero row; ``next_state`` given or read from ``state``; a ``bool`` done; a save after step 2 loaded into a
fresh trainer), recorded from the package's own kernels on the MI355X.  The file pins the bits of the trainers' host layer in
front of those kernels: tests/test_fit_trace.py replays ``run_scenarios()`` and compares every array bit for bit, so regenerate it
only for a change that is MEANT to move a result.  Only the trainers' public surface is used.

    python tests/golden/make_fit_trace.py [other.npz]

Every scenario: B = 3, T = 2, obs 3, act 2, G = 2, one hidden layer of 16 (Mish), ``torch.manual_seed`` in front of the
construction, four steps on fresh seeded data each.  M = B T = 6 rows leave most lanes of the 256-thread loss launch empty and the
tail of the row launch unfilled.  Recorded per scenario: ``losses`` (float32 [4] for the guide, [4, 2] = (L_Q, L_V) for the
critic) and ``steps`` (int64, each optimizer's step count), and as the SHA-256 of their fp32 bytes (uint8 [32]; equal digests,
equal bits) ``losses_sha256``, ``per_row_sha256`` (the last step's ``per_row``, or ``per_row_q | per_row_v | advantage``) and
``params_sha256`` (the concatenated parameters of every network, the critic's target last)."""
import hashlib
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
B, T, OBS, ACT, G, HIDDEN, STEPS, SAVE_AFTER = 3, 2, 3, 2, 2, 16, 4, 2
PATH = os.path.join(HERE, "fit_trace.npz")

# name -> (GuideTrainer loss, use_sigma, goal: 'own' [B, G, obs] / 'shared' [1, G, obs] / None, weights, save and load)
GUIDE = {
    "guide_mse_goal_own": ("mse", False, "own", False, False),
    "guide_bce_sigma_goal_shared": ("bce", True, "shared", False, False),
    "guide_mse_no_goal_weights": ("mse", False, None, True, False),
    "guide_save_load": ("mse", True, "own", True, True),
}
# name -> (next_state given, goal, weights, bool done, save and load)
CRITIC = {
    "critic_next_from_state_goal_own": (False, "own", False, False, False),
    "critic_next_given_goal_shared_weights_bool_done": (True, "shared", True, True, False),
    "critic_no_goal": (False, None, False, False, False),
    "critic_save_load": (True, "own", True, False, True),
}
SCENARIOS = (*GUIDE, *CRITIC)


def _sha256(*tensors):
    flat = torch.cat([t.detach().to(torch.float32).reshape(-1) for t in tensors]).cpu().contiguous().numpy()
    return np.frombuffer(hashlib.sha256(flat.tobytes()).digest(), dtype=np.uint8).copy()


def _steps(optimizer):
    return int(optimizer.export_state()["groups"][0]["step"])


def _data(seed, goal):
    """One step's tensors from a CPU generator: state [B, T + 1, obs], action, goal, next_state, and [B, T] draws."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                  # noqa: E731
    state, action, goals, nxt, values = r(B, T + 1, OBS), r(B, T, ACT), r(B, G, OBS), r(B, T, OBS), r(B, T)
    done = (torch.rand(B, T, generator=g) < 0.3).to(DEV)
    weight = torch.rand(B, T, generator=g).to(DEV)
    weight[1, 0] = 0.0                                                                    # one row without a say
    sigma = torch.rand(B, generator=g).mul(2.0).add(0.05).to(DEV)
    goal = None if goal is None else goals[:1].contiguous() if goal == "shared" else goals
    return state, action, goal, nxt, values, done, weight, sigma


def _network(input_dim):
    from beso_amd.networks.mlps.mlps import MLPNetwork
    return MLPNetwork(input_dim, HIDDEN, 1, 1, activation="Mish", device=DEV)


def _guide_trainer(seed, loss, use_sigma, goal):
    from beso_amd.agents.diffusion_agents.k_diffusion.guide_fit import GuideTrainer
    from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide
    torch.manual_seed(seed)
    guide = MLPGuide(_network(OBS + ACT + (OBS if goal else 0) + int(use_sigma)), use_goal=goal is not None, use_sigma=use_sigma)
    return GuideTrainer(guide, lr=1e-2, weight_decay=0.01, decoupled_weight_decay=True, loss=loss, seed=seed)


def _critic_trainer(seed, goal):
    from beso_amd.agents.diffusion_agents.k_diffusion.critic_fit import CriticTrainer, StateValue
    from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide
    torch.manual_seed(seed)
    gw = OBS if goal else 0
    q = MLPGuide(_network(OBS + ACT + gw), use_goal=goal is not None)
    v = StateValue(_network(OBS + gw), use_goal=goal is not None)
    return CriticTrainer(q, v, lr=1e-2, tau=0.05, weight_decay=0.01, decoupled_weight_decay=True)


def _run_guide(number, loss, use_sigma, goal, weights, save_load):
    tr = _guide_trainer(1000 + number, loss, use_sigma, goal)
    losses = []
    for step in range(STEPS):
        if save_load and step == SAVE_AFTER:            # a fresh guide and trainer, other weights and seed, loaded from the old one's
            saved = tr.state_dict()
            tr = _guide_trainer(9000 + number, loss, use_sigma, goal)
            tr.load_state_dict(saved)
        state, action, g, _, target, _, weight, sigma = _data(100 * number + step, goal)
        target = torch.sigmoid(target) if loss == "bce" else target
        losses.append(tr.train_step(state, action, g, target, weight=weight if weights else None,
                                    sigma=sigma if use_sigma else None))
    torch.cuda.synchronize()
    losses = torch.stack(losses)
    return {"losses": losses.cpu().numpy().copy(), "steps": np.asarray([_steps(tr.optimizer)], dtype=np.int64),
            "losses_sha256": _sha256(losses), "per_row_sha256": _sha256(tr.per_row), "params_sha256": _sha256(*tr.params)}


def _run_critic(number, given_next, goal, weights, bool_done, save_load):
    tr = _critic_trainer(2000 + number, goal)
    losses = []
    for step in range(STEPS):
        if save_load and step == SAVE_AFTER:
            saved = tr.state_dict()
            tr = _critic_trainer(9000 + number, goal)
            tr.load_state_dict(saved)
        state, action, g, nxt, reward, done, weight, _ = _data(100 * number + step, goal)
        losses.append(torch.stack(tr.train_step(state, action, g, reward, done if bool_done else done.float(),
                                                next_state=nxt if given_next else None, weight=weight if weights else None)))
    torch.cuda.synchronize()
    losses = torch.stack(losses)
    return {"losses": losses.cpu().numpy().copy(),
            "steps": np.asarray([_steps(tr.q_optimizer), _steps(tr.v_optimizer)], dtype=np.int64),
            "losses_sha256": _sha256(losses), "per_row_sha256": _sha256(tr.per_row_q, tr.per_row_v, tr.advantage),
            "params_sha256": _sha256(*tr.q_params, *tr.v_params, *tr.q_target_params)}


def run_scenarios():
    """{"<scenario>::<array>": numpy array} for every name of ``SCENARIOS``."""
    out = {}
    for number, name in enumerate(SCENARIOS):
        got = _run_guide(number, *GUIDE[name]) if name in GUIDE else _run_critic(number, *CRITIC[name])
        for key, v in got.items():
            out[f"{name}::{key}"] = v
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    out = run_scenarios()
    # members with a fixed date, so that equal arrays give an equal file
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, v in out.items():
            buf = io.BytesIO()
            np.save(buf, np.ascontiguousarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print(f"wrote {os.path.basename(path)}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
    for key, v in out.items():
        if key.endswith(("losses", "steps")):
            print(key, v.tolist())


if __name__ == "__main__":
    main()
