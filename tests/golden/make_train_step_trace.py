#!/usr/bin/env python3
"""Generate tests/golden/train_step_trace.npz: what four ``BesoAgent.train_step`` calls compute across the step's branch
combinations (fused or eager optimizer, clipping and the non-finite guard, the loss read on the loss stream or behind the whole
step, a trainable encoder with a per-sample or a shared goal), recorded from the package's own kernels on the MI355X.  The file
pins the bits of the host driver in front of those kernels: tests/test_train_step_trace.py replays ``run_scenarios()`` and
compares every array bit for bit, so regenerate it only for a change that is MEANT to move a result.

    python tests/golden/make_train_step_trace.py [other.npz]

Every scenario: ``O.TINY`` in fp32, seeded weights, B = 8, ``torch.manual_seed`` in front of the construction,
``deterministic_training=True``, four steps on one batch with ``update_ema_every_n_steps=2`` (steps 2 and 4 update the EMA
shadow, steps 1 and 3 do not).  Recorded: the four returned losses, ``steps``, the denoiser's parameters and EMA shadow after
step 4, ``last_grad_norm()`` where clipping is on, and the encoder's parameters and shadow where there is one.  The
denoiser's 58 k parameters and their shadow, twelve such arrays, would not fit a fixture of this repository's size; they are
recorded as the SHA-256 of their fp32 bytes (``params_sha256`` / ``ema_sha256``, uint8 [32]) -- equal digests, equal bits."""
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
B, STEPS, RAW, CLIP = 8, 4, 11, 1e-3           # RAW: the observation features in front of an encoder
PATH = os.path.join(HERE, "train_step_trace.npz")


def _scenarios():
    """name -> (BesoAgent keywords, optimizer class, environment, encoder: None / 'per_sample' / 'shared' goal)."""
    clip = dict(max_grad_norm=CLIP)
    sgd = lambda params: torch.optim.SGD(params, lr=1e-2, momentum=0.9)           # noqa: E731  (maybe_fuse leaves it alone)
    return {
        "fused_default": ({}, None, {}, None),
        "fused_clip_guard": (dict(clip, skip_nonfinite_steps=True), None, {}, None),
        "fused_sync_loss": ({}, None, {"BESO_AMD_ASYNC_LOSS": "0"}, None),
        "eager_sgd_clip": (clip, sgd, {}, None),
        "encoder_goal_per_sample": ({}, None, {}, "per_sample"),
        "encoder_goal_shared_clip": (clip, None, {}, "shared"),
    }


def make_agent(extra, optimization, encoder):
    import functools
    from beso_amd.agents.diffusion_agents.beso_agent import BesoAgent
    from beso_amd.agents.input_encoders.obs_encoder import MLPEncoder, NoEncoder
    from beso_amd.networks.mlps.mlps import MLPNetwork
    from beso_amd.networks.scaler.scaler_class import Scaler
    from oracle import beso_oracle as O
    from support import make_denoiser
    cfg = O.TINY
    w = O.make_weights(cfg, seed=2, std=0.05)
    enc = functools.partial(NoEncoder, device=DEV, state_modality="observation", goal_modality="goal_observation")
    if encoder:
        enc = functools.partial(MLPEncoder, device=DEV, state_modality="observation", goal_modality="goal_observation",
                                network=lambda: MLPNetwork(RAW, 48, 1, cfg.obs_dim, device=DEV), encode_goal=True)
    agent = BesoAgent(
        model=lambda: make_denoiser(cfg, w, "fp32", device=DEV), input_encoder=enc,
        optimization=optimization or (lambda params: torch.optim.AdamW(params, lr=1e-3)),
        device=DEV, obs_modalities=["observation"], goal_modalities=["goal_observation"], target_modality="action",
        max_train_steps=10, max_epochs=1, train_method="steps", eval_every_n_steps=5, use_ema=True, goal_conditioned=True,
        pred_last_action_only=False, rho=5.0, num_sampling_steps=3,
        lr_scheduler=lambda optimizer: torch.optim.lr_scheduler.StepLR(optimizer, 1, 0.9),          # changes every step
        sampler_type="ddim", sigma_data=cfg.sigma_data, sigma_min=0.005, sigma_max=1.0, sigma_sample_density_type="loglogistic",
        sigma_sample_density_mean=-0.6, sigma_sample_density_std=1.6, decay=0.999, update_ema_every_n_steps=2,
        window_size=cfg.obs_seq_len, goal_window_size=cfg.goal_seq_len, deterministic_training=True, **extra)
    raw = RAW if encoder else cfg.obs_dim
    rng = np.random.default_rng(0)
    agent.get_scaler(Scaler(rng.standard_normal((64, raw)).astype(np.float32),
                            rng.uniform(-1, 1, (64, cfg.act_dim)).astype(np.float32), True, DEV))
    agent.set_bounds(agent.scaler)
    return cfg, agent, raw


def _sha256(t):
    return np.frombuffer(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest(), dtype=np.uint8).copy()


def _flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params])


def run_scenarios():
    """{"<scenario>::<array>": numpy array}: ``losses`` float64 [4], ``steps`` int64 [1], ``params_sha256`` / ``ema_sha256``;
    ``grad_norm`` [1] with clipping; ``encoder_params`` / ``encoder_ema`` float32 for the two encoder scenarios."""
    from beso_amd.optim import FusedAdam
    out = {}
    for number, (name, (extra, optimization, env, encoder)) in enumerate(_scenarios().items()):
        torch.manual_seed(1000 + number)
        cfg, agent, raw = make_agent(extra, optimization, encoder)
        fused = isinstance(agent.optimizer, FusedAdam)
        assert fused == (optimization is None) and agent.deterministic_training
        rng = np.random.default_rng(200 + number)
        r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)        # noqa: E731
        batch = {"observation": r(B, cfg.obs_seq_len, raw), "action": r(B, cfg.obs_seq_len, cfg.act_dim),
                 "goal_observation": r(1 if encoder == "shared" else B, cfg.goal_seq_len, raw)}
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            losses = []
            for step in range(STEPS):
                losses.append(agent.train_step(batch))
                if step == 0 and agent.max_grad_norm is not None:           # the first step did clip
                    assert float(agent.last_grad_norm()) > CLIP
                    assert not fused or float(agent.optimizer.last_clip_coef()) < 1.0
        finally:
            for k, v in saved.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        torch.cuda.synchronize()
        got = {"losses": np.asarray(losses, dtype=np.float64), "steps": np.asarray([agent.steps], dtype=np.int64),
               "params_sha256": _sha256(_flat(agent.model.parameters())), "ema_sha256": _sha256(agent.ema_helper._flat)}
        if agent.max_grad_norm is not None:
            got["grad_norm"] = agent.last_grad_norm().detach().reshape(1).cpu().numpy().copy()
        if encoder:
            got["encoder_params"] = _flat(agent.input_encoder.get_params()).cpu().numpy().copy()
            got["encoder_ema"] = agent.encoder_ema._flat.detach().cpu().numpy().copy()
        if encoder and agent.max_grad_norm is not None:
            # last_grad_norm() is the denoiser's: the encoder's own clipped step saw another gradient
            assert float(agent.last_grad_norm()) == float(agent.optimizer.last_grad_norm())
            assert float(agent.last_grad_norm()) != float(agent.encoder_optimizer.last_grad_norm())
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
        if key.endswith(("losses", "grad_norm", "steps")):
            print(key, v.tolist())


if __name__ == "__main__":
    main()
