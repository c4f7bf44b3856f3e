#!/usr/bin/env python3
"""BASELINE config 3 on one GPU's share: kitchen train_step (score-matching loss, backward, AdamW, EMA) at
1024 samples per step, through BesoAgent.train_step: HIP forward + backward (beso_loss_grad) and the fused
Adam(W) + EMA launch; `--autograd` times the tests' torch-autograd comparator of the same step beside it;
`--max-grad-norm X` / `--skip-nonfinite` turn on gradient clipping / the non-finite guard of the fused step;
`--deterministic` times the step with BESO_TRAIN_DETERMINISTIC (BesoAgent(deterministic_training=True));
`--input-grads` makes every step also compute the gradients with respect to state and goal (beso_loss_grad_inputs: one more
launch and two output tensors per step; the agent itself does not use them);
`--encoder IN,HIDDEN,LAYERS[,KIND]` times the step with and without a trainable MLPEncoder (IN raw features -> HIDDEN x LAYERS ->
obs_dim) in front of the denoiser: the agents in ONE process, alternating in rounds of ten steps, median and spread per agent.
KIND: `mlp` (default: MLPNetwork, ReLU), `res` (ResidualMLPNetwork, Mish, no norm) or `resln` (... with LayerNorm); the flag may
be given more than once, one agent per encoder;
`--scaler minmax` times the step with a MinMaxScaler, its one-launch scale_many against the three per-tensor calls, in ONE process
(5 x 100 steps per agent, alternating; the record is appended to profiles/minmax_scaler_bench.jsonl).
    python tools/bench_train.py [batch] [kitchen|block_push] [--autograd] [--max-grad-norm X] [--skip-nonfinite] [--deterministic]
                                [--input-grads] [--encoder IN,HIDDEN,LAYERS[,KIND]]... [--scaler minmax]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from beso_amd import synthetic as O  # noqa: E402
from _agent import build_agent  # noqa: E402
from beso_amd.networks.scaler.scaler_class import Scaler  # noqa: E402


ENCODER_KINDS = {"mlp": "encoder", "res": "residual_encoder", "resln": "residual_layernorm_encoder"}      # KIND -> the agent's name


def encoder_ab(cfg, model, dev, B, encoders, det, clip, rounds=7, steps=10):
    """The same step without an encoder and with each MLPEncoder of `encoders` [(IN, HIDDEN, LAYERS, KIND)], alternating in one
    process: per agent the median seconds per step over `rounds` rounds of `steps` steps (each round synchronised and timed on
    its own), and the rounds' minimum and maximum."""
    import functools
    from beso_amd.agents.input_encoders.obs_encoder import MLPEncoder
    from beso_amd.networks.mlps.mlps import MLPNetwork, ResidualMLPNetwork
    specs = [("no_encoder", cfg.obs_dim, {})]
    for n_in, hidden, layers, kind in encoders:
        if kind == "mlp":
            net = functools.partial(MLPNetwork, n_in, hidden, layers, cfg.obs_dim, device=dev)
        else:
            net = functools.partial(ResidualMLPNetwork, n_in, hidden, layers, cfg.obs_dim, use_norm=kind == "resln",
                                    norm_style="LayerNorm", device=dev)
        enc = functools.partial(MLPEncoder, device=dev, state_modality="observation", goal_modality="goal_observation", network=net)
        specs.append((ENCODER_KINDS[kind], n_in, {"input_encoder": enc}))
    agents, batches = {}, {}
    for name, raw, extra in specs:
        agent = build_agent(cfg, model, device=dev, deterministic_training=det, **clip, **extra)
        rng = np.random.default_rng(0)
        agent.get_scaler(Scaler(rng.standard_normal((256, raw)).astype(np.float32),
                                rng.standard_normal((256, cfg.act_dim)).astype(np.float32), True, dev))
        agent.set_bounds(agent.scaler)
        torch.manual_seed(1234)
        batches[name] = {"observation": torch.randn(B, cfg.obs_seq_len, raw, device=dev),
                         "action": torch.randn(B, cfg.obs_seq_len, cfg.act_dim, device=dev),
                         "goal_observation": torch.randn(B, cfg.goal_seq_len, raw, device=dev)}
        agents[name] = agent
        for _ in range(3):
            agent.train_step(batches[name])
    torch.cuda.synchronize()
    times = {name: [] for name in agents}
    for _ in range(rounds):
        for name, agent in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = agent.train_step(batches[name])
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps)
    shapes = ", ".join(f"{ENCODER_KINDS[k]} {i}->{h}x{n}->{cfg.obs_dim}" for i, h, n, k in encoders)
    out = {"config": f"{B}-sample train_step, MLPEncoder ({shapes}) against NoEncoder", "batch": B,
           "rounds": rounds, "steps_per_round": steps, "deterministic": det, "loss": loss}
    for name, ts in times.items():
        out[name] = {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}
    for name in list(times)[1:]:
        out[name + "_cost_ms"] = out[name]["median_ms"] - out["no_encoder"]["median_ms"]
    print(json.dumps(out))


def minmax_ab(cfg, name, model, dev, B, det, clip, rounds=5, steps=100):
    """--scaler minmax: train_step with the block-push workspace's MinMaxScaler, its scale_many (one beso_scale_rows_mixed launch for
    state, goal and action) against the same scaler with scale_many restated as the three per-tensor calls, alternating in one
    process: per agent the median milliseconds per step over `rounds` rounds of `steps` steps.  Appends the record to
    profiles/minmax_scaler_bench.jsonl."""
    from beso_amd.networks.scaler.scaler_class import MinMaxScaler

    class PerTensor(MinMaxScaler):
        def scale_many(self, items):
            return [self.scale_input(x) if which == "x" else self.scale_output(x) for x, which in items]

    rng = np.random.default_rng(0)
    x_data = rng.standard_normal((256, cfg.obs_dim)).astype(np.float32)
    y_data = rng.standard_normal((256, cfg.act_dim)).astype(np.float32)
    torch.manual_seed(1234)
    batch = {"observation": torch.randn(B, cfg.obs_seq_len, cfg.obs_dim, device=dev),
             "action": torch.randn(B, cfg.obs_seq_len, cfg.act_dim, device=dev),
             "goal_observation": torch.randn(B, cfg.goal_seq_len, cfg.obs_dim, device=dev)}
    agents = {}
    for key, cls in (("scale_many", MinMaxScaler), ("per_tensor", PerTensor)):
        agent = build_agent(cfg, model, device=dev, deterministic_training=det, **clip)
        agent.get_scaler(cls(x_data, y_data, True, dev))
        agent.set_bounds(agent.scaler)
        agents[key] = agent
        for _ in range(5):
            agent.train_step(batch)
    torch.cuda.synchronize()
    times = {key: [] for key in agents}
    for _ in range(rounds):
        for key, agent in agents.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = agent.train_step(batch)
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) / steps)
    out = {"bench": "train_minmax_scaler", "config": name, "precision": "bf16", "batch": B, "rounds": rounds, "steps_per_round": steps,
           "deterministic": det, "loss": loss, "device": torch.cuda.get_device_name(0), "hip": torch.version.hip,
           "torch": torch.__version__}
    for key, ts in times.items():
        out[key + "_ms"] = {"median": round(1e3 * float(np.median(ts)), 4), "min": round(1e3 * min(ts), 4), "max": round(1e3 * max(ts), 4)}
    out["saved_ms"] = round(out["per_tensor_ms"]["median"] - out["scale_many_ms"]["median"], 4)
    line = json.dumps(out)
    print(line)
    path = os.path.join(ROOT, "profiles", "minmax_scaler_bench.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def main():
    scaler_kind = "zscore"
    if "--scaler" in sys.argv:                  # minmax: MinMaxScaler.scale_many against its three per-tensor calls (minmax_ab)
        i = sys.argv.index("--scaler")
        scaler_kind = sys.argv[i + 1]
        if scaler_kind not in ("zscore", "minmax"):
            raise SystemExit(f"--scaler zscore|minmax: got {scaler_kind!r}")
        del sys.argv[i:i + 2]
    if "--per-op-forward" in sys.argv:          # A/B: every layer of the training forward through the per-op kernels
        sys.argv.remove("--per-op-forward")
        from beso_amd import _lib
        from beso_amd.runtime import set_plan
        set_plan(train=_lib.TRAIN_PLAN_PER_OP)
    if "--tail-forward" in sys.argv:            # ... or through the tile kernel whatever the batch size
        sys.argv.remove("--tail-forward")
        from beso_amd import _lib
        from beso_amd.runtime import set_plan
        set_plan(train=_lib.TRAIN_PLAN_TILES)
    clip = {}
    if "--max-grad-norm" in sys.argv:           # clipping inside the optimizer launch (beso_grad_sumsq + beso_adam_step_clipped)
        i = sys.argv.index("--max-grad-norm")
        clip["max_grad_norm"] = float(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    if "--skip-nonfinite" in sys.argv:
        sys.argv.remove("--skip-nonfinite")
        clip["skip_nonfinite_steps"] = True
    det = "--deterministic" in sys.argv       # fixed-order reductions in the step (a second small launch per partial-sum slab)
    if det:
        sys.argv.remove("--deterministic")
    input_grads = "--input-grads" in sys.argv
    if input_grads:                             # the agent's HIP step with the state / goal gradients asked for (and dropped)
        sys.argv.remove("--input-grads")
        # (BesoAgent._hip_loss_backward calls step.loss_backward(state, action, goal, noise, sigma, **keywords); the counter below
        #  is checked after the timed window, so a changed call site cannot turn this into a silent flag-off run)
        from beso_amd.training import HipTrainStep
        plain, taken = HipTrainStep.loss_backward, [0]

        def with_input_grads(self, *a, **k):
            loss, state_grad, goal_grad = plain(self, *a, **dict(k, input_grads=True))
            assert state_grad is not None
            taken[0] += 1
            return loss
        HipTrainStep.loss_backward = with_input_grads
    encoders = []
    while "--encoder" in sys.argv:
        i = sys.argv.index("--encoder")
        parts = sys.argv[i + 1].split(",")
        kind = parts[3] if len(parts) > 3 else "mlp"
        if len(parts) not in (3, 4) or kind not in ENCODER_KINDS:
            raise SystemExit(f"--encoder IN,HIDDEN,LAYERS[,{'|'.join(ENCODER_KINDS)}]: got {sys.argv[i + 1]!r}")
        encoders.append((int(parts[0]), int(parts[1]), int(parts[2]), kind))
        del sys.argv[i:i + 2]
    if "--autograd" in sys.argv:
        sys.argv.remove("--autograd")
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from autograd_reference import install_autograd_training
        install_autograd_training()
    # one process per GPU under torchrun (python -m torch.distributed.run --nproc-per-node N tools/bench_train.py B):
    # every rank trains on its own B samples per step, gradients all-reduced (C1); single process otherwise
    from beso_amd import distributed as bdist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        bdist.init_from_env("nccl")
    dev = f"cuda:{local_rank}"
    torch.cuda.set_device(dev)
    name = sys.argv[2] if len(sys.argv) > 2 else "kitchen"
    cfg = O.SHAPES[name]
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    w = O.make_weights(cfg, seed=0, std=0.02)
    # the shipped dropouts (configs/franka_kitchen_main_config.yaml:56-57, configs/block_push_main_config.yaml:57-58)
    attn_p, resid_p = {"kitchen": (0.3, 0.0), "block_push": (0.05, 0.05)}.get(name, (0.0, 0.0))

    def model():
        m = build_model(cfg, w, "bf16", dev)
        inner = m.inner_model
        inner._pdrops = (0.0, attn_p, resid_p)
        for blk in inner.blocks:
            blk.attn.attn_drop.p = attn_p
            blk.attn.resid_drop.p = resid_p
            for mod in blk.mlp:
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = resid_p
        return m

    if encoders:
        return encoder_ab(cfg, model, dev, B, encoders, det, clip)
    if scaler_kind == "minmax":
        return minmax_ab(cfg, name, model, dev, B, det, clip)
    agent = build_agent(cfg, model, device=dev, deterministic_training=det, **clip)
    rng = np.random.default_rng(0)
    agent.get_scaler(Scaler(rng.standard_normal((256, cfg.obs_dim)).astype(np.float32),
                            rng.standard_normal((256, cfg.act_dim)).astype(np.float32), True, dev))
    agent.set_bounds(agent.scaler)
    if world > 1:
        bdist.broadcast_parameters(agent.model.get_params(), src=0)          # C2: replicas start identical
        agent.ema_helper.load_shadow_params(agent.model.get_params())
    torch.manual_seed(1234 + rank)
    batch = {"observation": torch.randn(B, cfg.obs_seq_len, cfg.obs_dim), "action": torch.randn(B, cfg.obs_seq_len, cfg.act_dim),
             "goal_observation": torch.randn(B, cfg.goal_seq_len, cfg.obs_dim)}
    batch = {k: v.to(dev) for k, v in batch.items()}
    for _ in range(3):
        loss = agent.train_step(batch)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    n = 10
    for _ in range(n):
        loss = agent.train_step(batch)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = (time.perf_counter() - t0) / n
    if world > 1:
        tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
        dt = float(tmax.item())
    if input_grads:
        assert taken[0] == 3 + n, f"--input-grads: {taken[0]} of {3 + n} steps went through HipTrainStep.loss_backward"
    if rank != 0:
        return
    B = B * world                                                              # samples per step of the whole job
    flops = 3.0 * cfg.flops_per_sample() * B
    if clip:                                    # (read after the timed window: the read synchronises)
        clip = dict(clip, grad_norm=float(agent.last_grad_norm()), clip_coef=float(agent.optimizer.last_clip_coef()),
                    skipped_steps=float(agent.skipped_steps()))
    print(json.dumps({**clip, "deterministic": det, "input_grads": input_grads, "config": ("3: kitchen train_step" if name == "kitchen" else name + " train_step"), "n_gpus": world, "batch": B, "attn_pdrop": attn_p, "resid_pdrop": resid_p, "seconds_per_step": dt,
                      "samples_per_s": B / dt, "tflops_fwd_bwd": flops / dt / 1e12, "loss": loss,
                      "path": ("HIP forward/backward (bf16 operands)" if getattr(agent, "_hip_step", None) is not None
                               else "torch autograd fp32 forward/backward") + " + " + type(agent.optimizer).__name__ + " (+EMA)"}))


if __name__ == "__main__":
    main()
