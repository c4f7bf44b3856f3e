"""``MLPEncoder`` in ``BesoAgent``: training by the HIP step, inference on the EMA encoder, checkpoints, what is refused, and
that a ``NoEncoder`` agent does what it did.  Comparator of the training: a torch-op agent step -- tests/autograd_reference.py
behind a torch copy of the encoder, ``torch.optim.AdamW`` on both parameter sets, reseeded to draw the same noise and sigma."""
import copy
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from beso_amd import _lib
from beso_amd.agents.input_encoders.obs_encoder import MLPEncoder, NoEncoder
from beso_amd.networks.mlps.mlps import MLPNetwork
from beso_amd.networks.scaler.scaler_class import Scaler
from oracle import beso_oracle as O
from support import TRAIN_BOUNDS, bits, build_agent, count_site_launches, grad_errors, make_denoiser

DEV = "cuda:0"
RAW = 11                      # raw observation features in front of the encoder; the denoiser's obs_dim is its output_dim


def encoder_factory(device, net=None, **kw):
    net = net or (lambda: MLPNetwork(RAW, 48, 1, O.TINY.obs_dim, device=device))
    return lambda: MLPEncoder(device=device, state_modality="observation", goal_modality="goal_observation", network=net, **kw)


def make_agent(device, encoder=True, lr=1e-3, net=None, **extra):
    cfg = O.TINY
    w = O.make_weights(cfg, seed=2, std=0.05)
    if encoder:
        extra["input_encoder"] = encoder_factory(device, net)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, "fp32", device=device), device=device, lr=lr, **extra)
    raw = RAW if encoder else cfg.obs_dim
    agent.get_scaler(Scaler(np.random.default_rng(0).standard_normal((64, raw)).astype(np.float32),
                            np.random.default_rng(1).standard_normal((64, cfg.act_dim)).astype(np.float32), True, device))
    agent.set_bounds(agent.scaler)
    return agent


def make_batch(device, B=6, raw=RAW, seed=7):
    cfg = O.TINY
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(device)                               # noqa: E731
    return {"observation": r(B, cfg.obs_seq_len, raw), "action": r(B, cfg.obs_seq_len, cfg.act_dim),
            "goal_observation": r(B, cfg.goal_seq_len, raw)}


class StubNet(nn.Module):
    """Stands in for an MLPNetwork where no kernel runs: the same parameter surface."""

    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(4, 16), nn.Linear(16, 3)])

    def get_params(self):
        return self.layers.parameters()

    def get_device(self, device):
        self.layers.to(device)


# -------------------------------------------------------------------------------------------------
# CPU
# -------------------------------------------------------------------------------------------------
def test_state_dict_keys_shapes_and_parameter_order():
    net = MLPNetwork(11, 48, 1, 7, device="cpu")
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [
        ("layers.0.weight", (48, 11)), ("layers.0.bias", (48,)), ("layers.1.weight", (7, 48)), ("layers.1.bias", (7,))]
    net = MLPNetwork(input_dim=30, hidden_dim=256, num_hidden_layers=3, output_dim=5, dropout=0, activation="Mish",
                     use_spectral_norm=False, device="cpu")
    want = [("layers.0.weight", (256, 30)), ("layers.0.bias", (256,)), ("layers.1.weight", (256, 256)), ("layers.1.bias", (256,)),
            ("layers.2.weight", (256, 256)), ("layers.2.bias", (256,)), ("layers.3.weight", (5, 256)), ("layers.3.bias", (5,))]
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    assert [(k, tuple(v.shape)) for k, v in net.named_parameters()] == want
    assert [tuple(p.shape) for p in net.get_params()] == [s for _, s in want]
    assert (net.network_type, net.input_dim, net.hidden_dim, net.num_hidden_layers, net.output_dim, net.dropout,
            net.spectral_norm) == ("mlp", 30, 256, 3, 5, 0, False)
    assert net.num_param_floats() == sum(int(np.prod(s)) for _, s in want) and net.keep_floats(10) == 10 * (30 + 3 * 256)


def test_encoder_forward_fetches_what_no_encoder_fetches():
    batch = make_batch("cpu")
    enc = encoder_factory("cpu")()
    plain = NoEncoder("cpu", "observation", "goal_observation")
    (s1, g1), (s2, g2) = enc(batch), plain(batch)
    assert torch.equal(s1, s2) and torch.equal(g1, g2)
    assert enc({"observation": batch["observation"]})[1] is None
    with pytest.raises(KeyError):
        enc({})
    assert isinstance(enc, NoEncoder) and enc.encode_goal and len(list(enc.get_params())) == 4
    assert not encoder_factory("cpu", encode_goal=False)().encode_goal


def test_encoder_checkpoint_round_trip(tmp_path):
    """store_model_weights writes encoder_state_dict.pth (EMA) and non_ema_encoder_state_dict.pth; load_pretrained_model reads
    the first into the encoder and re-seeds its EMA; a directory without them raises with an encoder and loads as before
    without one."""
    agent = make_agent("cpu", net=StubNet)
    assert agent.encoder_optimizer is not None and agent.encoder_ema is not None and agent.encoder_lr_scheduler is not None
    with torch.no_grad():
        agent.encoder_ema._flat.add_(0.5)
    agent.store_model_weights(str(tmp_path))
    ema = torch.load(tmp_path / "encoder_state_dict.pth")
    raw = torch.load(tmp_path / "non_ema_encoder_state_dict.pth")
    net = agent.input_encoder.network
    assert list(ema) == list(raw) == list(net.state_dict())
    for k, v in net.state_dict().items():
        assert torch.equal(raw[k], v) and torch.equal(ema[k], v + 0.5)
    other = make_agent("cpu", net=StubNet)
    other.load_pretrained_model(str(tmp_path))
    for k, v in other.input_encoder.network.state_dict().items():
        assert torch.equal(v, ema[k])
    assert torch.equal(other.encoder_ema._flat, torch.cat([ema[k].reshape(-1) for k in ema]))
    plain = make_agent("cpu", encoder=False)
    plain.load_pretrained_model(str(tmp_path))                      # the encoder files are not looked at
    assert plain.encoder_optimizer is None
    os.remove(tmp_path / "encoder_state_dict.pth")
    with pytest.raises(FileNotFoundError, match="encoder"):
        other.load_pretrained_model(str(tmp_path))
    plain.store_model_weights(str(tmp_path))
    assert not os.path.exists(tmp_path / "encoder_state_dict.pth")


def test_refused_combinations_raise_by_name(tmp_path):
    agent = make_agent("cpu", net=StubNet)
    with pytest.raises(NotImplementedError, match="vector_rollout"):
        agent.vector_rollout(2)
    with pytest.raises(NotImplementedError, match="store_training_state"):
        agent.store_training_state(str(tmp_path))
    with pytest.raises(NotImplementedError, match="load_training_state"):
        agent.load_training_state(str(tmp_path))


# -------------------------------------------------------------------------------------------------
# GPU
# -------------------------------------------------------------------------------------------------
class TorchEncoder(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.layers = copy.deepcopy(net.layers)

    def forward(self, x):
        for i, l in enumerate(self.layers):
            x = l(x)
            if i < len(self.layers) - 1:
                x = torch.relu(x)
        return x


@pytest.mark.gpu
def test_agent_trains_the_encoder_like_the_torch_op_step(monkeypatch, caplog):
    from autograd_reference import loss_autograd
    from beso_amd.optim import FusedAdam
    cfg, lr, B = O.TINY, 1e-3, 6
    agent = make_agent(DEV, lr=lr)
    assert isinstance(agent.optimizer, FusedAdam) and isinstance(agent.encoder_optimizer, FusedAdam)
    assert agent.encoder_optimizer is not agent.optimizer and len(agent.encoder_optimizer.param_groups) == 1
    enc = agent.input_encoder
    ref_model = make_denoiser(cfg, O.make_weights(cfg, seed=2, std=0.05), "fp32", train=True)
    ref_enc = TorchEncoder(enc.network)
    opts = [torch.optim.AdamW(ref_model.parameters(), lr=lr), torch.optim.AdamW(ref_enc.parameters(), lr=lr)]
    shadow = [p.detach().clone() for p in ref_enc.parameters()]
    batch = make_batch(DEV, B)
    init = [p.detach().clone() for p in enc.get_params()]
    monkeypatch.setenv("BESO_AMD_TRAIN_GRAPH", "1")                 # ignored with an encoder, with a log line
    losses, ref_losses = [], []
    with caplog.at_level(logging.INFO):
        for i in range(3):
            torch.manual_seed(100 + i)
            losses.append(agent.train_step(batch))
            torch.manual_seed(100 + i)
            state, action, goal = agent.process_batch(batch, predict=False)
            noise = torch.randn_like(action)
            sigma = agent.make_sample_density()(shape=(B,), device=DEV)
            loss = loss_autograd(ref_model, ref_enc(state), action, ref_enc(goal), noise, sigma)
            for o in opts:
                o.zero_grad()
            loss.backward()
            for o in opts:
                o.step()
            decay = min(0.999, (2 + i) / (11 + i))                   # ema.py:45-48 with num_updates = i + 1
            with torch.no_grad():
                for s, p in zip(shadow, ref_enc.parameters()):
                    s.sub_((1.0 - decay) * (s - p))
            ref_losses.append(loss.item())
    assert "BESO_AMD_TRAIN_GRAPH=1 ignored" in caplog.text
    torch.cuda.synchronize()
    loss_bound, grad_bound, floor = TRAIN_BOUNDS["fp32"]
    lerr = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_losses))
    perr = grad_errors([p.detach() for p in enc.get_params()], [p.detach() for p in ref_enc.parameters()], floor)
    serr = grad_errors(list(agent.encoder_ema.shadow_params), shadow, floor)
    moved = max((p.detach() - q).abs().max().item() for p, q in zip(enc.get_params(), init))
    print(f"agent + encoder, 3 steps: loss err {lerr:.3e}, parameter err {max(perr):.3e}, EMA shadow err {max(serr):.3e}, moved {moved:.2e}")
    assert moved > 1e-3                                               # the encoder was actually trained
    assert lerr <= loss_bound and max(perr) <= grad_bound and max(serr) <= grad_bound

    # inference runs on the EMA encoder: the raw weights do not matter, the shadow does
    sig, noise = torch.full((B,), 0.4, device=DEV), torch.randn(B, cfg.obs_seq_len, cfg.act_dim, device=DEV)
    obs = {"observation": batch["observation"][:, 0], "goal_observation": batch["goal_observation"][0]}

    def infer():
        agent.reset()
        torch.manual_seed(5)
        return agent.validation_loss(batch, sigma=sig, noise=noise), agent.predict(obs)

    v0, p0 = infer()
    assert np.isfinite(v0) and p0.shape[-1] == cfg.act_dim and p0.numel() == B * cfg.act_dim and bool(torch.isfinite(p0).all())
    with torch.no_grad():
        for p in enc.get_params():
            p.mul_(3.0)
    v1, p1 = infer()
    assert v1 == v0 and torch.equal(bits(p1), bits(p0))
    with torch.no_grad():
        agent.encoder_ema._flat.mul_(1.5)
    v2, p2 = infer()
    assert v2 != v0 and not torch.equal(p2, p0)
    agent.use_ema = False
    assert infer()[0] not in (v0, v2)

    # refused by name
    from beso_amd import distributed as bdist
    monkeypatch.setattr(bdist, "is_distributed", lambda: True)
    monkeypatch.setattr(bdist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        agent.train_step(batch)


@pytest.mark.gpu
def test_no_encoder_agent_enqueues_what_the_plain_step_enqueues(monkeypatch):
    """A NoEncoder agent's train_step: the launches of the HIP step called directly, and no encoder entry point."""
    agent = make_agent(DEV, encoder=False)
    assert agent.encoder_optimizer is None and agent._trainable_encoder() is None
    batch = make_batch(DEV, raw=O.TINY.obs_dim)
    agent.train_step(batch)                                          # warm: buffers, streams
    monkeypatch.setattr(_lib, "load_mlp", lambda: (_ for _ in ()).throw(AssertionError("an encoder entry point was asked for")))
    state, action, goal = agent.process_batch(batch, predict=False)
    noise, sigma = torch.randn_like(action), torch.full((len(action),), 0.5, device=DEV)
    for site in ("gemm_qkv", "attention", "layernorm", "embed", "fused_layer"):
        direct = count_site_launches(site, lambda: agent.model.hip_train_step(state, action, goal, noise, sigma)
                                     .loss_backward(state, action, goal, noise, sigma))
        assert count_site_launches(site, lambda: agent.train_step(batch)) == direct, site
    agent.predict({"observation": batch["observation"][:, 0], "goal_observation": batch["goal_observation"][0]})
    agent.validation_loss(batch)
