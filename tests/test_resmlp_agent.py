"""``MLPEncoder`` over a ``ResidualMLPNetwork`` in ``BesoAgent``: training by the HIP step, inference on the EMA encoder and
the checkpoint round trip -- the agent has no branch on the network's class.  Comparator of the training: a torch-op agent step
-- tests/autograd_reference.py behind a torch re-statement of the residual network, ``torch.optim.AdamW`` on both parameter
sets, reseeded to draw the same noise and sigma -- held to the bounds tests/test_encoder_agent.py uses for the MLP encoder."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from beso_amd.agents.input_encoders.obs_encoder import MLPEncoder
from beso_amd.networks.mlps.mlps import ResidualMLPNetwork
from beso_amd.networks.scaler.scaler_class import Scaler
from oracle import beso_oracle as O
from support import TRAIN_BOUNDS, bits, build_agent, grad_errors, make_denoiser

DEV = "cuda:0"
RAW, HIDDEN, B = 7, 32, 5


def make_agent(device, precision="fp32", encoder=True, lr=1e-3):
    cfg = O.TINY
    w = O.make_weights(cfg, seed=2, std=0.05)
    extra = {}
    if encoder:
        # the config form: _target_ + kwargs, as a user's yaml gives it
        net = {"_target_": "beso_amd.networks.mlps.mlps.ResidualMLPNetwork", "input_dim": RAW, "hidden_dim": HIDDEN,
               "num_hidden_layers": 2, "output_dim": cfg.obs_dim, "activation": "Mish", "use_norm": True,
               "norm_style": "LayerNorm", "device": device}
        extra["input_encoder"] = lambda: MLPEncoder(device=device, state_modality="observation",
                                                    goal_modality="goal_observation", network=net)
    torch.manual_seed(11)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, precision, device=device), device=device, lr=lr, **extra)
    raw = RAW if encoder else cfg.obs_dim
    agent.get_scaler(Scaler(np.random.default_rng(0).standard_normal((64, raw)).astype(np.float32),
                            np.random.default_rng(1).standard_normal((64, cfg.act_dim)).astype(np.float32), True, device))
    agent.set_bounds(agent.scaler)
    return agent


def make_batch(device, goal_batch=B, raw=RAW, seed=7):
    cfg = O.TINY
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(device)                               # noqa: E731
    return {"observation": r(B, cfg.obs_seq_len, raw), "action": r(B, cfg.obs_seq_len, cfg.act_dim),
            "goal_observation": r(goal_batch, cfg.goal_seq_len, raw)}


class TorchResidual(nn.Module):
    """The residual network in torch ops over copies of `net`'s parameters (one LayerNorm per block, used twice)."""

    def __init__(self, net):
        super().__init__()
        self.layers = copy.deepcopy(net.layers)

    def forward(self, x):
        x = self.layers[0](x)
        for blk in self.layers[1:-1]:
            v = blk.l1(nn.functional.mish(blk.normalizer(x)))
            x = blk.l2(nn.functional.mish(blk.normalizer(v))) + x
        return self.layers[-1](x)


def test_encoder_instantiates_from_a_config_and_checkpoints(tmp_path):
    """CPU: the `_target_` config builds the residual network inside MLPEncoder; store_model_weights writes both encoder files
    under the reference's keys and load_pretrained_model restores them (EMA weights into the encoder, the shadow re-seeded)."""
    agent = make_agent("cpu")
    net = agent.input_encoder.network
    assert isinstance(net, ResidualMLPNetwork) and agent._trainable_encoder() is agent.input_encoder
    assert agent.encoder_optimizer is not None and agent.encoder_ema is not None
    keys = ["layers.0.weight", "layers.0.bias", "layers.1.l1.weight", "layers.1.l1.bias", "layers.1.l2.weight", "layers.1.l2.bias",
            "layers.1.normalizer.weight", "layers.1.normalizer.bias", "layers.2.weight", "layers.2.bias"]
    assert list(net.state_dict()) == keys and len(list(agent.input_encoder.get_params())) == 10
    with torch.no_grad():
        agent.encoder_ema._flat.add_(0.5)
    agent.store_model_weights(str(tmp_path))
    ema = torch.load(tmp_path / "encoder_state_dict.pth")
    raw = torch.load(tmp_path / "non_ema_encoder_state_dict.pth")
    assert list(ema) == list(raw) == keys
    for k, v in net.state_dict().items():
        assert torch.equal(raw[k], v) and torch.equal(ema[k], v + 0.5)
    other = make_agent("cpu")
    other.load_pretrained_model(str(tmp_path))
    for k, v in other.input_encoder.network.state_dict().items():
        assert torch.equal(v, ema[k])
    assert torch.equal(other.encoder_ema._flat, torch.cat([ema[k].reshape(-1) for k in ema]))
    os.remove(tmp_path / "encoder_state_dict.pth")
    with pytest.raises(FileNotFoundError, match="encoder"):
        other.load_pretrained_model(str(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("goal_batch", [B, 1], ids=["goalB", "goal1"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_agent_trains_the_residual_encoder_like_the_torch_op_step(precision, goal_batch):
    from autograd_reference import loss_autograd
    from beso_amd.optim import FusedAdam
    cfg, lr = O.TINY, 1e-3
    agent = make_agent(DEV, precision, lr=lr)
    assert isinstance(agent.optimizer, FusedAdam) and isinstance(agent.encoder_optimizer, FusedAdam)
    enc = agent.input_encoder
    assert isinstance(enc.network, ResidualMLPNetwork)
    ref_model = make_denoiser(cfg, O.make_weights(cfg, seed=2, std=0.05), precision, train=True)
    ref_enc = TorchResidual(enc.network)
    opts = [torch.optim.AdamW(ref_model.parameters(), lr=lr), torch.optim.AdamW(ref_enc.parameters(), lr=lr)]
    shadow = [p.detach().clone() for p in ref_enc.parameters()]
    batch = make_batch(DEV, goal_batch)
    init = [p.detach().clone() for p in enc.get_params()]
    losses, ref_losses = [], []
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
    torch.cuda.synchronize()
    loss_bound, grad_bound, floor = TRAIN_BOUNDS[precision]
    lerr = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_losses))
    perr = grad_errors([p.detach() for p in enc.get_params()], [p.detach() for p in ref_enc.parameters()], floor)
    serr = grad_errors(list(agent.encoder_ema.shadow_params), shadow, floor)
    moved = max((p.detach() - q).abs().max().item() for p, q in zip(enc.get_params(), init))
    print(f"agent + residual encoder {precision} goal [{goal_batch},G,.], 3 steps: loss err {lerr:.3e}, parameter err {max(perr):.3e}, "
          f"EMA shadow err {max(serr):.3e}, moved {moved:.2e}")
    assert moved > 1e-3                                               # the encoder was actually trained
    assert lerr <= loss_bound and max(perr) <= grad_bound and max(serr) <= grad_bound

    # inference runs on the EMA encoder: the raw weights do not matter, the shadow does
    sig, noise = torch.full((B,), 0.4, device=DEV), torch.randn(B, cfg.obs_seq_len, cfg.act_dim, device=DEV)
    full = make_batch(DEV, B)
    obs = {"observation": full["observation"][:, 0], "goal_observation": full["goal_observation"][0]}

    def infer():
        agent.reset()
        torch.manual_seed(5)
        return agent.validation_loss(full, sigma=sig, noise=noise), agent.predict(obs)

    v0, p0 = infer()
    assert np.isfinite(v0) and p0.shape[-1] == cfg.act_dim and bool(torch.isfinite(p0).all())
    with torch.no_grad():
        for p in enc.get_params():
            p.mul_(3.0)
    v1, p1 = infer()
    assert v1 == v0 and torch.equal(bits(p1), bits(p0))
    with torch.no_grad():
        agent.encoder_ema._flat.mul_(1.5)
    v2, p2 = infer()
    assert v2 != v0 and not torch.equal(p2, p0)


@pytest.mark.gpu
def test_checkpoint_round_trip_on_the_gpu_and_the_no_encoder_step_is_undisturbed(tmp_path, monkeypatch):
    """Both encoder files come back after a trained step.  A NoEncoder agent's steps give the same bits before and after an
    agent with the residual encoder has trained in the process, and never ask for an encoder library."""
    from beso_amd import _lib
    plain_batch = make_batch(DEV, raw=O.TINY.obs_dim)

    def plain_steps():
        agent = make_agent(DEV, encoder=False)
        agent.deterministic_training = True
        assert agent.encoder_optimizer is None and agent._trainable_encoder() is None
        torch.manual_seed(9)
        losses = [agent.train_step(plain_batch) for _ in range(2)]
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in agent.model.get_params()]

    with monkeypatch.context() as m:
        m.setattr(_lib, "load_resmlp", lambda: (_ for _ in ()).throw(AssertionError("the residual library was asked for")))
        m.setattr(_lib, "load_mlp", lambda: (_ for _ in ()).throw(AssertionError("the MLP library was asked for")))
        before = plain_steps()

    agent = make_agent(DEV)
    torch.manual_seed(1)
    agent.train_step(make_batch(DEV))
    agent.store_model_weights(str(tmp_path))
    net = agent.input_encoder.network
    raw, ema = torch.load(tmp_path / "non_ema_encoder_state_dict.pth"), torch.load(tmp_path / "encoder_state_dict.pth")
    names = [k for k, _ in net.named_parameters()]
    assert list(raw) == list(ema) == list(net.state_dict())
    for k, v in net.state_dict().items():
        assert torch.equal(raw[k].to(DEV), v)
    for k, s in zip(names, agent.encoder_ema.shadow_params):
        assert torch.equal(ema[k].to(DEV), s)
    assert any(not torch.equal(ema[k], raw[k]) for k in names)          # the step moved the weights off their EMA
    other = make_agent(DEV)
    other.load_pretrained_model(str(tmp_path))
    for k, v in other.input_encoder.network.state_dict().items():
        assert torch.equal(v, ema[k].to(DEV))
    assert torch.equal(other.encoder_ema._flat, torch.cat([ema[k].reshape(-1) for k in ema]).to(DEV))

    with monkeypatch.context() as m:
        m.setattr(_lib, "load_resmlp", lambda: (_ for _ in ()).throw(AssertionError("the residual library was asked for")))
        m.setattr(_lib, "load_mlp", lambda: (_ for _ in ()).throw(AssertionError("the MLP library was asked for")))
        after = plain_steps()
    assert before[0] == after[0] and all(torch.equal(bits(p), bits(q)) for p, q in zip(before[1], after[1]))
