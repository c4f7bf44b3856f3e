#!/usr/bin/env python3
"""Generate tests/golden/resmlp_reference.npz by RUNNING THE REFERENCE's ``ResidualMLPNetwork`` (beso/networks/mlps/mlps.py:76-133
over networks/mlps/res_layers.py), imported unmodified from /root/reference on the CPU with ``device='cpu'``.

Run in the build container only (``/root/reference`` does not exist on the GPU box):

    python tests/golden/make_resmlp_fixtures.py

The modules the reference imports at module scope that are absent from this image are replaced by the same empty stand-ins
``make_fixtures.py`` uses.  Per case the file holds the state_dict keys IN ORDER, every weight, 33 input rows, the output, and
the gradients of ``loss = y.pow(2).mean()`` with respect to every parameter and to x.  Weights: the reference's own seeded
initialisation; a LayerNorm's gamma and beta are moved off 1 and 0 (seeded) so that their use in the forward and their
gradients are visible.  Only data is written -- no reference source in any form."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
ROWS = 33
# name -> the reference's constructor kwargs
CASES = {
    "mish_layernorm": dict(input_dim=11, hidden_dim=48, num_hidden_layers=4, output_dim=7, dropout=0, activation="Mish",
                           use_spectral_norm=False, use_norm=True, norm_style="LayerNorm"),
    "relu_plain": dict(input_dim=11, hidden_dim=48, num_hidden_layers=2, output_dim=7, dropout=0, activation="ReLU",
                       use_spectral_norm=False, use_norm=False),
}


def _install_stubs():
    hydra = types.ModuleType("hydra")
    hydra.utils = types.ModuleType("hydra.utils")
    hydra.utils.instantiate = lambda cfg, *a, **kw: cfg(*a, **kw)
    hydra.main = lambda *a, **k: (lambda f: f)
    omegaconf = types.ModuleType("omegaconf")
    omegaconf.DictConfig = dict
    omegaconf.OmegaConf = type("OmegaConf", (), {})
    torchsde = types.ModuleType("torchsde")
    torchsde.BrownianTree = object
    torchdiffeq = types.ModuleType("torchdiffeq")
    torchdiffeq.odeint = None
    wandb = types.ModuleType("wandb")
    wandb.log = lambda *a, **k: None
    for name, mod in [("hydra", hydra), ("hydra.utils", hydra.utils), ("omegaconf", omegaconf),
                      ("torchsde", torchsde), ("torchdiffeq", torchdiffeq), ("wandb", wandb)]:
        sys.modules.setdefault(name, mod)


def main():
    _install_stubs()
    sys.path.insert(0, REF)
    from beso.networks.mlps.mlps import ResidualMLPNetwork

    out = {"cases": np.array(list(CASES))}
    for seed, (name, kw) in enumerate(CASES.items(), start=50):
        torch.manual_seed(seed)
        net = ResidualMLPNetwork(device="cpu", **kw).eval()
        g = torch.Generator().manual_seed(seed + 100)
        with torch.no_grad():
            for key, p in net.named_parameters():
                if ".normalizer." in key:
                    p.add_(0.2 * torch.randn(p.shape, generator=g))
        x = torch.randn(ROWS, kw["input_dim"], generator=g).requires_grad_(True)
        y = net(x)
        y.pow(2).mean().backward()
        sd = net.state_dict()
        assert list(sd) == [k for k, _ in net.named_parameters()]
        out[f"{name}::keys"] = np.array(list(sd))
        for key, v in sd.items():
            out[f"{name}::w::{key}"] = v.detach().numpy().copy()
        for key, p in net.named_parameters():
            out[f"{name}::g::{key}"] = p.grad.numpy().copy()
        out[f"{name}::x"], out[f"{name}::y"], out[f"{name}::dx"] = x.detach().numpy().copy(), y.detach().numpy().copy(), x.grad.numpy().copy()
    path = os.path.join(HERE, "resmlp_reference.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {os.path.basename(path)}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
