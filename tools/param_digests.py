#!/usr/bin/env python3
"""SHA-256 digests of what the library makes of a caller's parameter list, one line per case -- the check of a change to the
host code that reads the list (csrc/params.h and its users): a role mix-up between two tensors of one shape is invisible to
every size, so two libraries are compared bit for bit, not against a tolerance.

    python tools/param_digests.py > new.txt;  BESO_HIP_LIB=<other library> python tools/param_digests.py > old.txt;  diff old.txt new.txt
                                        (GPU box: seeded weights and inputs, every case once)

    pack      the bytes beso_pack_weights wrote (into a zeroed image), every precision the shape has
    train     loss and grads_flat of one BESO_TRAIN_DETERMINISTIC step: the shapes, batch sizes, precisions, plans and dropouts
              of tests/test_reproducible_training.py
    vjp       denoised, x_grad, dot, state_grad and goal_grad of one beso_denoise_vjp_inputs call on those shapes
"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def build(cfg, precision, attn_p=0.0, resid_p=0.0, embed_p=0.0, goal_p=0.0, train=False):
    import torch
    from beso_amd import synthetic as O
    from beso_amd.agents.diffusion_agents.k_diffusion.score_gpts import DiffusionGPT
    from beso_amd.agents.diffusion_agents.k_diffusion.score_wrappers import GCDenoiser
    inner = DiffusionGPT(state_dim=cfg.obs_dim, device=DEV, goal_conditioned=cfg.goal_conditioned, action_dim=cfg.act_dim,
                         embed_dim=cfg.embed_dim, embed_pdrob=embed_p, attn_pdrop=attn_p, resid_pdrop=resid_p,
                         n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=cfg.goal_seq_len, obs_seq_len=cfg.obs_seq_len,
                         sigma_vocab_size=3, time_embedding_fn=None, goal_drop=goal_p, linear_output=cfg.linear_output,
                         precision=precision)
    m = GCDenoiser(inner, sigma_data=cfg.sigma_data)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v.copy()) for k, v in O.make_weights(cfg, seed=3, std=0.06).items()})
    m.load_state_dict(sd)
    return (m.train() if train else m.eval()).to(DEV)


def inputs(cfg, B, seed=4):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                      # noqa: E731
    return (r(B, cfg.obs_seq_len, cfg.obs_dim), r(B, cfg.obs_seq_len, cfg.act_dim), r(B, cfg.goal_seq_len, cfg.obs_dim),
            r(B, cfg.obs_seq_len, cfg.act_dim), (torch.rand(B, generator=g) * 0.9 + 0.05).to(DEV))


def main():
    import torch
    from beso_amd import _lib
    from beso_amd import synthetic as O
    from beso_amd.runtime import PackedWeights, plan
    S = O.ModelShape
    shapes = dict(O.SHAPES,
                  mlp_head=S(11, 3, 64, 3, 4, 2, 3, linear_output=False),          # generic shapes: the MLP head; one layer
                  one_layer=S(7, 3, 48, 1, 6, 2, 3),
                  hd4=S(6, 4, 32, 2, 8, 2, 3), d128=S(6, 4, 128, 2, 4, 2, 3),      # (tests/test_reproducible_training.py)
                  mlp_d8=S(5, 2, 8, 1, 2, 1, 2, linear_output=False, sigma_data=1.0))
    lib = _lib.load()
    for name in ("kitchen", "block_push", "long_horizon", "mlp_head", "one_layer"):
        cfg = shapes[name]
        for precision in ("fp32", "bf16", "bf16x3", "fp16"):
            m = build(cfg, precision)
            rt = m.inner_model.runtime(cfg.sigma_data)
            nbytes = lib.beso_packed_bytes(C.byref(rt.cfg), rt.precision)
            image = PackedWeights(torch.zeros(nbytes, dtype=torch.uint8, device=DEV), rt.precision, None)
            try:
                rt.pack(list(m.inner_model.parameters()), into=image)
            except ValueError as e:                                           # (no kernel of this precision for the shape)
                print(f"pack {name} {precision}: {e}")
                continue
            torch.cuda.synchronize()
            print(f"pack {name} {precision}: {nbytes} bytes {digest(image.buf)}")
    plans = {"default": 0, "per_op": _lib.TRAIN_PLAN_PER_OP, "tiles": _lib.TRAIN_PLAN_TILES}
    cases = [("kitchen", 48, "bf16", "default", 0.0, 0.0, 0.0, 0.0), ("kitchen", 48, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
             ("kitchen", 48, "bf16", "per_op", 0.3, 0.1, 0.1, 0.1), ("kitchen", 48, "bf16", "tiles", 0.3, 0.1, 0.1, 0.1),
             ("block_push", 40, "bf16", "default", 0.0, 0.05, 0.0, 0.0), ("block_push", 40, "fp32", "default", 0.0, 0.05, 0.0, 0.0),
             ("tiny_mlp_head", 9, "fp32", "default", 0.0, 0.0, 0.0, 0.0), ("tiny_mlp_head", 70, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
             ("tiny_mlp_head", 70, "bf16", "default", 0.0, 0.0, 0.0, 0.0), ("mlp_d8", 400, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
             ("d128", 40, "fp32", "default", 0.0, 0.0, 0.0, 0.0), ("d128", 40, "bf16", "default", 0.0, 0.0, 0.0, 0.0),
             ("kitchen", 192, "fp32", "default", 0.0, 0.0, 0.0, 0.0), ("kitchen", 192, "bf16", "per_op", 0.0, 0.0, 0.0, 0.0),
             ("hd4", 7, "fp32", "default", 0.0, 0.0, 0.0, 0.0)]
    for name, B, precision, hint, attn_p, resid_p, embed_p, goal_p in cases:
        cfg = shapes[name]
        m = build(cfg, precision, attn_p, resid_p, embed_p, goal_p, train=True)
        x = inputs(cfg, B)
        step = m.hip_train_step(*x)
        with plan(train=plans[hint]):
            loss, flat, _ = step.run(*x, seed=4242, deterministic=True)
            torch.cuda.synchronize()
            print(f"train {name} B={B} {precision} {hint}{' dropout' if attn_p or resid_p else ''}: loss {loss.item()!r} "
                  f"{digest(loss, flat)}")
            if attn_p or resid_p or embed_p:
                continue                                                      # (the input VJP is the eval-mode function)
            state, action, goal, cot, sigma = x
            out = step.denoise_vjp(state, action, goal, sigma, cot, input_grads=True)
            torch.cuda.synchronize()
            print(f"vjp {name} B={B} {precision} {hint}: {digest(*[t for t in out if t is not None])}")


if __name__ == "__main__":
    main()
