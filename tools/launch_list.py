#!/usr/bin/env python3
"""Which kernels the library launches, call by call, on the boundaries of fused.hip's launch selection -- the check of a change
to the host layer that must leave every launch as it was (the instances return equal bits, so results cannot show it).

    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python tools/launch_list.py run
                                        (GPU box: a fixed list of calls, once each; BESO_HIP_LIB picks the library)
    python tools/launch_list.py list OUT/**/run_kernel_trace.csv
                                        (the library's launches in dispatch order -- kernel, grid, workgroup, LDS bytes --
                                         and their sha1: two libraries launch the same when the lists are equal)
"""
import csv
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import torch
    from bench import build_model
    from beso_amd import _lib as L
    from beso_amd import synthetic as O
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    from beso_amd.runtime import plan
    dev = "cuda:0"

    def net(cfg, precision, **kw):
        m = build_model(cfg, O.make_weights(cfg, seed=0, std=0.02), precision, dev, **kw)
        inner = m.inner_model
        return m, inner.runtime(cfg.sigma_data), inner.packed_weights()

    def inputs(cfg, B):
        return tuple(torch.from_numpy(v).to(dev) for v in O.make_inputs(cfg, B, seed=1))

    def forward(rt, packed, cfg, B, sigma=None, **kw):
        s, g, a = inputs(cfg, B)
        sig = torch.linspace(0.05, 1.0, B, device=dev) if sigma is None else torch.full((B,), sigma, device=dev)
        with torch.no_grad():
            rt.denoise(packed, s, a, g, sig, **kw)
        torch.cuda.synchronize()

    def train(cfg, B, hint=0, **kw):
        m, _, _ = net(cfg, "bf16", train=True, **kw)
        s, g, a = inputs(cfg, B)
        noise, sig = torch.randn_like(a), torch.linspace(0.05, 1.0, B, device=dev)
        with plan(train=hint):
            m.hip_train_step(s, a, g, noise, sig).run(s, a, g, noise, sig, seed=1)
        torch.cuda.synchronize()

    torch.manual_seed(0)
    kitchen, block_push, long_h = O.SHAPES["kitchen"], O.SHAPES["block_push"], O.SHAPES["long_horizon"]
    _, rt, pk = net(kitchen, "bf16")
    for B in (512, 513, 1024, 1025):                     # two-, four-, eight-sample instances
        forward(rt, pk, kitchen, B)
    # every plan hint at a batch size where the library's own choice is another one
    for hint, B in ((L.PLAN_SPW2, 1025), (L.PLAN_SPW4, 1025), (L.PLAN_SIGMA_SHARED, 512), (L.PLAN_SIGMA_PRIVATE, 1025),
                    (L.PLAN_BLOCKS, 512), (L.PLAN_PER_OP, 512)):
        with plan(forward=hint):
            forward(rt, pk, kitchen, B)
    forward(rt, pk, kitchen, 1025, sigma=0.3)            # uniform sigma (the per-sample vector is the default above)
    forward(rt, pk, kitchen, 1025, cond_lambda=2.0)      # classifier-free pair
    with torch.no_grad():                                # sampler loops as one launch
        s, g, a = inputs(kitchen, 64)
        sigmas = ks.get_sigmas_exponential(3, 0.005, 1.0)
        rt.sample(pk, "ddim", s, torch.randn_like(a), g, sigmas)
        rt.sample(pk, "dpmpp_2m", s, torch.randn_like(a), g, sigmas)
    torch.cuda.synchronize()
    _, rt, pk = net(kitchen, "fp16")
    forward(rt, pk, kitchen, 1025)
    _, rt, pk = net(kitchen, "bf16x3")
    for B in (512, 1025):
        forward(rt, pk, kitchen, B)
    _, rt, pk = net(block_push, "bf16")
    for B in (512, 1025):
        forward(rt, pk, block_push, B)
    for precision in ("bf16", "bf16x3"):                 # one launch; the split-bf16 block kernels
        _, rt, pk = net(long_h, precision)
        forward(rt, pk, long_h, 5)
    wide_heads = O.ModelShape(30, 9, 360, 6, 18, 2, 4)   # (3, 12) rows with HG = 3: MLP-block kernels, not the one launch
    _, rt, pk = net(wide_heads, "bf16")
    forward(rt, pk, wide_heads, 300)
    for B in (1024, 1025):
        train(kitchen, B, attn_pdrop=0.3)
    train(block_push, 1024, attn_pdrop=0.05, resid_pdrop=0.05)
    for hint in (L.TRAIN_PLAN_PER_OP, L.TRAIN_PLAN_TILES):
        train(kitchen, 1024, hint=hint, attn_pdrop=0.3)
    print("launch_list: every call returned")


def launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    out = []
    for r in rows:
        if "beso::" not in r["Kernel_Name"]:
            continue                                     # (torch's own fills and random draws)
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        out.append(f"{r['Kernel_Name']} grid {grid} workgroup {wg} lds {r['LDS_Block_Size']}")
    return out


def main():
    if sys.argv[1] == "run":
        return run()
    lines = launches(sys.argv[2])
    print("\n".join(lines))
    print(f"# {len(lines)} launches, sha1 {hashlib.sha1(chr(10).join(lines).encode()).hexdigest()}")


if __name__ == "__main__":
    main()
