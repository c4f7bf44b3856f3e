"""The dropout-active training step against torch autograd, with the library's own masks.

``beso_dropout_mask`` / ``HipTrainStep.dropout_mask`` write out the keep-scale of every element of one training dropout
(embeddings, attention probabilities, out-projection, MLP output) for (batch, t, p, seed) -- the masks are a counter hash,
so nothing is recorded during the step.  The tests here replace the module's ``nn.Dropout`` layers by modules that
multiply by those tensors, run the unchanged comparator of tests/autograd_reference.py and hold the loss and every
parameter gradient of ``beso_loss_grad`` to it, as ``test_hip_training_goal_masking`` does for the goal mask.

Bounds (those of test_hip_training_goal_masking: the same comparator on the same kind of tensors):
fp32 loss 2e-5, gradients 1e-4 per tensor (floor 1e-4); bf16 loss 2e-3, gradients 2.6e-2 per tensor (floor 2e-3)."""
import contextlib
import ctypes as C

import pytest
import torch

from beso_amd import _lib
from beso_amd.runtime import ScoreNetShape
from oracle import beso_oracle as O
from support import Scale, TRAIN_BOUNDS, count_site_launches, grad_errors, lib, make_denoiser, train_inputs  # noqa: F401

DEV = "cuda:0"


# -------------------------------------------------------------------------------------------------
# CPU: the entry point exists and rejects bad arguments before anything is enqueued
# -------------------------------------------------------------------------------------------------
def test_dropout_mask_is_exported_and_bound(lib):
    assert "beso_dropout_mask" in _lib.EXPORTS
    fn = lib.beso_dropout_mask
    assert fn.restype is C.c_int and len(fn.argtypes) == 9
    assert (_lib.DROP_EMBED, _lib.DROP_ATTN, _lib.DROP_PROJ, _lib.DROP_MLP) == (0, 1, 2, 3)
    from beso_amd.training import HipTrainStep
    assert callable(HipTrainStep.dropout_mask)


def test_dropout_mask_argument_errors_do_not_touch_the_device(lib):
    """Dummy non-NULL pointers, as test_null_and_shape_errors_do_not_touch_the_device: a call that got past its argument
    checks would write through them."""
    cfg = ScoreNetShape(7, 3, 48, 2, 6, 2, 3, True, 0.5).c_struct()        # L = 2, W = 3
    one = C.c_void_p(16)
    call = lambda scale=one, kind=_lib.DROP_ATTN, layer=0, batch=4, t=3, p=0.3, cfgp=C.byref(cfg): \
        lib.beso_dropout_mask(cfgp, scale, kind, layer, batch, t, p, C.c_uint(7), None)             # noqa: E731
    assert call(scale=None) == -3
    assert call(cfgp=None) == -3
    assert call(kind=4) == -3 and call(kind=-1) == -3
    assert call(layer=2) == -3 and call(layer=-1) == -3 and call(kind=_lib.DROP_MLP, layer=2) == -3
    assert call(t=4) == -2 and call(t=0) == -2 and call(batch=0) == -2
    assert call(p=1.0) == -3 and call(p=-0.1) == -3 and call(p=float("nan")) == -3
    assert call(scale=C.c_void_p(20)) == -3                                 # not 16-byte aligned
    bad = ScoreNetShape(7, 3, 49, 2, 6, 2, 3, True, 0.5).c_struct()          # D % H != 0
    assert call(cfgp=C.byref(bad)) == -1
    with pytest.raises(ValueError):
        _lib.check(call(layer=2), "dropout_mask")


@contextlib.contextmanager
def injected_masks(inner, step, batch, t, seed, attn_after_v_layer=None):
    """The module's nn.Dropout layers replaced by the library's masks for (batch, t, seed); restored afterwards.  Only the
    dropouts with p > 0 are replaced.  forward_autograd calls inner.drop three times -- states, actions, goals -- so its
    stand-in hands out the state rows G+1+2k, the action rows G+2+2k and the goal rows 1..G of the [B, T, D] embedding mask
    in that order.
    attn_after_v_layer = l builds a deliberately WRONG comparator: the attention dropout of layer l is left out in front
    of `@ v` and applied behind it instead (the key axis is contracted away there, so query row i of head h is scaled by
    the keep-scale of its own diagonal element (i, i))."""
    embed_p, attn_p, resid_p = inner._pdrops
    G = inner.goal_seq_len
    saved, hooks = [], []

    def swap(owner, name, new):
        saved.append((owner, name, owner._modules[name]))
        owner._modules[name] = new

    try:
        if embed_p > 0:
            e = step.dropout_mask("embed", 0, batch, t, seed)
            swap(inner, "drop", Scale(e[:, G + 1::2], e[:, G + 2::2], e[:, 1:G + 1]))
        for l, blk in enumerate(inner.blocks):
            if attn_p > 0:
                a = step.dropout_mask("attn", l, batch, t, seed)
                if l == attn_after_v_layer:
                    swap(blk.attn, "attn_drop", torch.nn.Identity())
                    diag = torch.diagonal(a, dim1=2, dim2=3)                 # [B, H, T]
                    H = inner.n_heads

                    def after_v(mod, args, diag=diag, H=H):
                        y, = args                                            # [B, T, D] = heads side by side
                        b, T, D = y.shape
                        return ((y.view(b, T, H, D // H) * diag.transpose(1, 2).unsqueeze(-1)).reshape(b, T, D),)
                    hooks.append(blk.attn.proj.register_forward_pre_hook(after_v))
                else:
                    swap(blk.attn, "attn_drop", Scale(a))
            if resid_p > 0:
                swap(blk.attn, "resid_drop", Scale(step.dropout_mask("proj", l, batch, t, seed)))
                swap(blk.mlp, "3", Scale(step.dropout_mask("mlp", l, batch, t, seed)))
        yield
    finally:
        for h in hooks:
            h.remove()
        for owner, name, old in reversed(saved):
            owner._modules[name] = old


def _case(cfg_name, B, t, precision, attn_p=0.0, resid_p=0.0, embed_p=0.0, goal_drop=0.0):
    cfg = O.CONFIGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, attn_pdrop=attn_p, resid_pdrop=resid_p,
                      embed_pdrop=embed_p, goal_drop=goal_drop, train=True)
    state, action, goal, noise, sigma = train_inputs(cfg, B, seed=4)
    if t is not None:
        state, action, noise = state[:, :t].contiguous(), action[:, :t].contiguous(), noise[:, :t].contiguous()
    return m, (state, action, goal, noise, sigma)


def _hip(m, inputs, seed, per_op=False):
    """(loss, gradients, launches of the one-launch training forward) of the HIP step under the library's default plan,
    or under BESO_TRAIN_PLAN_PER_OP"""
    from beso_amd.runtime import set_plan
    step = m.hip_train_step(*inputs)
    assert step is not None
    out = {}
    set_plan(train=_lib.TRAIN_PLAN_PER_OP if per_op else 0)
    try:
        n = count_site_launches("fused_layer", lambda: out.update(r=step.run(*inputs, seed=seed, fresh_grads=True)))
    finally:
        set_plan(train=0)
    loss, _, views = out["r"]
    return step, loss.item(), [v.clone() for v in views], n


def _autograd(m, step, inputs, seed, mask_seed=None, attn_after_v_layer=None):
    """loss and gradients of tests/autograd_reference.py with the library's masks for `mask_seed` (default: seed) injected"""
    from autograd_reference import loss_autograd
    inner = m.inner_model
    state, action, goal, noise, sigma = inputs
    B, t = state.shape[0], state.shape[1]
    mask_seed = seed if mask_seed is None else mask_seed
    goal_p = inner.cond_mask_prob
    if goal_p:
        goal = goal * step.goal_mask(B, mask_seed)
    inner.cond_mask_prob = 0.0                                               # (its own mask_cond off: the mask is injected)
    try:
        with injected_masks(inner, step, B, t, mask_seed, attn_after_v_layer):
            ref_loss = loss_autograd(m, state, action, goal, noise.clone(), sigma)
            ref_loss.backward()
        return ref_loss.item(), [p.grad.clone() for p in m.parameters()]
    finally:
        inner.cond_mask_prob = goal_p
        for p in m.parameters():
            p.grad = None


def _compare(tag, m, precision, got_loss, got, ref_loss, ref):
    _, _, floor = TRAIN_BOUNDS[precision]
    lerr = abs(got_loss - ref_loss) / abs(ref_loss)
    errs = grad_errors(got, ref, floor)
    worst = max(range(len(errs)), key=lambda i: errs[i])
    print(f"[parity] dropout step {tag} {precision}: loss rel err {lerr:.2e}, worst gradient {errs[worst]:.2e} "
          f"({list(dict(m.named_parameters()))[worst]})")
    return lerr, errs[worst]


# -------------------------------------------------------------------------------------------------
# GPU: the masks themselves
# -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,p", [("embed", 0.1), ("attn", 0.3), ("proj", 0.05), ("mlp", 0.1)])
def test_mask_properties(kind, p):
    """Values in {0, 1/(1-p)}, kept fraction within 4 sigma of 1-p, a function of the seed, the layer and the element
    counter alone (the mask of samples [0, B) is the leading slice of the mask of [0, 2B): this pins the index layout),
    ones for p = 0 and on the rows the step draws no mask for."""
    from beso_amd.training import HipTrainStep
    cfg = O.KITCHEN                                                          # L = 6, H = 6, D = 360, G = 2, W = 4
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), "fp32", attn_pdrop=0.3, resid_pdrop=0.05, embed_pdrop=0.1, train=True)
    step = HipTrainStep(m.inner_model, cfg.sigma_data)
    B, t, seed, G = 8, 4, 4242, cfg.goal_seq_len
    T = 1 + G + 2 * t
    mask = step.dropout_mask(kind, 1, B, t, seed, p=p)
    assert mask.shape == ((B, cfg.n_heads, T, T) if kind == "attn" else (B, T, cfg.embed_dim)) and mask.is_contiguous()
    drawn = mask[:, 1:] if kind == "embed" else mask                         # (the sigma-token row of the embeddings)
    keep = 1.0 / (1.0 - p)
    assert bool(((drawn == 0) | ((drawn - keep).abs() <= 1e-6 * keep)).all())
    n = drawn.numel()
    frac = (drawn != 0).float().mean().item()
    print(f"[parity] dropout mask {kind} p={p}: kept fraction {frac:.4f} over {n} elements")
    assert abs(frac - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5, (frac, n)
    assert torch.equal(mask, step.dropout_mask(kind, 1, B, t, seed, p=p))
    assert not torch.equal(mask, step.dropout_mask(kind, 1, B, t, seed + 1, p=p))
    if kind == "embed":
        assert bool((mask[:, 0] == 1).all())
        assert torch.equal(mask, step.dropout_mask(kind, 99, B, t, seed, p=p))      # layer is ignored
        assert torch.equal(mask, step.dropout_mask(kind, 1, B, t, seed))             # p = None: the module's embed_pdrob
    else:
        assert not torch.equal(mask, step.dropout_mask(kind, 0, B, t, seed, p=p))
    assert torch.equal(step.dropout_mask(kind, 1, B, t, seed, p=0.0), torch.ones_like(mask))
    assert torch.equal(step.dropout_mask(kind, 1, 2 * B, t, seed, p=p)[:B], mask)
    assert torch.equal(step.dropout_mask(_lib.DROP_KINDS[kind], 1, B, t, seed, p=p), mask)   # the integer kind
    if kind in ("proj", "mlp"):
        # the last layer continues on the action tokens alone: their rows are drawn, the others carry no mask
        last = step.dropout_mask(kind, cfg.n_layers - 1, B, t, seed, p=p)
        act = last[:, G + 2::2]
        assert act.shape[1] == t and bool(((act == 0) | ((act - keep).abs() <= 1e-6 * keep)).all())
        fa = (act != 0).float().mean().item()
        assert abs(fa - (1 - p)) < 4 * (p * (1 - p) / act.numel()) ** 0.5, fa
        rest = torch.ones(T, dtype=torch.bool)
        rest[G + 2::2] = False
        assert bool((last[:, rest] == 1).all())
        assert torch.equal(step.dropout_mask(kind, cfg.n_layers - 1, 2 * B, t, seed, p=p)[:B], last)
    with pytest.raises(ValueError):                                          # t > obs_seq_len
        step.dropout_mask(kind, 0, B, cfg.obs_seq_len + 1, seed, p=p)
    if kind != "embed":
        with pytest.raises(ValueError):
            step.dropout_mask(kind, cfg.n_layers, B, t, seed, p=p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B,t", [("attn", 3, 2), ("attn", 8, 4), ("embed", 3, 2), ("proj", 5, 4), ("mlp", 5, 1)])
def test_every_element_of_the_mask_is_written_and_nothing_behind_it(kind, B, t):
    """The output is handed over uninitialised (include/beso_hip.h): prefilled with NaN bytes, every element is a number
    after the call and the guard floats behind the last one are untouched.  ("attn", 3, 2): 3 * 6 * 7 * 7 = 882 elements,
    not a multiple of the 16-byte store -- the last chunk is stored by element.)"""
    from beso_amd.training import HipTrainStep
    cfg = O.KITCHEN
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), "fp32", attn_pdrop=0.3, resid_pdrop=0.05, embed_pdrop=0.1, train=True)
    step = HipTrainStep(m.inner_model, cfg.sigma_data)
    T = 1 + cfg.goal_seq_len + 2 * t
    n = B * cfg.n_heads * T * T if kind == "attn" else B * T * cfg.embed_dim
    guard = 64
    for layer in (0, cfg.n_layers - 1):
        buf = torch.empty(n + guard, dtype=torch.float32, device=DEV)
        buf.view(torch.uint8).fill_(0xFF)
        assert bool(torch.isnan(buf).all())
        st = step.lib.beso_dropout_mask(C.byref(step.cfg), buf.data_ptr(), _lib.DROP_KINDS[kind], layer, B, t, 0.3, C.c_uint(9),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        assert not bool(torch.isnan(buf[:n]).any())
        assert bool(torch.isnan(buf[n:]).all())
        assert torch.equal(buf[:n].view(-1), step.dropout_mask(kind, layer, B, t, 9, p=0.3).view(-1))


# -------------------------------------------------------------------------------------------------
# GPU: the step against autograd with the library's masks
# -------------------------------------------------------------------------------------------------
# (48 kitchen samples: three token-tile groups of the four-sample instance of the one-launch forward; 37 x t = 2: a ragged
#  last workgroup and a short window; block-push: grouped heads (HG = 3) and both residual sites; TINY: the embedding site,
#  which only the per-op embedding kernel has; goal_drop: the goal mask on top -- all masks at once)
CASES = [
    ("kitchen", 48, None, "fp32", dict(attn_p=0.3), False),
    ("kitchen", 48, None, "bf16", dict(attn_p=0.3), False),
    ("kitchen", 37, 2, "fp32", dict(attn_p=0.3), False),
    ("block_push", 40, None, "fp32", dict(attn_p=0.05, resid_p=0.05), False),
    ("block_push", 40, None, "bf16", dict(attn_p=0.05, resid_p=0.05), False),
    ("tiny", 16, None, "fp32", dict(embed_p=0.1, attn_p=0.3, resid_p=0.1), False),
    ("kitchen", 48, None, "fp32", dict(attn_p=0.3, goal_drop=0.1), False),
    ("kitchen", 48, None, "fp32", dict(attn_p=0.3), True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,B,t,precision,drops,per_op", CASES,
                         ids=[f"{c[0]}-B{c[1]}-t{c[2]}-{c[3]}-{'-'.join(f'{k}{v}' for k, v in c[4].items())}{'-per_op' if c[5] else ''}"
                              for c in CASES])
def test_dropout_step_matches_autograd_with_the_librarys_masks(cfg_name, B, t, precision, drops, per_op):
    """Loss and every parameter gradient of the dropout-active HIP step against the autograd comparator with the masks of
    beso_dropout_mask (and beso_goal_mask) injected.  Default plan: the bf16 step's forward is the one-launch
    train_fwd_kernel (asserted at its launch site; the fp32 step has per-op kernels only); per_op: BESO_TRAIN_PLAN_PER_OP
    asked for explicitly -- the one-launch forward (bf16 cases) and the per-op forward are held to the same masks."""
    m, inputs = _case(cfg_name, B, t, precision, **drops)
    seed = 20240
    step, loss, got, launches = _hip(m, inputs, seed, per_op)
    whole = precision == "bf16" and not per_op and cfg_name in ("kitchen", "block_push")
    assert launches == (1 if whole else 0), launches
    ref_loss, ref = _autograd(m, step, inputs, seed)
    ltol, gtol, _ = TRAIN_BOUNDS[precision]
    lerr, gerr = _compare(f"{cfg_name} B={B} t={t} {drops}{' per-op' if per_op else ''}", m, precision, loss, got, ref_loss, ref)
    assert lerr < ltol, lerr
    assert gerr < gtol, gerr


@pytest.mark.gpu
def test_the_comparison_bites():
    """Kitchen, fp32, attn_pdrop 0.3.  With the masks of another seed the comparison fails by more than 10x its bound, and
    so does a deliberately wrong comparator that applies the layer-0 attention mask behind `@ v` instead of in front of it
    (injected_masks: attn_after_v_layer) -- while the right one passes."""
    m, inputs = _case("kitchen", 48, None, "fp32", attn_p=0.3)
    seed = 20240
    step, loss, got, _ = _hip(m, inputs, seed)
    ltol, gtol, _ = TRAIN_BOUNDS["fp32"]
    lerr, gerr = _compare("kitchen B=48 (right masks)", m, "fp32", loss, got, *_autograd(m, step, inputs, seed))
    assert lerr < ltol and gerr < gtol
    lerr, gerr = _compare("kitchen B=48 (masks of seed + 1)", m, "fp32", loss, got, *_autograd(m, step, inputs, seed, mask_seed=seed + 1))
    assert gerr > 10 * gtol and lerr > 10 * ltol, (lerr, gerr)
    lerr, gerr = _compare("kitchen B=48 (layer-0 attention mask behind @ v)", m, "fp32", loss, got,
                          *_autograd(m, step, inputs, seed, attn_after_v_layer=0))
    assert gerr > 10 * gtol, (lerr, gerr)
