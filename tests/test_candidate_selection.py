"""libbeso_select.so through ctypes (include/beso_select.h, csrc/select.hip): ``beso_candidates_expand`` against its torch-op
construction bit for bit, ``beso_candidates_select`` against a numpy restatement of the header's formulas -- the mean against
the sequential float32 sum bit for bit, the kernel-density scores against the fp64 evaluation within a tolerance taken from
the float32 numpy evaluation of the same inputs (never from the kernel)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from beso_amd import _lib
from support import bits

gpu = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, ACTS = (1, 2, 5, 67, 256), (1, 2, 9, 64)
MEAN, KDE = _lib.SELECT_MODES["mean"], _lib.SELECT_MODES["kde"]


# ------------------------------------------------------------------------------------------------ the yardstick
def kde_scores(c, bandwidth=0.0, dtype=np.float64):
    """The header's formulas on candidates c [K, act], every operation in `dtype` -> scores [K]."""
    c = c.astype(dtype)
    K, act = c.shape
    one = dtype(1)
    if bandwidth > 0:
        h = np.full(act, bandwidth, dtype=dtype)
    else:
        mu, sd = c.mean(axis=0, dtype=dtype), c.std(axis=0, dtype=dtype)
        floor = dtype(1e-6) * np.maximum(one, np.abs(mu))
        h = (np.maximum(sd, floor) * dtype(K) ** (dtype(-1) / dtype(act + 4))).astype(dtype)
    z = (c[:, None, :] - c[None, :, :]) / h
    q = (z * z).sum(axis=2, dtype=dtype)
    return np.log(np.exp(dtype(-0.5) * q).sum(axis=1, dtype=dtype)).astype(dtype)


def sequential_mean(c):
    """(((c[0] + c[1]) + c[2]) + ...) / float32(K) in float32, per component."""
    s = c[0].astype(np.float32).copy()
    for k in range(1, c.shape[0]):
        s = (s + c[k].astype(np.float32)).astype(np.float32)
    return (s / np.float32(c.shape[0])).astype(np.float32)


def kde_case(K, act, seed=1):
    """Candidates [N = 4, K, act] float32: environments 0 ... 2 are two or three well-separated clusters of unequal size
    (spread 0.25 around centres drawn with deviation 4), environment 3 is pure Gaussian noise.  Spread and seed were chosen
    on the fp64 yardstick alone (test_the_reference_alone_keeps_the_kde_inputs_decided): a tighter spread puts the members
    of one cluster within 2 tol of each other at act = 1."""
    rng = np.random.default_rng([seed, K, act])
    out = np.empty((4, K, act), dtype=np.float32)
    for n in range(3):
        n_cl = 2 + n % 2
        centres = rng.standard_normal((n_cl, act)) * 4.0
        share = np.array([0.6, 0.4] if n_cl == 2 else [0.55, 0.3, 0.15])
        who = rng.permutation(np.repeat(np.arange(n_cl), np.maximum(1, np.round(share * K).astype(int)))[:K])
        who = np.concatenate([who, np.zeros(K - len(who), dtype=who.dtype)])
        out[n] = centres[who] + 0.25 * rng.standard_normal((K, act))
    out[3] = rng.standard_normal((K, act))
    return out


@functools.lru_cache(maxsize=None)
def kde_reference():
    """Every (K, act) of the grid once: {(K, act): (candidates, fp64 scores [N, K])}, and the ONE score tolerance: 8 x the
    largest deviation of the float32 numpy evaluation from the fp64 one over all of these inputs (the factor covers another
    summation order and device exp / log a few ulp off)."""
    ref, worst = {}, 0.0
    for K in KS:
        for act in ACTS:
            c = kde_case(K, act)
            s64 = np.stack([kde_scores(c[n]) for n in range(len(c))])
            s32 = np.stack([kde_scores(c[n], dtype=np.float32) for n in range(len(c))])
            worst = max(worst, float(np.abs(s32.astype(np.float64) - s64).max()))
            ref[(K, act)] = (c, s64)
    tol = 8.0 * worst
    print(f"[select] float32 numpy against fp64 over the grid: {worst:.3e}; score tolerance {tol:.3e}")
    return ref, tol


def decided(s64, tol):
    """Per environment: the index the kernel must return, and whether the comparison holds it to that.  It does where the fp64
    lead over the runner-up exceeds 2 tol -- and for K = 2 always: the two scores are log(1 + e) and log(e + 1) of the same
    e in any arithmetic, an exact tie, so the contract's "lowest k among equal scores" decides and the index must be 0."""
    K = s64.shape[1]
    if K == 2:
        return np.zeros(len(s64), dtype=np.int64), np.ones(len(s64), dtype=bool)
    order = np.sort(s64, axis=1)
    gap = order[:, -1] - order[:, -2] if K > 1 else np.full(len(s64), np.inf)
    return s64.argmax(axis=1), gap > 2 * tol


# ------------------------------------------------------------------------------------------------ no GPU
def test_header_and_binding_table_name_the_same_symbols():
    """include/beso_select.h, _lib.SELECT_SIGNATURES and the library's dynamic symbol table name the same three functions; the
    table has the header's argument counts, and so has what load_select() bound; the mode and limit constants agree."""
    from beso_amd.build import build
    build(verbose=False)
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "beso_select.h")).read(), flags=re.S)
    protos = {fn: [a for a in args.split(",") if a.strip() != "void"]
              for fn, args in re.findall(r"\b(beso_candidates_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(protos) == sorted(_lib.SELECT_SIGNATURES) == sorted(_lib.SELECT_EXPORTS) and len(protos) == 3
    assert list(protos) == list(_lib.SELECT_SIGNATURES), "the table keeps the header's order"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SELECT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("beso_")) == sorted(protos)
    bound = _lib.load_select()
    for fn, args in protos.items():
        assert len(_lib.SELECT_SIGNATURES[fn][1]) == len(args) == len(getattr(bound, fn).argtypes), fn
    enum = dict(re.findall(r"\b(BESO_SELECT_[A-Z_]+)\s*=?\s*(\d+)", text))
    assert {k: int(v) for k, v in enum.items()} == {
        "BESO_SELECT_MEAN": _lib.SELECT_MODES["mean"], "BESO_SELECT_KDE": _lib.SELECT_MODES["kde"],
        "BESO_SELECT_MAX_K": _lib.SELECT_LIMITS["max_k"], "BESO_SELECT_MAX_ACT": _lib.SELECT_LIMITS["max_act"]}
    # the product library is untouched by the side library
    hip = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "beso_candidates" not in hip


def test_the_reference_alone_keeps_the_kde_inputs_decided():
    """The seeded inputs, judged by the numpy yardstick alone: at most 10 % of the environments of the whole grid have an fp64
    lead under 2 tol (at act = 64 every off-diagonal term underflows in the Gaussian environment: all scores are 0)."""
    ref, tol = kde_reference()
    assert 0 < tol < 1e-4
    total = undecided = 0
    for (K, act), (c, s64) in ref.items():
        _, ok = decided(s64, tol)
        if K == 2:
            assert (s64[:, 0] == s64[:, 1]).all()
        total += len(ok)
        undecided += int((~ok).sum())
    print(f"[select] {undecided} of {total} environments left out of the index comparison")
    assert undecided <= 0.10 * total


def test_unsupported_shapes_are_refused_by_name_without_a_launch():
    """K = 257, act = 65 and K = 0 return BESO_ERR_UNSUPPORTED with a message that names the limit; bad N / W / mode / pointers
    are refused too.  Nothing is enqueued: the calls run on a machine without a GPU."""
    from beso_amd.build import build
    build(verbose=False)
    lib = _lib.load_select()
    one = C.c_void_p(0x1000)

    def sel(**k):
        a = dict(x0_k=one, lengths=one, mode=KDE, bandwidth=0.0, N=2, W=3, act=4, K=5, x0=one, index=one, scores=one, stream=None)
        a.update(k)
        return lib.beso_candidates_select(*a.values())

    for bad, word in ((dict(K=257), "K = 257"), (dict(act=65), "act_dim = 65"), (dict(K=0), "K = 0")):
        assert sel(**bad) == _lib.ERR_UNSUPPORTED, bad
        msg = lib.beso_candidates_last_error().decode()
        assert word in msg and "supported" in msg, msg
        with pytest.raises(ValueError, match=word):
            _lib.check_select(sel(**bad), "candidates_select")
    for bad, status in ((dict(N=0), _lib.ERR_BAD_SHAPE), (dict(W=0), _lib.ERR_BAD_SHAPE), (dict(mode=2), _lib.ERR_BAD_ARG),
                        (dict(x0=None), _lib.ERR_BAD_ARG), (dict(bandwidth=float("nan")), _lib.ERR_BAD_ARG)):
        assert sel(**bad) == status, bad
        assert lib.beso_candidates_last_error().decode().startswith("beso_candidates_select: ")

    def exp(**k):
        a = dict(state=one, x=one, lengths=one, noise=one, sigma_max=1.0, N=2, W=3, obs=4, act=5, K=6, state_k=one, x_k=one,
                 stream=None)
        a.update(k)
        return lib.beso_candidates_expand(*a.values())

    for bad, status in ((dict(K=0), _lib.ERR_BAD_SHAPE), (dict(N=0), _lib.ERR_BAD_SHAPE), (dict(obs=0), _lib.ERR_BAD_SHAPE),
                        (dict(N=1 << 20, K=1 << 12), _lib.ERR_BAD_SHAPE), (dict(noise=None), _lib.ERR_BAD_ARG),
                        (dict(x_k=C.c_void_p(0x1002)), _lib.ERR_BAD_ARG)):
        assert exp(**bad) == status, bad
        assert lib.beso_candidates_last_error().decode().startswith("beso_candidates_expand: ")


# ------------------------------------------------------------------------------------------------ GPU
def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_expand(state, x, lengths, noise, sigma_max):
    """The raw entry point on NaN-filled outputs."""
    N, W, obs = state.shape
    act, K = x.shape[2], noise.shape[1]
    state_k = torch.full((N * K, W, obs), float("nan"), device=DEV)
    x_k = torch.full((N * K, W, act), float("nan"), device=DEV)
    st = _lib.load_select().beso_candidates_expand(state.data_ptr(), x.data_ptr(), lengths.data_ptr(), noise.data_ptr(), sigma_max,
                                                   N, W, obs, act, K, state_k.data_ptr(), x_k.data_ptr(), _stream())
    assert st == 0, _lib.load_select().beso_candidates_last_error()
    return state_k, x_k


def run_select(x0_k, lengths, mode, K, bandwidth=0.0):
    """The raw entry point on NaN- / sentinel-filled outputs -> (x0, index, scores) on the host."""
    NK, W, act = x0_k.shape
    N = NK // K
    x0 = torch.full((N, W, act), float("nan"), device=DEV)
    index = torch.full((N,), -77, dtype=torch.int32, device=DEV)
    scores = torch.full((N, K), float("nan"), device=DEV)
    st = _lib.load_select().beso_candidates_select(x0_k.data_ptr(), lengths.data_ptr(), mode, bandwidth, N, W, act, K,
                                                   x0.data_ptr(), index.data_ptr(), scores.data_ptr(), _stream())
    assert st == 0, _lib.load_select().beso_candidates_last_error()
    torch.cuda.synchronize()
    return x0.cpu(), index.cpu(), scores.cpu()


def windows(cand, W, lengths, seed=1):
    """Sampled windows x0_k [N K, W, act] (seeded noise in every slot) whose slot lengths[n] - 1 holds cand [N, K, act]."""
    N, K, act = cand.shape
    g = torch.Generator().manual_seed(seed)
    x0_k = torch.randn((N, K, W, act), generator=g)
    for n in range(N):
        x0_k[n, :, lengths[n] - 1] = torch.from_numpy(cand[n])
    return x0_k.reshape(N * K, W, act).to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV)


@gpu
@pytest.mark.parametrize("N,W,obs,act,K,lengths", [(3, 4, 5, 3, 5, [1, 4, 2]), (1, 1, 1, 1, 1, [1]), (2, 4, 8, 4, 3, [3, 4])])
def test_expand_equals_the_torch_op_construction_bit_for_bit(N, W, obs, act, K, lengths):
    """Every element of both outputs (pre-filled with NaN) equals repeat_interleave + an indexed write of noise * sigma_max;
    the third shape has rows of a multiple of four floats and takes the 16-byte path."""
    g = torch.Generator().manual_seed(3)
    state, x = torch.randn((N, W, obs), generator=g).to(DEV), torch.randn((N, W, act), generator=g).to(DEV)
    noise = torch.randn((N, K, act), generator=g).to(DEV)
    ln = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    sigma_max = 1.7
    state_k, x_k = run_expand(state, x, ln, noise, sigma_max)
    want_s = torch.repeat_interleave(state, K, dim=0)
    want_x = torch.repeat_interleave(x, K, dim=0)
    rows = torch.arange(N * K, device=DEV)
    want_x[rows, torch.repeat_interleave(ln.long() - 1, K)] = (noise * sigma_max).reshape(N * K, act)
    assert torch.equal(bits(state_k), bits(want_s)) and torch.equal(bits(x_k), bits(want_x))
    from beso_amd import candidates as best_of
    got = best_of.expand(state, x, ln, noise, sigma_max)
    assert torch.equal(bits(got[0]), bits(want_s)) and torch.equal(bits(got[1]), bits(want_x))


@gpu
@pytest.mark.parametrize("K", KS)
def test_mean_is_the_sequential_float32_sum_bit_for_bit(K):
    """N = 3, ragged lengths, every act of the grid: the newest slot is the sequential float32 numpy sum divided by K, the other
    slots are candidate 0's, index is -1 and the scores are zero."""
    W, lengths = 4, [2, 4, 1]
    for act in ACTS:
        rng = np.random.default_rng([7, K, act])
        cand = (rng.standard_normal((3, K, act)) * 3 + 0.5).astype(np.float32)
        x0_k, ln = windows(cand, W, lengths)
        x0, index, scores = run_select(x0_k, ln, MEAN, K)
        rows = x0_k.cpu().view(3, K, W, act)
        for n in range(3):
            want = rows[n, 0].clone()
            want[lengths[n] - 1] = torch.from_numpy(sequential_mean(cand[n]))
            assert torch.equal(bits(x0[n]), bits(want)), (K, act, n)
        assert index.tolist() == [-1] * 3 and not scores.any()


@gpu
@pytest.mark.parametrize("K", KS)
def test_kde_scores_and_index_against_fp64(K):
    """Every act of the grid on the clustered + Gaussian environments: scores within tol of fp64, index the fp64 argmax
    wherever its lead exceeds 2 tol, x0 the chosen row's window bit for bit."""
    ref, tol = kde_reference()
    W, lengths = 3, [3, 1, 2, 3]
    for act in ACTS:
        c, s64 = ref[(K, act)]
        x0_k, ln = windows(c, W, lengths)
        x0, index, scores = run_select(x0_k, ln, KDE, K)
        err = float(np.abs(scores.numpy().astype(np.float64) - s64).max())
        print(f"[select] kde K={K} act={act}: max |score - fp64| {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, (K, act, err, tol)
        best, ok = decided(s64, tol)
        idx = index.numpy()
        assert ((idx >= 0) & (idx < K)).all()
        assert (idx[ok] == best[ok]).all(), (K, act, idx, best, ok)
        if K == 2:
            assert torch.equal(bits(scores[:, 0]), bits(scores[:, 1]))
        rows = x0_k.cpu().view(len(c), K, W, act)
        for n in range(len(c)):
            assert torch.equal(bits(x0[n]), bits(rows[n, idx[n]])), (K, act, n)


@gpu
def test_kde_edge_cases():
    """K = 1; identical candidates; exact two-way ties; a fixed bandwidth; act = 1 with zero variance under Scott's rule (the
    floor); one NaN candidate."""
    W = 2
    # K = 1: index 0, score 0
    x0_k, ln = windows(np.array([[[0.3, -1.0]]], dtype=np.float32), W, [2])
    x0, index, scores = run_select(x0_k, ln, KDE, 1)
    assert index.tolist() == [0] and scores.tolist() == [[0.0]] and torch.equal(bits(x0[0]), bits(x0_k.cpu()[0]))
    # identical candidates (act = 1 among them: zero variance, the bandwidth floor): index 0, every score log K
    for K, act in ((6, 3), (5, 1)):
        cand = np.tile(np.array([[1.5, -2.0, 0.25][:act]], dtype=np.float32), (1, K, 1))
        x0, index, scores = run_select(*windows(cand, W, [1]), KDE, K)
        assert index.tolist() == [0]
        np.testing.assert_allclose(scores.numpy(), np.log(K), rtol=0, atol=4 * np.finfo(np.float32).eps * np.log(K))
    # an exact tie gives the lower index: K = 2 (symmetric by construction), and K = 4 with duplicated candidates
    x0, index, scores = run_select(*windows(np.array([[[0.0, 1.0], [2.0, -1.0]]], dtype=np.float32), W, [2]), KDE, 2)
    assert index.tolist() == [0] and scores[0, 0] == scores[0, 1]
    a, b = [0.5, 0.25, -1.0], [4.0, -3.0, 2.0]
    x0, index, scores = run_select(*windows(np.array([[b, a, b, a]], dtype=np.float32), W, [2]), KDE, 4, bandwidth=0.5)
    assert index.tolist() == [0] and scores[0, 0] == scores[0, 2] and scores[0, 1] == scores[0, 3]
    x0, index, scores = run_select(*windows(np.array([[b, a, a, b, a]], dtype=np.float32), W, [2]), KDE, 5, bandwidth=0.5)
    assert index.tolist() == [1] and scores[0, 1] == scores[0, 2] == scores[0, 4] > scores[0, 0]
    # a fixed bandwidth against the yardstick
    rng = np.random.default_rng(11)
    cand = rng.standard_normal((2, 9, 4)).astype(np.float32)
    x0, index, scores = run_select(*windows(cand, W, [1, 2]), KDE, 9, bandwidth=0.75)
    s64 = np.stack([kde_scores(c, 0.75) for c in cand])
    s32 = np.stack([kde_scores(c, 0.75, np.float32) for c in cand])
    tol = 8 * float(np.abs(s32 - s64).max())
    assert float(np.abs(scores.numpy() - s64).max()) <= tol
    assert index.tolist() == s64.argmax(axis=1).tolist()
    # one NaN candidate: the call returns, the index names a candidate, x0 is that candidate's window
    cand = rng.standard_normal((2, 7, 3)).astype(np.float32)
    cand[0, 4, 1] = np.nan
    for bw in (0.0, 0.5):
        x0_k, ln = windows(cand, W, [2, 2])
        x0, index, scores = run_select(x0_k, ln, KDE, 7, bandwidth=bw)
        assert 0 <= index[0] < 7 and torch.equal(bits(x0[0]), bits(x0_k.cpu()[index[0]]))
        assert index[1] == int(np.argmax(kde_scores(cand[1], bw))) and bool(torch.isfinite(scores[1]).all())


@gpu
@pytest.mark.parametrize("mode", [MEAN, KDE])
def test_two_calls_give_equal_bits(mode):
    c = kde_case(67, 9, seed=5)
    x0_k, ln = windows(c, 3, [3, 1, 2, 3])
    a, b = run_select(x0_k, ln, mode, 67), run_select(x0_k, ln, mode, 67)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(bits(a[2]), bits(b[2]))
