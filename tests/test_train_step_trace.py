"""``BesoAgent.train_step`` against a trace of its own results (tests/golden/train_step_trace.npz, written by
tests/golden/make_train_step_trace.py on the MI355X): six scenarios that cross the fused and the eager optimizer step, clipping
and the non-finite guard, the loss read on the loss stream or behind the whole step, and a trainable encoder with a per-sample or
a shared goal; four steps each, with and without the EMA update, every array bit for bit.  The other training tests pin these
branches one at a time against a reference computed beside them; this one pins the host driver in front of the kernels, so that a
change to it cannot move a bit unnoticed."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

SCENARIOS = ("fused_default", "fused_clip_guard", "fused_sync_loss", "eager_sgd_clip", "encoder_goal_per_sample",
             "encoder_goal_shared_clip")
ALWAYS = ("losses", "steps", "params_sha256", "ema_sha256")


@pytest.fixture(scope="module")
def replayed():
    spec = importlib.util.spec_from_file_location("make_train_step_trace", os.path.join(GOLDEN, "make_train_step_trace.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.run_scenarios()


@pytest.fixture(scope="module")
def recorded():
    return load_golden("train_step_trace.npz")


def test_the_trace_holds_every_scenario(recorded):
    """Four finite losses that differ from step to step, ``steps`` = 4 and the two digests for all six scenarios; the gradient
    norm (above the clipping bound: the step clipped) where clipping is on; the encoder's parameters and shadow, which differ
    (the shadow moved on two of the four steps), where there is one."""
    assert sorted({k.split("::")[0] for k in recorded}) == sorted(SCENARIOS)
    for name in SCENARIOS:
        have = {k.split("::")[1] for k in recorded if k.startswith(name + "::")}
        want = set(ALWAYS) | ({"grad_norm"} if "clip" in name else set()) \
            | ({"encoder_params", "encoder_ema"} if "encoder" in name else set())
        assert have == want, name
        losses = recorded[f"{name}::losses"]
        assert losses.shape == (4,) and losses.dtype == np.float64 and np.isfinite(losses).all() and len(set(losses.tolist())) == 4
        assert recorded[f"{name}::steps"].tolist() == [4]
        for k in ("params_sha256", "ema_sha256"):
            assert recorded[f"{name}::{k}"].shape == (32,) and recorded[f"{name}::{k}"].dtype == np.uint8
        assert recorded[f"{name}::params_sha256"].tobytes() != recorded[f"{name}::ema_sha256"].tobytes()
        if "clip" in name:
            norm = recorded[f"{name}::grad_norm"]
            assert norm.shape == (1,) and np.isfinite(norm[0]) and norm[0] > 1e-3
        if "encoder" in name:
            p, e = recorded[f"{name}::encoder_params"], recorded[f"{name}::encoder_ema"]
            assert p.shape == e.shape == (11 * 48 + 48 + 48 * 7 + 7,) and p.dtype == e.dtype == np.float32
            assert np.isfinite(p).all() and np.isfinite(e).all() and not np.array_equal(p, e)


@pytest.mark.parametrize("name", SCENARIOS)
def test_train_step_reproduces_the_recorded_trace_bit_for_bit(name, replayed, recorded):
    keys = sorted(k for k in recorded if k.startswith(name + "::"))
    assert keys == sorted(k for k in replayed if k.startswith(name + "::"))
    for k in keys:
        got, want = replayed[k], recorded[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert got.tobytes() == want.tobytes(), (k, int((got != want).sum()), got.size)
