"""``VectorRollout.step`` against a trace of its own results (tests/golden/rollout_step_trace.npz, written by
tests/golden/make_rollout_trace.py on the MI355X): six scenarios that cross the scaler tail, the sampler, best-of-K with both
selections and keyed / explicit / mixed noise, five steps each with a reset in between, every array bit for bit.  The other
rollout tests pin these branches pairwise against a reference computed beside them; this one pins the combinations, so that a
change to the host path in front of the kernels cannot move a bit unnoticed."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

SCENARIOS = ("scaler_ddim_explicit", "minmax_ddim_seeded_kde4", "scaler_ancestral_seeded_mean2", "declined_minmax_ddim_explicit",
             "unscaled_minmax_ddim_explicit", "scaler_ddim_seeded_explicit_at_2")
ALWAYS = ("pred", "lengths", "obs_ctx", "act_ctx", "x0")


@pytest.fixture(scope="module")
def replayed():
    spec = importlib.util.spec_from_file_location("make_rollout_trace", os.path.join(GOLDEN, "make_rollout_trace.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.run_scenarios()


@pytest.fixture(scope="module")
def recorded():
    return load_golden("rollout_step_trace.npz")


def test_the_trace_holds_every_scenario(recorded):
    """``pred`` of the five steps and the state after the last one for all six scenarios; the best-of-K scenarios their index and
    scores, the seeded ones their counters (environment 1 was reset in front of step 3: episode 1, step 1 at the end)."""
    assert sorted({k.split("::")[0] for k in recorded}) == sorted(SCENARIOS)
    for name in SCENARIOS:
        have = {k.split("::")[1] for k in recorded if k.startswith(name + "::")}
        want = set(ALWAYS) | ({"index", "scores"} if "kde4" in name or "mean2" in name else set()) \
            | ({"noise_episode", "noise_step"} if "seeded" in name else set())
        assert have == want, name
        assert recorded[f"{name}::pred"].shape[:2] == (5, 3) and recorded[f"{name}::lengths"].tolist() == [2, 2, 2]
        assert np.isfinite(recorded[f"{name}::pred"]).all() and np.abs(recorded[f"{name}::pred"]).max() > 0
        if "seeded" in name:
            assert recorded[f"{name}::noise_episode"].tolist() == [0, 1, 0] and recorded[f"{name}::noise_step"].tolist() == [4, 1, 4]
    assert recorded["minmax_ddim_seeded_kde4::scores"].shape == (3, 4) and recorded["scaler_ancestral_seeded_mean2::scores"].shape == (3, 2)


@pytest.mark.parametrize("name", SCENARIOS)
def test_step_reproduces_the_recorded_trace_bit_for_bit(name, replayed, recorded):
    keys = sorted(k for k in recorded if k.startswith(name + "::"))
    assert keys == sorted(k for k in replayed if k.startswith(name + "::"))
    for k in keys:
        got, want = replayed[k], recorded[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert got.tobytes() == want.tobytes(), (k, int((got != want).sum()), got.size)
