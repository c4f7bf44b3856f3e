"""``GuideTrainer.train_step`` and ``CriticTrainer.train_step`` against a trace of their own results (tests/golden/fit_trace.npz,
written by tests/golden/make_fit_trace.py on the MI355X): four guide and four critic scenarios that cross a per-sample, a shared
and no goal, ``use_sigma`` with generator-drawn noise, weights with a zero row, ``next_state`` given or read from ``state``, a
``bool`` done and a save / load after step 2; four steps each, every array bit for bit.  The other fit tests pin the kernels and
the step against references computed beside them; this one pins the trainers' host layer in front of the kernels, so that a
change to it cannot move a bit unnoticed."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

SCENARIOS = ("guide_mse_goal_own", "guide_bce_sigma_goal_shared", "guide_mse_no_goal_weights", "guide_save_load",
             "critic_next_from_state_goal_own", "critic_next_given_goal_shared_weights_bool_done", "critic_no_goal", "critic_save_load")
ARRAYS = ("losses", "steps", "losses_sha256", "per_row_sha256", "params_sha256")


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_fit_trace", os.path.join(GOLDEN, "make_fit_trace.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


@pytest.fixture(scope="module")
def replayed(generator):
    return generator.run_scenarios()


@pytest.fixture(scope="module")
def recorded():
    return load_golden("fit_trace.npz")


def test_the_trace_holds_every_scenario(generator, recorded):
    """The five arrays of all eight scenarios: four finite losses (the critic: four pairs) that differ from step to step, every
    optimizer at step 4, three digests that differ from each other."""
    assert generator.SCENARIOS == SCENARIOS
    assert sorted({k.split("::")[0] for k in recorded}) == sorted(SCENARIOS)
    for name in SCENARIOS:
        assert {k.split("::")[1] for k in recorded if k.startswith(name + "::")} == set(ARRAYS), name
        nets = 2 if name.startswith("critic") else 1
        losses = recorded[f"{name}::losses"]
        assert losses.dtype == np.float32 and losses.shape == ((4, 2) if nets == 2 else (4,)) and np.isfinite(losses).all()
        for column in losses.reshape(4, nets).T:
            assert len(set(column.tolist())) == 4 and (column > 0).all(), name
        assert recorded[f"{name}::steps"].dtype == np.int64 and recorded[f"{name}::steps"].tolist() == [4] * nets
        digests = [recorded[f"{name}::{k}"] for k in ARRAYS if k.endswith("sha256")]
        assert all(d.shape == (32,) and d.dtype == np.uint8 for d in digests) and len({d.tobytes() for d in digests}) == 3


@pytest.mark.parametrize("name", SCENARIOS)
def test_fit_steps_reproduce_the_recorded_trace_bit_for_bit(name, replayed, recorded):
    keys = sorted(k for k in recorded if k.startswith(name + "::"))
    assert keys == sorted(k for k in replayed if k.startswith(name + "::"))
    for k in keys:
        got, want = replayed[k], recorded[k]
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert got.tobytes() == want.tobytes(), (k, got.tolist(), want.tolist())
