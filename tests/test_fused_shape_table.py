"""fused.hip's shape predicates, pinned on the CPU: every size function of the library over a sweep of configurations on the
edges of the predicates returns what the library of commit c5d1d8e returned (tests/golden/fused_shape_table.npz, recorded
from that commit's build by tools/record_fused_shape_table.py, which also defines the sweep).  A predicate that starts or
stops looking at the head grouping, or moves a class edge, changes an image or workspace size somewhere in the sweep."""
import os
import sys

import numpy as np

from support import lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_fused_shape_table as rec  # noqa: E402


def test_sweep_holds_the_cases_where_the_predicates_disagree():
    cs = rec.cases()
    assert len(set(cs)) == len(cs)
    dims = {(c[2], c[4]) for c in cs}
    assert (360, 18) in dims and (240, 6) in dims        # (3, 12) rows with HG = 3; (2, 8) rows with HG = 1
    assert (360, 12) in dims                             # head size 30: no multiple of 4
    assert {c[2] for c in cs} >= {232, 240, 248, 256, 352, 360, 368, 376, 384, 504, 512, 520}
    assert {c[3] for c in cs} == {1, 6, 7} and {c[1] for c in cs} == {16, 17} and {c[7] for c in cs} == {0, 1}
    for G, below, above in ((2, 4, 5), (0, 5, 6)):       # 8 T on both sides of 96
        assert 8 * (1 + G + 2 * below) <= 96 < 8 * (1 + G + 2 * above)
    for G, below, above in ((2, 38, 39), (0, 39, 40)):   # T on both sides of 16 kLongNT
        assert 1 + G + 2 * below <= 80 < 1 + G + 2 * above
    assert {c[6] for c in cs} >= {4, 5, 6, 38, 39, 40} and {c[5] for c in cs} == {0, 2}


def test_sizes_match_the_recorded_commit(lib):
    want = np.load(os.path.join(ROOT, "tests", "golden", "fused_shape_table.npz"))
    assert str(want["commit"]) == rec.COMMIT
    cases, values = rec.sweep(lib)
    assert np.array_equal(cases, want["cases"]), "the sweep is not the recorded one: record the fixture again"
    assert values.shape == want["values"].shape and values.shape[1] == len(rec.columns())
    assert (want["values"] != 0).mean() > 0.25           # the fixture holds sizes, not a sweep of rejected configs
    bad = np.argwhere(values != want["values"])
    names = rec.columns()
    report = [f"{tuple(cases[i].tolist())} {names[j]}: {values[i, j]} != {want['values'][i, j]}" for i, j in bad[:8]]
    assert len(bad) == 0, f"{len(bad)} values differ:\n" + "\n".join(report)
