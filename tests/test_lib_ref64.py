"""tests/lib_ref64.py and tests/lib_edges.py alone, on the CPU: the float64
restatement of every known-answer case against the SwiftShader answers
(LIB_kat.npz), and the conditions on undecided points."""
import json
import os

import numpy as np
import pytest

from tests import lib_edges as edges
from tests import lib_ref64 as ref64
from tests.golden import lib_kat_cases as kat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE_IDS = [c[0] for c in kat.CASES]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "LIB_kat.npz"), allow_pickle=False)
    assert json.loads(str(z["meta"]))["cases"] == CASE_IDS
    return z


@pytest.mark.parametrize("i", range(len(kat.CASES)), ids=CASE_IDS)
def test_ref64_matches_the_known_answers(golden, i):
    """Within the case's class tolerance at all 64 golden points, no outliers:
    every output at decided points, the continuous ones at undecided points.
    At most 5 % of the 64 points are undecided by a near tie; exact ties in
    real arithmetic (margin 0 in float64: mengersponge's self-similar regions)
    are their own class and reported."""
    name, _, cls = kat.CASES[i]
    rel, ab, _ = kat.TOL[cls]
    res = ref64.evaluate(name, golden["points"])
    ok, dev = ref64.compare(res, golden["dist"][i], golden["mat"][i], rel, ab)
    und, tie = ref64.undecided(res, rel, ab)
    print(f"{name} [{cls}]: max deviation {dev:.3g}, undecided {int(und.sum())} of {len(und)} "
          f"({int(tie.sum())} exact ties)")
    assert ok.all(), (np.flatnonzero(~ok).tolist(), golden["points"][~ok][:2])
    assert (und & ~tie).sum() <= 0.05 * len(und), int((und & ~tie).sum())


@pytest.mark.parametrize("name", CASE_IDS + [c[0] for c in ref64.cases2()])
def test_edge_sets_are_mostly_decided(name):
    """Undecided points (exact ties included) are at most half of a case's
    edge set, and every deciding branch of the case has points on both sides."""
    cls = dict((c[0], c[2]) for c in kat.CASES)[name.split("@")[0]]
    rel, ab, _ = kat.TOL[cls]
    pts = edges.edge_points(name)
    assert 1000 <= len(pts) <= 4000 and pts.dtype == np.float32, len(pts)
    angle = 0.0 if name.endswith("@0") else 33.0
    res = ref64.evaluate(name, pts, angle)
    und, _ = ref64.undecided(res, rel, ab)
    assert und.sum() <= 0.5 * len(pts), (int(und.sum()), len(pts))
    for k, b in enumerate(res.branches):
        if b.decides:
            v = b.value[np.isfinite(b.value)]
            assert (v < 0).sum() >= 8 and (v > 0).sum() >= 8, (name, k)


def test_angle_variants_spell_their_angles():
    c2 = ref64.cases2()
    assert len(c2) == 2 * 21
    for name, body, _, angle in c2:
        assert ("u_mouse.x" in body) == (angle is None), body
        assert angle is None or "0.0" in body
    assert ref64.plugin_source2().count("if (fn ==") == len(kat.CASES) + len(c2)
