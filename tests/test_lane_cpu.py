"""The fleet step along a route (include/admpc_lane.h) without a GPU: the numpy / scipy restatement of the lane generator
(tests/lane_spec.py) reproduces what the reference's own RefTrajectory gives on the same lanes (tests/golden/lane.json, written by
scripts/make_golden_lane.py); the filter restatement the kernel follows agrees with scipy; the header declares exactly the new entry
points, the prototype table names them with the declared arity; and the refusals in front of the first device call."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
from scipy.signal import filtfilt

import lane_spec as LS
from ad_mpc_amd import _lib
from ad_mpc_amd.config import AdmpcLaneParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("admpc_waypoints_lane_batch", "admpc_control_step_lane_batch")
with open(os.path.join(ROOT, "tests", "golden", "lane.json")) as f:
    GOLD = json.load(f)
ATOL = 1e-13                                                          # the level test_ref_traj.py holds the oracle to


def _route(k):
    r = GOLD["routes"][k]
    return np.array(r["vel"]), np.array(r["x"]), np.array(r["y"]), np.array(r["psi"])


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: "route%d-i%d-L%d-H%d" % (c["route"], c["i0"], c["L"], c["H"]))
def test_spec_reproduces_the_reference_on_the_lane(case):
    route = _route(case["route"])
    tab = LS.lane_table(route, case["i0"], case["L"], case["speed"], case["acc_max"], case["clamp_dt"])
    gold = np.array(case["table"])
    assert tab.shape == gold.shape == (case["L"], 6)
    np.testing.assert_allclose(tab, gold, rtol=0, atol=ATOL)
    # the filter as the kernel runs it, in place of scipy's
    np.testing.assert_allclose(LS.lane_table(route, case["i0"], case["L"], case["speed"], case["acc_max"], case["clamp_dt"], LS.filtfilt_restated),
                               gold, rtol=0, atol=ATOL)
    for p in case["poses"]:
        # the pose is next to waypoint i0: the global search and a window around a stale answer both find it
        assert LS.nearest(route[1], route[2], p["X"], p["Y"]) == case["i0"]
        assert LS.nearest(route[1], route[2], p["X"], p["Y"], max(case["i0"] - 3, 0), 2, 5) == case["i0"]
        i0, ref, err, stop = LS.waypoints(route, -1, p["X"], p["Y"], p["psi"], case["L"], 0, 0, case["H"], case["dt"], case["speed"],
                                          case["acc_max"], case["clamp_dt"])
        assert i0 == case["i0"] and stop == int(p["out"]["stop"])
        for row, key in zip(ref, LS.KEYS):
            np.testing.assert_allclose(row, np.array(p["out"][key]), rtol=0, atol=ATOL, err_msg=key)
        np.testing.assert_allclose(err, [p["out"][k] for k in ("s0", "e_y0", "e_psi0")], rtol=0, atol=ATOL)


def test_the_fixture_covers_the_route_end_and_the_stop_flag():
    ends = {(c["route"], c["i0"] + c["L"] - len(GOLD["routes"][c["route"]]["x"])) for c in GOLD["cases"]}
    assert (0, 0) in ends and (0, 1) in ends and any(e > 30 for _, e in ends) and any(e < 0 for _, e in ends)
    assert any(c["i0"] == len(GOLD["routes"][c["route"]]["x"]) - 1 for c in GOLD["cases"])          # a lane that is all padding
    assert any(c["H"] > c["L"] for c in GOLD["cases"]) and any(c["speed"] is None for c in GOLD["cases"])
    stops = [p["out"]["stop"] for c in GOLD["cases"] for p in c["poses"]]
    assert any(stops) and not all(stops)


@pytest.mark.parametrize("L", [34, 35, 63, 64, 65, 100, 256])
def test_filter_restatement_agrees_with_scipy(L):
    rng = np.random.default_rng(L)
    for x in (rng.normal(size=L), np.cumsum(rng.normal(size=L)) * 0.01, np.zeros(L), np.full(L, 0.37),
              np.concatenate((rng.normal(size=L - 30), np.full(30, 0.2)))):
        want = filtfilt(np.ones((11,)) / 11, 1, x)
        got = LS.filtfilt_restated(x)
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15 * max(1.0, float(np.abs(x).max())))


def test_search_rules():
    x, y = np.arange(10.0), np.zeros(10)
    assert LS.search_range(10, -1, 2, 3) == (0, 9) and LS.search_range(10, 4, 2, 3) == (2, 7)
    assert LS.search_range(10, 0, 2, 3) == (0, 3) and LS.search_range(10, 8, 2, 3) == (6, 9) and LS.search_range(10, 50, 2, 3) == (7, 9)
    assert LS.search_range(10, 5, 0, 0) == (5, 5)
    assert LS.nearest(x, y, 3.5, 1.0) == 3                           # an exact tie: the first index
    assert LS.nearest(x, y, 3.5, 1.0, 6, 2, 3) == 4                   # the window [4, 9] does not hold waypoint 3
    assert LS.nearest(x, y, np.nan, 0.0, 6, 2, 3) == 4 and LS.nearest(x, y, np.nan, 0.0) == 0
    assert LS.nearest(x, y, 0.0, np.inf, 6, 2, 3) == 4
    assert LS.bisector_clearance(x, y, 3.2, 5.0) == pytest.approx(0.3) and LS.bisector_clearance(x, y, 3.5, 1.0) == 0.0
    assert LS.bisector_clearance(np.zeros(4), np.zeros(4), 1.0, 1.0) == np.inf


def _declared():
    """name -> number of parameters, from include/admpc_lane.h with its comments stripped."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admpc_lane.h")).read(), flags=re.S)
    return {name: len(params.split(",")) for name, params in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_the_header_declares_exactly_the_new_functions():
    assert set(_declared()) == set(NEW)
    assert isinstance(_lib.LANE_EXPORTS, tuple) and set(_lib.LANE_EXPORTS) == set(NEW)
    assert not set(_lib.LANE_EXPORTS) & set(_lib.EXPORTS + _lib.QUAD_EXPORTS + _lib.FLEET_EXPORTS)
    for other in ("admpc.h", "admpc_quad.h", "admpc_fleet.h"):
        assert not re.search(r"admpc_\w*lane|AdmpcLane", open(os.path.join(ROOT, "include", other)).read()), other


def test_the_library_exports_each_new_function_with_the_declared_arity(lib):
    arity = _declared()
    assert arity == {"admpc_waypoints_lane_batch": 17, "admpc_control_step_lane_batch": 26}
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity[name] and fn.restype is C.c_int, name
    assert C.sizeof(AdmpcLaneParams) == 12 and [f[0] for f in AdmpcLaneParams._fields_] == ["L", "back", "ahead"]


def test_host_side_refusals_need_no_device(lib):
    """The checks in front of the first device call: reachable on a machine without a GPU."""
    idx = (C.c_int32 * 4)()
    idx_p = C.cast(idx, C.c_void_p)

    def gen(lane, lane_idx=idx_p, bank=None, B=4):
        return lib.admpc_waypoints_lane_batch(bank, lane, B, None, lane_idx, None, None, None, None, None, 1, 5.0, 0.05, None, None, None, None)

    def step(lane, lane_idx=idx_p, B=4):
        return lib.admpc_control_step_lane_batch(None, None, lane, None, B, None, lane_idx, *([None] * 19))

    def refused(rc, words):
        assert rc == -1 and words in lib.admpc_last_error().decode(), (rc, lib.admpc_last_error())

    ok = AdmpcLaneParams(L=64, back=8, ahead=64)
    for call, who in ((gen, "admpc_waypoints_lane_batch"), (step, "admpc_control_step_lane_batch")):
        refused(call(None), who + ": the lane parameters are not set")
        for L in (33, 257, 0, -1):
            refused(call(C.byref(AdmpcLaneParams(L=L, back=8, ahead=64))), "L must be in [34, 256]")
        refused(call(C.byref(AdmpcLaneParams(L=64, back=-1, ahead=64))), "back and ahead")
        refused(call(C.byref(AdmpcLaneParams(L=64, back=0, ahead=-2))), "back and ahead")
        refused(call(C.byref(ok), lane_idx=None), "null lane_idx")
        for L in (34, 256):                                           # the bounds themselves pass on to the next refusal
            assert call(C.byref(AdmpcLaneParams(L=L, back=0, ahead=0))) == -1
            assert "L must be" not in lib.admpc_last_error().decode()
    refused(gen(C.byref(ok)), "null bank")
    refused(step(C.byref(ok)), "null solver / params")
    assert list(idx) == [0, 0, 0, 0]
