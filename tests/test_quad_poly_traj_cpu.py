"""The polynomial trajectory generator without a GPU (include/admpc_quad_poly_traj.h): the keyframes of ad_mpc_amd/quad_keyframes.py and
the numpy spec against the reference's own keyframes, coefficients and trajectories (tests/golden/quad_poly_traj_vectors.json, written by
tests/gen_quad_poly_traj_golden.py), the two routes to the coefficients against each other, the float64 spec inside the forward error
bound, the library's lengths and weight matrix on the host, the refusals in their listed order, the registration of the unit."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import gen_quad_poly_traj_golden as GEN
import quad_poly_traj_spec as PS
from ad_mpc_amd import _lib
from ad_mpc_amd.quad_config import QUAD_POLY_TRAJ_KEYS, QUAD_TRAJ_MAX_M, quad_plant_params, quad_poly_traj_args
from ad_mpc_amd.quad_keyframes import random_keyframes, raw_keyframes, straight_keyframes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "quad_poly_traj_vectors.json")
with open(GOLDEN) as _f:
    GOLD = json.load(_f)
KEYFRAMES = {k["seed"]: {n: GEN.unpack(k[n], shape) for n, shape in (("raw", (10, 3)), ("adjusted", (10, 3)), ("coefficients", (9, 8, 4)))}
             for k in GOLD["keyframes"]}
DBL = C.POINTER(C.c_double)


def golden_case(c):
    """The spec's case of a stored one: its keyframes are the stored adjusted ones of its seed, the reference's three, or its own."""
    keys = KEYFRAMES[c["seed"]]["adjusted"] if c["kind"] == "random" else straight_keyframes() if c["kind"] == "straight" else np.array(c["keys"])
    return dict(keys=keys, speed=c["speed"], dt=c["dt"], quad=c["quad"])


CASES = [golden_case(c) for c in GOLD["cases"]]
IDS = ["%s%s-n%d-v%g-dt%g-%d" % (g["kind"], g.get("seed", ""), len(c["keys"]), c["speed"], c["dt"], i) for i, (g, c) in enumerate(zip(GOLD["cases"], CASES))]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def solve64():
    """The float64 spec by the reference's route of every golden case, computed once."""
    return [PS.generate(c) for c in CASES]


@pytest.fixture(scope="module")
def weights64():
    return [PS.generate(c, route="weights") for c in CASES]


@pytest.fixture(scope="module")
def spec80():
    return [PS.generate(c, ft=np.longdouble, route="weights") for c in CASES]


def _lib_lengths(lib, dt, keys, speed):
    keys = np.ascontiguousarray(keys, dtype=np.float64)
    s, M = C.c_int32(-7), C.c_int32(-7)
    rc = lib.admpc_quad_poly_traj_lengths(dt, len(keys), keys.ctypes.data_as(DBL), speed, C.byref(s), C.byref(M))
    return rc, s.value, M.value


# -- the golden file --------------------------------------------------------------------------------------------------------------------
def test_the_golden_file_holds_the_cases_the_issue_lists():
    assert os.path.getsize(GOLDEN) < GEN.SIZE_CAP
    assert {1, 2, 303} <= set(KEYFRAMES) and len(KEYFRAMES) >= 8
    rnd = {(g["seed"], g["speed"], g["dt"]) for g in GOLD["cases"] if g["kind"] == "random" and g["quad"] == PS.TS.DEFAULT_QUAD}
    assert {(sd, v, dt) for sd in (1, 2, 303) for v in (2.0, 3.5, 8.0) for dt in (0.02, 0.01)} <= rnd
    assert any(g["quad"] != PS.TS.DEFAULT_QUAD for g in GOLD["cases"])
    assert any(g["kind"] == "straight" and g["speed"] == 3.0 for g in GOLD["cases"])
    assert {4, 17, 32} <= {len(g["keys"]) for g in GOLD["cases"] if g["kind"] == "given"}
    for g, c in zip(GOLD["cases"], CASES):
        n_seg, s, M = len(c["keys"]) - 1, g["s"], g["M"]
        want = {0, 1, 2, M - 3, M - 2, M - 1} | {seg * s - 1 for seg in range(1, n_seg)} | {seg * s for seg in range(1, n_seg)}
        assert M == n_seg * s + 1 and want <= set(g["rows"]) and len(g["rows"]) >= len(want) + 8
    ties = [r for r in GOLD["rounding"] if (r[0] / r[1] / r[2]) % 1.0 == 0.5]
    assert len(ties) >= 50 and any(r[3] % 2 == 0 and r[3] < r[0] / r[1] / r[2] for r in ties) and any(r[3] > r[0] / r[1] / r[2] for r in ties)


# -- the keyframes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sorted(KEYFRAMES))
def test_keyframes_reproduce_the_reference(seed):
    """The curve of random_periodical_trajectory and the adjusted keyframes of random_trajectory within 1e-12 max(1, |value|); measured:
    0.0 for every stored seed (the same numpy and LAPACK calls in the same order)."""
    for got, want in ((raw_keyframes(seed), KEYFRAMES[seed]["raw"]), (random_keyframes(seed), KEYFRAMES[seed]["adjusted"])):
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        print("seed %d: %.3g" % (seed, err.max()))
        assert got.shape == (10, 3) and err.max() <= 1e-12
    k = random_keyframes(seed)
    assert k[0, 0] == 0.0 and k[0, 1] == 0.0 and (k[-1] == k[0]).all() and k[:, 2].min() >= 0.0


def test_straight_keyframes_and_the_python_arguments():
    assert straight_keyframes().tolist() == [[0.0, -3.0, 1.0], [0.0, 0.0, 1.0], [0.0, 3.0, 1.0]]
    keys, sp = quad_poly_traj_args(straight_keyframes(), 3.0)
    assert keys.shape == (1, 3, 3) and sp.tolist() == [3.0] and keys.flags.c_contiguous and keys.dtype == sp.dtype == np.float64
    keys, sp = quad_poly_traj_args(straight_keyframes(), [2.0, 3.0])
    assert keys.shape == (2, 3, 3) and sp.tolist() == [2.0, 3.0] and (keys[1] == straight_keyframes()).all()
    keys, sp = quad_poly_traj_args(np.zeros((4, 10, 3)), 3.5)
    assert keys.shape == (4, 10, 3) and sp.tolist() == [3.5] * 4
    for bad in ((np.zeros((4, 10, 3)), [1.0, 2.0]), (np.zeros((10, 2)), 1.0), (np.zeros(3), 1.0), (np.zeros((0, 10, 3)), 1.0), (np.zeros((2, 10, 3)), [[1.0, 2.0]])):
        with pytest.raises(ValueError):
            quad_poly_traj_args(*bad)
    assert QUAD_POLY_TRAJ_KEYS == (PS.MIN_KEYS, PS.MAX_KEYS) == (3, 32)


# -- the spec against the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sorted(KEYFRAMES))
def test_solve_route_reproduces_the_reference_coefficients(seed):
    """fit_multi_segment_polynomial_trajectory's coefficients (descending powers) within 1e-12 max(1, |value|); measured: 0.0."""
    want = KEYFRAMES[seed]["coefficients"]
    got = PS.coefficients(KEYFRAMES[seed]["adjusted"])[:, ::-1, :]
    assert not want[:, :, 3].any()
    assert (np.abs(got - want[:, :, :3]) <= 1e-12 * np.maximum(1.0, np.abs(want[:, :, :3]))).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_solve_route_reproduces_the_reference(i, solve64):
    """States and inputs within 1e-12 max(1, |value|) at the stored rows and in the per-column sums; measured: 1.1e-15 at most."""
    g = GOLD["cases"][i]
    traj, u = solve64[i]
    assert PS.lengths(g["dt"], CASES[i]["keys"], g["speed"]) == (g["s"], g["M"])
    assert traj.shape == (g["M"], 13) and u.shape == (g["M"], 4)
    full = np.concatenate([traj, u], axis=1)
    ref = GEN.unpack(g["values"], (-1, 17))
    err = np.abs(full[g["rows"]] - ref) / np.maximum(1.0, np.abs(ref))
    print("states %.3g inputs %.3g" % (err[:, :13].max(), err[:, 13:].max()))
    assert err.max() <= 1e-12
    sums, want = np.abs(full).sum(axis=0), GEN.unpack(g["abs_sums"])
    assert (np.abs(sums - want) <= 1e-12 * g["M"] * np.maximum(1.0, want / g["M"])).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_two_routes_agree_within_the_route_bound(i, solve64, weights64):
    """c = W p against np.linalg.solve, both pushed through the whole rule in float64: within route_bound (8 cond(M_fit) u max|c| per
    coefficient through the tail).  Measured: at most 4.1e-7 of it."""
    bound = PS.route_bound(CASES[i])
    diff = PS.group_errors(*weights64[i], *[a.astype(np.longdouble) for a in solve64[i]])
    for k in diff:
        print("%-10s %.3g / %.3g = %.2g" % (k, diff[k], bound[k], diff[k] / bound[k]))
        assert diff[k] <= bound[k]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_float64_spec_lies_within_the_error_bound(i, weights64, solve64, spec80):
    """The float64 spec by the device's route against the longdouble spec within error_bound (np.cumsum: depth M - 1), the same with the
    kernel's scan within the kernel's bound, and the reference's route within route_bound of the longdouble spec."""
    c = CASES[i]
    bound, bound_k, route = PS.error_bound(c, "serial"), PS.error_bound(c, "kernel"), PS.route_bound(c)
    err = PS.group_errors(*weights64[i], *spec80[i])
    mirror = PS.group_errors(*PS.generate(c, route="weights", scan=PS.TS.kernel_scan), *spec80[i])
    solve = PS.group_errors(*solve64[i], *spec80[i])
    for k in err:
        print("%-10s serial %.3g / %.3g = %.2g   kernel scan %.3g / %.3g = %.2g   solve %.3g / %.3g = %.2g" % (
            k, err[k], bound[k], err[k] / bound[k], mirror[k], bound_k[k], mirror[k] / bound_k[k], solve[k], route[k], solve[k] / route[k]))
        assert err[k] <= bound[k] and mirror[k] <= bound_k[k] and solve[k] <= route[k]
        assert bound_k[k] <= bound[k] <= route[k]


# -- the host entries -------------------------------------------------------------------------------------------------------------------
def test_lengths_of_the_library_are_the_reference_s(lib):
    for g, c in zip(GOLD["cases"], CASES):
        assert _lib_lengths(lib, c["dt"], c["keys"], c["speed"]) == (0, g["s"], g["M"])
    for av_dist, speed, dt, want in GOLD["rounding"]:
        keys = np.array([[0.0, 0.0, 1.0], [av_dist, 0.0, 1.0], [2 * av_dist, 0.0, 1.0]])     # both distances, and their mean, are av_dist exactly
        assert PS.av_dist(keys) == av_dist
        assert int(round(np.float64(av_dist) / speed / dt)) == want
        rc, s, M = _lib_lengths(lib, dt, keys, speed)
        if want < 1:
            assert rc == -1 and "s < 1" in lib.admpc_last_error().decode(), (av_dist, speed, dt)
        else:
            assert (rc, s, M) == (0, want, 2 * want + 1), (av_dist, speed, dt, s, want)


def test_refusals_of_the_lengths_entry(lib):
    good = straight_keyframes()
    s, M = C.c_int32(7), C.c_int32(7)
    p = good.ctypes.data_as(DBL)
    err = lambda: lib.admpc_last_error().decode()
    assert lib.admpc_quad_poly_traj_lengths(0.02, 3, None, 3.0, C.byref(s), C.byref(M)) == -1 and "null argument" in err()
    assert lib.admpc_quad_poly_traj_lengths(0.02, 3, p, 3.0, None, C.byref(M)) == -1 and "null argument" in err()
    assert lib.admpc_quad_poly_traj_lengths(0.02, 3, p, 3.0, C.byref(s), None) == -1 and "null argument" in err()
    bad = good.copy()
    bad[1, 2] = math.nan
    big = np.zeros((33, 3))
    for keys, n_key, speed, dt, what in ((bad, 2, -1.0, 0.0, "n_key must be"), (big, 33, -1.0, 0.0, "n_key must be"), (bad, 3, -1.0, 0.0, "not finite"),
                                         (good, 3, 0.0, 0.0, "speed must be"), (good, 3, math.inf, 0.0, "speed must be"), (good, 3, 1e9, -0.02, "dt must be positive"),
                                         (good, 3, 1e9, math.nan, "dt must be positive"), (good, 3, 1e9, 5e-4, "at least 1e-3"), (good, 3, 1e9, 0.02, "s < 1"),
                                         (good, 3, 1e-3, 0.02, "MAX_M"), (good, 3, 1e-300, 0.02, "MAX_M")):
        assert lib.admpc_quad_poly_traj_lengths(dt, n_key, keys.ctypes.data_as(DBL), speed, C.byref(s), C.byref(M)) == -1 and what in err(), what
    assert (s.value, M.value) == (7, 7)                                        # a refused call writes nothing
    # the cap itself is served, one segment row more is not: n_seg s + 1 = 16384 has the solutions n_seg = 3, s = 5461 and n_seg = 1
    keys = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0], [3.0, 0.0, 1.0]])
    assert _lib_lengths(lib, 0.02, keys, PS.speed_for(keys, 5461, 0.02)) == (0, 5461, QUAD_TRAJ_MAX_M)
    assert _lib_lengths(lib, 0.02, keys, PS.speed_for(keys, 5462, 0.02))[0] == -1 and "MAX_M" in err()


@pytest.mark.parametrize("n_key", [3, 4, 10, 17, 32])
def test_host_weights_are_the_longdouble_inverse(lib, n_key):
    """W of the library (Gauss-Jordan in long double, rounded to double) against the longdouble spec's within u cond(M_fit) max|W|, and W
    reproduces the keyframes: the polynomial of segment m passes through keyframe m at t = -1 and keyframe m + 1 at t = +1."""
    W = np.full((8 * (n_key - 1), n_key), np.nan)
    assert lib.admpc_quad_poly_traj_weights(n_key, W.ctypes.data_as(DBL)) == 0
    want = PS.weights(n_key)
    cond = PS.fit_cond(n_key)
    err = float(np.max(np.abs(W - want)))
    print("n_key %d: cond %.3g, |W| <= %.3g, error %.3g" % (n_key, cond, np.abs(want).max(), err))
    assert 1e4 < cond < 3e4 and err <= PS.U64 * cond * float(np.max(np.abs(want)))
    w = W.reshape(n_key - 1, 8, n_key)
    sign = (-1.0) ** np.arange(8)
    eye = np.eye(n_key)
    assert np.abs(np.einsum("sak,a->sk", w, sign) - eye[:-1]).max() <= 64 * PS.U64 * np.abs(w).sum(axis=1).max()
    assert np.abs(w.sum(axis=1) - eye[1:]).max() <= 64 * PS.U64 * np.abs(w).sum(axis=1).max()


def test_refusals_of_the_weights_entry(lib):
    W = np.zeros((8 * 31, 32))
    assert lib.admpc_quad_poly_traj_weights(3, None) == -1 and "null argument" in lib.admpc_last_error().decode()
    for n_key in (2, 33, -1):
        assert lib.admpc_quad_poly_traj_weights(n_key, W.ctypes.data_as(DBL)) == -1 and "n_key must be" in lib.admpc_last_error().decode()


# -- the refusals of the generator, in the listed order -------------------------------------------------------------------------------------
def _generate(lib, keys, speed, plant, dt, K=None, n_key=None, device=0, null=None):
    keys = np.ascontiguousarray(keys, dtype=np.float64)
    speed = np.ascontiguousarray(speed, dtype=np.float64)
    h = C.c_void_p(0)
    rc = lib.admpc_quad_poly_traj_bank_generate(device, keys.shape[0] if K is None else K, keys.shape[1] if n_key is None else n_key,
                                                None if null == "keys" else keys.ctypes.data_as(DBL), None if null == "speed" else speed.ctypes.data_as(DBL),
                                                None if null == "plant" else C.byref(plant), dt, None, None if null == "bank" else C.byref(h))
    assert not h.value
    return rc, lib.admpc_last_error().decode()


def test_refusals_come_in_the_listed_order_before_any_device_call(lib):
    """Each call carries the fault under test AND every fault listed behind it; the message names the first.  A fault of one kind in the
    second trajectory comes in front of a later kind's in the first.  No GPU is needed: every refusal is raised in front of the first
    device call."""
    plant = quad_plant_params(None, 5e-4, 0.02)
    bad_plant = plant.copy()
    bad_plant.mass = 0.0
    good = straight_keyframes()
    nan_keys = good.copy()
    nan_keys[2, 0] = math.inf
    two = lambda a, b: np.stack([a, b])
    FAST, SLOW = 1e9, 1e-3                              # s = 0; M past the cap at dt = 0.02
    steps = [
        (dict(keys=two(nan_keys, nan_keys), speed=[-1.0, -1.0], dt=-1.0, null="bank", K=0, n_key=2), "null argument"),
        (dict(keys=two(nan_keys, nan_keys), speed=[-1.0, -1.0], dt=-1.0, null="keys", K=0, n_key=2), "null argument"),
        (dict(keys=two(nan_keys, nan_keys), speed=[-1.0, -1.0], dt=-1.0, null="speed", K=0, n_key=2), "null argument"),
        (dict(keys=two(nan_keys, nan_keys), speed=[-1.0, -1.0], dt=-1.0, null="plant", K=0, n_key=2), "null argument"),
        (dict(keys=two(nan_keys, nan_keys), speed=[-1.0, -1.0], dt=-1.0, K=0, n_key=2), "K must be at least 1"),
        (dict(keys=two(nan_keys, nan_keys), speed=[-1.0, -1.0], dt=-1.0, n_key=2), "n_key must be in [3, 32]"),
        (dict(keys=two(nan_keys, nan_keys), speed=[-1.0, -1.0], dt=-1.0, n_key=33), "n_key must be in [3, 32]"),
        (dict(keys=two(good, nan_keys), speed=[-1.0, 3.0], dt=-1.0), "keyframe coordinate is not finite"),
        (dict(keys=two(good, good), speed=[3.0, 0.0], dt=-1.0), "speed must be positive"),
        (dict(keys=two(good, good), speed=[3.0, math.nan], dt=-1.0), "speed must be positive"),
        (dict(keys=two(good, good), speed=[math.inf, 3.0], dt=-1.0), "speed must be positive"),
        (dict(keys=two(good, good), speed=[SLOW, FAST], dt=0.0), "dt must be positive"),
        (dict(keys=two(good, good), speed=[SLOW, FAST], dt=math.nan), "dt must be positive"),
        (dict(keys=two(good, good), speed=[SLOW, FAST], dt=math.inf), "dt must be positive"),
        (dict(keys=two(good, good), speed=[SLOW, FAST], dt=9.9e-4), "dt must be at least 1e-3"),
        (dict(keys=two(good, good), speed=[SLOW, FAST], dt=0.02), "s < 1"),
        (dict(keys=two(good, good), speed=[3.0, SLOW], dt=0.02), "ADMPC_QUAD_TRAJ_MAX_M"),
        (dict(keys=two(good, good), speed=[3.0, 1e-300], dt=0.02), "ADMPC_QUAD_TRAJ_MAX_M"),
        (dict(keys=two(good, good), speed=[3.0, 2.0], dt=0.02), "mass, J and max_thrust"),
    ]
    for kw, what in steps:
        rc, msg = _generate(lib, kw.pop("keys"), kw.pop("speed"), bad_plant, kw.pop("dt"), **kw)
        assert rc == -1 and what in msg and msg.startswith("admpc_quad_poly_traj_bank_generate: "), (what, rc, msg)
    for field, value in (("mass", -1.0), ("mass", math.nan), ("max_thrust", 0.0), ("J", (0.03, 0.0, 0.06))):
        p = plant.copy()
        setattr(p, field, (C.c_double * 3)(*value) if field == "J" else value)
        rc, msg = _generate(lib, two(good, good), [3.0, 2.0], p, 0.02)
        assert rc == -1 and "mass, J and max_thrust" in msg and msg.startswith("admpc_quad_poly_traj_bank_generate: "), (field, value, msg)
    p = plant.copy()
    for m in range(4):
        p.z_l_tau[m] = 0.0                                                     # a singular arm matrix, behind the plant's values
    rc, msg = _generate(lib, two(good, good), [3.0, 2.0], p, 0.02, device=10 ** 6)
    assert rc == -1 and "singular" in msg
    rc, msg = _generate(lib, two(good, good), [3.0, 2.0], plant, 0.02, device=10 ** 6)          # behind all of them: no such device
    assert rc == -2 and "no such device" in msg


# -- the registration ---------------------------------------------------------------------------------------------------------------------
def _declared_arity(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    return {name: 0 if params.strip() in ("", "void") else len(params.split(","))
            for name, params in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}


def test_the_table_of_the_new_header_has_the_declared_names_and_arity(lib):
    assert list(_lib.POLY_TRAJ_TABLES) == ["admpc_quad_poly_traj.h"]
    table = _lib.POLY_TRAJ_TABLES["admpc_quad_poly_traj.h"]
    assert tuple(table) == _lib.QUAD_POLY_TRAJ_EXPORTS
    arity = _declared_arity("admpc_quad_poly_traj.h")
    assert set(arity) == set(table) and len(table) == 3
    for name in table:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == arity[name], name
    others = [n for t in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES, _lib.TARGET_TABLES,
                          _lib.PRUNE_TABLES, _lib.EVAL_TABLES, _lib.TRAJ_TABLES) for tab in t.values() for n in tab]
    assert not set(others) & set(table)                                        # no name is declared by two headers
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_poly_traj.h")).read()
    assert (int(re.search(r"#define\s+ADMPC_QUAD_POLY_TRAJ_MIN_KEYS\s+(\d+)", hdr).group(1)),
            int(re.search(r"#define\s+ADMPC_QUAD_POLY_TRAJ_MAX_KEYS\s+(\d+)", hdr).group(1))) == QUAD_POLY_TRAJ_KEYS
    for word in ("THE RULE", "THE MAPPING", "trajectories.py:307-321", "trajectory_generator.py:91-144", "147-213, 255-265"):
        assert word in hdr, word
    old = open(os.path.join(ROOT, "include", "admpc_quad_traj.h")).read()
    assert "random_trajectory and the map" not in old and "admpc_quad_poly_traj.h" in old      # random trajectories are offered now


def test_the_makefile_builds_the_unit():
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    units = [u for line in re.findall(r"^UNITS\s*\+?=\s*(.*)$", mk, flags=re.M) for u in line.split()]
    assert units[-1] == "admpc_quad_poly_traj" and len(units) == len(set(units)) == 22
    hdrs = re.search(r"^HDRS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "../../include/admpc_quad_poly_traj.h" in hdrs and "quad_traj_tail_dev.h" in hdrs
    assert re.search(r"^#\s+admpc_quad_poly_traj\.hip\s", mk, flags=re.M)
    for unit in ("admpc_quad_traj.hip", "admpc_quad_poly_traj.hip"):           # ONE text of the passes B, C, D: neither unit has its own
        src = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", unit)).read()
        assert '#include "quad_traj_tail_dev.h"' in src and "quad_traj_tail(M, dt, gp, Xk, Uk, s_row, s_tot, s_carry);" in src
        assert "pass B:" not in src and "pass C:" not in src and "pass D:" not in src
