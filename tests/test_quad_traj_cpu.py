"""The trajectory generator without a GPU (include/admpc_quad_traj.h): the numpy spec against the reference's own trajectories
(tests/golden/quad_traj_vectors.json, written by tests/gen_quad_traj_golden.py), the phase lengths of the spec AND of the library against
the reference's np.arange, the float64 spec inside the forward error bound, the refusals in their listed order, the prototypes."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import quad_traj_spec as TS
from ad_mpc_amd import _lib
from ad_mpc_amd.quad_config import AdmpcQuadPlantParams, AdmpcQuadTrajSpec, QUAD_TRAJ_MAX_M, quad_plant_params, quad_traj_specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "quad_traj_vectors.json")) as _f:
    GOLD = json.load(_f)
CASES = GOLD["cases"]
IDS = ["%s-v%g-dt%g-%d" % (c["kind"], c["v_max"], c["dt"], i) for i, c in enumerate(CASES)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def spec64():
    """The float64 spec of every golden case, computed once."""
    return [TS.generate(c) for c in CASES]


@pytest.fixture(scope="module")
def spec80():
    return [TS.generate(c, ft=np.longdouble) for c in CASES]


def _spec(case):
    s = AdmpcQuadTrajSpec()
    s.kind, s.clockwise = {"loop": 0, "lemniscate": 1}[case["kind"]], 1 if case["clockwise"] else 0
    s.radius, s.z, s.lin_acc, s.v_max = case["radius"], case["z"], case["lin_acc"], case["v_max"]
    return s


def _lib_lengths(lib, dt, s):
    n = (C.c_int32 * 5)()
    rc = lib.admpc_quad_traj_lengths(dt, C.byref(s), n)
    return rc, list(n)


# -- the golden file ------------------------------------------------------------------------------------------------------------------
def test_the_golden_file_holds_the_cases_the_generator_lists():
    kinds = {(c["kind"], c["v_max"], c["dt"]) for c in CASES if c["clockwise"] and c["radius"] == 5.0 and c["lin_acc"] == 0.25 * c["v_max"]}
    assert {(k, v, dt) for k in ("loop", "lemniscate") for v in (2.0, 7.0, 12.0) for dt in (0.02, 0.01)} <= kinds
    assert any(c["kind"] == "loop" and not c["clockwise"] for c in CASES)
    assert any(c["radius"] != 5.0 and c["lin_acc"] != 0.25 * c["v_max"] for c in CASES)
    assert any(c["quad"] != TS.DEFAULT_QUAD for c in CASES)
    assert len(GOLD["lengths"]) >= 200
    for c in CASES:
        M, n = c["M"], c["n"]
        edges = np.cumsum(n)[:4]
        want = {0, 1, 2, M - 3, M - 2, M - 1} | {int(e) - 1 for e in edges} | {int(e) for e in edges}
        assert want <= set(c["rows"]) and len(c["rows"]) >= len(want) + 8 and sum(n) == M
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "quad_traj_vectors.json")) < \
        0.75 * os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_traj.json"))


# -- the lengths ----------------------------------------------------------------------------------------------------------------------
def test_lengths_of_the_spec_and_of_the_library_are_numpy_aranges(lib):
    exact = 0
    for dt, v_max, lin_acc, *n in GOLD["lengths"]:
        case = {"v_max": v_max, "lin_acc": lin_acc}
        assert TS.lengths(dt, case) == n, (dt, v_max, lin_acc)
        s = _spec(dict(case, kind="loop", clockwise=True, radius=5.0, z=1.0))
        rc, got = _lib_lengths(lib, dt, s)
        if sum(n) > QUAD_TRAJ_MAX_M:
            assert rc != 0
        else:
            assert rc == 0 and got == n, (dt, v_max, lin_acc, got, n)
        exact += dt in (0.02, 0.01, 0.05, 0.1, 0.25) and v_max / lin_acc in (2.5, 3.0, 4.0, 6.5)
    assert exact >= 20                                   # the triples whose quotients are integers in exact arithmetic are there
    for c in CASES:
        assert TS.lengths(c["dt"], c) == c["n"] and _lib_lengths(lib, c["dt"], _spec(c)) == (0, c["n"])


# -- the spec against the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_spec_reproduces_the_reference(i, spec64):
    """States and inputs within 1e-12 max(1, |value|) at the stored rows and in the per-column sums; measured: 0.0 and 5.6e-16."""
    c = CASES[i]
    traj, u = spec64[i]
    assert traj.shape == (c["M"], 13) and u.shape == (c["M"], 4)
    full = np.concatenate([traj, u], axis=1)
    ref = np.array(c["values"])
    err = np.abs(full[c["rows"]] - ref) / np.maximum(1.0, np.abs(ref))
    print("states %.3g inputs %.3g" % (err[:, :13].max(), err[:, 13:].max()))
    assert err.max() <= 1e-12
    sums, want = np.abs(full).sum(axis=0), np.array(c["abs_sums"])
    assert (np.abs(sums - want) <= 1e-12 * c["M"] * np.maximum(1.0, want / c["M"])).all()


def test_the_yaw_sum_may_start_at_row_0_or_1():
    """The reference's yaw sum starts at row 1.  Starting it at row 0 gives the same trajectory: alpha[0] = 0 makes q[0] the identity,
    q.z is 0 in every row before the correction, so the first pass' w0[0].z is an exact 0 -- the one mutation of the issue's list that no
    test can see."""
    for c in CASES:
        _, _, parts = TS.generate(c, parts=True)
        assert parts["alpha"][0] == 0.0 and parts["w0"][0, 2] == 0.0


def test_the_scan_mirror_is_an_inclusive_scan():
    rng = np.random.RandomState(5)
    for M in (1, 63, 64, 65, 255, 256, 257, 600, 1200):
        v = rng.standard_normal(M)
        got, want = TS.kernel_scan(v), np.cumsum(v)
        assert got.shape == want.shape and np.abs(got - want).max() <= 64 * TS.U64 * np.abs(v).sum()
    v = np.arange(1.0, 601.0)                            # integers: every order of the additions is exact
    assert (TS.kernel_scan(v) == np.cumsum(v)).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_float64_spec_lies_within_the_error_bound(i, spec64, spec80):
    """The float64 spec with np.cumsum (depth M - 1) and with the kernel's scan (depth 10 per tile) against the longdouble spec."""
    c = CASES[i]
    err = TS.group_errors(*spec64[i], *spec80[i])
    bound = TS.error_bound(c, "serial")
    mirror = TS.group_errors(*TS.generate(c, scan=TS.kernel_scan), *spec80[i])
    bound_k = TS.error_bound(c, "kernel")
    for k in err:
        print("%-10s serial %.3g / %.3g = %.2g   kernel scan %.3g / %.3g = %.2g" % (k, err[k], bound[k], err[k] / bound[k], mirror[k], bound_k[k],
                                                                                  mirror[k] / bound_k[k]))
        assert err[k] <= bound[k] and mirror[k] <= bound_k[k]
        assert bound_k[k] <= bound[k]


# -- the refusals, in the listed order ----------------------------------------------------------------------------------------------------
def _generate(lib, specs, plant, dt, K=None, device=0, null=None):
    arr = (AdmpcQuadTrajSpec * len(specs))(*specs)
    h = C.c_void_p(0)
    rc = lib.admpc_quad_traj_bank_generate(device, len(specs) if K is None else K, None if null == "specs" else arr,
                                           None if null == "plant" else C.byref(plant), dt, None, None if null == "bank" else C.byref(h))
    assert not h.value
    return rc, lib.admpc_last_error().decode()


def _good():
    return _spec(dict(kind="loop", clockwise=True, radius=5.0, z=1.0, lin_acc=1.0, v_max=4.0))


def _set(s, **kw):
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_refusals_come_in_the_listed_order_before_any_device_call(lib):
    """Each call carries the fault under test AND every fault listed behind it; the message names the first.  No GPU is needed: every
    refusal is raised in front of the first device call."""
    plant = quad_plant_params(None, 5e-4, 0.02)
    bad_plant = plant.copy()
    bad_plant.mass = 0.0
    capped = _set(_good(), lin_acc=1.0, v_max=400.0)                           # M past the cap at dt = 0.02
    empty = _set(_good(), lin_acc=2.0, v_max=4.0)                              # v_max / lin_acc = 2 exactly
    steps = [
        (dict(specs=[_set(_good(), kind=2)], null="bank", K=0, dt=-1.0), "null argument"),
        (dict(specs=[_set(_good(), kind=2)], null="specs", K=0, dt=-1.0), "null argument"),
        (dict(specs=[_set(_good(), kind=2)], null="plant", K=0, dt=-1.0), "null argument"),
        (dict(specs=[_set(_good(), kind=2)], K=0, dt=-1.0), "K must be at least 1"),
        (dict(specs=[_good(), _set(_good(), kind=2, radius=-1.0)], dt=-1.0), "kind must be"),
        (dict(specs=[_good(), _set(_good(), kind=-1)], dt=-1.0), "kind must be"),
        (dict(specs=[_set(_good(), clockwise=2)], dt=-1.0), "clockwise must be"),
        (dict(specs=[_good(), _set(_good(), radius=0.0)], dt=-1.0), "must be positive and finite"),
        (dict(specs=[_set(_good(), z=-1.0)], dt=-1.0), "radius, z, lin_acc and v_max"),
        (dict(specs=[_set(_good(), lin_acc=math.inf)], dt=-1.0), "radius, z, lin_acc and v_max"),
        (dict(specs=[_set(_good(), v_max=math.nan)], dt=-1.0), "radius, z, lin_acc and v_max"),
        (dict(specs=[empty, capped], dt=0.0), "dt must be positive"),
        (dict(specs=[empty, capped], dt=math.nan), "dt must be positive"),
        (dict(specs=[empty, capped], dt=math.inf), "dt must be positive"),
        (dict(specs=[capped, empty], dt=0.02), "coasting phase is empty"),
        (dict(specs=[_set(_good(), lin_acc=2.0, v_max=3.0), capped], dt=0.02), "coasting phase is empty"),
        (dict(specs=[_good(), capped], dt=0.02), "ADMPC_QUAD_TRAJ_MAX_M"),
        (dict(specs=[_good()], dt=0.02), "mass, J and max_thrust"),
    ]
    for kw, what in steps:
        rc, msg = _generate(lib, kw.pop("specs"), bad_plant, kw.pop("dt"), **kw)
        assert rc == -1 and what in msg and msg.startswith("admpc_quad_traj_bank_generate: "), (what, rc, msg)
    for field, value in (("mass", -1.0), ("mass", math.nan), ("max_thrust", 0.0), ("J", (0.03, 0.0, 0.06))):
        p = plant.copy()
        setattr(p, field, (C.c_double * 3)(*value) if field == "J" else value)
        rc, msg = _generate(lib, [_good()], p, 0.02)
        assert rc == -1 and "mass, J and max_thrust" in msg, (field, value, msg)
    p = plant.copy()
    for m in range(4):
        p.z_l_tau[m] = 0.0                                                     # a singular arm matrix, behind the plant's values
    rc, msg = _generate(lib, [_good()], p, 0.02)
    assert rc == -1 and "singular" in msg


def test_refusals_of_the_lengths_entry(lib):
    n = (C.c_int32 * 5)(7, 7, 7, 7, 7)
    good = _good()
    assert lib.admpc_quad_traj_lengths(0.02, None, n) == -1 and "null argument" in lib.admpc_last_error().decode()
    assert lib.admpc_quad_traj_lengths(0.02, C.byref(good), None) == -1 and "null argument" in lib.admpc_last_error().decode()
    for s, dt, what in ((_set(_good(), kind=5, z=0.0), 0.0, "kind must be"), (_set(_good(), z=0.0), 0.0, "radius, z"), (good, -0.02, "dt must be"),
                        (_set(_good(), lin_acc=2.0, v_max=4.0), 0.02, "coasting"), (_set(_good(), lin_acc=2.0, v_max=3.9), 0.02, "coasting"),
                        (_set(_good(), v_max=400.0), 0.02, "MAX_M")):
        assert lib.admpc_quad_traj_lengths(dt, C.byref(s), n) == -1 and what in lib.admpc_last_error().decode(), what
    assert list(n) == [7] * 5                                                  # a refused call writes nothing
    # the cap itself is served, one row more is not
    dt, r, want = TS.find_case(QUAD_TRAJ_MAX_M, [0.005, 0.004, 0.0025, 0.002, 0.001], [2.5 + 0.001 * i for i in range(40000)])
    assert _lib_lengths(lib, dt, _set(_good(), lin_acc=1.0, v_max=r)) == (0, want) and sum(want) == QUAD_TRAJ_MAX_M
    dt, r, want = TS.find_case(QUAD_TRAJ_MAX_M + 1, [0.0013, 0.0007], [2.5 + 0.001 * i for i in range(40000)])     # 4 / dt is not an integer: M can be odd
    assert sum(want) == QUAD_TRAJ_MAX_M + 1 and _lib_lengths(lib, dt, _set(_good(), lin_acc=1.0, v_max=r))[0] == -1
    assert "MAX_M" in lib.admpc_last_error().decode()


def test_the_info_copy_and_rows_entries_refuse_a_null_bank(lib):
    assert lib.admpc_quad_traj_bank_info(None, None, None, None) == -1 and "null bank" in lib.admpc_last_error().decode()
    assert lib.admpc_quad_traj_bank_copy(None, 0, None, None) == -1 and "null bank" in lib.admpc_last_error().decode()
    assert lib.admpc_quad_traj_rows_batch(None, 1, None, None, None, None, None) == -1 and "null bank" in lib.admpc_last_error().decode()


# -- the Python side's own arguments ------------------------------------------------------------------------------------------------------
def test_specs_from_scalars_and_sequences():
    s = quad_traj_specs("loop", 8.0)
    assert len(s) == 1 and (s[0].kind, s[0].clockwise, s[0].radius, s[0].z, s[0].lin_acc, s[0].v_max) == (0, 1, 5.0, 1.0, 2.0, 8.0)
    s = quad_traj_specs(["loop", "lemniscate", "loop"], [2.0, 4.5, 12.0], radius=3.0, lin_acc=[None, 1.5, None], clockwise=[True, False, True])
    assert [(t.kind, t.clockwise, t.radius, t.lin_acc, t.v_max) for t in s] == [(0, 1, 3.0, 0.5, 2.0), (1, 0, 3.0, 1.5, 4.5), (0, 1, 3.0, 3.0, 12.0)]
    assert C.sizeof(AdmpcQuadTrajSpec) == 40 and C.sizeof(AdmpcQuadPlantParams) == 216
    for bad in (dict(kind="circle", v_max=2.0), dict(kind=["loop", "loop"], v_max=[1.0, 2.0, 3.0]), dict(kind=[], v_max=2.0)):
        with pytest.raises(ValueError):
            quad_traj_specs(**bad)


# -- the prototypes ---------------------------------------------------------------------------------------------------------------------
def _declared_arity(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    return {name: 0 if params.strip() in ("", "void") else len(params.split(","))
            for name, params in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}


def test_the_table_of_the_new_header_has_the_declared_names_and_arity(lib):
    assert list(_lib.TRAJ_TABLES) == ["admpc_quad_traj.h"] and tuple(_lib.TRAJ_TABLES["admpc_quad_traj.h"]) == _lib.QUAD_TRAJ_EXPORTS
    arity = _declared_arity("admpc_quad_traj.h")
    table = _lib.TRAJ_TABLES["admpc_quad_traj.h"]
    assert set(arity) == set(table) and len(table) == 5
    for name in table:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == arity[name], name
    others = [n for t in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES, _lib.TARGET_TABLES,
                          _lib.PRUNE_TABLES, _lib.EVAL_TABLES) for tab in t.values() for n in tab]
    assert not set(others) & set(table)                                        # no name is declared by two headers
    m = re.search(r"#define\s+ADMPC_QUAD_TRAJ_MAX_M\s+(\d+)", open(os.path.join(ROOT, "include", "admpc_quad_traj.h")).read())
    assert int(m.group(1)) == QUAD_TRAJ_MAX_M == TS.MAX_M >= 8192


def test_the_makefile_builds_the_unit():
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    units = re.search(r"^UNITS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "admpc_quad_traj" in units and len(units) == 21 and "Twenty-one translation units" in mk
    assert "../../include/admpc_quad_traj.h" in re.search(r"^HDRS\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
