"""The quadrotor's closed loop (include/admpc_quad_fleet.h) without a GPU: the header and the prototype table; the numpy spec of the plant
step (tests/quad_plant_spec.py) against the reference's own simulator, live where the reference tree is present and through the golden
vectors everywhere; the closed form of the reference window against the reference's text restated; the sub-step count; the refusals of
the Python layer."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gen_quad_plant_golden as GG
import quad_plant_spec as QS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"admpc_quad_plant_step_batch": 7, "admpc_quad_traj_bank_create": 6, "admpc_quad_traj_bank_destroy": 1, "admpc_quad_ref_chunk_batch": 10,
         "admpc_quad_rollout_batch": 21, "admpc_quad_solver_info": 4}


def _plant(drag=False, payload=False, substeps=1, dt=GG.DT):
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    p = quad_plant_params(SimQuad(drag=drag, payload=payload), dt, dt)
    p.substeps = substeps
    return p


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree():
    from ad_mpc_amd import _lib
    from ad_mpc_amd.quad_config import AdmpcQuadPlantParams
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "admpc_quad_fleet.h")).read(), flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_FLEET_EXPORTS, tuple) and list(_lib.QUAD_FLEET_EXPORTS) == list(ARITY)
    others = _lib.EXPORTS + _lib.QUAD_EXPORTS + _lib.FLEET_EXPORTS + _lib.LANE_EXPORTS + _lib.PLANT_EXPORTS + _lib.LEARN_EXPORTS + _lib.HYPER_EXPORTS
    assert not set(_lib.QUAD_FLEET_EXPORTS) & set(others)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    for name, n in ARITY.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == n and fn.restype is (None if name.endswith("_destroy") else C.c_int), name
    assert C.sizeof(AdmpcQuadPlantParams) == 216
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_fleet.h")).read()
    for cite in ("quad_3d.py:175-220", "quad_3d_opt_utils.py:267-296", "quad_3d_optimizer.py:465-503", "trajectory_test.py:94-127", "trajectory_test.py:137"):
        assert cite in hdr, cite
    assert "noisy" in hdr and "motor_noise" in hdr and "NOT offered" in hdr
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_fleet\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_fleet\.h", mk, flags=re.M)


def test_refusals_in_front_of_the_device():
    """Every refusal of the plant parameters and of the batch arguments comes back without a device (this machine has none)."""
    from ad_mpc_amd import _lib
    L = _lib.load()

    def refused(rc, words):
        assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

    x = (C.c_double * 13)()
    call = lambda p, B=1, u=x, stride=4, xx=x: L.admpc_quad_plant_step_batch(None if p is None else C.byref(p), 0, B, u, stride, xx, None)
    refused(call(None), "plant parameters are not set")
    for kw, words in ((dict(dt=0.0), "dt must be"), (dict(dt=float("nan")), "dt must be"), (dict(substeps=0), "substeps must be in [1, 1024]"),
                      (dict(substeps=1025), "substeps must be in [1, 1024]"), (dict(mass=0.0), "mass and J"), (dict(u_min=2.0), "u_min <= u_max"),
                      (dict(u_max=float("inf")), "u_min <= u_max"), (dict(drag=2), "drag must be 0 or 1")):
        p = _plant()
        for k, v in kw.items():
            setattr(p, k, v)
        refused(call(p), words)
    p = _plant()
    p.dt, p.substeps = -1.0, 0                                   # the order: dt before substeps
    refused(call(p), "dt must be")
    p = _plant()
    refused(call(p, B=-1), "negative batch")
    assert call(p, B=0, u=None, xx=None) == 0
    refused(call(p, u=None), "null array")
    refused(call(p, stride=3), "u_stride must be at least 4")
    refused(L.admpc_quad_ref_chunk_batch(None, 1, 10, 5, None, None, None, None, None, None), "null bank")
    refused(L.admpc_quad_rollout_batch(None, None, C.byref(p), 5, 1, 1, *([None] * 15)), "null solver")
    h = C.c_void_p(0)
    M = (C.c_int32 * 1)(0)
    ptr = (C.c_void_p * 1)(C.addressof(x))
    refused(L.admpc_quad_traj_bank_create(0, 1, M, ptr, ptr, C.byref(h)), "M >= 1")
    refused(L.admpc_quad_traj_bank_create(0, 0, M, ptr, ptr, C.byref(h)), "K must be at least 1")
    refused(L.admpc_quad_solver_info(None, None, None, None), "null solver")


# ---- the Python helpers -------------------------------------------------------------------------------------------------------------

def test_substeps_are_counted_by_the_reference_loop():
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params, quad_substeps
    assert [quad_substeps(5e-4, 1.0 / (N * 5)) for N in (10, 20, 5)] == [40, 20, 80]
    assert quad_substeps(0.3, 1.0) == 4 and quad_substeps(1.0, 1.0) == 1 and quad_substeps(2.0, 1.0) == 1
    for bad in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (1e-6, 1.0), (1.0, 0.0)):
        with pytest.raises(ValueError):
            quad_substeps(*bad)
    p = quad_plant_params(SimQuad(drag=True, payload=True), 5e-4, 0.02)
    assert (p.substeps, p.dt, p.drag, p.payload_mass, p.aero_drag, p.g, p.u_min, p.u_max) == (40, 5e-4, 1, 0.3, 0.08, 9.81, 0.0, 1.0)
    assert list(p.rotor_drag) == [0.3, 0.3, 0.0] and list(p.J) == [0.03, 0.03, 0.06] and p.max_thrust == 20.0
    q = quad_plant_params(None, 5e-4, 0.01)
    assert q.substeps == 20 and q.drag == 0 and q.payload_mass == 0.0 and list(q.x_f) == list(p.x_f)


def test_random_disturbances_are_refused():
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    for attr in ("noisy", "motor_noise"):
        quad = SimQuad()
        setattr(quad, attr, True)
        with pytest.raises(NotImplementedError, match="random disturbances"):
            quad_plant_params(quad, 5e-4, 0.02)
        from ad_mpc_amd.quad_fleet import QuadFleet
        with pytest.raises(NotImplementedError, match="random disturbances"):
            QuadFleet(4, quad=quad)                              # refused before a handle (and so a GPU) is asked for


def test_clustered_ensembles_are_refused():
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    from ad_mpc_amd.quad_fleet import fleet_quad_config
    with pytest.raises(NotImplementedError, match="clustered"):
        fleet_quad_config(gp_regressors=QuadGPEnsemble([[], []], np.zeros((2, 1)), [7]))
    cfg = fleet_quad_config(n_nodes=20, t_horizon=2.0)
    assert cfg.N == 20 and cfg.Ts == 0.1 and cfg.sqp_iters == 1 and list(cfg.W[:7]) == [10, 10, 10, float(np.mean([0.1, 0.1, 0.1])), 0.1, 0.1, 0.1] and cfg.We[0] == 0.0


def test_circle_reference_is_consistent():
    """The rows satisfy the simulator's own model without drag: the spec's derivative at row i under u[i] gives the circle's velocity and
    centripetal acceleration, and a unit quaternion at yaw 0."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    traj, u = circle_reference(120, 0.02, 5.0, 3.0)
    assert traj.shape == (120, 13) and u.shape == (120, 4) and (u > 0.05).all() and (u < 0.5).all()
    assert np.abs(np.linalg.norm(traj[:, 3:7], axis=1) - 1).max() < 1e-15 and np.abs(np.linalg.norm(traj[:, 0:2], axis=1) - 5.0).max() < 1e-12
    p = _plant()
    for i in (0, 37, 119):
        s = [traj[i, 0:3], traj[i, 3:7], traj[i, 7:10], traj[i, 10:13]]
        k = QS.deriv(p, s, u[i] * p.max_thrust)
        acc = -traj[i, 0:3] * (3.0 / 5.0) ** 2; acc[2] = 0.0
        assert np.abs(k[2] - acc).max() < 1e-9, (i, k[2], acc)
        assert np.abs(np.diff(traj[:, 0:3], axis=0)[min(i, 118)] / 0.02 - traj[i, 7:10]).max() < 0.05


# ---- the plant spec against the reference's simulator -------------------------------------------------------------------------------

@pytest.mark.skipif(not GG.reference_present(), reason="the reference tree is not on this machine")
def test_spec_equals_the_live_reference_simulator():
    ref = GG.load_reference()
    X, U = GG.inputs()
    assert (U < 0).any() and (U > 1).any() and X[5, 8] == 0.0
    worst = 0.0
    for drag, payload, substeps in GG.CASES:
        want = GG.run_reference(ref, drag, payload, substeps, X, U)
        got, replaced = QS.step_batch(_plant(drag, payload, substeps), X, U)
        assert not replaced.any() and np.isfinite(want).all()
        worst = max(worst, _rel(got, want))
        assert np.abs(want - X).max() > 1e-4
    print("spec against Quadrotor3D.update: largest relative difference %.3g" % worst)
    assert worst <= 1e-15


def test_spec_equals_the_golden_vectors():
    with open(GG.OUT) as f:
        doc = json.load(f)
    X, U = np.array(doc["x"]), np.array(doc["u"])
    Xg, Ug = GG.inputs()
    assert np.array_equal(X, Xg) and np.array_equal(U, Ug) and doc["dt"] == GG.DT
    assert [(c["drag"], c["payload"], c["substeps"]) for c in doc["cases"]] == GG.CASES
    for c in doc["cases"]:
        got, _ = QS.step_batch(_plant(c["drag"], c["payload"], c["substeps"]), X, U)
        assert _rel(got, np.array(c["result"])) <= 1e-15, c["substeps"]
    a, b = (np.array(doc["cases"][i]["result"]) for i in (1, 3))
    assert np.abs(a - b)[:, 7:10].max() > 1e-3                   # the drag acts
    a, b = (np.array(doc["cases"][i]["result"]) for i in (3, 5))
    assert np.abs(a - b)[:, 9].min() > 1e-3                      # the payload pulls every vehicle down


def test_spec_edges():
    p = _plant(True, False, 3)
    X, U = QS.fleet67()
    x, rep = QS.step(p, X[9], U[9])
    u2 = U[9].copy(); u2[2] = p.u_min
    assert rep and np.array_equal(x, QS.step(p, X[9], u2)[0])                             # the NaN activation acts as u_min
    lo, hi = U[0].copy(), U[0].copy()
    lo[1], hi[1] = -0.2, 0.0
    assert np.array_equal(QS.step(p, X[0], lo)[0], QS.step(p, X[0], hi)[0])               # the clip
    vb = QS.rot(QS.conj(X[5, 3:7])).dot(X[5, 7:10])
    assert vb[1] == 0.0 and np.sign(vb[1]) == 0.0
    t, c = np.zeros(3), np.zeros(3, dtype=np.int32)
    QS.tally_step(t, c, [1.0, 2.0, 2.0], np.zeros(13), 0, False)
    QS.tally_step(t, c, [np.nan, 0.0, 0.0], np.zeros(13), 4, True)
    assert t.tolist() == [3.0, 9.0, 3.0] and c.tolist() == [2, 1, 1]


# ---- the window ---------------------------------------------------------------------------------------------------------------------

def _reference_window(traj, u, idx, N, over):
    """get_reference_chunk (quad_3d_opt_utils.py:284-296) and the padding of set_reference_trajectory (quad_3d_optimizer.py:476-502),
    restated step for step: slice, down-sample, cut the inputs, pad both with their last row, stack."""
    tc, uc = traj[idx:idx + (N + 1) * over, :], u[idx:idx + N * over, :]
    ds = np.arange(0, min(over * (N + 1), tc.shape[0]), over, dtype=int)
    tc, uc = tc[ds, :], uc[ds[:max(len(ds) - 1, 1)], :]
    assert tc.shape[0] == uc.shape[0] + 1 or tc.shape[0] == uc.shape[0]
    while tc.shape[0] < N + 1:
        tc = np.concatenate((tc, tc[-1:, :]), 0)
        uc = np.concatenate((uc, uc[-1:, :]), 0)
    return np.concatenate((tc[:N], uc[:N]), 1), tc[N]


@pytest.mark.parametrize("M", [1, 7, 61, 120])
def test_window_closed_form_equals_the_reference_text(M):
    rng = np.random.default_rng(M)
    traj, u = rng.standard_normal((M, 13)), rng.standard_normal((M, 4))
    for N in (10, 20):
        for over in (1, 5):
            for idx in range(M):
                yref, yref_e, pos = QS.chunk(traj, u, idx, N, over)
                want, want_e = _reference_window(traj, u, idx, N, over)
                assert np.array_equal(yref, want) and np.array_equal(yref_e, want_e) and np.array_equal(pos, traj[idx, :3]), (N, over, idx)
    for idx in (-1, M):
        assert all(np.isnan(a).all() for a in QS.chunk(traj, u, idx, 10, 5))
    assert QS.next_idx([(traj, u)], [0, 0, 0, 1], [0, M - 1, M, 0]).tolist() == [min(1, M - 1), M - 1, M, 0]


def test_vectorised_plant_agrees_with_the_spec():
    """step_fleet, the plant of the CPU closed loop in tests/test_quad_fleet_gpu.py, against the spec in the reference's order."""
    X, U = QS.fleet67()
    for drag, payload, substeps in ((False, False, 1), (True, True, 40)):
        p = _plant(drag, payload, substeps)
        want, rep = QS.step_batch(p, X[:16], U[:16])
        got, rep2 = QS.step_fleet(p, X[:16], U[:16])
        assert np.array_equal(rep, rep2) and rep[9] and _rel(got, want) <= 1e-13, _rel(got, want)
