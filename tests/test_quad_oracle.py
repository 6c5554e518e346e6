"""Quadrotor model and RTI step of the CPU oracle, CPU only.
Pins: (1) the model and its ERK4 sensitivities against golden vectors produced by the reference's own compiled CasADi code
(oracle/make_golden_quad.py); (2) the condensed QP against an independent numpy condensing of the same linearisation and its
solution against an exact active-set solver (scipy BVLS on the Cholesky-transformed QP) plus a KKT check."""
import json
import os

import numpy as np
import pytest

from ad_mpc_amd.quad_config import default_quad_config, tight_quad_config, QNX, QNU
from ad_mpc_amd.quad_scenarios import random_quad_scenarios, hover_input

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_shooting.json")


@pytest.fixture(scope="module")
def qoracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


def test_model_and_rk4_against_the_reference_golden_vectors(qoracle):
    cfg = default_quad_config()
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) == 60
    for c in cases:
        x, u = np.array(c["x"]), np.array(c["u"])
        assert np.abs(qoracle.f(cfg, x, u) - np.array(c["xdot"])).max() <= 1e-12 * max(1.0, np.abs(c["xdot"]).max())
        phi, A, B = qoracle.rk4_sens(cfg, x, u, c["h"])
        for got, ref in ((phi, c["phi"]), (A, c["A"]), (B, c["B"])):
            ref = np.array(ref)
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_hover_is_an_equilibrium(qoracle):
    cfg = default_quad_config()
    x = np.zeros(QNX); x[3] = 1.0
    assert np.abs(qoracle.f(cfg, x, np.full(4, hover_input(cfg)))).max() <= 1e-14


def _numpy_condense(cfg, qoracle, x0, yref, yref_e, xbar, ubar):
    N, n = cfg.N, cfg.N * QNU
    Qd = cfg.Ts * np.array(cfg.W[:QNX]); Rd = cfg.Ts * np.array(cfg.W[QNX:]); Qe = np.array(cfg.We[:])
    G = np.zeros((QNX, n)); xh = x0 - xbar[0]
    H = np.kron(np.eye(N), np.diag(Rd)); g = (np.tile(Rd, N) * (ubar - yref[:, QNX:]).reshape(-1)).copy()
    for k in range(N):
        phi, A, B = qoracle.rk4_sens(cfg, xbar[k], ubar[k], cfg.Ts)
        G = A @ G; G[:, k * QNU:(k + 1) * QNU] = B
        xh = A @ xh + (phi - xbar[k + 1])
        Q = Qd if k + 1 < N else Qe
        ref = yref[k + 1, :QNX] if k + 1 < N else yref_e
        H += G.T @ (Q[:, None] * G); g += G.T @ (Q * (xbar[k + 1] + xh - ref))
    return H, g


def test_condensed_qp_and_its_minimiser(qoracle):
    """H, g against an independent numpy condensing (matrix form); du against scipy's BVLS on the equivalent bounded least-squares
    problem; KKT: stationarity with multipliers of the right sign, feasibility."""
    from scipy.optimize import lsq_linear
    cfg = tight_quad_config()
    s = random_quad_scenarios(24, cfg, seed=3)
    nact = 0
    for b in range(24):
        d = qoracle.qp_debug(cfg, s["x0"][b], s["yref"][b], s["yref_e"][b], s["xbar"][b], s["ubar"][b])
        assert d["status"] == 0 and d["iters"] < cfg.ipm_iter_max
        H, g = _numpy_condense(cfg, qoracle, s["x0"][b], s["yref"][b], s["yref_e"][b], s["xbar"][b], s["ubar"][b])
        assert np.abs(d["H"] - H).max() <= 1e-11 * np.abs(H).max() and np.abs(d["g"] - g).max() <= 1e-11 * max(1.0, np.abs(g).max())
        du = (d["u"] - s["ubar"][b]).reshape(-1)
        lo = np.tile(np.array(cfg.lbu[:]), cfg.N) - s["ubar"][b].reshape(-1); hi = np.tile(np.array(cfg.ubu[:]), cfg.N) - s["ubar"][b].reshape(-1)
        Lc = np.linalg.cholesky(H)
        r = lsq_linear(Lc.T, -np.linalg.solve(Lc, g), bounds=(lo, hi), method="bvls", tol=1e-14, max_iter=500)
        f = lambda v: 0.5 * v @ H @ v + g @ v
        assert np.abs(du - r.x).max() <= 1e-5 and f(du) - f(r.x) <= 1e-11 * abs(f(r.x)), (np.abs(du - r.x).max(), f(du) - f(r.x))   # (flat directions: cond(H) ~ 2e5)
        grad = H @ du + g                                        # KKT of the box QP
        atl, atu = du - lo <= 1e-7, hi - du <= 1e-7
        nact += int(atl.sum() + atu.sum())
        assert (du >= lo - 1e-9).all() and (du <= hi + 1e-9).all()
        assert np.abs(grad[~atl & ~atu]).max(initial=0) <= 1e-5 and (grad[atl] >= -1e-5).all() and (grad[atu] <= 1e-5).all()
    assert nact > 20                                             # the batch really has active input bounds


def test_batch_solve_statuses_and_failure(qoracle):
    cfg = default_quad_config()
    s = random_quad_scenarios(32, cfg, seed=11)
    s["x0"][5, 2] = np.nan
    x, u, cost, st, it = qoracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"], nthreads=4)
    assert st[5] == 4 and np.isinf(cost[5]) and (x[5] == s["xbar"][5]).all() and (u[5] == s["ubar"][5]).all()
    ok = np.arange(32) != 5
    assert (st[ok] == 0).all() and np.isfinite(cost[ok]).all() and it[ok].max() < cfg.ipm_iter_max
    assert (u[ok] >= -1e-9).all() and (u[ok] <= 1 + 1e-9).all()
    np.testing.assert_allclose(x[ok][:, 0], s["x0"][ok], atol=1e-15)        # x_0 pinned to the measured state
    # a second step from the new iterate lowers the (linearised) cost for most instances: RTI steps converging on the tracking problem
    x2, u2, cost2, st2, _ = qoracle.solve_batch(cfg, s["x0"][ok], s["yref"][ok], s["yref_e"][ok], x[ok], u[ok], nthreads=4)
    assert (st2 == 0).all() and (cost2 <= cost[ok] * (1 + 1e-9) + 1e-12).mean() >= 0.7


def test_no_limit_cycle_on_aggressive_scenarios(qoracle):
    """ADMPC_QUAD_IPM_BLOCKED_STEP: instance 1540 of this batch cycled until iter_max with the car solver's threshold (0.05) and came
    back 0.09 away from the minimiser; now every instance converges well before iter_max and the former cycler agrees with the exact
    active-set solution."""
    from scipy.optimize import lsq_linear
    cfg = default_quad_config()
    s = random_quad_scenarios(2048, cfg, seed=1)
    x, u, cost, st, it = qoracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"], nthreads=8)
    assert (st == 0).all() and it.max() <= 20
    b = 1540
    d = qoracle.qp_debug(cfg, s["x0"][b], s["yref"][b], s["yref_e"][b], s["xbar"][b], s["ubar"][b])
    lo = -s["ubar"][b].reshape(-1); hi = 1 - s["ubar"][b].reshape(-1)
    Lc = np.linalg.cholesky(d["H"])
    r = lsq_linear(Lc.T, -np.linalg.solve(Lc, d["g"]), bounds=(lo, hi), method="bvls", tol=1e-14, max_iter=2000)
    assert np.abs((d["u"] - s["ubar"][b]).reshape(-1) - r.x).max() <= 1e-6


def test_fallback_mode_ends_the_remaining_limit_cycle(qoracle):
    """ADMPC_QUAD_IPM_FALLBACK_ITER: instance 3012 of this batch (found by the GPU parity census on unseen seeds) cycled until iter_max
    even with the centring safeguard; with the fallback it starts over after 30 iterations without the second-order term, converges
    (47 iterations in all) and agrees with the exact active-set solution.  Nothing else of the batch gets near the threshold."""
    from scipy.optimize import lsq_linear
    cfg = tight_quad_config()
    s = random_quad_scenarios(4096, cfg, seed=202)
    x, u, cost, st, it = qoracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"], nthreads=8)
    b = 3012
    assert (st == 0).all() and it[b] == 47 and np.delete(it, b).max() <= 20
    d = qoracle.qp_debug(cfg, s["x0"][b], s["yref"][b], s["yref_e"][b], s["xbar"][b], s["ubar"][b])
    lo = -s["ubar"][b].reshape(-1); hi = 1 - s["ubar"][b].reshape(-1)
    Lc = np.linalg.cholesky(d["H"])
    r = lsq_linear(Lc.T, -np.linalg.solve(Lc, d["g"]), bounds=(lo, hi), method="bvls", tol=1e-14, max_iter=2000)
    assert np.abs((d["u"] - s["ubar"][b]).reshape(-1) - r.x).max() <= 1e-6


def quad_gps(seed=1):
    """Three residual GPs of the body-frame acceleration: v_bx -> a_bx, (v_by, u_0) -> a_by with two length scales, v_bz -> a_bz."""
    rng = np.random.default_rng(seed)
    gps = [dict(feat=7 + i, out=7 + i, Z=np.linspace(-3, 3, 15), alpha=0.3 * rng.standard_normal(15), length_scale=1.0, sigma_f=1.0, ymean=0.01 * i) for i in range(3)]
    gps[1] = dict(feat=[8, 13], out=8, Z=np.c_[rng.uniform(-3, 3, 20), rng.uniform(0, 1, 20)], alpha=0.3 * rng.standard_normal(20), length_scale=[1.0, 0.3], sigma_f=0.8, ymean=0.0)
    return gps


def test_quad_gp_residual_formula_and_sensitivities(qoracle):
    """quad_3d_optimizer.py:289-327: the GP means of the body-frame acceleration, features from the body-frame velocity (and an input),
    rotated back to the world frame.  The oracle against a direct numpy evaluation, and its ERK4 sensitivities (forward-mode tangents
    through the rotation and the kernels) against central differences."""
    from ad_mpc_amd.quad_config import set_quad_gp
    from ad_mpc_amd.quad_3d_optimizer import q_to_rot_mat
    cfg = default_quad_config(); gps = quad_gps()
    cg = default_quad_config(); set_quad_gp(cg, gps)
    rng = np.random.default_rng(9)
    for trial in range(5):
        x = rng.standard_normal(QNX); x[3:7] /= np.linalg.norm(x[3:7]); u = rng.uniform(0, 1, QNU)
        R = q_to_rot_mat(x[3:7])
        z = np.concatenate([x[:7], R.T @ x[7:10], x[10:], u])
        mu = np.zeros(3)
        for g in gps:
            feats = np.atleast_1d(g["feat"]); Z = np.asarray(g["Z"]).reshape(len(g["alpha"]), -1)
            ell = np.broadcast_to(np.atleast_1d(g["length_scale"]), (len(feats),))
            mu[g["out"] - 7] += g["sigma_f"] * np.exp(-0.5 * (((z[feats] - Z) / ell) ** 2).sum(1)) @ g["alpha"] + g["ymean"]
        d = qoracle.f(cg, x, u) - qoracle.f(cfg, x, u)
        assert np.abs(d[7:10] - R @ mu).max() <= 1e-13 and np.abs(np.delete(d, [7, 8, 9])).max() == 0.0
        phi, A, B = qoracle.rk4_sens(cg, x, u, 0.1)
        h = 1e-6
        for i in range(QNX):
            e = np.zeros(QNX); e[i] = h
            np.testing.assert_allclose(A[:, i], (qoracle.rk4_sens(cg, x + e, u, 0.1)[0] - qoracle.rk4_sens(cg, x - e, u, 0.1)[0]) / (2 * h), atol=5e-8)
        for j in range(QNU):
            e = np.zeros(QNU); e[j] = h
            np.testing.assert_allclose(B[:, j], (qoracle.rk4_sens(cg, x, u + e, 0.1)[0] - qoracle.rk4_sens(cg, x, u - e, 0.1)[0]) / (2 * h), atol=5e-8)
    with pytest.raises(ValueError):
        set_quad_gp(default_quad_config(), [dict(feat=2, out=7, Z=[0.0], alpha=[0.0], length_scale=1.0)])      # position is not an offered feature


def _fd_check(qoracle, cfg, x, u, gpx=None, atol=5e-8):
    phi, A, B = qoracle.rk4_sens(cfg, x, u, 0.1, gpx=gpx)
    h = 1e-6
    for i in range(QNX):
        e = np.zeros(QNX); e[i] = h
        np.testing.assert_allclose(A[:, i], (qoracle.rk4_sens(cfg, x + e, u, 0.1, gpx=gpx)[0] - qoracle.rk4_sens(cfg, x - e, u, 0.1, gpx=gpx)[0]) / (2 * h), atol=atol)
    for j in range(QNU):
        e = np.zeros(QNU); e[j] = h
        np.testing.assert_allclose(B[:, j], (qoracle.rk4_sens(cfg, x, u + e, 0.1, gpx=gpx)[0] - qoracle.rk4_sens(cfg, x, u - e, 0.1, gpx=gpx)[0]) / (2 * h), atol=atol)
    return phi, A, B


def test_linear_drag_term_formula_and_sensitivities(qoracle):
    """quad_3d_optimizer.py:364-381 (rdrv_d_mat of the class; not in the shipped generated code, so pinned by a numpy restatement and
    central differences): v' += R(q) D R(q)' v with D = diag(cfg.rdrv).  Zero D is the shipped model bit for bit."""
    from ad_mpc_amd.quad_3d_optimizer import q_to_rot_mat
    cfg = default_quad_config()
    cd = default_quad_config(); cd.rdrv[0], cd.rdrv[1], cd.rdrv[2] = -0.3, -0.4, -0.1
    rng = np.random.default_rng(4)
    for trial in range(5):
        x = rng.standard_normal(QNX); x[3:7] /= np.linalg.norm(x[3:7]); u = rng.uniform(0, 1, QNU)
        R = q_to_rot_mat(x[3:7])
        d = qoracle.f(cd, x, u) - qoracle.f(cfg, x, u)
        assert np.abs(d[7:10] - R @ (np.diag([-0.3, -0.4, -0.1]) @ (R.T @ x[7:10]))).max() <= 1e-13 and np.abs(np.delete(d, [7, 8, 9])).max() == 0.0
        _fd_check(qoracle, cd, x, u)
    z = default_quad_config(); z.rdrv[0] = z.rdrv[1] = z.rdrv[2] = 0.0
    assert np.array_equal(qoracle.rk4_sens(z, x, u, 0.1)[1], qoracle.rk4_sens(cfg, x, u, 0.1)[1])


def test_first_node_gp_state_parameter(qoracle):
    """quad_3d_optimizer.py:291-297, :546-552: at the first optimisation node the GP features and the rotation of the means come from a
    PARAMETER (p = [gp_x, 1]; default: the initial state), at the other nodes from the integrated state.  (a) value: the residual is
    R(q_gp) mu(z(gp_x, u)) whatever x is; (b) the ERK4 sensitivities with the parameter held fixed match central differences -- the state
    columns lose the GP's contribution, the input columns keep it; (c) an RTI step of the oracle uses x0 as the default GP state and a
    different gp_state changes the step; without GPs the argument is ignored."""
    from ad_mpc_amd.quad_config import set_quad_gp
    from ad_mpc_amd.quad_3d_optimizer import q_to_rot_mat
    cfg = default_quad_config(); gps = quad_gps()
    cg = default_quad_config(); set_quad_gp(cg, gps)
    rng = np.random.default_rng(12)
    for trial in range(4):
        x = rng.standard_normal(QNX); x[3:7] /= np.linalg.norm(x[3:7]); u = rng.uniform(0, 1, QNU)
        gx = rng.standard_normal(QNX); gx[3:7] /= np.linalg.norm(gx[3:7])
        R = q_to_rot_mat(gx[3:7])
        z = np.concatenate([gx[:7], R.T @ gx[7:10], gx[10:], u])
        mu = np.zeros(3)
        for g in gps:
            feats = np.atleast_1d(g["feat"]); Z = np.asarray(g["Z"]).reshape(len(g["alpha"]), -1)
            ell = np.broadcast_to(np.atleast_1d(g["length_scale"]), (len(feats),))
            mu[g["out"] - 7] += g["sigma_f"] * np.exp(-0.5 * (((z[feats] - Z) / ell) ** 2).sum(1)) @ g["alpha"] + g["ymean"]
        d = qoracle.f(cg, x, u, gpx=gx) - qoracle.f(cfg, x, u)
        assert np.abs(d[7:10] - R @ mu).max() <= 1e-13 and np.abs(np.delete(d, [7, 8, 9])).max() == 0.0
        assert np.array_equal(qoracle.f(cg, x, u, gpx=x), qoracle.f(cg, x, u))             # same value when the parameter is the state ...
        _, A_p, B_p = _fd_check(qoracle, cg, x, u, gpx=gx)
        _, A_s, _ = qoracle.rk4_sens(cg, x, u, 0.1)
        _, A_n, B_n = qoracle.rk4_sens(cfg, x, u, 0.1)
        assert np.abs(A_p - A_n).max() <= 1e-12 and np.abs(A_s - A_n).max() > 1e-6          # ... but no state sensitivity through the GP
        assert np.abs(B_p - B_n).max() > 1e-6                                                # the input feature (u_0 of the second GP) stays
    s = random_quad_scenarios(6, cg, seed=3)
    base = qoracle.solve_batch(cg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
    same = qoracle.solve_batch(cg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"], gp_state=s["x0"])
    other = s["x0"].copy(); other[:, 7:10] += 1.5
    moved = qoracle.solve_batch(cg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"], gp_state=other)
    assert np.array_equal(base[1], same[1]) and np.abs(base[1] - moved[1]).max() > 1e-6
    n0 = qoracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
    n1 = qoracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"], gp_state=other)
    assert np.array_equal(n0[1], n1[1])


def test_sqp_mode_and_its_stopping_test(qoracle):
    """solver_type "SQP" (create_ros_gp_mpc.py:63-68, quad_3d_optimizer.py:203) in the oracle: cfg.sqp_iters QPs with acados' stopping test.
    (a) the C restatement of the four residuals against an independent numpy statement (multipliers by the adjoint recursion, residuals on
    a fresh linearisation); (b) the loop: statuses 0 / 2, a converged instance has residuals <= tol and stays where it is when solved
    again; the limit gives status 2 with a valid iterate; more QPs never hurt."""
    cfg = default_quad_config(); N = cfg.N
    s = random_quad_scenarios(12, cfg, seed=7, aggressive=0.3)
    # ---- (a): one RTI step, then the residuals at the new iterate with the multipliers of that QP
    for i in range(4):
        A = np.empty((N, QNX, QNX)); Bm = np.empty((N, QNX, QNU))
        for k in range(N):
            _, A[k], Bm[k] = qoracle.rk4_sens(cfg, s["xbar"][i, k], s["ubar"][i, k], cfg.Ts)
        x, u, *_ = qoracle.solve_batch(cfg, s["x0"][i], s["yref"][i], s["yref_e"][i], s["xbar"][i], s["ubar"][i])
        x, u = x[0], u[0]
        Q = cfg.Ts * np.array(cfg.W[:QNX]); R = cfg.Ts * np.array(cfg.W[QNX:]); We = np.array(cfg.We[:])
        pi = np.empty((N, QNX)); m = np.empty((N, QNU))
        pk = We * (x[N] - s["yref_e"][i])
        for k in range(N - 1, -1, -1):
            pi[k] = pk
            m[k] = R * (u[k] - s["yref"][i, k, QNX:]) + Bm[k].T @ pk
            if k >= 1:
                pk = Q * (x[k] - s["yref"][i, k, :QNX]) + A[k].T @ pk
        rs = re = ri = rc = 0.0
        re = np.abs(x[0] - s["x0"][i]).max()
        for k in range(N):
            phi, An, Bn = qoracle.rk4_sens(cfg, x[k], u[k], cfg.Ts)
            re = max(re, np.abs(phi - x[k + 1]).max())
            rs = max(rs, np.abs(R * (u[k] - s["yref"][i, k, QNX:]) + Bn.T @ pi[k] - m[k]).max())
            if k >= 1:
                rs = max(rs, np.abs(Q * (x[k] - s["yref"][i, k, :QNX]) + An.T @ pi[k] - pi[k - 1]).max())
            lb = np.array(cfg.lbu[:]); ub = np.array(cfg.ubu[:])
            ri = max(ri, np.maximum(lb - u[k], 0).max(), np.maximum(u[k] - ub, 0).max())
            rc = max(rc, (np.maximum(m[k], 0) * (u[k] - lb)).max(), (np.maximum(-m[k], 0) * (ub - u[k])).max())
        rs = max(rs, np.abs(We * (x[N] - s["yref_e"][i]) - pi[N - 1]).max())
        got = qoracle.nlp_residuals(cfg, s["x0"][i], s["yref"][i], s["yref_e"][i], x, u, pi, m)
        np.testing.assert_allclose(got, [rs, re, ri, rc], rtol=1e-9, atol=1e-13)
        assert got[1] > 1e-6                         # one RTI step from a cold iterate leaves shooting defects: not converged
    # ---- (b): the loop
    # (full-step Gauss-Newton SQP, acados' FIXED_STEP globalisation: no line search.  On this problem it converges linearly where it
    # converges and settles into a small two-cycle of the inputs elsewhere -- about half of the mild scenarios within 100 QPs; what the loop
    # must get right is the bookkeeping: 0 exactly for the instances that pass the test, 2 with a valid iterate for the others)
    s = random_quad_scenarios(24, cfg, seed=7, pos_err=0.8, tilt=0.2, aggressive=0.0)
    c100 = cfg.copy(); c100.sqp_iters, c100.sqp_tol = 100, 1e-6
    x, u, cost, st, it = qoracle.solve_batch(c100, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
    assert set(st.tolist()) <= {0, 2} and (st == 0).sum() >= 8 and np.isfinite(x).all()
    x2, u2, _, st2, _ = qoracle.solve_batch(c100, s["x0"], s["yref"], s["yref_e"], x, u)
    ok = st == 0
    # a converged iterate: one more QP is solved (a cold solver has no multipliers for the first test), then the test passes; the QP barely moves it
    assert (st2[ok] == 0).all() and np.abs(x2[ok] - x[ok]).max() < 1e-5 and np.abs(u2[ok] - u[ok]).max() < 1e-5
    c3 = cfg.copy(); c3.sqp_iters, c3.sqp_tol = 3, 1e-6
    x3, u3, _, st3, _ = qoracle.solve_batch(c3, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
    assert (st3 == 2).sum() >= 12 and np.isfinite(x3).all()
    crti = cfg.copy(); crti.sqp_iters, crti.sqp_tol = 3, 0.0       # three plain RTI steps: the same iterates as three calls
    xa, ua = s["xbar"], s["ubar"]
    for _ in range(3):
        xa, ua, *_ = qoracle.solve_batch(cfg, s["x0"], s["yref"], s["yref_e"], xa, ua)
    xb, ub, _, stb, _ = qoracle.solve_batch(crti, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
    assert (stb == 0).all() and np.abs(xa - xb).max() == 0.0 and np.abs(ua - ub).max() == 0.0
    np.testing.assert_array_equal(x3, xb)            # ... and the first three QPs of the SQP loop are exactly those


@pytest.mark.parametrize("N,gp,tol", [(10, False, 2e-11), (10, True, 2e-11), (20, False, 4e-9), (20, True, 4e-9)])
def test_fp64_quad_oracle_against_80_bit_arithmetic(qoracle, N, gp, tol):
    """The fp64 quadrotor oracle against the same file with every real in x87 extended precision (libquad_oracle_ld.so, the yardstick of
    tests/test_accuracy_80bit.py): same statuses, the same iteration count on >= 90 % of the instances, inputs and states within `tol`
    (measured here, max |du| / max |dx|: N = 10 1.5e-12 / 2.6e-12 nominal, 1.7e-12 / 2.7e-12 GP; N = 20 3.5e-10 / 5.6e-10 nominal,
    4.3e-10 / 6.1e-10 GP -- the condensed Hessian of the longer horizon is worse conditioned).  At least one instance must differ in its bits: a slip of the ORACLE_LONG_DOUBLE switch that
    builds the fp64 arithmetic twice fails here."""
    from oracle.quad_oracle import QuadOracle
    from ad_mpc_amd.quad_config import set_quad_gp
    ld = QuadOracle(variant="ld")
    cfg = default_quad_config(N=N, t_horizon=0.1 * N)
    if gp:
        set_quad_gp(cfg, quad_gps())
    s = random_quad_scenarios(128, cfg, seed=17 + N)
    a = (cfg, s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])
    x8, u8, _, st8, it8 = ld.solve_batch(*a, nthreads=4)
    x, u, _, st, it = qoracle.solve_batch(*a, nthreads=4)
    np.testing.assert_array_equal(st8, st)
    assert (st == 0).all()
    same = it8 == it
    assert same.mean() >= 0.9
    du = np.abs(u8 - u)[same].max(); dx = np.abs(x8 - x)[same].max()
    print("quad N=%d gp=%d  max|du| fp64 vs 80-bit = %.2e, max|dx| = %.2e  (same iteration count: %d of %d)" % (N, gp, du, dx, same.sum(), len(st)))
    assert du <= tol and dx <= tol
    assert (u8 != u).any(axis=(1, 2)).sum() >= 1
