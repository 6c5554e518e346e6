"""The GP sets of tests/gp_structures.py on the CPU: what they cover, the oracles against an independent numpy-longdouble statement of
the GP residual on structures the oracles had never seen (repeated features, shared rows, no training point), the oracles' immunity
to what a caller leaves in the unused entries of AdmpcGp, the reference condition of the GPU tests, and the refusals of the C ABI.

Reference condition (a cap on the inputs of tests/test_gp_structures.py, not a measurement of a kernel): for every set and the batch it
is solved on, the fp64 oracle is at most the kernel's parity tolerance / 1000 from the 80-bit oracle in max |du| and max |dx|, on the
instances (>= 98 %) where both end with status 0 and the same iteration count.  Measured (B = 64; worst set per horizon):

    car        N = 13   |du| 5.2e-14  |dx| 5.0e-14   cap 1e-11
               N = 20   |du| 1.5e-13  |dx| 6.4e-14   cap 1e-11
               N = 40   |du| 7.8e-13  |dx| 1.4e-13   cap 1e-10
    quadrotor  N = 10   |du| 1.3e-12  |dx| 2.2e-12   cap 1e-11
               N = 17   |du| 2.7e-12  |dx| 5.2e-12   cap 1e-11
               N = 20   |du| 4.6e-12  |dx| 5.9e-12   cap 1e-11

The quadrotor batches keep the shipped horizon time of 1 s at every N >= 10 (gp_structures.quad_nominal).  With 0.1 s per stage, as the
parity tests of the longer horizons take it, the quadrotor WITHOUT a GP is already 7.1e-11 / 8.8e-11 (N = 17, 1.7 s) and 4.4e-10 /
5.4e-10 (N = 20, 2 s) from 80-bit, on calmer draws of the generator too: the conditioning of the condensed quadrotor QP over a long
horizon time, which tests/test_accuracy_80bit.py records as Q17_wide / Q20_wide / Q20_seg, and no choice of alpha could meet the cap
there.  The device path depends on N alone.
"""
import ctypes as C

import numpy as np
import pytest

import gp_structures as G
from ad_mpc_amd.config import AdmpcConfig, GP_MAX, GP_MAX_FEAT, GP_MAX_POINTS, default_config, set_gp
from ad_mpc_amd.quad_config import AdmpcQuadConfig, QUAD_GP_MAX, QNX, QNU, default_quad_config, set_quad_gp
from test_cabi import lib  # noqa: F401  (fixture)

L = np.longdouble
CAR_HORIZONS = (13, 20, 40)            # kernel R (13, 40), kernel F / fp32 kernel R / SQP (20), kernel S (40)
QUAD_HORIZONS = (10, 17, 20)           # one-wave dense and generic, wide, two-wave


def parity_tol(vehicle, N):
    return 1e-7 if vehicle == "car" and N > 32 else 1e-8


@pytest.fixture(scope="module")
def car_oracles():
    from oracle.oracle import Oracle
    return Oracle(omp=True), Oracle(variant="ld")


@pytest.fixture(scope="module")
def quad_oracles():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle(), QuadOracle(variant="ld")


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage

@pytest.mark.parametrize("vehicle", ["car", "quad"])
def test_coverage(vehicle):
    sets = G.car_structures() if vehicle == "car" else G.quad_structures()
    spec = dict(G.CAR_SETS if vehicle == "car" else G.QUAD_SETS)
    want = G.COVERAGE[vehicle]
    rows = (3, 4, 5) if vehicle == "car" else (7, 8, 9)
    assert [n for n, _ in sets] == list(spec) and len(sets) >= (12 if vehicle == "car" else 8)
    gps = [g for _, s in sets for g in s]
    assert {len(s) for _, s in sets} == set(want["n_gp"])
    assert max(want["n_gp"]) == (GP_MAX if vehicle == "car" else QUAD_GP_MAX)
    assert {len(g["feat"]) for g in gps} == set(want["n_feat"])
    assert set(want["n_points"]) <= {len(g["alpha"]) for g in gps}
    have = {(f, k) for g in gps for k, f in enumerate(g["feat"])}
    for item in want["slots"]:
        assert item in have, "feature %d never sits in slot %d" % item
    for f in want.get("one_feature_on", ()):
        assert any(g["feat"] == [f] for g in gps), f
    outs = [[g["out"] for g in s] for _, s in sets]
    assert any(len(set(o)) < len(o) for o in outs) == want["shared_row"]
    if "empty_row" in want:                                       # a row with none while another has two
        assert any(len(set(o)) < len(o) and set(rows) - set(o) for o in outs)
    assert any(len(set(g["feat"])) < len(g["feat"]) for g in gps) == want["repeated_feature"]
    assert all(g["ymean"] != 0.0 and g["sigma_f"] != 1.0 for g in gps)
    assert any(max(g["length_scale"]) >= want["length_scale_ratio"] * min(g["length_scale"]) for g in gps)
    ranges = G.CAR_RANGE if vehicle == "car" else G.QUAD_RANGE
    for g in gps:                                                 # training inputs inside the range the batches visit
        for k, f in enumerate(g["feat"]):
            assert ((g["Z"][:, k] >= ranges[f][0]) & (g["Z"][:, k] <= ranges[f][1])).all()
    four = G.CAR_FOUR if vehicle == "car" else G.QUAD_FOUR
    sub = [s for n, s in sets if n in four]
    assert len(sub) == 4
    assert any(len(s) == max(want["n_gp"]) for s in sub) and any(len({g["out"] for g in s}) < len(s) for s in sub)
    first_input = 7 if vehicle == "car" else 13
    assert any(g["feat"][0] >= first_input for s in sub for g in s) and any(len(g["alpha"]) == GP_MAX_POINTS for s in sub for g in s)
    two = [s for n, s in sets if n in (G.CAR_TWO if vehicle == "car" else G.QUAD_TWO)]
    assert len(two) == 2 and any(f >= first_input for g in two[1] for f in g["feat"])


def test_the_scenario_batches_visit_the_training_ranges():
    """The state features of the batches lie inside CAR_RANGE / QUAD_RANGE and the inputs of the initial iterate inside the input ranges."""
    s = G.car_batch(20)
    for f in (3, 4, 5, 6):
        assert s["x0"][:, f].min() >= G.CAR_RANGE[f][0] and s["x0"][:, f].max() <= G.CAR_RANGE[f][1]
    assert (s["ubar"] == 0).all() and G.CAR_RANGE[7][0] < 0 < G.CAR_RANGE[7][1] and G.CAR_RANGE[8][0] < 0 < G.CAR_RANGE[8][1]
    q = G.quad_batch(10)
    assert q["ubar"].min() >= G.QUAD_RANGE[13][0] and q["ubar"].max() <= G.QUAD_RANGE[13][1]
    assert np.abs(q["x0"][:, 10:13]).max() <= 0.5 and np.abs(q["x0"][:, 7:10]).max() <= 1.0      # |v| is kept by the rotation to the body frame only in norm
    for x, u, _ in G.car_rows():
        assert G.CAR_RANGE[7][0] <= u[0] <= G.CAR_RANGE[7][1] and G.CAR_RANGE[8][0] <= u[1] <= G.CAR_RANGE[8][1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the independent reference

def _car_gp_terms(cfg, x, u):
    """GP part of f, Jx, Ju from the formula of include/admpc.h: mean into row `out`, gradient into the column of each feature (added once
    per slot: a repeated feature adds twice)."""
    y = np.concatenate([x, u])
    f = np.zeros(7, dtype=L); J = np.zeros((7, 9), dtype=L)
    for g in range(cfg.n_gp):
        gp = cfg.gp[g]
        mu, dmu = G.gp_mean_longdouble(gp, [y[gp.feat[d]] for d in range(gp.n_feat)])
        f[gp.out] += mu
        for d in range(gp.n_feat):
            J[gp.out, gp.feat[d]] += dmu[d]
    return f, J


@pytest.mark.parametrize("name,gps", G.car_structures(), ids=[n for n, _ in G.CAR_SETS])
def test_car_oracles_against_the_longdouble_statement(name, gps, car_oracles):
    cfg = G.car_cfg(gps, 2); nominal = default_config(N=2)
    for x, u, p in G.car_rows(6):
        ft, Jt = _car_gp_terms(cfg, x, u)
        for o, rel in zip(car_oracles, (64 * np.finfo(np.float64).eps, 4 * np.finfo(np.float64).eps)):
            f = o.f(cfg, x, u, p); f0 = o.f(nominal, x, u, p)
            Jx, Ju = o.jac(cfg, x, u, p); Jx0, Ju0 = o.jac(nominal, x, u, p)
            J = np.c_[Jx, Ju]; J0 = np.c_[Jx0, Ju0]
            # the oracle returns doubles: each side of the difference is rounded once, the 80-bit build no further
            assert (np.abs((f - f0) - ft.astype(np.float64)) <= rel * np.maximum(1.0, np.abs(f0) + np.abs(f))).all(), (name, f - f0, ft)
            assert (np.abs((J - J0) - Jt.astype(np.float64)) <= rel * np.maximum(1.0, np.abs(J0) + np.abs(J))).all(), (name, (J - J0) - Jt)
    if any(len(g["alpha"]) == 0 for g in gps):                     # no training point: the mean is ymean, the gradient zero
        g0 = [g for g in gps if len(g["alpha"]) == 0][0]
        one = set_gp(default_config(N=2), [g0])
        x, u, p = G.car_rows(1)[0]
        d = car_oracles[1].f(one, x, u, p) - car_oracles[1].f(nominal, x, u, p)
        assert abs(d[g0["out"]] - g0["ymean"]) <= 1e-14 and np.count_nonzero(d) == 1


def _rot(q):
    w, x, y, z = [L(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=L)


def _quad_gp_accel(cfg, x, u):
    """World-frame acceleration of the GP residual: R(q) m, m[out - 7] += mu(z), z = [x with R(q)' v in place of v; u]."""
    R = _rot(x[3:7])
    z = np.concatenate([np.asarray(x, dtype=L), np.asarray(u, dtype=L)])
    z[7:10] = R.T @ np.asarray(x[7:10], dtype=L)
    m = np.zeros(3, dtype=L)
    for g in range(cfg.n_gp):
        gp = cfg.gp[g]
        m[gp.out - 7] += G.gp_mean_longdouble(gp, [z[gp.feat[d]] for d in range(gp.n_feat)])[0]
    return R @ m


@pytest.mark.parametrize("name,gps", G.quad_structures(), ids=[n for n, _ in G.QUAD_SETS])
def test_quad_oracles_against_the_longdouble_statement(name, gps, quad_oracles):
    """f against the statement with the body-frame rotation, with and without a GP state of the first node; the sensitivities of one RK4
    step against central differences of the 80-bit oracle's own step (a gradient added to the wrong column, or once for a repeated
    feature, is an error of the size of the gradient times the step)."""
    cfg = G.quad_cfg(gps, 2); nominal = G.quad_nominal(2)
    xbar, ubar, gs = G.quad_rows(5)
    for b in range(5):
        x, u = xbar[b, 0], ubar[b, 0]
        for gpx in (None, gs[b]):
            acc = _quad_gp_accel(cfg, x if gpx is None else gpx, u).astype(np.float64)
            for o, rel in zip(quad_oracles, (64 * np.finfo(np.float64).eps, 4 * np.finfo(np.float64).eps)):
                f = o.f(cfg, x, u, gpx=gpx); f0 = o.f(nominal, x, u)
                want = np.zeros(QNX); want[7:10] = acc
                assert (np.abs((f - f0) - want) <= rel * np.maximum(1.0, np.abs(f0) + np.abs(f))).all(), (name, b, (f - f0) - want)
        o = quad_oracles[1]
        phi, A, Bm = o.rk4_sens(cfg, x, u, cfg.Ts)
        h = 1e-6
        for j in range(QNX + QNU):
            e = np.zeros(QNX + QNU); e[j] = h
            d = (o.rk4_sens(cfg, x + e[:QNX], u + e[QNX:], cfg.Ts)[0] - o.rk4_sens(cfg, x - e[:QNX], u - e[QNX:], cfg.Ts)[0]) / (2 * h)
            col = A[:, j] if j < QNX else Bm[:, j - QNX]
            assert np.abs(d - col).max() <= 1e-7 * max(1.0, np.abs(col).max()), (name, b, j, np.abs(d - col).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# poison

def test_poison_overwrites_exactly_the_unused_entries():
    cfg = G.car_cfg(dict(G.car_structures())["shared_row"], 20)
    for v in G.POISON_VALUES:
        c = G.poison(cfg, v)
        bad = (lambda a: np.isnan(a)) if v != v else (lambda a: a == v)
        assert c.n_gp == cfg.n_gp == 3 and bytes(c)[:AdmpcConfig.gp.offset] == bytes(cfg)[:AdmpcConfig.gp.offset]
        for g in range(GP_MAX):
            s, t = c.gp[g], cfg.gp[g]
            Z = np.array([list(s.Z[k]) for k in range(GP_MAX_FEAT)]); al = np.array(list(s.alpha)); il = np.array(list(s.inv_l2))
            if g >= 3:
                assert s.n_feat == s.out == s.n_points == G.INT_POISON and list(s.feat) == [G.INT_POISON] * 3
                assert bad(Z).all() and bad(al).all() and bad(il).all() and bad(np.array([s.sigma_f, s.ymean])).all()
                continue
            nf, n = t.n_feat, t.n_points
            assert (s.n_feat, s.out, s.n_points, s.sigma_f, s.ymean) == (nf, t.out, n, t.sigma_f, t.ymean)
            assert list(s.feat)[:nf] == list(t.feat)[:nf] and list(s.feat)[nf:] == [G.INT_POISON] * (GP_MAX_FEAT - nf)
            assert (il[:nf] == np.array(list(t.inv_l2))[:nf]).all() and bad(il[nf:]).all()
            assert (Z[:nf, :n] == np.array([list(t.Z[k]) for k in range(nf)])[:, :n]).all() and bad(Z[nf:]).all() and bad(Z[:, n:]).all()
            assert (al[:n] == np.array(list(t.alpha))[:n]).all() and bad(al[n:]).all()


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and (x.view(np.uint8) == y.view(np.uint8)).all(), what


@pytest.mark.parametrize("name,gps", G.car_structures(), ids=[n for n, _ in G.CAR_SETS])
def test_car_oracles_ignore_the_unused_entries(name, gps, car_oracles):
    """fp64 and 80-bit: shooting and solve bit-identical between the zero-filled and both poisoned configs -- only then is the oracle a
    reference for the unused-slot tests on the device."""
    cfg = G.car_cfg(gps, 20)
    s = G.car_batch(20, 16); a = [s[k] for k in G.CAR_ARGS]
    rows = G.car_rows(4)
    for o in car_oracles:
        want = o.solve_batch(cfg, *a); shoot = [o.rk4_sens(cfg, x, u, p, cfg.Ts) for x, u, p in rows]
        assert (want[3] == 0).all()
        for v in G.POISON_VALUES:
            c = G.poison(cfg, v)
            _same_bits(o.solve_batch(c, *a), want, (name, v))
            for (x, u, p), w in zip(rows, shoot):
                _same_bits(o.rk4_sens(c, x, u, p, cfg.Ts), w, (name, v))


@pytest.mark.parametrize("name,gps", G.quad_structures(), ids=[n for n, _ in G.QUAD_SETS])
def test_quad_oracles_ignore_the_unused_entries(name, gps, quad_oracles):
    cfg = G.quad_cfg(gps, 10)
    s = G.quad_batch(10, 16); a = [s[k] for k in G.QUAD_ARGS]
    xbar, ubar, gs = G.quad_rows(4)
    for o in quad_oracles:
        want = o.solve_batch(cfg, *a); shoot = [o.rk4_sens(cfg, xbar[b, 0], ubar[b, 0], cfg.Ts, gpx=gs[b]) for b in range(4)]
        assert (want[3] == 0).all()
        for v in G.POISON_VALUES:
            c = G.poison(cfg, v)
            _same_bits(o.solve_batch(c, *a), want, (name, v))
            for b in range(4):
                _same_bits(o.rk4_sens(c, xbar[b, 0], ubar[b, 0], cfg.Ts, gpx=gs[b]), shoot[b], (name, v))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference condition

def _distance(g, t):
    same = (g[3] == t[3]) & (g[4] == t[4]) & (t[3] == 0)
    B = len(same)
    return same.mean(), np.abs(g[1] - t[1]).reshape(B, -1).max(axis=1)[same].max(), np.abs(g[0] - t[0]).reshape(B, -1).max(axis=1)[same].max()


def _condition(vehicle, N, oracles):
    if vehicle == "car":
        sets, s, make, nominal = G.car_structures(), G.car_batch(N), G.car_cfg, default_config(N=N)
        a = [s[k] for k in G.CAR_ARGS]
        solve = lambda o, c: o.solve_batch(c, *a, nthreads=8)
    else:
        sets, s, make, nominal = G.quad_structures(), G.quad_batch(N), G.quad_cfg, G.quad_nominal(N)
        a = [s[k] for k in G.QUAD_ARGS]
        solve = lambda o, c: o.solve_batch(c, *a, nthreads=8)
    base = solve(oracles[0], nominal)
    _, u0, x0 = _distance(base, solve(oracles[1], nominal))
    cap = parity_tol(vehicle, N) / 1000.0
    print("REFCOND %-4s N %2d without GPs        fp64 from 80-bit |du| %.1e |dx| %.1e   cap %.0e" % (vehicle, N, u0, x0, cap))
    out = []
    for name, gps in sets:
        cfg = make(gps, N)
        r64 = solve(oracles[0], cfg)
        share, du, dx = _distance(r64, solve(oracles[1], cfg))
        moved = np.abs(r64[1] - base[1]).max()
        print("REFCOND %-4s N %2d %-16s share %.3f  fp64 from 80-bit |du| %.1e |dx| %.1e   against the model without GPs |du| %.1e"
              % (vehicle, N, name, share, du, dx, moved))
        out.append((name, share, du, dx, moved))
    return cap, (u0, x0), out


@pytest.mark.parametrize("vehicle,N", [("car", n) for n in CAR_HORIZONS] + [("quad", n) for n in QUAD_HORIZONS])
def test_reference_condition(vehicle, N, car_oracles, quad_oracles):
    """See the module docstring."""
    cap, (u0, x0), rows = _condition(vehicle, N, car_oracles if vehicle == "car" else quad_oracles)
    for name, share, du, dx, moved in rows:
        assert share >= 0.98, (name, share)
        assert moved >= 1e-3, (name, moved)                       # every draw changes the answer
        assert du <= cap and dx <= cap, (vehicle, N, name, du, dx, cap)


@pytest.mark.parametrize("name", G.QUAD_TWO)
def test_quad_sqp_reference_condition(name, quad_oracles):
    """The SQP-mode runs of tests/test_gp_structures.py:test_quad_sqp (gp_structures.quad_sqp_case): on every instance, converged or
    at the QP limit, the fp64 oracle has the 80-bit oracle's status and is at most the tolerance of the leg / 1000 from it -- the
    iteration contracts, so the device can be held to the tolerance on the whole batch.  At least 30 instances converge and at
    least 10 end at the limit of 100 QPs, as tests/test_quad_gpu.py:test_quad_sqp_mode_on_the_device asks of its batch, and the GPs
    move the inputs by more than 1e-3."""
    cfg, nominal, a = G.quad_sqp_case(name)
    for iters, tol, lim in G.QUAD_SQP_LEGS:
        c = cfg.copy(); c.sqp_iters, c.sqp_tol = iters, tol
        n = nominal.copy(); n.sqp_iters, n.sqp_tol = iters, tol
        r, q = (o.solve_batch(c, *a, nthreads=8) for o in quad_oracles)
        du, dx = np.abs(r[1] - q[1]).max(), np.abs(r[0] - q[0]).max()
        moved = np.abs(r[1] - quad_oracles[0].solve_batch(n, *a, nthreads=8)[1]).max()
        print("REFCOND quad SQP %3d QPs %-12s fp64 from 80-bit |du| %.1e |dx| %.1e  cap %.0e / %.0e  statuses %s  against the model without GPs |du| %.1e"
              % (iters, name, du, dx, lim / 1000, lim / 100, np.bincount(r[3], minlength=3), moved))
        np.testing.assert_array_equal(r[3], q[3])
        assert set(r[3].tolist()) <= {0, 2}
        assert du <= lim / 1000 and dx <= 10 * lim / 1000, (name, iters, du, dx)
        assert moved >= 1e-3, (name, iters, moved)
        if iters == 100:
            assert (r[3] == 0).sum() >= 30 and (r[3] == 2).sum() >= 10, np.bincount(r[3])


def test_fp32_rows_meet_the_batch_conditions_on_the_emulator(oracle_omp):
    """The four sets of the fp32 kernel-R row (N = 20) with the float emulator on the float oracle's linearisation: the conditions of
    tests/fp32_path.py:batch_conditions hold and the inputs stay inside the documented bound of the float path."""
    import fp32_path as F
    from ad_mpc_amd.config import tight_ipm
    from emu.emu import Emu
    from oracle.oracle import Oracle
    emu, o32 = Emu(), Oracle(variant="f32")
    s = G.car_batch(20)
    for name, gps in G.car_structures():
        if name not in G.CAR_FOUR:
            continue
        cfg = tight_ipm(G.car_cfg(gps, 20))
        o = F.oracle_solve(oracle_omp, cfg, s)
        g = F.emu_passes(emu, cfg, s, F.cpu_lineariser(o32, cfg))
        F.batch_conditions(o, g, cfg)
        su, sx = F.stats(g, o)
        print("EMU %-14s |du| %.1e / %.1e / %.1e  |dx| %.1e / %.1e / %.1e" % ((name,) + su + sx))
        assert su[2] <= F.F32_BOUND, (name, su)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals

EINVAL, ENODEV = -1, -2
CAR_MSG = b"GP: out must be in {3,4,5}, 1..3 features in {3..8}, n_points <= 32"
QUAD_MSG = b"quad GP: out must be in {7,8,9}, 1..3 features in [7,17), n_points <= 32"


def _create(lib, cfg, quad=False):  # noqa: F811
    h = C.c_void_p(0)
    rc = (lib.admpc_quad_create if quad else lib.admpc_create)(C.byref(cfg), 0, C.byref(h))
    if rc == 0:                                                   # a device is present: the configuration was accepted
        (lib.admpc_quad_destroy if quad else lib.admpc_destroy)(h)
    return rc, lib.admpc_last_error()


def _accepted(rc):
    import torch
    return rc == (0 if torch.cuda.is_available() else ENODEV)


@pytest.mark.parametrize("field,value,msg", [("n_gp", -1, b"n_gp out of range"), ("n_gp", GP_MAX + 1, b"n_gp out of range"),
                                             ("n_feat", 0, CAR_MSG), ("n_feat", GP_MAX_FEAT + 1, CAR_MSG), ("feat", 2, CAR_MSG), ("feat", 9, CAR_MSG),
                                             ("out", 2, CAR_MSG), ("out", 6, CAR_MSG), ("n_points", -1, CAR_MSG), ("n_points", GP_MAX_POINTS + 1, CAR_MSG)])
def test_car_refusals(lib, field, value, msg):  # noqa: F811
    """admpc_create validates before it looks for a device: ADMPC_EINVAL with the documented message, on the last GP and the last slot."""
    cfg = G.car_cfg(dict(G.car_structures())["four_gps"], 20)
    assert _accepted(_create(lib, cfg)[0])
    g = cfg.gp[GP_MAX - 1]
    if field == "n_gp":
        cfg.n_gp = value
    elif field == "feat":
        g.feat[g.n_feat - 1] = value
    else:
        setattr(g, field, value)
    rc, err = _create(lib, cfg)
    assert rc == EINVAL and err == msg, (rc, err)


def test_car_largest_admissible_values_pass_validation(lib):  # noqa: F811
    rng = np.random.default_rng(1)
    gps = [dict(feat=[8, 8, 8] if g else [3, 3, 3], out=5 if g else 3, Z=rng.uniform(-1, 1, (GP_MAX_POINTS, 3)), alpha=rng.normal(size=GP_MAX_POINTS), length_scale=1.0)
           for g in range(GP_MAX)]
    rc, err = _create(lib, G.car_cfg(gps, 128))
    assert _accepted(rc), (rc, err)
    unused = G.poison(G.car_cfg(gps[:1], 20), float("nan"))      # validate() does not look at what the counts do not name
    assert _accepted(_create(lib, unused)[0])


@pytest.mark.parametrize("field,value,msg", [("n_gp", -1, b"quad: n_gp out of range"), ("n_gp", QUAD_GP_MAX + 1, b"quad: n_gp out of range"),
                                             ("n_feat", 0, QUAD_MSG), ("n_feat", GP_MAX_FEAT + 1, QUAD_MSG), ("feat", 6, QUAD_MSG), ("feat", 17, QUAD_MSG),
                                             ("out", 6, QUAD_MSG), ("out", 10, QUAD_MSG), ("n_points", -1, QUAD_MSG), ("n_points", GP_MAX_POINTS + 1, QUAD_MSG)])
def test_quad_refusals(lib, field, value, msg):  # noqa: F811
    """admpc_quad_create validates first as well."""
    cfg = G.quad_cfg(dict(G.quad_structures())["three_gps"], 10)
    assert _accepted(_create(lib, cfg, quad=True)[0])
    g = cfg.gp[QUAD_GP_MAX - 1]
    if field == "n_gp":
        cfg.n_gp = value
    elif field == "feat":
        g.feat[g.n_feat - 1] = value
    else:
        setattr(g, field, value)
    rc, err = _create(lib, cfg, quad=True)
    assert rc == EINVAL and err == msg, (rc, err)


def test_quad_largest_admissible_values_pass_validation(lib):  # noqa: F811
    top = [dict(feat=[16, 16, 16], out=9, Z=np.zeros((GP_MAX_POINTS, 3)), alpha=np.ones(GP_MAX_POINTS), length_scale=1.0)] * QUAD_GP_MAX
    rc, err = _create(lib, G.quad_cfg(top, 24), quad=True)
    assert _accepted(rc), (rc, err)


def test_the_python_mirrors_refuse_oversized_sets():
    one = dict(feat=3, out=3, Z=np.zeros(4), alpha=np.zeros(4), length_scale=1.0)
    with pytest.raises(ValueError):
        set_gp(default_config(), [one] * (GP_MAX + 1))
    with pytest.raises(ValueError):
        set_gp(default_config(), [dict(one, feat=[3, 4, 5, 6], Z=np.zeros((4, 4)))])
    with pytest.raises(ValueError):
        set_gp(default_config(), [dict(one, Z=np.zeros(GP_MAX_POINTS + 1), alpha=np.zeros(GP_MAX_POINTS + 1))])
    qone = dict(one, feat=7, out=7)
    with pytest.raises(ValueError):
        set_quad_gp(default_quad_config(), [qone] * (QUAD_GP_MAX + 1))
    with pytest.raises(ValueError):
        set_quad_gp(default_quad_config(), [dict(qone, feat=[7, 8, 9, 10], Z=np.zeros((4, 4)))])
    with pytest.raises(ValueError):
        set_quad_gp(default_quad_config(), [dict(qone, Z=np.zeros(GP_MAX_POINTS + 1), alpha=np.zeros(GP_MAX_POINTS + 1))])
    none = set_gp(default_config(), [dict(one, Z=np.zeros((0, 1)), alpha=np.zeros(0), ymean=0.5)])     # no training point is admitted
    assert none.gp[0].n_points == 0 and none.gp[0].n_feat == 1 and none.gp[0].ymean == 0.5
