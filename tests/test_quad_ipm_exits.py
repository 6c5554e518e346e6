"""The rare exits of the quadrotor's box-QP interior point on every kernel path: the fallback restart, the iteration limit, status 4.

admpc_quad.hip holds two copies of the loop (the one-block kernel text, three instantiations, and the two-wave kernel of N = 20); at the
shipped settings no instance of WidePath or of the two-wave kernel, and no GenericPath instance away from N = 10, gets near the restart
level of 30 iterations, and no test set ipm_iter_max.  The cases of quad_ipm_exits_spec drive the exits through the configuration (an
ipm_mu0 far too close to the boundary, a small ipm_iter_max) on ordinary scenarios.  Each path of quad_routed_spec.ROUTED_PATHS is held

  1. at every case against the oracle: statuses identical and 0, iteration counts identical on every instance, |du| and |dx| within the
     case's bound, the cost within its relative bound, x_0 pinned bit for bit, the inputs inside the box;
  2. on the restart case: a second solve gives the same bytes; the restarted instances alone give the bytes they have inside the batch,
     and so does the instance behind each of them; and in a batch of 16 num_cu instances drawn from the 64 with replacement, where every
     work-group runs several instances in a row (Dense40Path keeps its factor's diagonal slots, the two-wave kernel IF_Z and the H slot),
     every instance has the bytes of its solve in the batch of 64: a restart leaves nothing behind for the next instance;
  3. with a NaN in x0 of an instance beside a restarted one: status 4, iterate untouched, cost +inf, every other instance unchanged;
  4. (generic_N5, wide_N17, seg_N20) in solver_type "SQP" against the oracle, and three passes in one call against three calls.

tests/test_quad_ipm_exits_cpu.py holds the inputs against passing vacuously and measures the figures below.  Bounds: max(1e-8, 4 x the
distance between the fp64 and the 80-bit oracle) on |du| and |dx|, max(1e-9, 4 x their relative distance) on the cost.

fp64 oracle against 80-bit, max |du| / |dx| / relative cost distance (the two agree in status and iteration count everywhere):
case                   N = 5                    N = 10                   N = 16                   N = 17                   N = 20                   N = 24
restart                7.5e-11 5.8e-10 1.7e-12  1.6e-12 1.0e-11 7.0e-14  2.7e-10 2.6e-09 1.4e-10  1.6e-10 4.4e-10 4.8e-12  1.4e-09 6.6e-09 2.8e-10  1.6e-09 2.8e-09 1.8e-10
limit_1                8.4e-16 1.1e-14 9.4e-16  2.0e-14 1.8e-13 1.2e-14  6.1e-13 5.7e-12 4.2e-13  2.9e-13 5.0e-12 5.3e-13  1.5e-12 2.4e-11 3.9e-12  8.3e-13 8.5e-12 1.5e-12
limit_3                1.3e-14 1.1e-13 1.4e-15  3.6e-13 2.1e-12 5.7e-14  8.7e-12 2.5e-11 5.4e-13  1.3e-11 6.7e-11 5.6e-13  1.3e-10 1.6e-09 8.2e-11  9.1e-11 2.5e-10 4.3e-12
limit_8                7.2e-14 1.3e-13 1.1e-15  1.1e-12 1.8e-12 1.3e-15  5.2e-11 8.8e-11 2.7e-15  8.0e-11 1.4e-10 2.6e-14  3.3e-10 5.5e-10 5.6e-14  5.4e-10 8.0e-10 1.9e-14
edge_29                7.1e-11 5.7e-10 6.4e-16  2.0e-10 1.6e-09 3.3e-13  3.8e-10 2.6e-09 4.2e-12  5.5e-10 7.0e-09 7.5e-11  5.1e-10 4.1e-09 3.2e-11  1.6e-09 2.8e-09 4.6e-12
edge_30                7.7e-13 6.2e-12 7.4e-16  5.8e-11 1.5e-10 1.1e-13  2.3e-10 4.1e-09 1.1e-11  4.4e-10 4.0e-09 3.2e-11  4.4e-10 3.3e-09 1.3e-11  1.6e-09 2.0e-09 2.1e-11
edge_31                4.1e-13 3.2e-12 9.8e-15  1.6e-12 1.0e-11 5.1e-14  2.2e-10 2.6e-09 4.1e-12  2.6e-10 2.0e-09 4.9e-11  5.1e-10 1.6e-09 4.9e-11  1.6e-09 2.0e-09 9.1e-12
restart_tight_budget   8.1e-11 5.0e-10 4.6e-12  1.6e-12 1.0e-11 1.3e-14  3.0e-10 3.5e-09 1.6e-10  1.6e-10 7.1e-10 2.5e-11  2.7e-10 1.6e-09 5.4e-11  1.6e-09 8.0e-09 2.4e-10
largest bound          1e-8                     1e-8                     1.7e-8 (edge_30)         2.8e-8 (edge_29)         2.6e-8 (restart)         3.2e-8 (restart_tight_budget)
SQP (4, 1e-6)          2.1e-14 7.2e-14 1.1e-15                                                    6.8e-11 2.0e-10 3.6e-12  3.8e-10 9.8e-10 2.2e-11
SQP (3, 0)             5.0e-14 7.2e-14 8.8e-16                                                    1.0e-10 1.6e-10 2.2e-12  1.1e-09 1.8e-09 1.2e-11
SQP (100, 1e-6)        1.5e-14 4.3e-14 5.6e-16                                                    2.2e-10 1.9e-09 1.6e-11  6.4e-10 4.6e-09 4.1e-11
"""
import contextlib

import numpy as np
import pytest

import batch_regimes as R
import quad_ipm_exits_spec as E
import quad_routed_spec as Q
from test_batch_regimes import _bits, _take

pytestmark = pytest.mark.gpu

NAMES = ("x", "u", "cost", "status", "iters")
SQP_PATHS = [p for p in E.PATHS if p in E.SQP_HORIZONS.values()]
assert len(SQP_PATHS) == 3


@pytest.fixture(scope="module")
def nc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return R.num_cu()


@pytest.fixture(scope="module")
def qoracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


@contextlib.contextmanager
def _engine(path, cfg):
    """A QuadBatchSolver of `cfg` created under the path's environment (read at the creation of a handle), closed at the end."""
    from ad_mpc_amd.engine import QuadBatchSolver
    with pytest.MonkeyPatch.context() as mp:
        for k, v in Q.ROUTED_PATHS[path][1].items():
            mp.setenv(k, v)
        eng = QuadBatchSolver(cfg, device=0)
    try:
        yield eng
    finally:
        eng.close()


_ORACLE, _RESTART = {}, {}


def _oracle(qoracle, path, name):
    """The oracle on one case, computed once per horizon."""
    N = Q.ROUTED_PATHS[path][0]
    if (N, name) not in _ORACLE:
        cfg, s = E.case(path, name)
        _ORACLE[N, name] = qoracle.solve_batch(cfg, *Q.quad_args(s), nthreads=16)
    return _ORACLE[N, name]


def _restart_run(path, eng=None):
    """The device's results on the restart case of `path`: part 1's run when it has taken place."""
    if path not in _RESTART:
        cfg, s = E.case(path, "restart")
        if eng is not None:
            _RESTART[path] = eng.solve_numpy(*Q.quad_args(s))
        else:
            with _engine(path, cfg) as e:
                _RESTART[path] = e.solve_numpy(*Q.quad_args(s))
    return _RESTART[path]


# ---- 1. parity at every exit ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,name", [(p, c) for p in E.PATHS for c in E.CASES])
def test_exit_parity_with_the_oracle(nc, qoracle, path, name):
    N = Q.ROUTED_PATHS[path][0]
    cfg, s = E.case(path, name)
    with _engine(path, cfg) as eng:
        g = eng.solve_numpy(*Q.quad_args(s))
    if name == "restart":
        _RESTART[path] = g
    o = _oracle(qoracle, path, name)
    tol, ctol = E.bounds(N, name)
    what = "%s %s" % (path, name)
    du, dx = np.abs(g[1] - o[1]).max(), np.abs(g[0] - o[0]).max()
    dc = (np.abs(g[2] - o[2]) / np.abs(o[2])).max()
    differ = np.flatnonzero(g[4] != o[4])
    print("EXITS %-34s %2d instances, iterations up to %2d (%d instances differ): max|du| %.1e max|dx| %.1e  bound %.1e; cost %.1e relative, bound %.1e"
          % (what, len(g[4]), o[4].max(), len(differ), du, dx, tol, dc, ctol))
    np.testing.assert_array_equal(g[3], o[3], err_msg=what); assert (o[3] == 0).all(), what
    assert not len(differ), "%s: iteration counts differ at %s: device %s, oracle %s" % (what, differ, g[4][differ], o[4][differ])
    assert du <= tol and dx <= tol, (what, du, dx, tol)
    assert dc <= ctol, (what, dc, ctol)
    _bits(g[0][:, 0], s["x0"], what + ": x_0")
    lb, ub = np.array(cfg.lbu[:]), np.array(cfg.ubu[:])
    assert (g[1] >= lb - 1e-9).all() and (g[1] <= ub + 1e-9).all(), what


# ---- 2. repeatable, and independent of the batch ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", E.PATHS)
def test_a_restart_is_repeatable_and_leaves_nothing_behind(nc, path):
    cfg, s = E.case(path, "restart")
    args = Q.quad_args(s)
    with _engine(path, cfg) as eng:
        g = _restart_run(path, eng)
        again = eng.solve_numpy(*args)
        for k, (a, b) in enumerate(zip(g, again)):
            _bits(a, b, "%s, a second solve: %s" % (path, NAMES[k]))
        r = np.flatnonzero(E.restarted(g[4]))
        assert len(r) >= E.B // 16 and (g[4][r] < 50 + E.FALLBACK).any() and (g[4][r] == 50 + E.FALLBACK).any(), (path, g[4][r])
        alone = eng.solve_numpy(*_take(args, r))
        for k, (a, b) in enumerate(zip(g, alone)):
            _bits(a[r], b, "%s, the restarted instances alone: %s" % (path, NAMES[k]))
        behind = [int(b) + 1 for b in r if b + 1 < E.B]
        for b in behind:
            solo = eng.solve_numpy(*_take(args, slice(b, b + 1)))
            for k, (a, c) in enumerate(zip(g, solo)):
                _bits(a[b:b + 1], c, "%s, instance %d (behind a restarted one) alone: %s" % (path, b, NAMES[k]))
        # every work-group runs several instances in a row: B > 8 num_cu >= the grid of any footprint (batch_regimes.quad_grid)
        Bp = 16 * nc
        assert Bp > R.quad_grid(nc, Bp, Q.ROUTED_PATHS[path][2] == Q.SEG)[1]
        draw = np.random.default_rng(Q.ROUTED_PATHS[path][0]).integers(0, E.B, Bp)
        draw[:E.B] = np.arange(E.B)
        many = eng.solve_numpy(*_take(args, draw))
        for k, (a, b) in enumerate(zip(g, many)):
            _bits(a[draw], b, "%s, %d instances drawn from the batch: %s" % (path, Bp, NAMES[k]))
    print("EXITS %-14s restart: %d restarted instances %s, %d behind them; alone, twice and in a batch of %d: the same bytes"
          % (path, len(r), g[4][r].tolist(), len(behind), Bp))


# ---- 3. a NaN beside a restart ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", E.PATHS)
def test_a_nan_beside_a_restart(nc, path):
    cfg, s = E.case(path, "restart")
    with _engine(path, cfg) as eng:
        clean = _restart_run(path, eng)
        r = np.flatnonzero(E.restarted(clean[4]))
        b = int(next(i for i in r if i + 1 < E.B)) + 1
        x0 = s["x0"].copy(); x0[b, 1] = np.nan
        g = eng.solve_numpy(x0, *Q.quad_args(s)[1:])
    assert g[3][b] == 4 and np.isposinf(g[2][b]), (path, g[3][b], g[2][b])
    _bits(g[0][b:b + 1], s["xbar"][b:b + 1], path + ": iterate of the failed instance")
    _bits(g[1][b:b + 1], s["ubar"][b:b + 1], path + ": inputs of the failed instance")
    keep = np.arange(E.B) != b
    for a, c, k in zip(g, clean, NAMES):
        _bits(a[keep], c[keep], "%s, the neighbours of the failed instance %d: %s" % (path, b, k))
    print("EXITS %-14s NaN in x0 of instance %d behind the restarted instance %d (%d iterations): status 4, the other %d unchanged" % (path, b, b - 1, clean[4][b - 1], E.B - 1))


# ---- 4. SQP mode away from N = 10 -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,iters,sqp_tol", [(p,) + m for p in SQP_PATHS for m in E.SQP_MODES])
def test_sqp_mode_away_from_the_shipped_horizon(nc, qoracle, path, iters, sqp_tol):
    """(4, 1e-6) and (100, 1e-6) against the oracle: statuses identical, |du| within the bound of the mode and |dx| within 10 x the bound
    (test_quad_gpu.py::test_quad_sqp_mode_on_the_device); (3, 0): the bits of three single calls on an RTI handle."""
    N = Q.ROUTED_PATHS[path][0]
    cfg, s = E.sqp_case(N, iters, sqp_tol)
    args = Q.quad_args(s)
    with _engine(path, cfg) as eng:
        g = eng.solve_numpy(*args)
    if sqp_tol == 0.0:
        with _engine(path, Q.path_config(path)) as rti:
            xa, ua = s["xbar"], s["ubar"]
            for _ in range(iters):
                xa, ua, ca, sa, ia = rti.solve_numpy(*args[:3], xa, ua)
        _bits(g[0], xa, path + ": x of three passes in one call"); _bits(g[1], ua, path + ": u of three passes in one call")
        assert (g[3] == 0).all() and (sa == 0).all()
        print("EXITS %-14s SQP (%d, %g): the bits of %d single calls" % (path, iters, sqp_tol, iters))
        return
    o = qoracle.solve_batch(cfg, *args, nthreads=16)
    tol = E.sqp_bound(N, iters, sqp_tol)
    du, dx = np.abs(g[1] - o[1]).max(), np.abs(g[0] - o[0]).max()
    print("EXITS %-14s SQP (%d, %g): statuses %s, max|du| %.1e (bound %.1e) max|dx| %.1e (bound %.1e)" % (path, iters, sqp_tol, np.bincount(o[3]).tolist(), du, tol, dx, 10 * tol))
    np.testing.assert_array_equal(g[3], o[3])
    assert set(o[3].tolist()) <= {0, 2}
    if iters == 100:
        assert (o[3] == 0).sum() >= 8 and (o[3] == 2).sum() >= 8
    assert du <= tol and dx <= 10 * tol, (path, iters, du, dx, tol)
