"""The in-kernel SQP loop (admpc_quad_solve_kernel<Dense40Path | GenericPath, true>) away from the corner test_quad_sqp_gpu.py holds it in, on
the four paths with N >= 5.  The lines that exist in these two instantiations alone -- the adjoint recursion, the four stopping
residuals, the three exits -- read Ts, W, We, lbu and ubu themselves, and the interior point in front of them is a compile of its own.

  1. random problem data (W[3] != 0, We != 0, a box inside [0, 1], other Ts and vehicle; one draw per horizon with a GP and a first-node
     GP state away from x0), modes (30, 1e-6) and (3, 0): statuses the oracle's, the iterate within the bound of the draw, everything bit
     for bit the host loop's;
  2. a failure at QP 2 (a huge, finite reference; GenericPath leaves through its Cholesky's pivot test): status 4, qps 2, cost +inf, the
     iterate bit for bit that of ONE RTI step and not the caller's, the neighbours untouched; Dense40Path, whose LDL' has no pivot test,
     fails later through a NaN and keeps the iterate of the QP before that one; at N = 5 the same input does not fail: status 2;
  3. ipm_iter_max = 3 (every QP ends at the limit) and the restart draws of quad_ipm_exits_spec in mode (2, 0) (the last QP goes through
     the fallback restart, QP 1 of other instances did): statuses and iters the oracle's, bit for bit the host loop's; past the grid a
     work-group solves restarted and ordinary instances back to back;
  4. B = 1, a call with every optional output NULL, and poisoned and plain batches alternating on one handle.

tests/test_quad_sqp_edges_cpu.py holds the inputs against passing vacuously and measures the distances every bound comes from
(quad_sqp_edges_spec's tables through quad_sqp_spec.bounds); everything else is bit equality.

Measured on the MI355X (every comparison with the host loop bit for bit, statuses and iters equal to the oracle's on every instance;
largest max |du| / max |dx| against the fp64 oracle over the cases of a row, the bound on |du| is 1e-8 unless given):
                random data, 3 draws x 2 modes    ipm_iter_max = 3, 2 modes    restart draw, (2, 0)
generic_N5      4.8e-13  8.7e-13                  9.4e-15  4.0e-14             2.8e-11  3.0e-09
dense40_N10     3.7e-11  7.9e-11                  2.5e-13  1.5e-12             1.2e-11  3.1e-11
generic_N10     5.8e-11  8.0e-11                  2.8e-13  1.4e-12             1.5e-12  7.3e-12
generic_N16     2.0e-09  4.6e-09 (1.4e-8)         1.9e-11  7.1e-11             3.1e-10  2.4e-09 (1.2e-8)
the late failure: generic_N10 and generic_N16 status 4, qps 2, iters 0; dense40_N10 at 1e150 status 4, qps 4, iters 26, and at 1e100
status 2, qps 30, cost 5e200 (no pivot test); generic_N5 status 2, qps 30, cost 2.5e200.  The whole module: 54 cases in 5 s.
Value-only mutants of the SQP block, each run once: W[cm] for W[QX + cm] in the recursion, lbu and ubu swapped in the ri rows, and
wts[tid] for wts[QX + tid] in the terminal row each fail the twelve (30, 1e-6) cases of test_random_problem_data and the five late cases;
the failed QP's step written back, and the caller's iterate restored at status 4, each fail the three cases of
test_a_late_failure_keeps_the_iterate_of_the_qp_before_it; alpha_prev and cons carried from QP to QP fails the four restart cases, both
no-failure cases and the late failure on dense40_N10.
"""
import numpy as np
import pytest

import batch_regimes as R
import quad_ipm_exits_spec as X
import quad_routed_spec as Q
import quad_sqp_edges_spec as E
import quad_sqp_spec as S
import test_quad_sqp_gpu as T
from test_quad_sqp_gpu import _bits, _engine, _solve_sqp

pytestmark = pytest.mark.gpu

ALL = T.NAMES + ("qps",)


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def qoracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


_ORACLE, _LATE, _RESTART = {}, {}, {}


def _oracle(qoracle, key, cfg, s, gs=None):
    """The fp64 oracle's solve of one case, computed once per horizon (two paths share N = 10)."""
    if key not in _ORACLE:
        _ORACLE[key] = qoracle.solve_batch(cfg, *Q.quad_args(s), nthreads=16, gp_state=gs)
    return _ORACLE[key]


def _host_loop(path, cfg, s, gs=None):
    """(x, u, cost, status, iters) by the launch-per-QP loop of a handle built with cfg.sqp_iters, sqp_tol."""
    assert cfg.sqp_iters > 1
    with _engine(path, cfg) as host:
        return host.solve_numpy(*Q.quad_args(s), gp_state=gs)


def _equals_the_host_loop(g, h, what):
    for k in range(5):
        _bits(g[k], h[k], "%s: %s against the host loop" % (what, ALL[k]))


def _within(g, o, gap, mode, what, rows=slice(None)):
    bu, bx = S.bounds(gap, mode)
    du, dx = np.abs(g[1][rows] - o[1][rows]).max(), np.abs(g[0][rows] - o[0][rows]).max()
    print("EDGES %s: statuses %s, max|du| %.1e (bound %.1e) max|dx| %.1e (bound %.1e)" % (what, np.bincount(o[3], minlength=5).tolist(), du, bu, dx, bx))
    assert du <= bu and dx <= bx, (what, du, bu, dx, bx)


def _qps_follow_the_status(g, mode):
    assert (g[5][g[3] == 2] == mode[0]).all() and (g[5] >= 1).all() and (g[5] <= mode[0]).all()
    if mode[1] > 0:
        assert (g[5][g[3] == 0] < mode[0]).all()
    else:
        assert (g[5][g[3] == 0] == mode[0]).all()


# ---- 1. random problem data -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("qp_max,tol", E.DATA_MODES)
@pytest.mark.parametrize("d", range(E.DRAWS))
@pytest.mark.parametrize("path", E.PATHS)
def test_random_problem_data(qoracle, path, d, qp_max, tol):
    N, mode = S.PATHS[path][0], (qp_max, tol)
    cfg, s, gs = E.data_case(N, d)
    with _engine(path, cfg, mode) as eng:
        g = _solve_sqp(eng, s, gp_state=gs)
    o = _oracle(qoracle, ("data", N, d, mode), E.data_case(N, d, mode)[0], s, gs)
    np.testing.assert_array_equal(g[3], o[3])
    _within(g, o, E.DATA_GAPS[(N, d) + mode], mode, "data %-12s draw %d (%d, %g)" % ((path, d) + mode))
    _equals_the_host_loop(g, _host_loop(path, E.data_case(N, d, mode)[0], s, gs), "draw %d" % d)
    _qps_follow_the_status(g, mode)


# ---- 2. a failure at QP 2 ---------------------------------------------------------------------------------------------------------------

def _late(path, name=None):
    """The in-kernel solve of the batch with the huge reference on one instance (the path's input of the spec), computed once, by a handle
    of its own."""
    name = name or E.LATE[path][0]
    if (path, name) not in _LATE:
        N = S.PATHS[path][0]
        with _engine(path, S.config(N), E.LATE_MODE) as eng:
            _LATE[path, name] = _solve_sqp(eng, E.late_scenario(name))
    return _LATE[path, name]


def _neighbours_as_in_the_plain_batch(r, path):
    ok = np.arange(len(r[3])) != E.LATE_INSTANCE
    plain = T._run(path, E.LATE_MODE)
    for k in range(6):
        _bits(r[k][ok], plain[k][ok], "%s of the neighbours" % ALL[k])


@pytest.mark.parametrize("path", [p for p in E.PATHS if E.LATE_FAILS[p]])
def test_a_late_failure_keeps_the_iterate_of_the_qp_before_it(qoracle, path):
    """GenericPath: QP 2 fails at the Cholesky's pivot test, as the oracle's does; the iterate is bit for bit that of ONE step.  Dense40Path
    has no pivot test and fails at a later QP through a NaN (measured: QP 4 -- the count is read from qps, and the iterate is held against
    that many single steps less one)."""
    N, mode, b = S.PATHS[path][0], E.LATE_MODE, E.LATE_INSTANCE
    name, fails_at = E.LATE[path]
    s = E.late_scenario(name)
    r = _late(path)
    q = int(r[5][b])
    print("EDGES late %-12s %s: status %d, qps %d, cost %g, iters %d" % (path, name, r[3][b], q, r[2][b], r[4][b]))
    assert r[3][b] == 4 and q >= 2 and r[2][b] == np.inf
    if fails_at is not None:
        assert q == fails_at
    with _engine(path, S.config(N), mode) as rti:                # single steps on the same inputs: the mode turned off
        rti.set_sqp(1)
        assert rti.sqp == (0, 0.0)
        xa, ua = s["xbar"], s["ubar"]
        for _ in range(q - 1):
            xa, ua, ca, sa, ia = rti.solve_numpy(s["x0"], s["yref"], s["yref_e"], xa, ua)
            assert sa[b] == 0 and np.isfinite(xa[b]).all() and np.isfinite(ua[b]).all()
    assert np.abs(ua[b] - s["ubar"][b]).max() > 1e-3
    _bits(r[0][b], xa[b], "the iterate of the failed instance against %d single steps" % (q - 1)); _bits(r[1][b], ua[b], "its inputs")
    h = _host_loop(path, S.config(N, mode), s)
    assert r[4][b] == h[4][b]
    _equals_the_host_loop(r, h, "the batch with the failure")
    _neighbours_as_in_the_plain_batch(r, path)
    o = _oracle(qoracle, ("late", name), S.config(N, mode), s)
    assert o[3][b] == 4
    np.testing.assert_array_equal(r[3], o[3])


@pytest.mark.parametrize("path,name", [("generic_N5", E.LATE["generic_N5"][0]), E.LATE_NO_PIVOT_TEST])
def test_a_huge_reference_that_fails_no_qp(qoracle, path, name):
    """N = 5: the Hessian stays positive definite, status 2 as the oracle.  Dense40Path on the input that fails QP 2 everywhere else: no
    pivot test, no failure, status 2 -- not the oracle's 4; the host loop on that path does the same, bit for bit."""
    N, mode, b = S.PATHS[path][0], E.LATE_MODE, E.LATE_INSTANCE
    s = E.late_scenario(name)
    r = _late(path, name)
    print("EDGES late %-12s %s: status %d, qps %d, cost %g, iters %d" % (path, name, r[3][b], r[5][b], r[2][b], r[4][b]))
    assert r[3][b] == 2 and r[5][b] == mode[0] and np.isfinite(r[0][b]).all() and np.isfinite(r[1][b]).all() and 1e200 < r[2][b] < np.inf
    _equals_the_host_loop(r, _host_loop(path, S.config(N, mode), s), "the batch with the huge reference")
    _neighbours_as_in_the_plain_batch(r, path)
    o = _oracle(qoracle, ("late", name), S.config(N, mode), s)
    ok = np.arange(len(r[3])) != b
    np.testing.assert_array_equal(r[3][ok], o[3][ok])
    assert o[3][b] == (2 if E.LATE_INPUTS[name][3] is None else 4)


# ---- 3. the interior point's rare exits inside the loop -----------------------------------------------------------------------------------

@pytest.mark.parametrize("qp_max,tol", E.LIMIT_MODES)
@pytest.mark.parametrize("path", E.PATHS)
def test_every_qp_ends_at_the_iteration_limit(qoracle, path, qp_max, tol):
    N, mode = S.PATHS[path][0], (qp_max, tol)
    cfg, s = E.limit_case(N)
    with _engine(path, cfg, mode) as eng:
        g = _solve_sqp(eng, s)
    o = _oracle(qoracle, ("limit", N, mode), E.limit_case(N, mode)[0], s)
    np.testing.assert_array_equal(g[3], o[3]); np.testing.assert_array_equal(g[4], o[4])
    assert (g[4] == E.LIMIT).all() and (g[3] == (2 if tol > 0 else 0)).all() and (g[5] == qp_max).all()
    _within(g, o, E.LIMIT_GAPS[(N,) + mode], mode, "limit %-12s (%d, %g)" % ((path,) + mode))
    _equals_the_host_loop(g, _host_loop(path, E.limit_case(N, mode)[0], s), "ipm_iter_max = %d" % E.LIMIT)


def _restart(path):
    if path not in _RESTART:
        N = S.PATHS[path][0]
        cfg, s = E.restart_case(N)
        with _engine(path, cfg, E.RESTART_MODE) as eng:
            _RESTART[path] = _solve_sqp(eng, s)
    return _RESTART[path]


@pytest.mark.parametrize("path", E.PATHS)
def test_the_last_qp_goes_through_the_restart(qoracle, path):
    N, mode = S.PATHS[path][0], E.RESTART_MODE
    cfg, s = E.restart_case(N, mode)
    g = _restart(path)
    o = _oracle(qoracle, ("restart", N), cfg, s)
    np.testing.assert_array_equal(g[3], o[3]); np.testing.assert_array_equal(g[4], o[4])
    assert np.flatnonzero(X.restarted(g[4])).tolist() == E.RESTARTED[N] and (g[3] == 0).all() and (g[5] == mode[0]).all()
    _equals_the_host_loop(g, _host_loop(path, cfg, s), "the restart draw")
    _within(g, o, E.RESTART_GAPS[N], mode, "restart %-12s (%d, %g)" % ((path,) + mode), rows=E.kept(N))


def test_past_the_grid_a_work_group_solves_restarted_and_ordinary_instances_back_to_back():
    path = "dense40_N10"
    cfg, s = E.restart_case(10)
    Bb = R.quad_grid(R.num_cu(), 10 ** 9, False)[1] + X.B + 37
    idx = np.arange(Bb) % X.B
    big = {k: v[idx] for k, v in s.items()}
    g = _restart(path)
    with _engine(path, cfg, E.RESTART_MODE) as eng:
        a = _solve_sqp(eng, big)
        b = _solve_sqp(eng, big)
    for k in range(6):
        _bits(a[k], g[k][idx], "%s of every copy" % ALL[k])
        _bits(a[k], b[k], "%s of two runs" % ALL[k])


# ---- 4. small things ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", E.PATHS)
def test_a_batch_of_one(path):
    """An ordinary instance and the instance with the huge reference, each alone in its batch, as in the batch."""
    N, mode = S.PATHS[path][0], E.LATE_MODE
    with _engine(path, S.config(N), mode) as eng:
        for s, whole, b in ((S.scenario(N), T._run(path, mode), 0), (E.late_scenario(E.LATE[path][0]), _late(path), E.LATE_INSTANCE)):
            r = _solve_sqp(eng, {k: v[b:b + 1] for k, v in s.items()})
            for k in range(6):
                _bits(r[k], whole[k][b:b + 1], "%s of instance %d alone" % (ALL[k], b))


@pytest.mark.parametrize("path", E.PATHS)
def test_a_call_without_the_optional_outputs(path):
    """cost, status, iters and qps NULL: the iterate is the full call's, the instance that fails included."""
    import torch
    N = S.PATHS[path][0]
    s, whole = E.late_scenario(E.LATE[path][0]), _late(path)
    with _engine(path, S.config(N), E.LATE_MODE) as eng:
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=eng.device)
        tx, tu = d(s["xbar"]).clone(), d(s["ubar"]).clone()
        eng.solve_sqp(d(s["x0"]), d(s["yref"]), d(s["yref_e"]), tx, tu)
        torch.cuda.synchronize()
    _bits(tx.cpu().numpy(), whole[0], "x without the optional outputs"); _bits(tu.cpu().numpy(), whole[1], "u without the optional outputs")


@pytest.mark.parametrize("path", E.PATHS)
def test_alternating_batches_on_one_handle_each_as_its_first_run(path):
    """Nothing survives in LDS or in the work counter between launches: the batch with the failure and the plain batch, twice each on one
    handle, each as solved first by a handle of its own."""
    N, mode = S.PATHS[path][0], E.LATE_MODE
    first = (_late(path), T._run(path, mode))
    with _engine(path, S.config(N), mode) as eng:
        for call in range(4):
            r = _solve_sqp(eng, (E.late_scenario(E.LATE[path][0]), S.scenario(N))[call % 2])
            for k in range(6):
                _bits(r[k], first[call % 2][k], "%s of call %d" % (ALL[k], call))
