"""solver_type "SQP" inside the one-wave solve kernel (include/admpc_quad_sqp.h; admpc_quad_solve_kernel<P, true>), on the device.

  1. every path and mode of quad_sqp_spec against the oracle: statuses equal, the iterate within the mode's bound;
  2. against the host loop of a handle built with cfg.sqp_iters, sqp_tol on the same inputs: statuses and iters equal, iterate and cost bit
     for bit; (3, 0) bit for bit three single RTI calls;
  3. qps against the oracle swept over the limit, at the limit, and on an instance with a NaN in x0;
  4. past the grid, where the work counter runs: every copy of the batch as the batch, two runs alike;
  5. with a GP on the first node and gp_state given;
  6. the refusals of the three entries and of the routed solve, in the header's order; set_sqp(1) turns the mode off;
  7. the closed loop: QuadFleet(solver_type="SQP", terminal_cost=True) in rollout and rollout_targets against their single entries, with
     noise, with learning, captured, and a handle built with sqp_iters = 5 still refused.

tests/test_quad_sqp_cpu.py holds the inputs against passing vacuously and measures the distances the bounds come from.

Measured on the MI355X (statuses, iters, iterate and cost equal to the host loop's on every case, bit for bit; max |du| / max |dx|
against the fp64 oracle, with the bound on |du|; mean qps):
                  (100, 1e-6)                      (30, 1e-6)                       (4, 1e-6)                   (3, 0)
generic_N2    7.8e-16 1.1e-15 (1e-6)   3.2                                      7.8e-16 1.1e-15 (1e-8)      7.8e-16 9.4e-16 (1e-8)
generic_N5    9.2e-15 3.2e-14 (1e-6)  54.2    2.3e-14 3.7e-14 (1e-8)  25.3      2.8e-14 9.5e-14 (1e-8)      4.0e-14 6.8e-14 (1e-8)
dense40_N10   8.4e-13 1.9e-12 (1e-6)  67.5    1.1e-12 4.4e-12 (1e-8)  27.2      1.4e-12 5.2e-12 (1e-8)      2.2e-12 3.7e-12 (1e-8)
generic_N10   1.6e-12 3.3e-12 (1e-6)  67.5    9.4e-13 3.6e-12 (1e-8)  27.2      9.1e-13 2.1e-12 (1e-8)      1.0e-12 2.0e-12 (1e-8)
generic_N16   4.7e-11 5.0e-11 (1e-6)  71.9    7.5e-11 1.1e-09 (1e-8)  28.3      1.1e-10 3.4e-10 (1e-8)      1.2e-10 2.5e-10 (1e-8)
with a GP on the first node, N = 10, (30, 1e-6): 1.0e-12 7.7e-12 (1e-8); the first period of the SQP rollout: 1.5e-12 2.3e-12, 11 x 0, 5 x 2.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import batch_regimes as R
import quad_learn_spec as QL
import quad_routed_spec as Q
import quad_sqp_spec as S
import test_quad_fleet_gpu as TQ
import test_quad_noise_gpu as TN
import test_quad_targets_gpu as TT
from test_quad_fleet_gpu import _bits, _host, _p, _stream

pytestmark = pytest.mark.gpu

NAMES = ("x", "u", "cost", "status", "iters")


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def qoracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


@contextlib.contextmanager
def _engine(path, cfg, sqp=None):
    """A QuadBatchSolver of `cfg` created under the path's environment (read at the creation of a handle), closed at the end."""
    from ad_mpc_amd.engine import QuadBatchSolver
    with pytest.MonkeyPatch.context() as mp:
        for k, v in S.PATHS[path][1].items():
            mp.setenv(k, v)
        eng = QuadBatchSolver(cfg, device=0)
    try:
        if sqp is not None:
            eng.set_sqp(*sqp)
        yield eng
    finally:
        eng.close()


def _solve_sqp(eng, s, gp_state=None, x0=None):
    """(x, u, cost, status, iters, qps) of solve_sqp on host arrays; the outputs start from patterns the kernel has to overwrite."""
    import torch
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=eng.device)
    B = len(s["x0"])
    tx, tu = d(s["xbar"]).clone(), d(s["ubar"]).clone()
    cost = torch.full((B,), -7.0, dtype=torch.float64, device=eng.device)
    st, it, qp = (torch.full((B,), -7, dtype=torch.int32, device=eng.device) for _ in range(3))
    eng.solve_sqp(d(s["x0"] if x0 is None else x0), d(s["yref"]), d(s["yref_e"]), tx, tu, cost, st, it,
                  gp_state=None if gp_state is None else d(gp_state), qps=qp)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (tx, tu, cost, st, it, qp))


_ORACLE, _RUN = {}, {}


def _oracle(qoracle, N, mode):
    """The oracle on the batch of horizon N with sqp_iters, sqp_tol = mode, computed once."""
    if (N, mode) not in _ORACLE:
        _ORACLE[N, mode] = qoracle.solve_batch(S.config(N, mode), *Q.quad_args(S.scenario(N)), nthreads=16)
    return _ORACLE[N, mode]


def _run(path, mode):
    """The device's in-kernel SQP solve of one path and mode, computed once."""
    if (path, mode) not in _RUN:
        N = S.PATHS[path][0]
        with _engine(path, S.config(N), mode) as eng:
            assert eng.sqp == mode
            _RUN[path, mode] = _solve_sqp(eng, S.scenario(N))
    return _RUN[path, mode]


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,qp_max,tol", S.CASES)
def test_in_kernel_sqp_against_the_oracle(qoracle, path, qp_max, tol):
    N, mode = S.PATHS[path][0], (qp_max, tol)
    g, o = _run(path, mode), _oracle(qoracle, N, mode)
    bu, bx = S.bounds(S.SQP_GAPS[(N,) + mode], mode)
    du, dx = np.abs(g[1] - o[1]).max(), np.abs(g[0] - o[0]).max()
    print("SQP %-12s (%3d, %g): statuses %s, qps mean %.1f max %d, max|du| %.1e (bound %.1e) max|dx| %.1e (bound %.1e)"
          % (path, qp_max, tol, np.bincount(o[3], minlength=3).tolist(), g[5].mean(), g[5].max(), du, bu, dx, bx))
    np.testing.assert_array_equal(g[3], o[3])
    assert set(o[3].tolist()) <= ({0, 2} if tol > 0 else {0})
    if tol > 0 and min(S.STATUS_MIX.get((N, qp_max), (0, 0))) > 0:                # the table is the oracle's at tol = 1e-6: both exits occur
        assert (o[3] == 0).sum() >= 4 and (o[3] == 2).sum() >= 4
    assert du <= bu and dx <= bx, (path, mode, du, dx)


# ---- 2. against the host loop ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path,qp_max,tol", S.CASES)
def test_in_kernel_sqp_equals_the_host_loop_bit_for_bit(path, qp_max, tol):
    """The QPs are the same text, so equal QP counts give equal bits; the statuses are equal when the stopping test decides alike."""
    N, mode = S.PATHS[path][0], (qp_max, tol)
    s = S.scenario(N)
    g = _run(path, mode)
    with _engine(path, S.config(N, mode)) as host:
        h = host.solve_numpy(*Q.quad_args(s))
    np.testing.assert_array_equal(g[3], h[3]); np.testing.assert_array_equal(g[4], h[4])
    for k in (0, 1, 2):
        _bits(g[k], h[k], "%s against the host loop" % NAMES[k])
    if tol == 0.0:
        with _engine(path, S.config(N)) as rti:
            xa, ua = s["xbar"], s["ubar"]
            for _ in range(qp_max):
                xa, ua, ca, sa, ia = rti.solve_numpy(s["x0"], s["yref"], s["yref_e"], xa, ua)
        for k, a in enumerate((xa, ua, ca, sa, ia)):
            _bits(g[k], a, "%s against %d single calls" % (NAMES[k], qp_max))
        assert (g[5] == qp_max).all()


# ---- 3. qps -----------------------------------------------------------------------------------------------------------------------------

def test_qps_at_the_shortest_horizon_against_the_oracle_swept_over_the_limit(qoracle):
    g = _run("generic_N2", (100, 1e-6))
    first = np.full(len(g[5]), -1)
    for L in S.QPS_SWEEP_N2:
        st = _oracle(qoracle, 2, (L, 1e-6))[3]
        first[(first < 0) & (st == 0)] = L
    assert (first > 0).all() and (g[3] == 0).all()
    np.testing.assert_array_equal(g[5], first - 1)
    assert len(set(g[5].tolist())) >= 3


@pytest.mark.parametrize("path", ["generic_N5", "dense40_N10", "generic_N10", "generic_N16"])
def test_qps_against_the_oracle_at_three_limits(qoracle, path):
    N = S.PATHS[path][0]
    g = _run(path, (100, 1e-6))
    for L in S.QPS_LIMITS:
        st = _oracle(qoracle, N, (L, 1e-6))[3]
        np.testing.assert_array_equal(g[5] <= L - 1, st == 0, err_msg="limit %d" % L)
    for mode in S.modes(path):
        r = _run(path, mode)
        assert (r[5][r[3] == 2] == mode[0]).all() and (r[5] >= 1).all() and (r[5] <= mode[0]).all()
        if mode[1] > 0:
            assert (r[5][r[3] == 0] < mode[0]).all()


@pytest.mark.parametrize("path", ["dense40_N10", "generic_N5"])
def test_an_instance_with_a_nan_ends_at_its_first_qp(path):
    N, mode, bad = S.PATHS[path][0], (30, 1e-6), 5
    s = S.scenario(N)
    x0 = s["x0"].copy(); x0[bad, 1] = np.nan
    with _engine(path, S.config(N), mode) as eng:
        r = _solve_sqp(eng, s, x0=x0)
    g = _run(path, mode)
    assert r[3][bad] == 4 and r[5][bad] == 1 and np.isinf(r[2][bad])
    _bits(r[0][bad], s["xbar"][bad], "the iterate of the instance with the NaN"); _bits(r[1][bad], s["ubar"][bad], "its inputs")
    ok = np.arange(len(x0)) != bad
    for k in range(6):
        _bits(r[k][ok], g[k][ok], "%s of the neighbours" % (NAMES + ("qps",))[k])


# ---- 4. past the grid -------------------------------------------------------------------------------------------------------------------

def test_past_the_grid_every_copy_equals_the_batch():
    path, mode = "dense40_N10", (100, 1e-6)
    s = S.scenario(10)
    nc = R.num_cu()
    Bb = R.quad_grid(nc, 10 ** 9, False)[1] + 96 + 37
    idx = np.arange(Bb) % 96
    big = {k: v[idx] for k, v in s.items()}
    g = _run(path, mode)
    with _engine(path, S.config(10), mode) as eng:
        a = _solve_sqp(eng, big)
        b = _solve_sqp(eng, big)
    for k in range(6):
        what = (NAMES + ("qps",))[k]
        _bits(a[k], g[k][idx], "%s of every copy" % what)
        _bits(a[k], b[k], "%s of two runs" % what)


# ---- 5. with a GP on the first node -----------------------------------------------------------------------------------------------------

def test_with_a_gp_on_the_first_node(qoracle):
    mode = S.MID_MODE
    s = S.scenario(10)
    gs = Q.gp_state(s)
    o = qoracle.solve_batch(S.gp_config(mode), *Q.quad_args(s), nthreads=16, gp_state=gs)
    with _engine("dense40_N10", S.gp_config(), mode) as eng:
        g = _solve_sqp(eng, s, gp_state=gs)
    plain = _run("dense40_N10", mode)
    bu, bx = S.bounds(S.GP_GAP, mode)
    du, dx = np.abs(g[1] - o[1]).max(), np.abs(g[0] - o[0]).max()
    print("SQP with a GP: statuses %s, max|du| %.1e (bound %.1e) max|dx| %.1e (bound %.1e)" % (np.bincount(o[3], minlength=3).tolist(), du, bu, dx, bx))
    np.testing.assert_array_equal(g[3], o[3])
    assert du <= bu and dx <= bx
    assert np.abs(g[1] - plain[1]).max() > 1e-4, "the GP moves the answer"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_mode_turned_off():
    import torch
    from ad_mpc_amd.engine import QuadBatchSolver, QuadEnsembleBatchSolver
    from ad_mpc_amd import _lib
    L = _lib.load()
    N = 10
    s = S.scenario(N)
    eng, host, wide = QuadBatchSolver(S.config(N)), QuadBatchSolver(S.config(N, (5, 1e-6))), QuadBatchSolver(S.config(17))
    try:
        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        nan = float("nan")
        refused(L.admpc_quad_set_sqp(None, -1, nan), "null solver")
        refused(L.admpc_quad_set_sqp(host._h, -1, nan), "qp_max must be in [0, 10000]")
        refused(L.admpc_quad_set_sqp(host._h, 10001, nan), "qp_max must be in [0, 10000]")
        refused(L.admpc_quad_set_sqp(host._h, 100, nan), "tolerance must be >= 0")
        refused(L.admpc_quad_set_sqp(host._h, 100, -1e-9), "tolerance must be >= 0")
        refused(L.admpc_quad_set_sqp(host._h, 0, 0.0), "built with sqp_iters > 1")
        refused(L.admpc_quad_set_sqp(wide._h, 2, 1e-6), "serves N <= 16")
        assert L.admpc_quad_set_sqp(wide._h, 1, 1e-6) == 0 and wide.sqp == (0, 0.0)
        refused(L.admpc_quad_get_sqp(None, None, None), "null solver")
        assert L.admpc_quad_get_sqp(eng._h, None, None) == 0 and eng.sqp == (0, 0.0)

        d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=eng.device)
        x0, yr, ye, xb, ub = (d(a) for a in Q.quad_args(s))

        def solve(h=eng._h, B=len(s["x0"]), x0=_p(x0), ub=_p(ub)):
            return L.admpc_quad_solve_batch_sqp(h, B, x0, _p(yr), _p(ye), None, _p(xb), ub, None, None, None, None, _stream())

        refused(solve(h=None, B=-1), "null solver")
        refused(solve(B=-1), "SQP loop is off")                                                   # the mode before the batch
        eng.set_sqp(4, 1e-6)
        refused(solve(B=-1, x0=None), "negative batch")
        assert solve(B=0, x0=None) == 0
        refused(solve(x0=None), "null array")
        refused(solve(ub=None), "null array")
        torch.cuda.synchronize()
        _bits(_host(xb), s["xbar"], "the iterate after the refusals")

        # the routed solve: a handle in the launch-per-QP mode with the old words, a handle with the mode on with new ones
        ens = QuadEnsembleBatchSolver(S.config(N), Q.clusters(2), Q.CENT[:2], Q.FEATS)
        try:
            route = torch.zeros(len(s["x0"]), dtype=torch.int32, device=eng.device)
            ens.solvers[1].set_sqp(4, 1e-6)
            with pytest.raises(_lib.AdmpcError, match="in-kernel SQP loop .* is not offered for routed"):
                ens.solve(route, x0, yr, ye, xb, ub)
            ens.solvers[1].set_sqp(1)
            ens.solve(route, x0, yr, ye, xb.clone(), ub.clone())
            hs = (C.c_void_p * 2)(ens.solvers[0]._h, host._h)
            refused(L.admpc_quad_solve_batch_routed(hs, 2, 4, _p(route), _p(x0), _p(yr), _p(ye), None, _p(xb), _p(ub), None, None, None, _stream()),
                    "solver_type SQP (sqp_iters > 1) is not implemented for routed")
        finally:
            ens.close()

        # set_sqp(1, ...) turns the mode off: the solve after it is the RTI step
        eng.set_sqp(1, 1e-6)
        assert eng.sqp == (0, 0.0)
        with pytest.raises(_lib.AdmpcError, match="SQP loop is off"):
            eng.solve_sqp(x0, yr, ye, xb, ub)
        off = eng.solve_numpy(*Q.quad_args(s))
        fresh = QuadBatchSolver(S.config(N))
        try:
            rti = fresh.solve_numpy(*Q.quad_args(s))
        finally:
            fresh.close()
        for k in range(5):
            _bits(off[k], rti[k], "%s with the mode turned off" % NAMES[k])
        # solve() with the mode on is solve_sqp without qps
        eng.set_sqp(4, 1e-6)
        on = eng.solve_numpy(*Q.quad_args(s))
        for k in range(5):
            _bits(on[k], _run("dense40_N10", (4, 1e-6))[k], "%s of solve() with the mode on" % NAMES[k])
    finally:
        eng.close(); host.close(); wide.close()


# ---- 7. the closed loop -----------------------------------------------------------------------------------------------------------------

FLY = dict(solver_type="SQP", terminal_cost=True)
B7 = 16


def _bank_fleet(noisy=False, learn=None, **kw):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    trajs = TQ._circles(10, 3.0)
    traj_of = (np.arange(B7) % 2).astype(np.int32)
    idx0 = np.where(traj_of == 1, 6, (np.arange(B7) * 3) % 110).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=10)
    fl = QuadFleet(B7, quad=SimQuad(drag=True, noisy=noisy, motor_noise=noisy), n_nodes=10, learn=learn, noise_seed=TN.SEED if noisy else None,
                   **dict(FLY, **kw))
    fl.set_trajectories(trajs)
    fl.reset(traj_of, idx0, x0)
    return fl, trajs


def _target_fleet(noisy=False, learn=None, **kw):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    fl = QuadFleet(B7, quad=SimQuad(drag=True, noisy=noisy, motor_noise=noisy), n_nodes=10, learn=learn, noise_seed=TT.NOISE_SEED if noisy else None,
                   **dict(FLY, **kw))
    fl.set_targets(seed=TT.SEED, **TT.ROLL)
    fl.reset_targets(TT._start(B7, 10))
    return fl


@pytest.mark.parametrize("noisy,observe", [(False, False), (True, False), (False, True)])
def test_rollout_in_sqp_equals_its_single_entries(qoracle, noisy, observe):
    """rollout(T = 6) over a bank: window, eng.solve, plant step, each a call of its own, bit for bit; the first period's solve against
    the oracle's SQP on the window read back; counts[:, 1] the periods with a status other than 0."""
    T = 6
    learn = QL.EXP_LEARN if observe else None
    (whole, trajs), (loop, _) = (_bank_fleet(noisy, learn) for _ in range(2))
    try:
        assert whole._eng.sqp == (100, 1e-6) and whole.solver_type == "SQP" and [whole.cfg.We[i] for i in range(13)] == [whole.cfg.W[i] for i in range(13)]
        if observe:
            assert whole._nominal.sqp == (0, 0.0)
        out = whole.rollout(T, record=True, observe=observe)
        traj, us, tally, counts = (TN._python_loop(loop, trajs, T, observe=observe) if noisy or observe else TQ._python_loop(loop, trajs, T))
        got, want = TQ._state(whole), TQ._state(loop)
        for k in ("x", "idx", "x_opt", "w_opt", "status", "yref", "yref_e", "cost", "iters"):
            _bits(got[k], want[k], k)
        _bits(_host(out.traj), traj, "traj_out"); _bits(_host(out.u), us, "u_out")
        _bits(got["tally"], tally, "tally"); _bits(got["counts"], counts, "counts")
        assert set(got["status"].tolist()) <= {0, 2}
        if observe:
            for k in ("samples", "bins", "dropped", "_prev"):
                _bits(_host(getattr(whole, k)), _host(getattr(loop, k)), k)
        if not noisy and not observe:
            # the first period by the oracle: the window of the start state, a zero iterate
            first, _ = _bank_fleet()
            try:
                first.ref_chunk()
                yr, ye, x0 = _host(first.yref), _host(first.yref_e), _host(first.x)
                cfg = first.cfg.copy(); cfg.sqp_iters, cfg.sqp_tol = 100, 1e-6
                o = qoracle.solve_batch(cfg, x0, yr, ye, np.zeros((B7, 11, 13)), np.zeros((B7, 10, 4)), nthreads=16)
                first.rollout(1)
                g = TQ._state(first)
                np.testing.assert_array_equal(g["status"], o[3])
                du, dx = np.abs(g["w_opt"] - o[1]).max(), np.abs(g["x_opt"] - o[0]).max()
                print("SQP rollout, first period: statuses %s, max|du| %.1e max|dx| %.1e" % (np.bincount(o[3], minlength=3).tolist(), du, dx))
                assert du <= 1e-6 and dx <= 1e-5
                assert g["counts"][:, 1].tolist() == (o[3] != 0).astype(int).tolist()
            finally:
                first.close()
    finally:
        whole.close(); loop.close()


@pytest.mark.parametrize("noisy,observe", [(False, False), (True, False), (False, True)])
def test_rollout_targets_in_sqp_equals_its_single_entries(noisy, observe):
    """rollout_targets(T = 8, record=True): recovery and window, eng.solve, plant step with the reach test, bit for bit."""
    T = 8
    learn = QL.EXP_LEARN if observe else None
    whole, loop = (_target_fleet(noisy, learn) for _ in range(2))
    try:
        out = whole.rollout_targets(T, record=True, observe=observe)
        traj, us, ns, tg = TT._loop(loop, T, observe)
        got, want = TT._state(whole), TT._state(loop)
        for k in TT.TARGET_STATE:
            _bits(got[k], want[k], k)
        _bits(_host(out.traj), traj, "traj_out"); _bits(_host(out.u), us, "u_out")
        _bits(_host(out.nsub), ns, "nsub_out"); _bits(_host(out.targets), tg, "target_out")
        if observe:
            for k in ("samples", "bins", "dropped", "_prev"):
                _bits(_host(getattr(whole, k)), _host(getattr(loop, k)), k)
        assert (got["tcounts"][:, 2] == T).all() and set(got["status"].tolist()) <= {0, 2}
    finally:
        whole.close(); loop.close()


def test_counts_hold_the_periods_with_a_status_other_than_zero():
    """A limit of 3 QPs leaves most periods at status 2: counts[:, 1] and tcounts[:, 3] count them, period by period."""
    T = 5
    (fl, _), tf = _bank_fleet(sqp=(3, 1e-6)), _target_fleet(sqp=(3, 1e-6))
    try:
        n, nt = np.zeros(B7, dtype=np.int32), np.zeros(B7, dtype=np.int32)
        for _ in range(T):
            fl.step(); n += _host(fl.status) != 0
            tf.rollout_targets(1); nt += _host(tf.status) != 0
        assert n.sum() >= B7 and set(_host(fl.status).tolist()) <= {0, 2}
        np.testing.assert_array_equal(_host(fl.counts)[:, 1], n)
        np.testing.assert_array_equal(_host(tf.tcounts)[:, 3], nt)
        assert nt.sum() >= B7
    finally:
        fl.close(); tf.close()


def test_captured_rollout_targets_in_sqp_replays_the_eager_run():
    import torch
    T = 4
    eager, graphed = _target_fleet(), _target_fleet()
    try:
        x0 = TT._start(B7, 10)
        graphed.rollout_targets(T)                                   # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = graphed.rollout_targets(T, record=True)
        graphed.reset_targets(x0); eager.reset_targets(x0)
        ref = eager.rollout_targets(T, record=True)
        g.replay()
        _bits(_host(out.traj)[1:], _host(ref.traj)[1:], "traj"); _bits(_host(out.u), _host(ref.u), "u")
        _bits(_host(out.nsub), _host(ref.nsub), "nsub"); _bits(_host(out.targets), _host(ref.targets), "targets")
        want, got = TT._state(eager), TT._state(graphed)
        for k in TT.TARGET_STATE:
            _bits(got[k], want[k], "%s after the replay" % k)
    finally:
        eager.close(); graphed.close()


def test_a_handle_built_in_sqp_mode_is_still_refused_by_the_rollouts():
    from ad_mpc_amd.engine import QuadBatchSolver
    (fl, _), tf = _bank_fleet(), _target_fleet()
    host = QuadBatchSolver(S.config(10, (5, 1e-6)))
    try:
        L = fl.lib
        rc = L.admpc_quad_rollout_batch(*fl._rollout_args(host._h, 2, None, None), _stream())
        assert rc == -1 and "SQP mode" in L.admpc_last_error().decode(), L.admpc_last_error()
        rc = L.admpc_quad_rollout_targets_batch(host._h, C.byref(tf._plant), C.byref(tf._tp), B7, 2, _p(tf.x), _p(tf.x_opt), _p(tf.w_opt), _p(tf.yref),
                                                _p(tf.yref_e), _p(tf.cost), _p(tf.status), _p(tf.iters), None, _p(tf.target), _p(tf.target_no),
                                                _p(tf.n_iter), _p(tf.fast), _p(tf.tcounts), _p(tf.nsub), None, None, None, None, None, None, None,
                                                None, None, None, None, None, _stream())
        assert rc == -1 and "SQP mode" in L.admpc_last_error().decode(), L.admpc_last_error()
    finally:
        fl.close(); tf.close(); host.close()
