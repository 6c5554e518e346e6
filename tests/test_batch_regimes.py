"""Every solve kernel on both sides of the batch size at which its launch changes regime.

Past its persistent grid a kernel solves instances in a loop: kernels F and S draw them from the bins of the work-order pre-pass
(admpc_f20_order_kernel, work_order.h: f20_next), the quadrotor kernels from an atomic ticket counter (quad_solve, beyond eight
instances per workgroup), and admpc_nlp_res_kernel, admpc_waypoints_kernel and admpc_quad_shoot_kernel by a grid stride.  Each case
below runs one side of one switch and checks three things:
  - parity with the oracle at the stated tolerances of the existing suite (statuses and iteration counts identical);
  - the bits do not depend on the batch: the same instances solved in sub-batches that fit the smallest grid any LDS footprint gives
    (no work order, no tickets, no stride there) are bit-identical;
  - a seeded permutation of the batch gives the same permutation of the outputs, bit for bit.
Sizes come from the device's CU count and the launch formulas mirrored in batch_regimes.py (pinned by test_batch_regimes_cpu.py).
"""
import numpy as np
import pytest

import batch_regimes as R
from ad_mpc_amd.config import default_config, set_gp
from ad_mpc_amd.scenarios import random_scenarios, grid_gp
from ad_mpc_amd.quad_config import default_quad_config
from ad_mpc_amd.quad_scenarios import random_quad_scenarios
from test_gpu_parity import _assert_parity, TOL, TOL_LONG

pytestmark = pytest.mark.gpu

CAR = ("x0", "yref", "yref_e", "p", "xbar", "ubar")
QUAD = ("x0", "yref", "yref_e", "xbar", "ubar")


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


def _bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    same = (a.view(np.uint8) == b.view(np.uint8)).reshape(len(a), -1).all(axis=1)
    assert same.all(), "%s: %d instances differ in bits, first %s" % (what, (~same).sum(), np.nonzero(~same)[0][:8])


def _take(args, idx):
    return tuple(a[idx] for a in args)


def _composition_free(solve, args, chunk, seed, names=("x", "u", "cost", "status", "iters")):
    """One launch over the batch; the same instances in sub-batches of `chunk`; a seeded permutation: the same bits each time."""
    B = len(args[0])
    g = solve(*args)
    parts = [solve(*_take(args, slice(i, min(i + chunk, B)))) for i in range(0, B, chunk)]
    for k, a in enumerate(g):
        _bits(a, np.concatenate([p[k] for p in parts]), "sub-batches of %d: %s" % (chunk, names[k]))
    perm = np.random.default_rng(seed).permutation(B)
    gp = solve(*_take(args, perm))
    for k, a in enumerate(g):
        _bits(a[perm], gp[k], "permuted batch: %s" % names[k])
    return g


def _car_args(s):
    return tuple(s[k] for k in CAR)


def _quad_args(s):
    return tuple(s[k] for k in QUAD)


# ---- kernel S at N = 60 / 80 (S = 3 / 4 waves per instance, at most 2 workgroups per CU) and at N = 40 with GP residuals

@pytest.mark.parametrize("side", ["below", "past"])
@pytest.mark.parametrize("N", [60, 80])
def test_seg_kernel_work_order_long_horizons(gpu_engine_factory, oracle_omp, nc, N, side):
    """Kernel S at N = 60 / 80: below the grid (B = num_cu, one instance per workgroup) and past it (B > 2 num_cu >= grid for any
    LDS footprint: admpc_f20_order_kernel and the bins run)."""
    S = N // 20
    B = R.s_below(nc) if side == "below" else R.s_past(nc, S)
    lo, hi = R.s_grid(nc, B, S)
    assert R.work_ordered(lo, B) == R.work_ordered(hi, B) == (side == "past")
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=600 + N, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    g = _composition_free(eng.solve_numpy, _car_args(s), R.s_below(nc), seed=N)
    o = oracle_omp.solve_batch(cfg, *_car_args(s), nthreads=16)
    assert (o[3] == 0).all()
    _assert_parity(g, o, TOL_LONG)


def _assert_seg_gp_parity(g, o):
    """test_seg_gpu.py:test_segmented_kernel_with_gp_residuals_on_request's stated tolerances for kernel S on GP models."""
    np.testing.assert_array_equal(g[3], o[3]); np.testing.assert_array_equal(g[4], o[4])
    ok = o[3] == 0
    assert np.abs(g[1][ok] - o[1][ok]).max(initial=0.0) <= 1e-5
    assert np.abs(g[0][ok] - o[0][ok]).max(initial=0.0) <= 1e-1 and np.abs(g[0][ok][:, :20] - o[0][ok][:, :20]).max(initial=0.0) <= 1e-5


@pytest.mark.parametrize("side", ["below", "past"])
def test_seg_kernel_with_gp_work_order_n40(gpu_engine_factory, oracle_omp, nc, monkeypatch, side):
    """Kernel S on GP models (ADMPC_QP=seg) at N = 40: below the grid (B = num_cu) and past it (B > 4 num_cu: work order)."""
    monkeypatch.setenv("ADMPC_QP", "seg")
    B = R.s_below(nc) if side == "below" else R.s_past(nc, 2)
    assert R.work_ordered(R.s_grid(nc, B, 2)[1], B) == (side == "past")
    cfg = default_config(N=40); set_gp(cfg, grid_gp())
    s = random_scenarios(B, N=40, seed=401)
    eng = gpu_engine_factory(cfg)
    g = _composition_free(eng.solve_numpy, _car_args(s), R.s_below(nc), seed=40)
    _assert_seg_gp_parity(g, oracle_omp.solve_batch(cfg, *_car_args(s), nthreads=16))


# ---- non-finite instances inside a work-ordered batch (their work estimate puts them in bin 0)

@pytest.mark.parametrize("N", [20, 40, 80])
def test_nonfinite_instances_in_a_work_ordered_batch(gpu_engine_factory, nc, N):
    """Past the grid of kernel F (N = 20) and kernel S (N = 40, 80): NaN in x0 at the first and last instance and on both sides of every
    grid size a footprint can give.  Those fail (status 4, cost +inf, iterate untouched); every other instance keeps the bits it has in
    the same batch without them."""
    S = N // 20
    B = R.f_past(nc) if N == 20 else R.s_past(nc, S)
    grids = [R.f_grid(nc, B)] if N == 20 else [nc * k for k in range(1, 8 // S + 1)]
    bad = sorted({0, B - 1} | {g - 1 for g in grids} | {g for g in grids})
    assert max(bad) < B
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=70 + N, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    clean = eng.solve_numpy(*_car_args(s))
    assert (clean[3] == 0).all()
    x0 = s["x0"].copy(); x0[bad, 0] = np.nan
    g = eng.solve_numpy(x0, *_car_args(s)[1:])
    assert (g[3][bad] == 4).all() and np.isposinf(g[2][bad]).all(), (g[3][bad], g[2][bad])
    _bits(g[0][bad], s["xbar"][bad], "iterate of a failed instance"); _bits(g[1][bad], s["ubar"][bad], "inputs of a failed instance")
    keep = np.ones(B, dtype=bool); keep[bad] = False
    for a, b, k in zip(g, clean, ("x", "u", "cost", "status", "iters")):
        _bits(a[keep], b[keep], "neighbours of the failed instances: " + k)


# ---- routed ensembles (admpc_solve_batch_routed: every handle runs over the whole batch with first = 0)

def _car_ensemble(tmp_path):
    from test_gp_loader import _ensemble_models
    from ad_mpc_amd import gp_loader
    return gp_loader.GPEnsemble.from_pickled({"models": _ensemble_models(tmp_path)})


@pytest.mark.parametrize("side", ["below", "past"])
@pytest.mark.parametrize("N", [20, 40])
def test_routed_car_ensemble_across_the_grid(tmp_path, oracle_omp, nc, monkeypatch, N, side):
    """EnsembleBatchSolver at N = 20 (kernel F; past: B > 8 num_cu) and at N = 40 with ADMPC_QP=seg (kernel S; past: B > 4 num_cu),
    below the grid at B = num_cu.  Every instance equals the oracle with its cluster's GP; an out-of-range route fails untouched."""
    import torch
    from ad_mpc_amd.engine import EnsembleBatchSolver
    if N == 40:
        monkeypatch.setenv("ADMPC_QP", "seg")
    B = nc if side == "below" else (R.f_past(nc) if N == 20 else R.s_past(nc, 2))
    ens = _car_ensemble(tmp_path)
    cfg = default_config(N=N)
    s = random_scenarios(B, N=N, seed=170 + N, blend=(3.0, 5.0))
    eng = EnsembleBatchSolver(cfg, ens, device=0)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    route = eng.select(d(s["x0"]), d(s["ubar"][:, 0, :])).cpu().numpy()
    assert len(np.unique(route)) == 3
    off = [5, B // 2, B - 1]
    route[off] = [7, -1, 3]

    def solve(rt, x0, yref, yref_e, p, xbar, ubar):
        n = len(rt)
        xb, ub = d(xbar).clone(), d(ubar).clone()
        cost = torch.empty(n, dtype=torch.float64, device="cuda"); st = torch.empty(n, dtype=torch.int32, device="cuda"); it = torch.empty_like(st)
        eng.solve(d(rt.astype(np.int32)), d(x0), d(yref), d(yref_e), d(p), xb, ub, cost, st, it)
        torch.cuda.synchronize()
        return xb.cpu().numpy(), ub.cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()

    g = _composition_free(solve, (route,) + _car_args(s), nc, seed=N)
    assert (g[3][off] == 4).all() and np.isposinf(g[2][off]).all()
    _bits(g[0][off], s["xbar"][off]); _bits(g[1][off], s["ubar"][off])
    for c in range(3):
        m = route == c
        cc = cfg.copy(); set_gp(cc, ens.clusters[c])
        o = oracle_omp.solve_batch(cc, *_take(_car_args(s), m), nthreads=16)
        gm = _take(g, m)
        if N == 20:
            _assert_parity(gm, o, TOL)
        else:
            _assert_seg_gp_parity(gm, o)
    eng.close()


# ---- graph capture of a work-ordered solve (kernel F at N = 20, kernel S at N = 40 and 80)

@pytest.mark.parametrize("N", [20, 40, 80])
def test_captured_work_ordered_solve_replays(gpu_engine_factory, nc, N):
    """Past the grid (work order on), one launch captured into a graph replays the same scheduler state every time: it must be re-armed
    by the last workgroup of each replay.  Four replays with new inputs copied into the captured buffers, two of them back to back and
    an eager solve on the same handle in between the others; each equals the eager solve of its inputs, bit for bit."""
    import torch
    B = R.f_past(nc) if N == 20 else R.s_past(nc, N // 20)
    cfg = default_config(N=N)
    eng = gpu_engine_factory(cfg)
    sets = [random_scenarios(B, N=N, seed=900 + 10 * N + k, blend=(3.0, 5.0) if k != 1 else (100.0, 110.0)) for k in range(3)]
    want = [eng.solve_numpy(*_car_args(s)) for s in sets]
    d = eng.to_device
    bufs = [d(sets[0][k]).clone() for k in CAR]
    cost = torch.empty(B, dtype=torch.float64, device=eng.device)
    st = torch.empty(B, dtype=torch.int32, device=eng.device); it = torch.empty_like(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            eng.solve(*bufs, cost, st, it)
    torch.cuda.current_stream().wait_stream(side)

    def replay(k):
        for b, key in zip(bufs, CAR):
            b.copy_(d(sets[k][key]))
        cost.zero_(); st.fill_(-1); it.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got = (bufs[4].cpu().numpy(), bufs[5].cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy())
        for a, b, name in zip(got, want[k], ("x", "u", "cost", "status", "iters")):
            _bits(a, b, "replay of set %d: %s" % (k, name))

    replay(0); replay(1)                                   # back to back: nothing but the re-arm resets the captured state
    again = eng.solve_numpy(*_car_args(sets[2]))           # eager, same handle, between two replays
    for a, b in zip(again, want[2]):
        _bits(a, b, "eager solve between replays")
    replay(2); replay(0)


# ---- the quadrotor kernels: static stride below 8 instances per workgroup, tickets past it

QUAD_KERNELS = [(10, "dense40"), (5, "generic"), (13, "generic"), (16, "generic"), (17, "wide"), (24, "wide"), (20, "seg20")]


@pytest.mark.parametrize("side", ["below", "past"])
@pytest.mark.parametrize("N,kernel", QUAD_KERNELS, ids=["N%d-%s" % q for q in QUAD_KERNELS])
def test_quad_kernels_across_the_ticket_switch(qoracle, nc, N, kernel, side):
    """Below: B = 8 num_cu (static stride for every footprint); past: B > 64 num_cu (32 num_cu for the two-wave N = 20 kernel),
    the ticket counter for every footprint.  Every instance against the oracle."""
    from ad_mpc_amd.engine import QuadBatchSolver
    seg20 = kernel == "seg20"
    B = R.quad_below(nc) if side == "below" else R.quad_past(nc, seg20)
    lo, hi = R.quad_grid(nc, B, seg20)
    assert R.quad_tickets(lo, B) == R.quad_tickets(hi, B) == (side == "past")
    cfg = default_quad_config(N=N, t_horizon=0.1 * N)
    s = random_quad_scenarios(B, cfg, seed=300 + N)
    eng = QuadBatchSolver(cfg, device=0)
    g = _composition_free(eng.solve_numpy, _quad_args(s), nc, seed=N)
    o = qoracle.solve_batch(cfg, *_quad_args(s), nthreads=16)
    np.testing.assert_array_equal(g[3], o[3]); assert (o[3] == 0).all()
    np.testing.assert_array_equal(g[4], o[4])
    assert np.abs(g[1] - o[1]).max() <= 1e-8 and np.abs(g[0] - o[0]).max() <= 1e-8, (np.abs(g[1] - o[1]).max(), np.abs(g[0] - o[0]).max())
    np.testing.assert_allclose(g[2], o[2], rtol=1e-9)
    eng.close()


@pytest.mark.parametrize("iters,tol", [(3, 0.0), (8, 1e-6)])
@pytest.mark.parametrize("N", [10, 20])
def test_quad_sqp_past_the_shoot_stride_and_tickets(qoracle, nc, N, iters, tol):
    """solver_type SQP at N = 10 and 20, with and without a tolerance, at B past the shoot kernel's stride (2 num_cu) and the ticket
    counter of the solve kernel (which then also skips the instances the d_act mask retires)."""
    from ad_mpc_amd.engine import QuadBatchSolver
    B = R.quad_past(nc, seg20=N == 20)
    assert R.quad_shoot_grid(nc, B) < B and R.quad_tickets(R.quad_grid(nc, B, N == 20)[1], B)
    cfg = default_quad_config(N=N, t_horizon=0.1 * N); cfg.sqp_iters, cfg.sqp_tol = iters, tol
    s = random_quad_scenarios(B, cfg, seed=500 + N, pos_err=0.8, tilt=0.2, aggressive=0.0)
    eng = QuadBatchSolver(cfg, device=0)
    g = _composition_free(eng.solve_numpy, _quad_args(s), nc, seed=N + iters)
    o = qoracle.solve_batch(cfg, *_quad_args(s), nthreads=16)
    np.testing.assert_array_equal(g[3], o[3])
    assert set(o[3].tolist()) <= {0, 2}
    if tol > 0:
        assert (o[3] == 0).any() and (o[3] == 2).any()         # the stopping test retires instances between the passes
    assert np.abs(g[1] - o[1]).max() <= 1e-8 and np.abs(g[0] - o[0]).max() <= 1e-7, (np.abs(g[1] - o[1]).max(), np.abs(g[0] - o[0]).max())
    eng.close()


@pytest.mark.parametrize("side", ["below", "past"])
def test_quad_routed_ensemble_across_the_ticket_switch(qoracle, nc, side):
    """QuadEnsembleBatchSolver at N = 10: every cluster handle runs over the whole batch, below (B = 8 num_cu) and past (B > 64 num_cu)
    the ticket switch; every instance equals the oracle with its cluster's GPs, out-of-range routes fail untouched."""
    import torch
    from ad_mpc_amd.engine import QuadEnsembleBatchSolver
    from ad_mpc_amd.quad_config import set_quad_gp, QNX, QNU
    from test_quad_oracle import quad_gps
    clusters = [quad_gps(seed=1), quad_gps(seed=2), quad_gps(seed=3)]
    cent = np.array([[-1.0, 0.25], [0.5, 0.5], [2.0, 0.75]]); feats = [7, 13]
    cfg = default_quad_config()
    B = R.quad_below(nc) if side == "below" else R.quad_past(nc)
    ens = QuadEnsembleBatchSolver(cfg, clusters, cent, feats, device=0)
    s = random_quad_scenarios(B, cfg, seed=61)
    rng = np.random.default_rng(6)
    xs = s["x0"] + rng.standard_normal((B, QNX)); xs[:, 3:7] /= np.linalg.norm(xs[:, 3:7], axis=1, keepdims=True)
    us = rng.uniform(0, 1, (B, QNU))
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    route = ens.select(d(xs), d(us)).cpu().numpy()
    assert len(np.unique(route)) == 3
    off = [5, B // 2, B - 1]
    route[off] = [7, -1, 3]

    def solve(rt, x0, yref, yref_e, xbar, ubar):
        n = len(rt)
        xb, ub = d(xbar).clone(), d(ubar).clone()
        cost = torch.empty(n, dtype=torch.float64, device="cuda"); st = torch.empty(n, dtype=torch.int32, device="cuda"); it = torch.empty_like(st)
        ens.solve(d(rt.astype(np.int32)), d(x0), d(yref), d(yref_e), xb, ub, cost, st, it)
        torch.cuda.synchronize()
        return xb.cpu().numpy(), ub.cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()

    g = _composition_free(solve, (route,) + _quad_args(s), nc, seed=10)
    assert (g[3][off] == 4).all() and np.isposinf(g[2][off]).all()
    _bits(g[0][off], s["xbar"][off]); _bits(g[1][off], s["ubar"][off])
    for c in range(3):
        m = route == c
        cc = cfg.copy(); set_quad_gp(cc, clusters[c])
        o = qoracle.solve_batch(cc, *_take(_quad_args(s), m), nthreads=16)
        np.testing.assert_array_equal(g[3][m], o[3]); np.testing.assert_array_equal(g[4][m], o[4])
        assert np.abs(g[1][m] - o[1]).max() <= 1e-8 and np.abs(g[0][m] - o[0]).max() <= 1e-8
    ens.close()


# ---- stride kernels

@pytest.mark.parametrize("side", ["below", "past"])
def test_nlp_residuals_across_the_stride(gpu_engine_factory, oracle, nc, side):
    """admpc_nlp_residuals_batch: one workgroup per instance up to 32 num_cu (below: B = 32 num_cu), a grid-stride loop past it.
    A sample (first and last instances of the grid, every one around its end, the last of the batch, seeded others) against the
    oracle; every row bitwise against sub-batches and a permutation of the same iterates."""
    import torch
    B = R.nlp_res_grid(nc, 10 ** 9) if side == "below" else R.nlp_res_past(nc)
    grid = R.nlp_res_grid(nc, B)
    assert (grid < B) == (side == "past")
    cfg = default_config(N=20)
    s = random_scenarios(B, N=20, seed=33, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    d = eng.to_device
    args = [d(s[k]) for k in ("x0", "yref", "yref_e", "p")]
    xb, ub = d(s["xbar"]).clone(), d(s["ubar"]).clone()
    st = torch.empty(B, dtype=torch.int32, device=eng.device)
    pi, ineq = eng.solve_with_multipliers(*args, xb, ub, None, st, None)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    full = (*args, xb, ub, pi, ineq)

    def res(*t):
        r = eng.nlp_residuals(*(x.contiguous() for x in t))
        torch.cuda.synchronize()
        return (r.cpu().numpy(),)

    idx = np.arange(B)
    got = _composition_free(lambda *i: res(*(t[torch.as_tensor(i[0], device=eng.device)] for t in full)), (idx,), nc, seed=3, names=("res",))[0]
    rng = np.random.default_rng(4)
    sample = sorted(set(range(8)) | set(range(grid - 8, min(grid + 8, B))) | set(range(B - 8, B)) | set(rng.integers(0, B, 40).tolist()))
    xn, un, pin, iqn = (t.cpu().numpy() for t in (xb, ub, pi, ineq))
    for i in sample:
        want = oracle.nlp_residuals(cfg, s["x0"][i], s["yref"][i], s["yref_e"][i], s["p"][i], xn[i], un[i], pin[i], iqn[i])
        assert np.all(np.abs(got[i] - want) <= 1e-9 * (1.0 + np.abs(want))), (i, got[i], want)
    assert np.median(got[:, 0]) > 1e-6 and np.median(got[:, 1]) > 1e-6


def test_car_sqp_with_tolerance_past_the_nlp_res_stride(gpu_engine_factory, oracle_omp, nc):
    """An SQP solve with sqp_tol > 0 at B > 32 num_cu: the residual test in front of every QP but the first runs the stride loop of
    admpc_nlp_res_kernel.  Statuses as the oracle's, iterates within 1e-7 where full Newton steps stay bounded."""
    B = R.nlp_res_past(nc)
    cfg = default_config(N=20, sqp_iters=6, sqp_tol=1e-6)
    s = random_scenarios(B, N=20, seed=44, blend=(3.0, 5.0))
    eng = gpu_engine_factory(cfg)
    g = _composition_free(eng.solve_numpy, _car_args(s), nc, seed=44)
    o = oracle_omp.solve_batch(cfg, *_car_args(s), nthreads=16)
    np.testing.assert_array_equal(g[3], o[3])
    assert (o[3] == 0).sum() >= B // 50 and (o[3] == 2).any()
    good = (o[3] != 4) & (np.abs(o[0]).max(axis=(1, 2)) < 1e3) & (np.abs(o[1]).max(axis=(1, 2)) < 1e3)
    assert good.sum() >= B - B // 20
    assert np.abs(g[1][good] - o[1][good]).max() <= 1e-7 and np.abs(g[0][good] - o[0][good]).max() <= 1e-7


@pytest.mark.parametrize("short_path", [False, True])
@pytest.mark.parametrize("side", ["below", "past"])
def test_waypoints_across_the_stride(nc, side, short_path):
    """admpc_waypoints_kernel: one workgroup per pose up to 4096 (below: B = 4096), a stride loop past it.  Every pose against the
    numpy restatement, bitwise against sub-batches and a permutation.  The window is laid from the start of the path (ref_traj.py:124-131),
    so the end-of-path branch (stop = 1) is a property of the path: a 1.95 m path runs out within the horizon, the 200 m one does not."""
    import torch
    from ad_mpc_amd.ref_traj import RefTrajectory
    from oracle.ref_traj_oracle import get_waypoints
    from test_fleet_step import _path
    from test_ref_traj import KEYS
    B = 4096 if side == "below" else R.WAYPOINTS_PAST
    assert (R.waypoints_grid(B) < B) == (side == "past")
    H, dt = 20, 0.05
    rt = RefTrajectory(traj_horizon=H, traj_dt=dt)
    rt.set_traj(*(_path(M=40, ds=0.05) if short_path else _path()))
    t = rt.trajectory
    rng = np.random.default_rng(8)
    idx = rng.integers(0, t.shape[0], B)
    idx[rng.uniform(size=B) < 0.1] = t.shape[0] - 1                 # closest to the last waypoint
    X = t[idx, 1] + rng.normal(0, 1.0, B); Y = t[idx, 2] + rng.normal(0, 1.0, B); P = rng.uniform(-10, 10, B)
    dev = torch.device("cuda", 0)

    def run(x, y, p):
        ref, err, stop = rt.get_waypoints_batch(*(torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev) for a in (x, y, p)))
        torch.cuda.synchronize()
        return ref.cpu().numpy(), err.cpu().numpy(), stop.cpu().numpy()

    ref, err, stop = _composition_free(run, (X, Y, P), nc, seed=9, names=("ref", "err", "stop"))
    assert (stop == int(short_path)).all()
    for b in range(B):
        o = get_waypoints(t, H, dt, X[b], Y[b], P[b])
        for i, k in enumerate(KEYS):
            np.testing.assert_allclose(ref[b, i], o[k], rtol=0, atol=1e-12, err_msg="pose %d: %s" % (b, k))
        np.testing.assert_allclose(err[b], [o["s0"], o["e_y0"], o["e_psi0"]], rtol=0, atol=1e-12)
        assert bool(stop[b]) == o["stop"], b


# ---- the fleet step past 4096 vehicles (waypoint stride, kernel F / S work order)

@pytest.mark.parametrize("N", [20, 40])
def test_fleet_step_past_4096_vehicles(N, nc):
    """One FleetController of B > 4096 vehicles (the waypoint kernel's stride; kernel F or S past its grid) over a few steps: bitwise
    equal to controllers of at most 1000 vehicles fed the same slices, a sample of 32 vehicles equal to the per-vehicle host pipelines,
    and one step captured in a graph and replayed equal to the eager step."""
    import torch
    from test_fleet_step import _path, _poses, _fleet, _dev_step, _HostFleet, _compare
    B, T, part = 4096 + 555, 3, 1000
    assert R.waypoints_grid(B) < B and R.work_ordered(R.f_grid(nc, B) if N == 20 else R.s_grid(nc, B, 2)[1], B)
    path = _path()
    poses = _poses(B, T, seed=12)
    big, graphed = _fleet(N, B, path), _fleet(N, B, path)
    small = [(sl, _fleet(N, sl.stop - sl.start, path)) for sl in (slice(i, min(i + part, B)) for i in range(0, B, part))]
    rng = np.random.default_rng(13)
    pick = np.array(sorted({0, 1, 2047, 2048, 4095, 4096, B - 2, B - 1} | set(rng.integers(0, B, 24).tolist())))
    host = _HostFleet(N, len(pick), path)
    keys = ("status", "mode", "valid", "safe", "ack", "x", "u")
    for t in range(T):
        dev = _dev_step(big, poses[t])
        for sl, fc in small:
            sub = _dev_step(fc, poses[t][:, sl])
            for k in keys:
                _bits(dev[k][sl], sub[k], "step %d, vehicles %d..%d: %s" % (t, sl.start, sl.stop, k))
        ref = host.step(poses[t][:, pick])
        _compare(t, {k: v[pick] for k, v in dev.items()}, ref)
        if t < T - 1:
            _dev_step(graphed, poses[t])
    ins = [torch.zeros(B, dtype=torch.float64, device=graphed.device) for _ in range(7)]
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        graphed.step(*ins)
    for i in range(7):
        ins[i].copy_(torch.as_tensor(poses[T - 1][i], device=graphed.device))
    g.replay()
    torch.cuda.synchronize()
    got = {"status": graphed.status, "mode": graphed.mode, "valid": graphed.valid, "safe": graphed.safe_count, "ack": graphed.ack,
           "x": graphed.x_opt, "u": graphed.w_opt}
    for k in keys:
        _bits(got[k].cpu().numpy(), dev[k], "captured step: " + k)
