"""The car's routed solve (admpc_solve_batch_routed) on every kernel and launch regime it takes.

Every cluster handle runs over the whole batch with first = 0; a status array filled with 0 / -2 tells each kernel which instances are
its own.  Kernel R (admpc_linearize_kernel + admpc_rowqp_kernel) is where that is most delicate: up to four instances share a wave, the
row past the end recomputes the last instance, a split batch reads the status again in its second phase, a chunked batch offsets it.
Each path of car_routed_spec.PATHS is held

  1. against the oracle run with the config of each instance's own cluster (statuses and iteration counts identical, |du|, |dx| within
     the suite's figures: 1e-8 up to N = 32, 1e-7 beyond and in SQP mode with a tolerance), out-of-range routes failing untouched,
     every output leaving its sentinel;
  2. bit for bit against the plain solve, on a fresh handle, of exactly the instances routed to each cluster, on the drawn route and
     on degenerate ones (all to one cluster, an empty cluster, b % K, blocks of four);
  3. (rows2, rows4, split) in sub-batches and under a permutation: the same bits;
  4. with a non-finite instance per cluster; 5. without the optional outputs; 6. on one ensemble over growing and shrinking batches;
  7. captured into a graph and replayed on a new route; and 8. admpc_select_cluster_batch against its numpy statement.

tests/test_car_routed_paths_cpu.py holds the table against the launch code and the inputs against passing vacuously.  The short horizon
is N = 17, not 13: on gp_structures.car_batch 10 % of the instances iterate at N = 13 and none of the fastest third, 30 % at N = 17.
In the two paths with an SQP tolerance every fourth instance starts from its converged iterate (car_routed_spec.scenario): from the cold
iterate three QPs end every instance at the limit, and the stop test would never fire.

Measured on an MI355X (256 CUs); the oracle's own distance from 80-bit arithmetic is on the whole routed batch:

path               N   B     fp64 oracle from 80-bit |du| / |dx|   device from oracle |du| / |dx|   bound   wall time of case 1
R17_rows1          17  96    1.0e-13 / 5.7e-14                     4.5e-14 / 3.9e-14                1e-8    0.32 s
R17_rows2          17  1189  1.3e-13 / 5.7e-14                     1.6e-13 / 1.1e-13                1e-8    0.03 s
R17_rows4          17  2213  1.4e-13 / 5.7e-14                     1.6e-13 / 1.2e-13                1e-8    0.06 s
R17_split          17  4261  1.4e-13 / 6.4e-14                     1.8e-13 / 1.2e-13                1e-8    0.12 s
R17_forced_split   17  97    1.0e-13 / 5.7e-14                     4.5e-14 / 3.9e-14                1e-8    0.03 s
R17_chunked        17  97    1.0e-13 / 5.7e-14                     4.5e-14 / 3.9e-14                1e-8    0.01 s
R40                40  96    2.6e-13 / 1.4e-13                     1.4e-13 / 4.3e-14                1e-7    0.01 s
S40_mixed          40  96    2.3e-13 / 1.0e-13                     5.0e-14 / 2.8e-14                1e-7    0.01 s
F20_sqp3           20  96    3.8e-14 / 1.6e-14                     1.6e-14 / 7.1e-15                1e-8    0.01 s
R20_sqp_tol        20  96    3.8e-14 / 1.6e-14                     1.3e-14 / 7.1e-15                1e-7    0.06 s
R17_sqp_tol_split  17  97    3.0e-14 / 2.1e-14                     1.8e-14 / 7.1e-15                1e-7    0.05 s
(the first case also loads the library and warms the device up; the SQP rows hold 23 converged and 70 / 71 unconverged instances)
"""
import time

import numpy as np
import pytest

import batch_regimes as R
import car_routed_spec as CR
import gp_structures as G
from test_batch_regimes import _bits, _composition_free, _take
from test_gpu_parity import _assert_parity, tol_for, TOL_LONG

pytestmark = pytest.mark.gpu

PATHS = list(CR.PATHS)
NAMES = ("x", "u", "cost", "status", "iters")
SENT = (-7.25, -3, -5)                                            # cost, status, iters before a solve: values no solve writes


@pytest.fixture(scope="module")
def nc():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return R.num_cu()


def _ensemble_class():
    from ad_mpc_amd.engine import EnsembleBatchSolver, _Ensemble

    class ConfigEnsemble(EnsembleBatchSolver):
        """EnsembleBatchSolver over a list of configs: every cluster with its own GP structure, or none."""

        def __init__(self, cfgs, centroids, feats, device=0):
            self.ensemble = None
            _Ensemble.__init__(self, cfgs, centroids, feats, device)

    return ConfigEnsemble


def _under(env, make):
    """make() with the environment of a path set: the library reads it at the creation of a handle; removed afterwards."""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        out = make()
        for k in env:
            mp.delenv(k)
    return out


def _fresh_ensemble(path, cent=None):
    cfgs = CR.path_configs(path)
    cent = np.array([[4.0], [8.0], [12.0]]) if cent is None else cent
    return _under(CR.PATHS[path]["env"], lambda: _ensemble_class()(cfgs, cent, CR.FEATS, device=0))


@pytest.fixture(scope="module")
def ensembles(nc, oracle_omp):
    """ensembles(path): the ensemble of a path, its handles created under the path's environment, its centroids those of the path's
    batch; kept for the module."""
    made = {}

    def get(path):
        if path not in made:
            made[path] = _fresh_ensemble(path, CR.scenario(path, nc, oracle_omp)[3])
        return made[path]

    yield get
    for e in made.values():
        e.close()


def _plain(path, c, args):
    """Handle c's plain solve of `args` on a BatchSolver of its own, created under the path's environment."""
    from ad_mpc_amd.engine import BatchSolver
    eng = _under(CR.PATHS[path]["env"], lambda: BatchSolver(CR.path_configs(path)[c], device=0))
    out = eng.solve_numpy(*args)
    eng.close()
    return out


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _routed(ens, route, x0, yref, yref_e, p, xbar, ubar, outputs=(True, True, True)):
    """One routed solve from sentinel-filled outputs: host (x, u, cost, status, iters); outputs: which of cost, status, iters are passed
    (the others stay at their sentinels)."""
    import torch
    n = len(route)
    xb, ub = _dev(xbar).clone(), _dev(ubar).clone()
    cost = torch.full((n,), SENT[0], dtype=torch.float64, device="cuda")
    st = torch.full((n,), SENT[1], dtype=torch.int32, device="cuda"); it = torch.full((n,), SENT[2], dtype=torch.int32, device="cuda")
    ens.solve(_dev(np.asarray(route, dtype=np.int32)), _dev(x0), _dev(yref), _dev(yref_e), _dev(p), xb, ub,
              cost if outputs[0] else None, st if outputs[1] else None, it if outputs[2] else None)
    torch.cuda.synchronize()
    return xb.cpu().numpy(), ub.cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


def _assert_written_and_off(g, route, args, what):
    """Every in-range entry of cost, status and iters has left its sentinel; an instance whose route names no cluster has status 4, cost
    +inf, no iterations and its iterate's bits."""
    inr = CR.in_range(route)
    for a, sent, name in zip(g[2:], SENT, NAMES[2:]):
        assert (a != sent).all(), "%s: %s of %s was not written" % (what, name, np.flatnonzero(a == sent)[:8])
    assert (g[3][~inr] == 4).all() and np.isposinf(g[2][~inr]).all() and (g[4][~inr] == 0).all(), (what, g[3][~inr], g[2][~inr], g[4][~inr])
    if not inr.all():
        _bits(g[0][~inr], args[4][~inr], what + ": iterate of an instance without a cluster")
        _bits(g[1][~inr], args[5][~inr], what + ": inputs of an instance without a cluster")


def _assert_routed_is_plain(path, route, args, g, what):
    """For every cluster c the routed results of the instances with route == c carry the bits of handle c's plain solve, on a fresh
    handle, of exactly those instances.  Returns the plain results scattered back into batch order."""
    route = np.asarray(route)
    plain = [np.zeros_like(a) for a in g]
    for c in range(CR.K):
        m = route == c
        if not m.any():
            continue
        p = _plain(path, c, _take(args, m))
        for k, (a, b) in enumerate(zip(g, p)):
            _bits(a[m], b, "%s: %s of cluster %d, routed against handle %d's plain solve" % (what, NAMES[k], c, c))
            plain[k][m] = b
    _assert_written_and_off(g, route, args, what)
    return plain


# ---- 1. every path against the oracle ---------------------------------------------------------------------------------------------------

def _finite(o):
    """Instances whose SQP iteration stayed bounded in the oracle: full Newton steps without a line search may diverge, to finite
    garbage on both sides that cannot be compared (test_gp_structures.py::test_car_sqp_with_a_tolerance)."""
    return (o[3] != 4) & (np.abs(o[0]).max(axis=(1, 2)) < 1e3) & (np.abs(o[1]).max(axis=(1, 2)) < 1e3)


@pytest.mark.parametrize("path", PATHS)
def test_routed_path_against_the_oracle(ensembles, oracle_omp, nc, path):
    """K = 3 clusters of different structure, the route from `select` on (x0, the first row of ubar) -- equal to the numpy rule's --
    with three routes out of range; the oracle per cluster on route == c."""
    t0 = time.perf_counter()
    r = CR.PATHS[path]
    cfgs, s, want, cent = CR.scenario(path, nc, oracle_omp)
    B = len(want)
    assert B == CR.batch_size(path, nc)
    if "R" in r["kernels"]:                                         # the regime the table claims, on this device
        assert all(rows == r["rows"] and two == (r["split"] is not None) for rows, two in CR.regime(path, nc)), CR.regime(path, nc)
        assert R.rowqp_lds_rows(r["N"], 8) == 4 and R.rowqp_per_cu(r["N"], 8, r["rows"]) == 4
    ens = ensembles(path)
    args = CR.car_args(s)
    route = ens.select(_dev(s["x0"]), _dev(s["ubar"])[:, 0, :]).cpu().numpy()
    np.testing.assert_array_equal(route, want)
    route = CR.with_off(route)
    assert (np.bincount(route[CR.in_range(route)], minlength=CR.K) >= B // 4).all()
    g = _routed(ens, route, *args)
    _assert_written_and_off(g, route, args, path)
    idx, o = CR.oracle_routed(oracle_omp, cfgs, route, s)
    assert sorted(set(range(B)) - set(idx.tolist())) == sorted(CR.OFF)
    gi = _take(g, idx)
    tol_on = path in CR.SQP_TOL_PATHS
    if not r.get("sqp"):
        assert (o[4] > 0).mean() >= 0.25
    np.testing.assert_array_equal(gi[3], o[3], err_msg=path)
    if tol_on:
        assert set(np.unique(o[3]).tolist()) <= {0, 2} and (o[3] == 0).any() and (o[3] == 2).any(), np.bincount(o[3])
        good = _finite(o)
        assert good.sum() >= len(good) - 8
        bound = CR.SQP_TOL
    else:
        assert (o[3] == 0).all()
        np.testing.assert_array_equal(gi[4], o[4], err_msg=path)
        good = np.ones(len(idx), dtype=bool)
        bound = tol_for(r["N"])
    du, dx = np.abs(gi[1][good] - o[1][good]).max(), np.abs(gi[0][good] - o[0][good]).max()
    print("CAR-ROUTED %-18s N %2d B %5d  device from oracle max|du| %.1e max|dx| %.1e  bound %.0e  statuses %s"
          % (path, r["N"], B, du, dx, bound, np.bincount(g[3], minlength=5).tolist()))
    assert du <= bound and dx <= bound, (path, du, dx)
    if not tol_on:
        rc = route[idx]
        for c in range(CR.K):                                       # kernel S's nominal cluster: TOL_LONG, the figure of kernel S without GPs
            m = rc == c
            _assert_parity(_take(gi, m), _take(o, m), TOL_LONG if r["kernels"][c] == "S" else tol_for(r["N"]))
    print("CAR-ROUTED %-18s wall time of the case %.2f s" % (path, time.perf_counter() - t0))


# ---- 2. routed equals plain, bit for bit ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
def test_routed_results_carry_the_bits_of_the_plain_solves(ensembles, oracle_omp, nc, path):
    """The batch of part 1 under the drawn route and the degenerate ones of car_routed_spec.degenerate_routes.  A write by a handle that
    should have skipped, before or after the owner's, changes bits: every handle solves in place.  A skipped row that costs its wave an
    iteration changes the iteration counts of its neighbours."""
    cfgs, s, route, _ = CR.scenario(path, nc, oracle_omp)
    args = CR.car_args(s)
    ens = ensembles(path)
    for what, rt in CR.degenerate_routes(route).items():
        used = set(rt.tolist())
        assert {"drawn": used == {0, 1, 2, 7, -1, CR.K}, "all to cluster 1": used == {1}, "none to cluster 1": used == {0, 2},
                "b % K": used == {0, 1, 2}, "blocks of four": used == {0, 1, 2}}[what]
        g = _routed(ens, rt, *args)
        _assert_routed_is_plain(path, rt, args, g, "%s, %s" % (path, what))
    assert CR.quadruple_mix(CR.degenerate_routes(route)["blocks of four"]) <= {1, 2}           # 2: the last, shorter block alone
    one = _take(args, slice(17, 18))
    _assert_routed_is_plain(path, [2], one, _routed(ens, [2], *one), path + ", B = 1")


# ---- 3. composition on both sides of the row-count switches and past one round of waves -------------------------------------------------

@pytest.mark.parametrize("path", ["R17_rows2", "R17_rows4", "R17_split"])
def test_routed_kernel_r_does_not_depend_on_the_composition_of_the_batch(ensembles, oracle_omp, nc, path):
    """Two and four instances per wave and the two phases of a batch past one round of waves, each against sub-batches of num_cu
    instances (one per wave, one launch) and against a permuted batch: the same bits.  fp64 on both sides of the switches that
    test_fp32_path.py::test_row_count_and_split_switches pins for fp32."""
    r = CR.PATHS[path]
    cfgs, s, route, _ = CR.scenario(path, nc, oracle_omp)
    B = len(route)
    assert R.rowqp_lds_rows(17, 8) == 4 and R.rowqp_per_cu(17, 8, 4) == 4
    rows = R.rowqp_rows(nc, B)
    assert rows == r["rows"] and R.rowqp_splits(nc, B, rows) == (r["split"] == "default")
    assert R.rowqp_rows(nc, nc) == 1 and not R.rowqp_splits(nc, nc, 1)
    ens = ensembles(path)
    route = CR.with_off(route)
    args = CR.car_args(s)
    g = _composition_free(lambda rt, *a: _routed(ens, rt, *a), (route,) + args, nc, seed=B)
    _assert_written_and_off(g, route, args, path)
    inr = CR.in_range(route)
    assert (g[3][inr] == 0).all() and (g[4][inr] > 0).mean() >= 0.25


# ---- 4. a failing instance per cluster --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["R17_rows4", "R40"])
def test_a_failing_instance_per_cluster(ensembles, oracle_omp, nc, path):
    """NaN in x0, +inf and NaN in yref, one instance per cluster, each in a wave it shares with another cluster: those fail (status 4,
    cost +inf, the iterate's bits kept), and every other instance keeps the bits it has without them -- a non-finite row that a handle
    skips must not cost a live row of its wave an iteration."""
    cfgs, s, route, _ = CR.scenario(path, nc, oracle_omp)
    ens = ensembles(path)
    route = CR.with_off(route)
    clean = _routed(ens, route, *CR.car_args(s))
    sp, bad = CR.poisoned(s, route, rows=4)
    assert sorted(route[bad].tolist()) == [0, 1, 2] and (clean[3][bad] == 0).all()
    args = CR.car_args(sp)
    g = _routed(ens, route, *args)
    _assert_written_and_off(g, route, args, path)
    assert (g[3][bad] == 4).all() and np.isposinf(g[2][bad]).all(), (g[3][bad], g[2][bad])
    _bits(g[0][bad], s["xbar"][bad], "iterate of a failed instance"); _bits(g[1][bad], s["ubar"][bad], "inputs of a failed instance")
    keep = np.ones(len(route), dtype=bool); keep[bad] = False
    for a, b, k in zip(g, clean, NAMES):
        _bits(a[keep], b[keep], "%s, neighbours of the failed instances: %s" % (path, k))


# ---- 5. optional outputs ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["R17_rows1", "R17_forced_split", "F20_sqp3", "R20_sqp_tol"])
def test_optional_outputs(ensembles, oracle_omp, nc, path):
    """status = NULL (no merge kernel runs; the handles' internal arrays alone carry the skip), cost = iters = NULL, and all three: the
    iterate carries the bits of the full call, and so does every output that is passed."""
    cfgs, s, route, _ = CR.scenario(path, nc, oracle_omp)
    ens = ensembles(path)
    route = CR.with_off(route)
    args = CR.car_args(s)
    full = _routed(ens, route, *args)
    for outputs in ((True, False, True), (False, True, False), (False, False, False)):
        g = _routed(ens, route, *args, outputs=outputs)
        what = "%s, cost / status / iters passed: %s" % (path, outputs)
        _bits(g[0], full[0], what + ": x"); _bits(g[1], full[1], what + ": u")
        for k, on in enumerate(outputs):
            if on:
                _bits(g[2 + k], full[2 + k], what + ": " + NAMES[2 + k])
            else:
                assert (g[2 + k] == SENT[k]).all(), what


# ---- 6. one ensemble, several calls -----------------------------------------------------------------------------------------------------

def test_one_ensemble_over_growing_and_shrinking_batches(nc):
    """B = 96, then the two-instances-per-wave size (the workspaces grow), then 31 on the stale status, key and order arrays of the larger
    call: each equals a fresh ensemble's result, bit for bit."""
    path = "R17_rows1"
    one = _fresh_ensemble(path)
    for step, B in enumerate((96, R.rowqp_sizes(nc)["rows2"], 31)):
        s = G.car_batch(17, B)
        route = CR.with_off(CR.select_numpy(s["x0"], s["ubar"][:, 0, :], CR.FEATS, CR.tercile_centroids(s["x0"][:, 3])))
        assert (np.bincount(route[CR.in_range(route)], minlength=CR.K) >= B // 4).all()
        args = CR.car_args(s)
        got = _routed(one, route, *args)
        fresh = _fresh_ensemble(path)
        want = _routed(fresh, route, *args)
        fresh.close()
        for a, b, k in zip(got, want, NAMES):
            _bits(a, b, "call %d (B = %d): %s" % (step, B, k))
        _assert_written_and_off(got, route, args, "call %d" % step)
        assert (got[4] > 0).any()
    one.close()


# ---- 7. capture -------------------------------------------------------------------------------------------------------------------------

def test_captured_routed_solve_replays_on_a_new_route(ensembles, oracle_omp, nc):
    """R40 after an eager call has sized the workspaces: one routed solve captured into a graph (the pattern of
    test_batch_regimes.py::test_captured_work_ordered_solve_replays), replayed with new routes and new inputs written into the captured
    buffers; every replay equals the eager result of its inputs, bit for bit."""
    import torch
    path = "R40"
    cfgs, s, route, _ = CR.scenario(path, nc, oracle_omp)
    B = len(route)
    ens = ensembles(path)
    s2 = G.car_batch(40, 2 * B); s2 = {k: v[B:] for k, v in s2.items()}
    cases = [(CR.with_off(route), s), ((np.arange(B) % CR.K).astype(np.int32), s2), (CR.with_off(route[::-1].copy()), s2)]
    want = [_routed(ens, rt, *CR.car_args(sc)) for rt, sc in cases]
    assert (want[0][1] != want[2][1]).any()
    rbuf = _dev(cases[0][0])
    bufs = [_dev(cases[0][1][k]).clone() for k in G.CAR_ARGS]
    cost = torch.empty(B, dtype=torch.float64, device="cuda")
    st = torch.empty(B, dtype=torch.int32, device="cuda"); it = torch.empty_like(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ens.solve(rbuf, *bufs, cost, st, it)
    torch.cuda.current_stream().wait_stream(side)

    def replay(k):
        rbuf.copy_(_dev(cases[k][0]))
        for b, key in zip(bufs, G.CAR_ARGS):
            b.copy_(_dev(cases[k][1][key]))
        cost.fill_(SENT[0]); st.fill_(SENT[1]); it.fill_(SENT[2])
        g.replay()
        torch.cuda.synchronize()
        got = (bufs[4].cpu().numpy(), bufs[5].cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy())
        for a, b, name in zip(got, want[k], NAMES):
            _bits(a, b, "replay of case %d: %s" % (k, name))

    replay(1); replay(2); replay(2); replay(0)


# ---- 8. the selection kernel ------------------------------------------------------------------------------------------------------------

def _select(feats, xs, us, cent, B=None):
    """admpc_select_cluster_batch through the ABI: (return code, route)."""
    import ctypes as C
    import torch
    from ad_mpc_amd import _lib
    L = _lib.load()
    B = len(xs) if B is None else B
    route = torch.full((max(B, 1),), -9, dtype=torch.int32, device="cuda")
    f = (C.c_int32 * max(len(feats), 1))(*feats)
    cent = _dev(np.asarray(cent, dtype=np.float64))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = L.admpc_select_cluster_batch(0, B, len(feats), f, ptr(xs), ptr(us), int(cent.shape[0]), ptr(cent), ptr(route), None)
    torch.cuda.synchronize()
    return rc, route.cpu().numpy()[:B]


SELECT_FEATS = [[3], [8], [3, 4], [7, 8], [6, 7], [3, 5, 6], [8, 0, 7], [7, 8, 7]]


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_select_cluster_against_the_numpy_statement(nc, B):
    """One, two and three features from the state alone, the inputs alone (7, 8) and both; K = 1, 3 and 9; around the workgroup size;
    the input a row view ubar[:, 0, :] made contiguous by EnsembleBatchSolver.select; every cluster chosen at K = 9."""
    rng = np.random.default_rng(B)
    xs = rng.uniform(-2.0, 2.0, (B, 7)); ubar = rng.uniform(-2.0, 2.0, (B, 3, 2))
    for feats in SELECT_FEATS:
        for K in (1, 3, 9):
            cent = rng.uniform(-2.0, 2.0, (K, len(feats)))
            if K == 9 and B >= 255:                                 # next to nine instances: every cluster is somebody's nearest
                cent = np.c_[xs, ubar[:, 0, :]][:9, feats] + 0.01
            want = CR.select_numpy(xs, ubar[:, 0, :], feats, cent)
            rc, got = _select(feats, _dev(xs), _dev(ubar)[:, 0, :].contiguous(), cent)
            assert rc == 0
            np.testing.assert_array_equal(got, want, err_msg="%s K = %d" % (feats, K))
            if K == 9 and B >= 255:
                assert len(set(want.tolist())) == 9
    ens = _ensemble_class()([CR.path_configs("R17_rows1")[0]] * 3, [[-1.0, 0.5], [0.0, 0.0], [1.0, -0.5]], [4, 8], device=0)
    got = ens.select(_dev(xs), _dev(ubar)[:, 0, :]).cpu().numpy()                   # the row view itself
    ens.close()
    np.testing.assert_array_equal(got, CR.select_numpy(xs, ubar[:, 0, :], [4, 8], [[-1.0, 0.5], [0.0, 0.0], [1.0, -0.5]]))


def test_select_cluster_ties_and_non_finite_features(nc):
    """Exact ties go to the lower index: centroids symmetric about feature values that are small multiples of 1/8, at offsets that are
    too, so that both distances are the same double, in one, two and three features.  NaN and +-inf in a feature route to 0."""
    B = 64
    v = (np.arange(B) - 32) / 8.0
    xs = np.zeros((B, 7)); us = np.zeros((B, 2))
    xs[:, 3] = v; us[:, 1] = v[::-1]; xs[:, 5] = 0.25
    # cluster 1 and cluster 2 mirror each other about (v, v[::-1]) = (0.5, -0.625) -- instance 36 -- and about the line through it;
    # cluster 0 is far away
    for feats, cent in (([3], [[40.0], [1.0], [0.0]]),
                        ([3, 8], [[40.0, 40.0], [1.0, -0.625], [0.0, -0.625]]),
                        ([8, 3, 5], [[40.0, 40.0, 40.0], [-0.375, 0.75, 0.5], [-0.875, 0.25, 0.0]])):
        want = CR.select_numpy(xs, us, feats, cent)
        assert want[36] == 1 and CR.select_numpy(xs, us, feats, [cent[0], cent[2], cent[1]])[36] == 1          # the tie is exact: the lower index either way
        for cc in (cent, [cent[0], cent[2], cent[1]], [cent[2], cent[1], cent[0]]):
            rc, got = _select(feats, _dev(xs), _dev(us), cc)
            assert rc == 0
            np.testing.assert_array_equal(got, CR.select_numpy(xs, us, feats, cc), err_msg=str(feats))
    assert len(set(CR.select_numpy(xs, us, [3], [[40.0], [1.0], [0.0]]).tolist())) == 2
    xs2 = xs.copy(); xs2[5, 3] = np.nan; xs2[6, 3] = np.inf; xs2[7, 3] = -np.inf
    us2 = us.copy(); us2[9, 1] = np.nan
    cent = [[3.0, 3.0], [0.0, 0.0], [-3.0, -3.0]]
    rc, got = _select([3, 8], _dev(xs2), _dev(us2), cent)
    want = CR.select_numpy(xs2, us2, [3, 8], cent)
    assert rc == 0 and (want[[5, 6, 7, 9]] == 0).all() and (want != 0).sum() > B // 2
    np.testing.assert_array_equal(got, want)


def test_select_cluster_refusals(nc):
    """n_feat 0 and 4, a feature index 9 or -1, K = 0, null arrays: refused with ADMPC_EINVAL and nothing written; B = 0 is a no-op."""
    import ctypes as C
    from ad_mpc_amd import _lib
    L = _lib.load()
    xs, us = _dev(np.zeros((4, 7))), _dev(np.zeros((4, 2)))
    cent = [[0.0], [1.0]]
    for feats in ([], [3, 4, 5, 6], [9], [-1], [3, 9]):
        c = [[0.0] * max(len(feats), 1)] * 2
        rc, got = _select(feats, xs, us, c)
        assert rc != 0 and (got == -9).all(), feats
        assert L.admpc_last_error()
    rc, got = _select([3], xs, us, np.zeros((0, 1)))
    assert rc != 0 and (got == -9).all()
    for nul in range(4):
        a = [xs, us, _dev(np.asarray(cent)), _dev(np.zeros(4, dtype=np.int32))]
        a[nul] = None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        f = (C.c_int32 * 1)(3)
        assert L.admpc_select_cluster_batch(0, 4, 1, f, ptr(a[0]), ptr(a[1]), 2, ptr(a[2]), ptr(a[3]), None) != 0
    assert L.admpc_select_cluster_batch(0, 4, 1, None, C.c_void_p(xs.data_ptr()), C.c_void_p(us.data_ptr()), 2, None, None, None) != 0
    assert L.admpc_select_cluster_batch(0, -1, 1, (C.c_int32 * 1)(3), None, None, 2, None, None, None) != 0
    rc, got = _select([3], xs, us, cent, B=0)
    assert rc == 0
    assert L.admpc_select_cluster_batch(0, 0, 1, (C.c_int32 * 1)(3), None, None, 2, None, None, None) == 0
