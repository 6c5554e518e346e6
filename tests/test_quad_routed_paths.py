"""The quadrotor's routed solve (admpc_quad_solve_batch_routed) on every kernel path it takes.

Every cluster handle runs over the whole batch and skips the instances whose route names another cluster: one skip in the one-block kernel
text (three instantiations; WidePath's next() crosses two barriers) and one in the two-wave kernel of N = 20 (a draw on wave 0, a barrier,
the hand-over at the loop head).  Each path of quad_routed_spec.ROUTED_PATHS is held

  1. against the oracle run with the GPs of each instance's own cluster (statuses and iteration counts identical, |du|, |dx| <= 1e-8, cost
     1e-9 relative: the figures of every unrouted quadrotor path), out-of-range routes failing untouched;
  2. bit for bit against the plain solve of handle c over exactly the instances routed to c -- the suite holds that a quadrotor solve
     does not depend on the composition of its batch -- on the drawn route and on degenerate ones, from sentinel-filled outputs;
  3. (the kernels whose skip crosses a barrier, and the largest one-wave footprint) on both sides of the ticket switch;
  4. with a first-node GP state that is not x0, and with an instance per cluster that fails.

tests/test_quad_routed_paths_cpu.py holds the table against the launch sites and the inputs against passing vacuously.

path          N   fp64 oracle against 80-bit on the path's routed batch, max |du| / |dx|     bound
dense40_N10   10  1.5e-12 / 2.7e-12                                                          1e-8
generic_N10   10  1.5e-12 / 2.7e-12                                                          1e-8
generic_N5     5  3.1e-14 / 5.3e-14                                                          1e-8
generic_N16   16  5.0e-11 / 1.2e-10                                                          1e-8
wide_N17      17  1.1e-10 / 1.9e-10                                                          1e-8
wide_N24      24  4.6e-10 / 1.2e-09                                                          1e-8
wide_N20      20  2.2e-10 / 4.0e-10                                                          1e-8
seg_N20       20  2.2e-10 / 4.0e-10                                                          1e-8
"""
import numpy as np
import pytest

import batch_regimes as R
import quad_routed_spec as Q
from test_batch_regimes import _bits, _composition_free, _quad_args, _take

pytestmark = pytest.mark.gpu

PATHS = Q.TWO_WAVE_FIRST
NAMES = ("x", "u", "cost", "status", "iters")
SENT = (-7.25, -3, -5)                                            # cost, status, iters before a solve: values no solve writes


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


@pytest.fixture(scope="module")
def ensembles(nc):
    """ensembles(path, K=3): the QuadEnsembleBatchSolver of a path with clusters quad_gps(seed=1 .. K), created under the path's
    environment (read at the creation of a handle, removed afterwards); kept for the module."""
    from ad_mpc_amd.engine import QuadEnsembleBatchSolver
    made = {}

    def get(path, K=3):
        if (path, K) not in made:
            N, env, _ = Q.ROUTED_PATHS[path]
            cent = Q.CENT if K == 3 else np.c_[np.linspace(-2.0, 2.0, K), np.full(K, 0.5)]
            with pytest.MonkeyPatch.context() as mp:
                for k, v in env.items():
                    mp.setenv(k, v)
                made[path, K] = QuadEnsembleBatchSolver(Q.path_config(path), Q.clusters(K), cent, Q.FEATS, device=0)
                for k in env:
                    mp.delenv(k)
        return made[path, K]

    yield get
    for e in made.values():
        e.close()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _routed(ens, route, x0, yref, yref_e, xbar, ubar, gp_state=None):
    """One routed solve from sentinel-filled outputs: host (x, u, cost, status, iters)."""
    import torch
    n = len(route)
    xb, ub = _dev(xbar).clone(), _dev(ubar).clone()
    cost = torch.full((n,), SENT[0], dtype=torch.float64, device="cuda")
    st = torch.full((n,), SENT[1], dtype=torch.int32, device="cuda"); it = torch.full((n,), SENT[2], dtype=torch.int32, device="cuda")
    ens.solve(_dev(np.asarray(route, dtype=np.int32)), _dev(x0), _dev(yref), _dev(yref_e), xb, ub, cost, st, it, gp_state=None if gp_state is None else _dev(gp_state))
    torch.cuda.synchronize()
    return xb.cpu().numpy(), ub.cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


def _assert_routed_is_plain(ens, route, args, g, what, gp_state=None):
    """For every cluster c the routed results of the instances with route == c carry the bits of handle c's plain solve of exactly those
    instances; every entry of cost, status and iters has left its sentinel; an instance whose route names no cluster has status 4, cost
    +inf and its iterate's bits.  Returns the plain results scattered back into batch order."""
    route = np.asarray(route)
    K = len(ens.solvers)
    inr = (route >= 0) & (route < K)
    plain = [np.zeros_like(a) for a in g]
    for c in range(K):
        m = route == c
        if not m.any():
            continue
        p = ens.solvers[c].solve_numpy(*_take(args, m), gp_state=None if gp_state is None else gp_state[m])
        for k, (a, b) in enumerate(zip(g, p)):
            _bits(a[m], b, "%s: %s of cluster %d, routed against handle %d's plain solve" % (what, NAMES[k], c, c))
            plain[k][m] = b
    for a, sent, name in zip(g[2:], SENT, NAMES[2:]):
        assert (a != sent).all(), "%s: %s of %s was not written" % (what, name, np.flatnonzero(a == sent)[:8])
    assert (g[3][~inr] == 4).all() and np.isposinf(g[2][~inr]).all(), (what, g[3][~inr], g[2][~inr])
    if not inr.all():
        _bits(g[0][~inr], args[3][~inr], what + ": iterate of an instance without a cluster")
        _bits(g[1][~inr], args[4][~inr], what + ": inputs of an instance without a cluster")
    return plain


# ---- 1. every path against the oracle ---------------------------------------------------------------------------------------------------

_ORACLE = {}


def _oracle96(qoracle, path):
    """The oracle on the batch of `path` under each instance's own cluster, computed once per horizon."""
    N = Q.ROUTED_PATHS[path][0]
    if N not in _ORACLE:
        cfg, s, xs, us, route = Q.scenario(path)
        _ORACLE[N] = Q.oracle_routed(qoracle, cfg, Q.clusters(), Q.with_off(route), s)
    return _ORACLE[N]


@pytest.mark.parametrize("path", PATHS)
def test_routed_path_against_the_oracle(ensembles, qoracle, path):
    """K = 3 distinct GP sets, B = 96, the route from `select` on drawn features (equal to the numpy spec's), two routes out of range."""
    cfg, s, xs, us, want = Q.scenario(path)
    ens = ensembles(path)
    route = ens.select(_dev(xs), _dev(us)).cpu().numpy()
    np.testing.assert_array_equal(route, want)
    route = Q.with_off(route)
    g = _routed(ens, route, *_quad_args(s))
    idx, o = _oracle96(qoracle, path)
    off = sorted(Q.OFF)
    assert sorted(set(range(Q.B1)) - set(idx.tolist())) == off
    Q.assert_parity(_take(g, idx), o, cfg, path)
    np.testing.assert_array_equal(g[0][idx][:, 0], s["x0"][idx])
    assert (g[3][off] == 4).all() and np.isposinf(g[2][off]).all()
    _bits(g[0][off], s["xbar"][off], "iterate of an out-of-range route"); _bits(g[1][off], s["ubar"][off], "inputs of an out-of-range route")


# ---- 2. routed equals plain, bit for bit ------------------------------------------------------------------------------------------------

def _degenerate_routes(route):
    B = len(route)
    return {
        "drawn": Q.with_off(route),
        "all to cluster 1": np.ones(B, dtype=np.int32),
        "none to cluster 1": np.where(route == 1, (np.arange(B) % 2) * 2, route).astype(np.int32),
        "all out of range": np.where(np.arange(B) % 2 == 0, 3, -1 - np.arange(B) % 5).astype(np.int32),
    }


@pytest.mark.parametrize("path", PATHS)
def test_routed_results_carry_the_bits_of_the_plain_solves(ensembles, path):
    """The batch of part 1 under the drawn route and under degenerate ones (every instance to cluster 1: handles 0 and 2 pass over the
    whole batch and write nothing; no instance to cluster 1; every route out of range), then B = 1 with route 2, K = 1, and K = 8 with
    every route used.  A write by a handle that should have skipped, before or after the owner's, changes bits: handle c solves in place."""
    cfg, s, xs, us, route = Q.scenario(path)
    args = _quad_args(s)
    ens = ensembles(path)
    for what, rt in _degenerate_routes(route).items():
        used = set(rt.tolist())
        assert {"drawn": used == {0, 1, 2, 7, -1}, "all to cluster 1": used == {1}, "none to cluster 1": used == {0, 2},
                "all out of range": not used & {0, 1, 2}}[what]
        g = _routed(ens, rt, *args)
        _assert_routed_is_plain(ens, rt, args, g, "%s, %s" % (path, what))
        if what == "all out of range":
            assert (g[4] == 0).all()
    one = _take(args, slice(17, 18))
    _assert_routed_is_plain(ens, [2], one, _routed(ens, [2], *one), path + ", B = 1")
    for K in (1, 8):
        ek = ensembles(path, K)
        rt = ((np.arange(Q.B1) * 5 + 3) % K).astype(np.int32)
        assert set(rt.tolist()) == set(range(K))
        g = _routed(ek, rt, *args)
        _assert_routed_is_plain(ek, rt, args, g, "%s, K = %d" % (path, K))
        assert (g[3] == 0).all()
        if K == 8:                                                 # the clusters differ: a neighbour's handle gives other bits
            other = ek.solvers[1].solve_numpy(*_take(args, rt == 0))
            assert (other[1] != g[1][rt == 0]).any(axis=(1, 2)).all()


# ---- 3. both sides of the ticket switch -------------------------------------------------------------------------------------------------

SWITCH_PATHS = ["seg_N20", "wide_N17", "wide_N24", "generic_N16"]


def _run_route(B, seed):
    """Clusters drawn uniformly; the first half of the batch sorted by cluster (long runs: a workgroup meets many skips in a row), the
    second half mixed; three routes that name no cluster."""
    rt = np.random.default_rng(seed).integers(0, 3, B).astype(np.int32)
    rt[:B // 2] = np.sort(rt[:B // 2])
    off = [5, B // 2, B - 1]
    rt[off] = [7, -1, 3]
    return rt, off


@pytest.mark.parametrize("side", ["below", "past"])
@pytest.mark.parametrize("path", SWITCH_PATHS)
def test_routed_path_across_the_ticket_switch(ensembles, qoracle, nc, path, side):
    """Below: B = 8 num_cu (static stride for every footprint); past: B > 64 num_cu (32 num_cu for the two-wave N = 20 kernel), the
    ticket counter for every footprint.  The same bits in sub-batches and under a permutation; the bits of the plain solves; the oracle on
    every instance below the switch and on 512 past it (the first and the last instance, seeded others: the plain solve is held against
    the oracle everywhere by test_batch_regimes.py, and the bits tie the rest to it)."""
    from ad_mpc_amd.quad_scenarios import random_quad_scenarios
    N, _, kernel = Q.ROUTED_PATHS[path]
    seg20 = kernel == Q.SEG
    B = R.quad_below(nc) if side == "below" else R.quad_past(nc, seg20)
    lo, hi = R.quad_grid(nc, B, seg20)
    assert R.quad_tickets(lo, B) == R.quad_tickets(hi, B) == (side == "past")
    cfg = Q.path_config(path)
    s = random_quad_scenarios(B, cfg, seed=330 + N)
    route, off = _run_route(B, seed=N)
    assert (np.bincount(route[(route >= 0) & (route < 3)]) >= B // 6).all()
    ens = ensembles(path)
    args = _quad_args(s)
    g = _composition_free(lambda rt, *a: _routed(ens, rt, *a), (route,) + args, nc, seed=N)
    _assert_routed_is_plain(ens, route, args, g, "%s %s" % (path, side))
    assert (g[3][off] == 4).all()
    sample = np.arange(B)
    if side == "past":
        must = {0, B - 1} | set(off)
        rest = [int(i) for i in np.random.default_rng(N + 1).permutation(B) if int(i) not in must][:512 - len(must)]
        sample = np.array(sorted(must | set(rest)))
        assert len(sample) == 512 and sample[0] == 0 and sample[-1] == B - 1
    idx, o = Q.oracle_routed(qoracle, cfg, Q.clusters(), route, s, idx=sample)
    assert len(idx) == len(sample) - len(off)
    Q.assert_parity(_take(g, idx), o, cfg, "%s %s" % (path, side))


# ---- 4. first-node GP state and a failing instance --------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", PATHS)
def test_first_node_gp_state_and_a_failing_instance_per_cluster(ensembles, qoracle, path):
    """B = 32.  A gp_state that is not x0 through QuadEnsembleBatchSolver.solve against the oracle's gp_state= (and it moves the solution).
    Then NaN in x0 of one instance per cluster: each fails as handle c's plain solve fails it (status, cost and iterate from that solve),
    and every other instance keeps the bits it has without the NaN."""
    cfg, s, xs, us, route = Q.scenario(path)
    B = 32
    s = {k: v[:B] for k, v in s.items()}
    route = route[:B]
    assert (np.bincount(route, minlength=3) >= 3).all()
    args = _quad_args(s)
    ens = ensembles(path)
    gs = Q.gp_state(s)
    g = _routed(ens, route, *args, gp_state=gs)
    idx, o = Q.oracle_routed(qoracle, cfg, Q.clusters(), route, s, gp_state=gs)
    assert len(idx) == B
    Q.assert_parity(g, o, cfg, path + " gp_state")
    _assert_routed_is_plain(ens, route, args, g, path + ", gp_state", gp_state=gs)
    clean = _routed(ens, route, *args)
    assert (np.abs(clean[1] - g[1]).reshape(B, -1).max(axis=1) > 1e-9).sum() > B // 2
    bad = [int(np.flatnonzero(route == c)[1]) for c in range(3)]
    x0 = s["x0"].copy(); x0[bad, 1] = np.nan
    nargs = (x0,) + args[1:]
    gn = _routed(ens, route, *nargs)
    plain = _assert_routed_is_plain(ens, route, nargs, gn, path + ", NaN in x0")
    assert (plain[3][bad] != 0).all() and (gn[3][bad] == plain[3][bad]).all() and (gn[2][bad] == plain[2][bad]).all(), (gn[3][bad], plain[3][bad])
    _bits(gn[0][bad], s["xbar"][bad], "iterate of a failed instance"); _bits(gn[1][bad], s["ubar"][bad], "inputs of a failed instance")
    keep = np.ones(B, dtype=bool); keep[bad] = False
    for a, b, k in zip(gn, clean, NAMES):
        _bits(a[keep], b[keep], "%s, neighbours of the failed instances: %s" % (path, k))
