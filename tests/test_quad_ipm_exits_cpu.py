"""What tests/test_quad_ipm_exits.py relies on, checked without a GPU, with the oracle alone: the inputs of quad_ipm_exits_spec reach every
exit of the interior point's loop (class counts), the fp64 and the 80-bit oracle take every instance through the same number of
iterations to the same status, their distance is what the spec's table says (the device tests' bounds come from it), and a restart moves
the answer by far more than any bound."""
import numpy as np
import pytest

import quad_ipm_exits_spec as E
import quad_routed_spec as Q

_ORACLES, _SOL = {}, {}


def _oracle(variant):
    from oracle.quad_oracle import QuadOracle
    if variant not in _ORACLES:
        _ORACLES[variant] = QuadOracle(variant)
    return _ORACLES[variant]


def _solve(variant, cfg, s):
    return _oracle(variant).solve_batch(cfg, *Q.quad_args(s), nthreads=16)


def _sol(variant, N, name):
    """(x, u, cost, status, iters) of the fp64 (variant None) or the 80-bit ("ld") oracle on one case, computed once."""
    if (variant, N, name) not in _SOL:
        _SOL[variant, N, name] = _solve(variant, *E.case(E.path_of(N), name))
    return _SOL[variant, N, name]


def _at_or_below(g, table, what):
    assert all(a <= b for a, b in zip(g, table)), "%s: measured %s, the spec's table has %s" % (what, ["%.2e" % v for v in g], table)


@pytest.mark.parametrize("N", E.HORIZONS)
def test_the_inputs_reach_every_exit(N):
    """The class counts of every case by the fp64 oracle: the conditions that keep the device tests from passing vacuously."""
    o = _sol(None, N, "restart")
    it, B = o[4], E.B
    assert len(it) == B and (o[3] == 0).all()
    lim = 50 + E.FALLBACK
    cls = ((it > 30).sum(), (it == lim).sum(), np.flatnonzero((it > 30) & (it < lim)).tolist(), (it == 30).sum(), (it < 30).sum())
    print("EXITS N=%d restart (seed %d, ipm_mu0 %g): it > 30 %d, at %d %d, restarted and converged %s (counts %s), it == 30 %d, it < 30 %d"
          % ((N,) + E.RESTART[N] + cls[:1] + (lim,) + cls[1:3] + (it[cls[2]].tolist(),) + cls[3:]))
    assert (it >= 30).sum() >= B // 16 and ((it >= 30) & (it < lim)).sum() >= 1 and (it == lim).sum() >= 1 and (it < 30).sum() >= B // 2
    # an instance at exactly 30 converged at its 30th test and did not restart (the spec's docstring): the same counts on it > 30
    assert E.restarted(it).sum() >= B // 16 and (E.restarted(it) & (it < lim)).sum() >= 1
    assert (it <= lim).all()
    for name, k in E.LIMITS.items():
        o = _sol(None, N, name)
        print("EXITS N=%d %s: %d of %d at the limit" % (N, name, (o[4] == k).sum(), B))
        assert (o[3] == 0).all() and (o[4] <= k).all() and (o[4] == k).sum() >= B // 2
    at = []
    for name, k in E.EDGE_ITERS.items():
        o = _sol(None, N, name)
        assert len(o[4]) == B - len(E.EDGE_SKIP[N]) >= 32 and (o[3] == 0).all() and (o[4] <= k).all()
        at.append(int((o[4] == k).sum()))
        assert at[-1] >= 1, (name, np.bincount(o[4]))
    # nothing but the restart separates edge_30 from edge_31: the instances at 30 there are the ones at 61 here or converged at 30
    assert ((_sol(None, N, "edge_30")[4] == 30) >= (_sol(None, N, "edge_31")[4] == 61)).all()
    o = _sol(None, N, "restart_tight_budget")
    print("EXITS N=%d edge cases: %d / %d / %d instances at 29 / 30 / 61; restart_tight_budget: %d at %d"
          % (N, at[0], at[1], at[2], (o[4] == E.TIGHT + E.FALLBACK).sum(), E.TIGHT + E.FALLBACK))
    assert (o[3] == 0).all() and (o[4] <= E.TIGHT + E.FALLBACK).all() and (o[4] == E.TIGHT + E.FALLBACK).sum() >= 1


@pytest.mark.parametrize("name", E.CASES)
@pytest.mark.parametrize("N", E.HORIZONS)
def test_fp64_oracle_against_80_bit_arithmetic_on_every_exit(N, name):
    """The two oracles agree in the status and the iteration count of every instance; their distance stands in the spec's table (GAPS)
    and gives a bound of at most 1e-6."""
    o, o8 = _sol(None, N, name), _sol("ld", N, name)
    np.testing.assert_array_equal(o[3], o8[3]); np.testing.assert_array_equal(o[4], o8[4])
    g = E.gaps(o, o8)
    tol, ctol = E.bounds(N, name)
    print("EXITS N=%d %-20s fp64 oracle against 80-bit: max|du| %.1e max|dx| %.1e cost %.1e relative -> bounds %.1e, %.1e" % ((N, name) + g + (tol, ctol)))
    _at_or_below(g, E.GAPS[N, name], (N, name))
    assert tol <= 1e-6 and ctol <= 1e-6


@pytest.mark.parametrize("N", E.HORIZONS)
def test_the_skipped_edge_instances_are_the_ill_conditioned_ones(N):
    """Stopped at pass 29 or 30, every instance the edge cases leave out moves by more than 1e-8 between the fp64 and the 80-bit oracle
    or under a change of ubar by one unit in the last place (the fp64 oracle against itself, four draws), the iteration counts staying
    the same; no instance left in moves that far under either."""
    cfg, s = E.case(E.path_of(N), "restart")
    dist = lambda a, b: np.maximum(np.abs(a[1] - b[1]).reshape(E.B, -1).max(axis=1), np.abs(a[0] - b[0]).reshape(E.B, -1).max(axis=1))
    wide, moved = np.zeros(E.B), np.zeros(E.B)
    for k in (29, 30):
        c = cfg.copy(); c.ipm_iter_max = k
        o, o8 = _solve(None, c, s), _solve("ld", c, s)
        np.testing.assert_array_equal(o[4], o8[4])
        wide = np.maximum(wide, dist(o, o8))
        for draw in range(4):
            p = _solve(None, c, dict(s, ubar=E.one_ulp(s["ubar"], draw)))
            np.testing.assert_array_equal(o[4], p[4])
            moved = np.maximum(moved, dist(o, p))
    print("EXITS N=%d edge cases leave out %s: against 80-bit %s, one unit in the last place of ubar %s; the instances left in: %.1e, %.1e"
          % (N, E.EDGE_SKIP[N], ["%.0e" % wide[i] for i in E.EDGE_SKIP[N]], ["%.0e" % moved[i] for i in E.EDGE_SKIP[N]],
             np.delete(wide, E.EDGE_SKIP[N]).max(), np.delete(moved, E.EDGE_SKIP[N]).max()))
    assert set(np.flatnonzero(np.maximum(wide, moved) > 1e-8).tolist()) == set(E.EDGE_SKIP[N])


@pytest.mark.parametrize("N", E.HORIZONS)
def test_a_restart_changes_the_answer(N):
    """The restarted instances against a solve of the same inputs that stops where the restart would begin (ipm_iter_max = 30): the median
    of max |du| is above 100 x the case's bound, so a kernel that skipped the restart could not stay inside it."""
    cfg, s = E.case(E.path_of(N), "restart")
    o = _sol(None, N, "restart")
    c = cfg.copy(); c.ipm_iter_max = 30
    stop = _solve(None, c, s)
    d = np.abs(o[1] - stop[1]).reshape(E.B, -1).max(axis=1)
    tol, _ = E.bounds(N, "restart")
    m, r = o[4] >= 30, E.restarted(o[4])
    assert (stop[4][m] == 30).all()
    print("EXITS N=%d: median max|du - du stopped at 30| %.1e over it >= 30, %.1e over it > 30; bound %.1e" % (N, np.median(d[m]), np.median(d[r]), tol))
    assert np.median(d[m]) > 100 * tol and np.median(d[r]) > 100 * tol and (d[r] > 100 * tol).all()
    assert (d[~m] == 0).all()


@pytest.mark.parametrize("N", sorted(E.SQP_HORIZONS))
def test_the_sqp_inputs_away_from_the_shipped_horizon(N):
    """solver_type "SQP" at N = 5 / 17 / 20: the two oracles agree in status in every mode, (100, 1e-6) has converged instances and
    instances at the limit, and the distances stand in the spec's table."""
    for iters, tol in E.SQP_MODES:
        cfg, s = E.sqp_case(N, iters, tol)
        o, o8 = _solve(None, cfg, s), _solve("ld", cfg, s)
        np.testing.assert_array_equal(o[3], o8[3])
        g = E.gaps(o, o8)
        print("EXITS N=%d SQP (%d, %g): statuses %s; fp64 oracle against 80-bit: max|du| %.1e max|dx| %.1e cost %.1e relative -> bound %.1e"
              % ((N, iters, tol, np.bincount(o[3]).tolist()) + g + (E.sqp_bound(N, iters, tol),)))
        assert set(o[3].tolist()) <= {0, 2}
        if iters == 100:
            assert (o[3] == 0).sum() >= 8 and (o[3] == 2).sum() >= 8
        _at_or_below(g, E.SQP_GAPS[N, iters, tol], (N, iters, tol))
        assert E.sqp_bound(N, iters, tol) <= 1e-6
