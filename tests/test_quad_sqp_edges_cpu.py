"""What tests/test_quad_sqp_edges_gpu.py relies on, checked without a GPU, with the fp64 and the 80-bit oracle alone: the inputs of
quad_sqp_edges_spec leave the SQP loop the way the device tests need them to (status mixes, converged instances on a bound, the failure at
QP 2 and not at QP 1, every QP at the iteration limit, the last QP through the restart), the two oracles agree on every status and
iteration count, and their distances are the spec's tables, which the device tests' bounds come from."""
import numpy as np
import pytest

import quad_ipm_exits_spec as X
import quad_routed_spec as Q
import quad_sqp_edges_spec as E
import quad_sqp_spec as S

_ORACLES = {}


def _oracle(variant):
    from oracle.quad_oracle import QuadOracle
    if variant not in _ORACLES:
        _ORACLES[variant] = QuadOracle(variant)
    return _ORACLES[variant]


def _both(cfg, s, gp_state=None):
    """(x, u, cost, status, iters) of the fp64 and of the 80-bit oracle."""
    return tuple(_oracle(v).solve_batch(cfg, *Q.quad_args(s), nthreads=16, gp_state=gp_state) for v in (None, "ld"))


def _table(g, rec, what):
    """The measured distances are the table's: at or below it, and the table is the figure rounded up to two digits, not a wider one."""
    assert all(a <= b for a, b in zip(g, rec)), "%s: measured %s, the spec's table has %s" % (what, ["%.2e" % v for v in g], rec)
    assert all(b <= 1.12 * a + 1e-17 for a, b in zip(g, rec)), "%s: measured %s, the spec's table has %s" % (what, ["%.2e" % v for v in g], rec)


# ---- 1. random problem data -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", range(E.DRAWS))
@pytest.mark.parametrize("N", E.HORIZONS)
def test_random_problem_data_leaves_through_both_exits_with_inputs_on_a_bound(N, d):
    cfg, s, gs = E.data_case(N, d)
    shipped = S.config(N)
    assert cfg.W[3] > 0 and all(cfg.We[i] > 0 for i in range(13)) and cfg.Ts != shipped.Ts
    assert all(cfg.lbu[m] > 0 and cfg.ubu[m] < 1 for m in range(4)) and len({cfg.W[13 + m] for m in range(4)}) == 4
    assert (gs is not None) == (d == E.GP_DRAW) == (cfg.n_gp > 0) and len(s["x0"]) == E.B
    if gs is not None:
        assert np.abs(gs - s["x0"]).max() >= 1.0
    for mode in E.DATA_MODES:
        cfg = E.data_case(N, d, mode)[0]
        o, o8 = _both(cfg, s, gs)
        np.testing.assert_array_equal(o[3], o8[3])
        g, rec = S.gaps(o, o8), E.DATA_GAPS[(N, d) + mode]
        n0, n2, nb = (o[3] == 0).sum(), (o[3] == 2).sum(), (E.on_a_bound(cfg, o[1]) & (o[3] == 0)).sum()
        print("EDGES data N=%d draw %d (%d, %g): %d x 0, %d x 2, %d converged with an input on a bound; fp64 oracle against 80-bit: max|du| %.1e "
              "max|dx| %.1e cost %.1e relative -> bounds %.1e / %.1e" % ((N, d) + mode + (n0, n2, nb) + g + S.bounds(rec, mode)))
        _table(g, rec, (N, d, mode))
        assert S.bounds(rec, mode)[0] <= 1e-6
        if mode[1] > 0:
            assert n0 >= 4 and n2 >= 4 and n0 + n2 == E.B and nb >= 4
        else:
            assert n0 == E.B
        if gs is not None and mode[1] > 0:                        # the GP moves the answer, and so does the state it is evaluated at
            plain = cfg.copy(); plain.n_gp = 0
            assert np.abs(_oracle(None).solve_batch(plain, *Q.quad_args(s), nthreads=16)[1] - o[1]).max() > 1e-4
            assert np.abs(_oracle(None).solve_batch(cfg, *Q.quad_args(s), nthreads=16)[1] - o[1]).max() > 1e-4


# ---- 2. a failure at QP 2 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.LATE_INPUTS))
def test_the_huge_reference_fails_qp_2_and_not_qp_1(name):
    """One QP: status 0, a finite iterate away from the caller's.  N = 10, 16 at every limit >= 2: status 4, cost +inf, iters 0 with a finite
    Hessian and gradient (the pivot test, not a NaN), the iterate bit for bit the one-QP solve's (QP 2 failed and left it alone).  N = 5: no
    failure, status 2 at the limit with a finite iterate."""
    N, col, val, fails_at = E.LATE_INPUTS[name]
    s, b = E.late_scenario(name), E.LATE_INSTANCE
    plain = S.scenario(N)
    assert np.isfinite(s["yref"]).all() and [k for k in s if not np.array_equal(s[k], plain[k])] == ["yref"]
    assert (np.abs(s["yref"] - plain["yref"]).reshape(len(s["x0"]), -1).max(axis=1) > 0).nonzero()[0].tolist() == [b]
    one = _both(S.config(N, (1, 0.0)), s)
    for o in one:
        assert o[3][b] == 0 and np.isfinite(o[0][b]).all() and np.isfinite(o[1][b]).all() and 1e200 < o[2][b] < np.inf
        assert np.abs(o[1][b] - s["ubar"][b]).max() > 1e-3
    for L in (2, 3) + E.LATE_MODE[:1]:
        both = _both(S.config(N, (L, E.LATE_MODE[1])), s)
        for o, o1 in zip(both, one):
            print("EDGES late %s limit %d: status %d, cost %g, iters %d" % (name, L, o[3][b], o[2][b], o[4][b]))
            if fails_at == 2:
                assert o[3][b] == 4 and o[2][b] == np.inf and o[4][b] == 0
                assert o[0][b].tobytes() == o1[0][b].tobytes() and o[1][b].tobytes() == o1[1][b].tobytes()
            else:
                assert fails_at is None
                assert o[3][b] == 2 and np.isfinite(o[0][b]).all() and np.isfinite(o[1][b]).all() and 1e200 < o[2][b] < np.inf
        np.testing.assert_array_equal(both[0][3], both[1][3])
    # the QP at the one-step iterate: finite, and indefinite exactly where QP 2 fails
    q = _oracle(None).qp_debug(S.config(N), s["x0"][b], s["yref"][b], s["yref_e"][b], one[0][0][b], one[0][1][b])
    assert np.isfinite(q["H"]).all() and np.isfinite(q["g"]).all() and q["status"] == (4 if fails_at else 0)
    assert (np.linalg.eigvalsh(q["H"]).min() < 0) == (fails_at is not None)
    # the neighbours are those of the plain batch, and leave through both exits
    ref = _oracle(None).solve_batch(S.config(N, E.LATE_MODE), *Q.quad_args(plain), nthreads=16)
    ok = np.arange(len(s["x0"])) != b
    for k in range(5):
        assert both[0][k][ok].tobytes() == ref[k][ok].tobytes()
    assert (ref[3][ok] == 0).sum() >= 4 and (ref[3][ok] == 2).sum() >= 4


def test_every_path_has_its_late_input():
    assert sorted(E.LATE) == sorted(E.PATHS) and E.LATE_NO_PIVOT_TEST[0] in E.PATHS
    for path, (name, q) in E.LATE.items():
        N, _, _, fails_at = E.LATE_INPUTS[name]
        assert N == S.PATHS[path][0] and E.LATE_FAILS[path] == (fails_at is not None) and q in (None, fails_at)
    assert E.LATE_INPUTS[E.LATE_NO_PIVOT_TEST[1]][0] == S.PATHS[E.LATE_NO_PIVOT_TEST[0]][0]


# ---- 3. the interior point's rare exits inside the loop -----------------------------------------------------------------------------------

@pytest.mark.parametrize("qp_max,tol", E.LIMIT_MODES)
@pytest.mark.parametrize("N", E.HORIZONS)
def test_every_qp_ends_at_the_iteration_limit(N, qp_max, tol):
    mode = (qp_max, tol)
    cfg, s = E.limit_case(N, mode)
    o, o8 = _both(cfg, s)
    np.testing.assert_array_equal(o[3], o8[3]); np.testing.assert_array_equal(o[4], o8[4])
    assert (o[4] == E.LIMIT).all() and (o[3] == (2 if tol > 0 else 0)).all()
    for q in range(1, qp_max):                                    # every QP of the loop, not the last alone
        assert (_oracle(None).solve_batch(E.limit_case(N, (q, 0.0))[0], *Q.quad_args(s), nthreads=16)[4] == E.LIMIT).all()
    g, rec = S.gaps(o, o8), E.LIMIT_GAPS[(N,) + mode]
    print("EDGES limit N=%d (%d, %g): fp64 oracle against 80-bit: max|du| %.1e max|dx| %.1e cost %.1e relative -> bounds %.1e / %.1e"
          % ((N,) + mode + g + S.bounds(rec, mode)))
    _table(g, rec, (N, mode))
    assert max(rec[:2]) <= 3e-10 and np.isfinite(o[0]).all() and np.isfinite(o[1]).all()
    # the limit changes the answer: the same loop with the shipped ipm_iter_max is far outside the bound
    free = _oracle(None).solve_batch(S.config(N, mode), *Q.quad_args(s), nthreads=16)
    assert np.abs(free[1] - o[1]).max() > 1e3 * S.bounds(rec, mode)[0]


@pytest.mark.parametrize("N", E.HORIZONS)
def test_the_last_qp_goes_through_the_restart(N):
    cfg, s = E.restart_case(N, E.RESTART_MODE)
    assert cfg.ipm_mu0 == X.RESTART[N][1] and len(s["x0"]) == X.B == 64
    o, o8 = _both(cfg, s)
    np.testing.assert_array_equal(o[3], o8[3]); np.testing.assert_array_equal(o[4], o8[4])
    assert (o[3] == 0).all()
    assert np.flatnonzero(X.restarted(o[4])).tolist() == E.RESTARTED[N]
    d = E.per_instance(o, o8)
    assert np.flatnonzero(d > E.RESTART_NEAR).tolist() == E.RESTART_LEFT_OUT[N]
    k = E.kept(N)
    assert len(k) >= X.B - 2 and len(set(E.RESTARTED[N]) & set(k.tolist())) >= 1
    g = S.gaps(tuple(a[k] for a in o), tuple(a[k] for a in o8))
    print("EDGES restart N=%d: last QP restarted on %s, left out %s (%s apart); the rest, fp64 oracle against 80-bit: max|du| %.1e max|dx| %.1e "
          "cost %.1e relative -> bounds %.1e / %.1e" % ((N, E.RESTARTED[N], E.RESTART_LEFT_OUT[N], ["%.1e" % v for v in d[E.RESTART_LEFT_OUT[N]]]) + g
                                                          + S.bounds(E.RESTART_GAPS[N], E.RESTART_MODE)))
    _table(g, E.RESTART_GAPS[N], N)
    assert max(E.RESTART_GAPS[N][:2]) <= 3.1e-9
    # instances that restart in QP 1 and not in QP 2: a fallback flag or a blocked-step memory left over from QP 1 would change their QP 2
    first = _oracle(None).solve_batch(E.restart_case(N, (1, 0.0))[0], *Q.quad_args(s), nthreads=16)
    assert (first[3] == 0).all()
    print("EDGES restart N=%d: restarted in QP 1 %s" % (N, np.flatnonzero(X.restarted(first[4])).tolist()))
    assert (X.restarted(first[4]) & ~X.restarted(o[4])).sum() >= 1 and (~X.restarted(o[4])).sum() >= X.B // 2
