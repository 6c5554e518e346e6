"""What tests/test_quad_sqp_gpu.py relies on, checked without a GPU: the header of the in-kernel SQP loop (include/admpc_quad_sqp.h), the
prototype table, the Makefile and the library agree; the inputs of quad_sqp_spec leave through both exits of the loop (the status mixes
by the oracle); the fp64 and the 80-bit oracle agree in status and are as far apart as the spec's table says (the device tests' bounds
come from it); the refusals of the Python layer that come before a handle exists; and the kernel's SQP text stays inside
`if constexpr (SQP)` blocks beside the launch lines test_batch_regimes_cpu.py pins."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import quad_routed_spec as Q
import quad_sqp_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "admpc_quad_sqp.h"
ARITY = {"admpc_quad_set_sqp": 3, "admpc_quad_get_sqp": 3, "admpc_quad_solve_batch_sqp": 13}

_ORACLES, _SOL = {}, {}


@pytest.fixture(scope="module")
def lib():
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _oracle(variant):
    from oracle.quad_oracle import QuadOracle
    if variant not in _ORACLES:
        _ORACLES[variant] = QuadOracle(variant)
    return _ORACLES[variant]


def _sol(variant, N, mode):
    """(x, u, cost, status, iters) of the fp64 (variant None) or the 80-bit ("ld") oracle on the batch of horizon N, computed once."""
    if (variant, N, mode) not in _SOL:
        _SOL[variant, N, mode] = _oracle(variant).solve_batch(S.config(N, mode), *Q.quad_args(S.scenario(N)), nthreads=16)
    return _SOL[variant, N, mode]


# ---- 1. the header, the table, the Makefile and the library ------------------------------------------------------------------------------

def test_header_table_makefile_and_library_agree(lib):
    from ad_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: len(p.split(",")) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert list(_lib.SQP_TABLES) == [HEADER] and tuple(_lib.SQP_TABLES[HEADER]) == _lib.QUAD_SQP_EXPORTS == tuple(ARITY)
    known = [t for group in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES, _lib.TARGET_TABLES,
                             _lib.PRUNE_TABLES, _lib.EVAL_TABLES, _lib.TRAJ_TABLES, _lib.POLY_TRAJ_TABLES, _lib.SELECT_TABLES) for t in group.values()]
    assert not set(ARITY) & {n for t in known for n in t}                          # no name is declared by two headers
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n == len(_lib.SQP_TABLES[HEADER][name][1]) and fn.restype is C.c_int, name
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert "../../include/" + HEADER in mk
    for words in ("DEVIATION", "no test precedes QP 0", "counts[b][1]", "NOT offered", "N > 16", "routed solves", "line search"):
        assert words in hdr, words


def test_the_entries_refuse_without_a_device(lib):
    """The refusals in front of the first device call."""
    for rc, words in ((lib.admpc_quad_set_sqp(None, 100, 1e-6), "null solver"), (lib.admpc_quad_get_sqp(None, None, None), "null solver"),
                      (lib.admpc_quad_solve_batch_sqp(None, -1, None, None, None, None, None, None, None, None, None, None, None), "null solver")):
        assert rc == -1 and words in lib.admpc_last_error().decode()


def test_the_kernel_text_keeps_the_sqp_loop_beside_the_existing_lines():
    """The SQP instantiations are the one text of admpc_quad_solve_kernel, their launches are in a function of their own, and the LDS of the
    other instantiations is sized as before."""
    src = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "admpc_quad.hip")).read()
    assert "template <class P, bool SQP = false>" in src and src.count("if constexpr (SQP)") >= 2
    assert "admpc_quad_solve_kernel<Dense40Path, true>" in src and "admpc_quad_solve_kernel<GenericPath, true>" in src
    assert "admpc_quad_solve_kernel<WidePath, true>" not in src
    body = src[src.index("static int quad_solve_sqp("):]
    body = body[:body.index("\n}")]
    assert "int* ticket = B > grid ? s->d_ticket : nullptr;" in body and "quad_sqp_lds_doubles(s->cfg.N)" in body
    assert "s->lds_bytes = (quad_lds_doubles(cfg->N) + (cfg->N * QU > 64 ? cfg->N * QU + 4 : 0)) * (int)sizeof(double);" in src
    # the footprint the header states: 43 400 bytes at N = 10, three workgroups per CU; two at N = 16
    lds = lambda N: N * (169 + 52 + 13) + 4 * N * (4 * N + 1) + 13 * 4 * N + 64 + 2 * (N + 1) * 13 + N * 17 + 13 + 13 + 26
    sqp = lambda N: 8 * (lds(N) + (N + 1) * 13 + 4 * N + 17 * N)
    assert sqp(10) == 43400 and (160 * 1024) // sqp(10) == 3 and (160 * 1024) // sqp(16) == 2


# ---- 2. the inputs ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", S.HORIZONS)
def test_the_inputs_leave_through_both_exits(N):
    """The status mixes of the spec's table by the fp64 oracle, and a tested mode of the horizon with at least four instances at each exit."""
    for (n, L), (n0, n2) in S.STATUS_MIX.items():
        if n != N:
            continue
        st = _sol(None, N, (L, 1e-6))[3]
        print("SQP N=%d limit %d: %d x status 0, %d x status 2" % (N, L, (st == 0).sum(), (st == 2).sum()))
        assert set(st.tolist()) <= {0, 2} and len(st) == S.batch(N)
        assert ((st == 0).sum(), (st == 2).sum()) == (n0, n2)
    both = [L for (n, L), (n0, n2) in S.STATUS_MIX.items() if n == N and n0 >= 4 and n2 >= 4]
    assert both and any((L, 1e-6) in [m for p in S.PATHS if S.PATHS[p][0] == N for m in S.modes(p)] for L in both), "a tested mode with both exits"
    if N == 2:                                                    # the sweep of the qps test: every instance converges, at three different counts
        first = np.full(S.batch(2), -1)
        for L in S.QPS_SWEEP_N2:
            st = _sol(None, 2, (L, 1e-6))[3]
            first[(first < 0) & (st == 0)] = L
        assert (first > 0).all() and len(set(first.tolist())) >= 3
    else:
        for L in S.QPS_LIMITS:
            assert (N, L) in S.STATUS_MIX


@pytest.mark.parametrize("path,qp_max,tol", [c for c in S.CASES if c[0] != "generic_N10"])
def test_the_two_oracles_agree_and_their_distance_is_the_tables(path, qp_max, tol):
    N, mode = S.PATHS[path][0], (qp_max, tol)
    o, o8 = _sol(None, N, mode), _sol("ld", N, mode)
    np.testing.assert_array_equal(o[3], o8[3])
    g, rec = S.gaps(o, o8), S.SQP_GAPS[(N,) + mode]
    print("SQP N=%d (%d, %g): statuses %s; fp64 oracle against 80-bit: max|du| %.1e max|dx| %.1e cost %.1e relative -> bounds %.1e / %.1e"
          % ((N, qp_max, tol, np.bincount(o[3], minlength=3).tolist()) + g + S.bounds(rec, mode)))
    assert all(a <= 2.0 * b for a, b in zip(g, rec)), (g, rec)
    assert S.bounds(rec, mode)[0] <= 1e-6
    assert set(o[3].tolist()) <= ({0, 2} if tol > 0 else {0})


def test_the_two_oracles_with_a_gp_on_the_first_node():
    s = S.scenario(10)
    gs = Q.gp_state(s)
    cfg = S.gp_config(S.MID_MODE)
    o, o8 = (_oracle(v).solve_batch(cfg, *Q.quad_args(s), nthreads=16, gp_state=gs) for v in (None, "ld"))
    np.testing.assert_array_equal(o[3], o8[3])
    g = S.gaps(o, o8)
    print("SQP N=10 with a GP (%d, %g): statuses %s, distances %s" % (S.MID_MODE + (np.bincount(o[3], minlength=3).tolist(), g)))
    assert all(a <= 2.0 * b for a, b in zip(g, S.GP_GAP)), (g, S.GP_GAP)
    assert (o[3] == 0).sum() >= 4 and (o[3] == 2).sum() >= 4
    plain = _sol(None, 10, S.MID_MODE)
    assert np.abs(o[1] - plain[1]).max() > 1e-4


# ---- 3. the Python layer ----------------------------------------------------------------------------------------------------------------

def test_the_fleets_refuse_before_a_handle_exists(monkeypatch):
    from ad_mpc_amd import engine, quad_fleet, quad_ensemble_fleet
    from ad_mpc_amd.quad_fleet import QuadFleet, fleet_solver_type
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet

    def no_handle(*a, **k):
        raise AssertionError("a handle was created")
    for mod in (engine, quad_fleet, quad_ensemble_fleet):
        monkeypatch.setattr(mod, "QuadBatchSolver", no_handle)
    with pytest.raises(ValueError, match='solver_type must be "SQP_RTI" or "SQP"'):
        QuadFleet(4, solver_type="DDP")
    with pytest.raises(ValueError, match="up to n_nodes = 16"):
        QuadFleet(4, n_nodes=17, t_horizon=1.7, solver_type="SQP")
    with pytest.raises(ValueError, match="sqp must be"):
        QuadFleet(4, solver_type="SQP", sqp=(1, 1e-6))
    with pytest.raises(ValueError, match="sqp must be"):
        QuadFleet(4, solver_type="SQP", sqp=(100, float("nan")))
    with pytest.raises(ValueError, match='solver_type must be "SQP_RTI" or "SQP"'):
        QuadEnsembleFleet(4, solver_type="SQP_FULL")
    with pytest.raises(ValueError, match="not served for clustered GP ensembles"):
        QuadEnsembleFleet(4, solver_type="SQP")
    assert fleet_solver_type("f", "SQP_RTI", 20, (100, 1e-6)) is None and fleet_solver_type("f", "SQP", 16, (100, 1e-6)) == (100, 1e-6)
    # the constructor's new arguments are appended: __new__ still reads learn at args[11]
    import inspect
    names = list(inspect.signature(QuadFleet.__init__).parameters)
    assert names.index("learn") == 12 and names[-3:] == ["solver_type", "terminal_cost", "sqp"] and names[-4] == "noise_seed"
