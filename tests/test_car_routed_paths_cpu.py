"""What tests/test_car_routed_paths.py relies on, checked without a GPU: its path table states what the launch code does, the oracle it
compares with is a reference at the tolerances it uses, and the inputs it draws cannot pass vacuously (every cluster is used, the
clusters' GPs change the solution, the batches iterate, the split paths defer, the waves are mixed).

The batches whose size follows the CU count are drawn for car_routed_spec.NC_CPU = 256 CUs here; an instance of gp_structures.car_batch
depends on its index alone, so another CU count solves a prefix or an extension of the same batch, and the GPU module asserts the shares
again on the batch it runs."""
import os

import numpy as np
import pytest

import batch_regimes as R
import car_routed_spec as CR
from test_batch_regimes_cpu import CSRC, _body
from test_gpu_parity import tol_for

NC = CR.NC_CPU


# ---- the table against the source -------------------------------------------------------------------------------------------------------

DISPATCH_LINES = (
    ("admpc_kernels.hip", "admpc_create", 's->use_dense = (cfg->N == 20) && !(e && strcmp(e, "riccati") == 0);'),
    ("admpc_kernels.hip", "admpc_create", 's->use_seg = admpc_seg_supports(cfg->N) && (cfg->n_gp == 0 ? !(e && strcmp(e, "riccati") == 0) : (e && strcmp(e, "seg") == 0));'),
    ("admpc_kernels.hip", "solve_impl", "const bool dense = s->use_dense && !snap && !(nsqp > 1 && s->cfg.sqp_tol > 0.0);"),
    ("admpc_kernels.hip", "solve_impl", "if (s->use_seg && !snap && !(nsqp > 1 && s->cfg.sqp_tol > 0.0)) {"),
    ("admpc_kernels.hip", "rowqp_chunk", "if (s->row_chunk > 0 && (unsigned long long)s->row_chunk < m) m = (unsigned long long)s->row_chunk;"),
)


def test_the_dispatch_lines_are_pinned():
    """The lines car_routed_spec.car_kernel, split_mode and chunks mirror are entries of batch_regimes.LAUNCH_LINES, which
    test_batch_regimes_cpu.py finds in the source one by one."""
    for entry in DISPATCH_LINES:
        assert entry in R.LAUNCH_LINES, entry
    fns = {(f, g) for f, g, _ in R.LAUNCH_LINES}
    assert ("admpc_kernels.hip", "solve_rows") in fns and ("admpc_seg.hip", "admpc_seg_supports") in fns and ("admpc_rowqp.hip", "admpc_rowqp_kernel") in fns


def test_the_path_table_agrees_with_the_launch_code():
    """Every row of PATHS: each cluster's handle runs the kernel the row names (by the mirrored dispatch, on the configs the GPU module
    creates the handles from); the environment it sets is read by admpc_create; on 64, 256 and 304 CUs every chunk of its batch gets the
    instances per wave and the number of phases the row claims; the footprint the mirrored plan assumes holds at its horizon."""
    with open(os.path.join(CSRC, "admpc_kernels.hip")) as f:
        create = _body(f.read(), "admpc_create")
    for var in ("ADMPC_ROWQP_SPLIT", "ADMPC_ROWQP_CHUNK", "ADMPC_QP"):
        assert 'getenv("%s")' % var in create
    seen = set()
    for path, r in CR.PATHS.items():
        cfgs = CR.path_configs(path)
        assert len(cfgs) == CR.K == len(r["kernels"])
        it, tol = r.get("sqp", (1, 0.0))
        for c, cfg in enumerate(cfgs):
            assert cfg.N == r["N"] and (cfg.n_gp == 0) == (c in r.get("nominal", ())) and (cfg.sqp_iters, cfg.sqp_tol) == (it, tol), (path, c)
            assert CR.car_kernel(cfg.N, r["env"], cfg.n_gp, cfg.sqp_iters, cfg.sqp_tol) == r["kernels"][c], (path, c)
        assert all('getenv("%s")' % var in create for var in r["env"])
        seen |= set(r["kernels"])
        if "R" not in r["kernels"]:
            continue
        assert R.rowqp_lds_rows(r["N"], 8) == 4 and R.rowqp_per_cu(r["N"], 8, r["rows"]) == 4, path
        for nc in (64, 256, 304):
            B = CR.batch_size(path, nc)
            assert CR.chunks(r["N"], B, r["env"]) == r.get("chunks", (B,)), (path, nc)
            for rows, two in CR.regime(path, nc):
                assert rows == r["rows"] and two == (r["split"] is not None), (path, nc, rows, two)
            if r["split"] == "default":                             # by batch size, not by request
                assert CR.split_mode(r["env"]) == -1
    assert seen == {"F", "S", "R"}
    assert {r["rows"] for r in CR.PATHS.values() if "rows" in r} == {1, 2, 4}
    assert {r["split"] for r in CR.PATHS.values() if "split" in r} == {None, "default", "forced"}
    # the GP default at the reference's shipped horizon is kernel R, and a tolerance takes every horizon there
    assert CR.car_kernel(40, {}, 3) == "R" and CR.car_kernel(40, {}, 0) == "S" and CR.car_kernel(40, {"ADMPC_QP": "seg"}, 3) == "S"
    assert CR.car_kernel(20, {}, 3, 3, 0.0) == "F" and CR.car_kernel(20, {}, 3, 3, 1e-6) == "R" and CR.car_kernel(40, {}, 0, 3, 1e-6) == "R"
    assert CR.car_kernel(17, {}, 0) == "R" and CR.car_kernel(20, {"ADMPC_QP": "riccati"}, 0) == "R"


def test_the_clusters_have_their_own_structures():
    gps = CR.clusters()
    assert [len(g) for g in gps] == [4, 3, 2]
    assert any(f >= 7 for g in gps for gp in g for f in gp["feat"]) and max(len(gp["alpha"]) for g in gps for gp in g) == 32
    assert all(set(gp["feat"]) <= {7, 8} for gp in gps[2])          # a cluster whose GPs see the inputs alone


# ---- the numpy statements ---------------------------------------------------------------------------------------------------------------

def test_the_numpy_select_statement():
    """A hand-made tie goes to the lower index; K = 1 routes everything to 0; input features read u; NaN and inf route to 0."""
    xs = np.zeros((5, 7)); us = np.zeros((5, 2))
    xs[:, 3] = [1.0, 2.0, 3.0, np.nan, np.inf]
    cent = np.array([[1.5], [2.5], [0.5]])
    assert CR.select_numpy(xs, us, [3], cent).tolist() == [0, 0, 1, 0, 0]          # 1.0: 0.5 from centroids 0 and 2; 2.0: from 0 and 1
    assert CR.select_numpy(xs, us, [3], cent[::-1]).tolist() == [0, 1, 1, 0, 0]
    assert CR.select_numpy(xs, us, [3], [[9.0]]).tolist() == [0] * 5
    us[:, 1] = [0.0, 1.0, 2.0, 3.0, 4.0]; xs[:, 3] = 0.0
    assert CR.select_numpy(xs, us, [8, 3], [[0.0, 0.0], [2.0, 0.0], [4.0, 0.0]]).tolist() == [0, 0, 1, 1, 2]
    assert CR.select_numpy(xs, us, [3, 8], [[0.0, 0.0], [0.0, 2.0], [0.0, 4.0]]).tolist() == [0, 0, 1, 1, 2]


def test_with_off_and_the_tercile_centroids():
    r = np.arange(20, dtype=np.int32) % 3
    w = CR.with_off(r)
    assert [int(w[b]) for b in sorted(CR.OFF)] == [7, -1, CR.K] and (np.delete(w, sorted(CR.OFF)) == np.delete(r, sorted(CR.OFF))).all()
    assert r[5] == 2 and w.dtype == np.int32 and not CR.in_range(w)[sorted(CR.OFF)].any() and CR.in_range(w).sum() == 17
    assert CR.with_off(np.zeros(6, dtype=np.int32)).tolist() == [0, 0, 0, 0, 0, 7]
    v = np.array([5.0, 1.0, 9.0, 2.0, 8.0, 4.0, 7.0])
    cent = CR.tercile_centroids(v)
    assert cent[:, 0].tolist() == [1.0, 5.0, 10.0]                                  # boundaries 3 and 7.5
    route = CR.select_numpy(np.c_[np.zeros((7, 3)), v, np.zeros((7, 3))], np.zeros((7, 2)), [3], cent)
    assert route.tolist() == [1, 0, 2, 0, 2, 1, 1]
    assert CR.quadruple_mix([0, 0, 0, 0, 1, 2, 1, 7, 0, 1, 2, -1]) == {1, 2, 3}
    deg = CR.degenerate_routes(np.arange(24) % 3)
    assert set(deg["none to cluster 1"].tolist()) == {0, 2} and CR.quadruple_mix(deg["blocks of four"]) == {1} and CR.quadruple_mix(deg["b % K"]) == {3}


# ---- the oracle as a reference, and the inputs against passing vacuously ----------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_ld():
    from oracle.oracle import Oracle
    return Oracle(variant="ld")


_ORACLE = {}


def _oracle(oracle_omp, path):
    """The fp64 oracle on the path's batch (NC CUs) under own-cluster routing, once per (horizon, batch, configs)."""
    r = CR.PATHS[path]
    key = (r["N"], CR.batch_size(path, NC), r.get("nominal", ()), r.get("sqp", (1, 0.0)))
    if key not in _ORACLE:
        cfgs, s, route, _ = CR.scenario(path, NC, oracle_omp)
        _ORACLE[key] = CR.oracle_routed(oracle_omp, cfgs, route, s)[1]
    return _ORACLE[key]


@pytest.mark.parametrize("path", list(CR.PATHS))
def test_fp64_oracle_against_80_bit_arithmetic_on_the_routed_batch(oracle_omp, oracle_ld, path):
    """The reference condition of the suite on the path's own batch and configs, each instance under its own cluster: where the two
    oracles take the same iterations, the fp64 oracle is within the path's tolerance / 1000 of the 80-bit one.  In SQP mode with a tolerance the statuses agree as well."""
    r = CR.PATHS[path]
    cfgs, s, route, _ = CR.scenario(path, NC, oracle_omp)
    o = _oracle(oracle_omp, path)
    idx, o8 = CR.oracle_routed(oracle_ld, cfgs, route, s, nthreads=1)
    tol_on = path in CR.SQP_TOL_PATHS
    same = (o[3] == o8[3]) & (o[4] == o8[4]) & ((o8[3] == 0) | tol_on)
    if tol_on:
        np.testing.assert_array_equal(o[3], o8[3])
        same &= (np.abs(o8[0]).max(axis=(1, 2)) < 1e3) & (np.abs(o8[1]).max(axis=(1, 2)) < 1e3) & (o8[3] != 4)
    du, dx = np.abs(o[1] - o8[1])[same].max(), np.abs(o[0] - o8[0])[same].max()
    cap = (CR.SQP_TOL if tol_on else tol_for(r["N"])) / 1000.0
    print("CAR-ROUTED %-18s fp64 oracle against 80-bit on %d instances: max|du| %.1e max|dx| %.1e (same iterations: %d)  cap %.0e"
          % (path, len(idx), du, dx, same.sum(), cap))
    assert same.mean() >= 0.98, same.mean()
    assert du <= cap and dx <= cap, (path, du, dx, cap)


@pytest.mark.parametrize("path", list(CR.PATHS))
def test_the_routed_inputs_cannot_pass_vacuously(oracle_omp, path):
    """On the path's batch: every cluster holds at least a quarter of it; at least a quarter iterates in the interior point (the
    unconstrained trial does not solve it); each cluster's instances move by more than 1e-6 in u under the next cluster's GPs; the
    out-of-range places hold in-range routes before with_off; and per regime what makes the skip bite -- deferred instances in every
    cluster where the kernel runs in two phases, waves of one, two and three clusters at four instances per wave, and converged next to
    unconverged instances in every cluster where the SQP stop test runs."""
    r = CR.PATHS[path]
    cfgs, s, route, cent = CR.scenario(path, NC, oracle_omp)
    B = len(route)
    assert B == CR.batch_size(path, NC) and cent.shape == (CR.K, 1)
    share = np.bincount(route, minlength=CR.K) / B
    assert (share >= 0.25).all() and CR.in_range(route).all(), share
    assert (np.bincount(CR.with_off(route)[CR.in_range(CR.with_off(route))], minlength=CR.K) / B >= 0.25).all()
    o = _oracle(oracle_omp, path)
    tol_on = path in CR.SQP_TOL_PATHS
    assert set(np.unique(o[3])) <= ({0, 2, 4} if tol_on else {0}), np.bincount(o[3])
    first = o
    if r.get("sqp"):                                                # the interior point of the first QP: the RTI step of the same batch
        first = CR.oracle_routed(oracle_omp, CR.path_configs(path, sqp=(1, 0.0)), route, s)[1]
    iterates = first[4] > 0
    assert iterates.mean() >= 0.25, iterates.mean()
    _, other = CR.oracle_routed(oracle_omp, cfgs, route, s, rotate=1)
    moved = np.abs(o[1] - other[1]).reshape(B, -1).max(axis=1)
    per = [float(moved[route == c].max()) for c in range(CR.K)]
    assert min(per) > 1e-6, per
    line = "CAR-ROUTED %-18s B %5d  share %s  iterating %.2f  max|u - u under the next cluster| %s" \
        % (path, B, np.round(share, 3).tolist(), iterates.mean(), ["%.1e" % v for v in per])
    if r.get("split"):
        deferred = [int((iterates & (route == c)).sum()) for c in range(CR.K)]
        done = [int((~iterates & (route == c)).sum()) for c in range(CR.K)]
        line += "  deferred per cluster %s" % deferred
        assert min(deferred) >= 1 and min(done) >= 1, (deferred, done)
    if r.get("rows") == 4:
        assert {1, 2, 3} <= CR.quadruple_mix(CR.with_off(route)), CR.quadruple_mix(route)
    if tol_on:
        line += "  statuses %s" % np.bincount(o[3], minlength=5).tolist()
        assert all((o[3][route == c] == 0).sum() >= 3 and (o[3][route == c] == 2).sum() >= 3 for c in range(CR.K)), np.bincount(o[3])
    print(line)


@pytest.mark.parametrize("path", ["R17_rows4", "R40"])
def test_the_poisoned_instances_fail_in_the_oracle_and_share_their_waves(oracle_omp, path):
    """car_routed_spec.poisoned: one instance per cluster, each in a wave of four that holds another cluster, no two in one wave; the
    oracle fails exactly those (status 4) and solves the others as before."""
    cfgs, s, route, _ = CR.scenario(path, NC, oracle_omp)
    route = CR.with_off(route)
    sp, bad = CR.poisoned(s, route, rows=4)
    assert sorted(route[bad].tolist()) == [0, 1, 2] and len({b // 4 for b in bad}) == 3
    assert all(len(set(route[b - b % 4: b - b % 4 + 4].tolist()) & {0, 1, 2}) >= 2 for b in bad)
    assert sum(int((~np.isfinite(sp[k])).sum()) for k in ("x0", "yref")) == 3 and all(np.array_equal(sp[k], s[k]) for k in ("yref_e", "p", "xbar", "ubar"))
    idx, o = CR.oracle_routed(oracle_omp, cfgs, route, sp)
    clean = _oracle(oracle_omp, path)
    st = np.full(len(route), -9); st[idx] = o[3]
    assert (st[bad] == 4).all() and (np.delete(st, bad + sorted(CR.OFF)) == 0).all()
    keep = ~np.isin(idx, bad)
    assert np.array_equal(o[1][keep], clean[1][idx][keep])
