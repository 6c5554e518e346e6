"""What tests/test_quad_routed_paths.py relies on, checked without a GPU: its path table covers every kernel quad_solve launches with a
route, and the inputs it draws cannot pass vacuously (every cluster is used, and the clusters' GPs change the solution)."""
import os
import re

import numpy as np
import pytest

import quad_routed_spec as Q
from test_batch_regimes_cpu import CSRC, _body


@pytest.fixture(scope="module")
def src():
    with open(os.path.join(CSRC, "admpc_quad.hip")) as f:
        return f.read()


def _launches(body):
    """(kernel, argument text) of every hipLaunchKernelGGL in a function body."""
    return [(m.group(1).replace(" ", ""), m.group(2)) for m in re.finditer(r"hipLaunchKernelGGL\(\s*([A-Za-z_0-9]+(?:\s*<[^>]*>)?)\s*,([^;]*)\);", body)]


def test_the_routed_path_table_covers_the_launch_sites_of_quad_solve(src):
    """Every kernel quad_solve launches with a `route` argument has a row in ROUTED_PATHS; every row names a kernel that is launched there
    and defined, an environment switch the library reads, and the kernel the mirrored dispatch picks for its horizon and environment."""
    body = _body(src, "quad_solve")
    routed = {k for k, args in _launches(body) if re.search(r"\broute\b", args)}
    assert len(routed) >= 4, routed                                 # the pattern still finds the launches
    named = {k for _, _, k in Q.ROUTED_PATHS.values()}
    assert routed <= named, "quad_solve launches %s with a route and no routed test runs it: add rows to quad_routed_spec.ROUTED_PATHS" % sorted(routed - named)
    assert named <= routed, "ROUTED_PATHS names %s, which quad_solve does not launch" % sorted(named - routed)
    assert all(re.search(r"\b%s\b" % a, args) for k, args in _launches(body) if k in routed for a in ("route", "which"))
    for path, (N, env, kernel) in Q.ROUTED_PATHS.items():
        fn, _, arg = kernel.partition("<")
        assert re.search(r"__global__[^;{]*\bvoid\s+%s\s*\(" % fn, src), "%s: no kernel %s" % (path, fn)
        if arg:
            assert re.search(r"\b(struct|typedef[^;]*)\s+%s\b" % arg[:-1], src), "%s: no path %s" % (path, arg[:-1])
        for var in env:
            assert 'getenv("%s"); s->%s = e && e[0] == \'1\';' % (var, Q.SWITCHES[var]) in src, "%s: the library does not read %s" % (path, var)
        assert Q.quad_kernel(N, env) == kernel, path
        assert 2 <= N <= 24
    # every routed skip in the kernels compares with `which`: the texts the table's rows run
    assert len(re.findall(r"if \(routeg && routeg\[inst\] != which\)", src)) == 2


@pytest.fixture(scope="module")
def qoracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


HORIZONS = sorted({N for N, _, _ in Q.ROUTED_PATHS.values()})


@pytest.mark.parametrize("N", HORIZONS)
def test_the_routed_inputs_cannot_pass_vacuously(qoracle, N):
    """The batch of B = 96 every path of horizon N solves: each cluster receives at least B / 6 instances (with the two out-of-range routes
    in), no feature lies within 1e-6 of a cell boundary, the oracle solves every instance under every cluster's GPs (status 0), and the
    median over the instances of max |u - u under the next cluster's GPs| is above 1e-5: a wrong `which` cannot stay within 1e-8."""
    path = next(p for p, r in Q.ROUTED_PATHS.items() if r[0] == N)
    cfg, s, xs, us, route = Q.scenario(path)
    r = Q.with_off(route)
    assert (np.bincount(r[(r >= 0) & (r < 3)], minlength=3) >= Q.B1 // 6).all(), np.bincount(route)
    assert all(route[b] != v for b, v in Q.OFF.items())
    gps = Q.clusters()
    sol = [qoracle.solve_batch(Q.cluster_config(cfg, g), *Q.quad_args(s), nthreads=16) for g in gps]
    assert all((o[3] == 0).all() for o in sol)
    other = np.array([np.abs(sol[route[b]][1][b] - sol[(route[b] + 1) % 3][1][b]).max() for b in range(Q.B1)])
    print("ROUTED N=%d: instances per cluster %s, median max|u - u_next cluster| %.1e" % (N, np.bincount(route).tolist(), np.median(other)))
    assert np.median(other) > 1e-5
    # the rearranged routes of the other tests keep the counts; the first-node GP state of part 4 moves the solution
    gs = Q.gp_state(s)
    _, o = Q.oracle_routed(qoracle, cfg, gps, route[:32], {k: v[:32] for k, v in s.items()}, gp_state=gs[:32])
    assert np.median(np.abs(o[1] - np.stack([sol[route[b]][1][b] for b in range(32)])).reshape(32, -1).max(axis=1)) > 1e-5


@pytest.mark.parametrize("N", HORIZONS)
def test_fp64_oracle_against_80_bit_arithmetic_on_the_routed_inputs(qoracle, N):
    """The distance between the fp64 and the 80-bit oracle on the routed batch of horizon N, each instance under its own cluster's GPs:
    the figure quad_routed_spec.bound turns into a path's bound, were 1e-8 out of reach.  Asserted: the two agree in status, and the
    bound it gives stays below the median effect of a wrong cluster by a factor of 10."""
    from oracle.quad_oracle import QuadOracle
    path = next(p for p, r in Q.ROUTED_PATHS.items() if r[0] == N)
    cfg, s, xs, us, route = Q.scenario(path)
    gps = Q.clusters()
    _, o = Q.oracle_routed(qoracle, cfg, gps, route, s)
    _, o8 = Q.oracle_routed(QuadOracle(variant="ld"), cfg, gps, route, s)
    np.testing.assert_array_equal(o[3], o8[3])
    same = o[4] == o8[4]
    du, dx = np.abs(o[1] - o8[1])[same].max(), np.abs(o[0] - o8[0])[same].max()
    print("ROUTED N=%d: fp64 oracle against 80-bit, max|du| %.1e max|dx| %.1e (same iteration count: %d of %d) -> bound %.1e"
          % (N, du, dx, same.sum(), len(same), Q.bound(max(du, dx))))
    assert same.mean() >= 0.9 and Q.bound(max(du, dx)) <= 1e-6
