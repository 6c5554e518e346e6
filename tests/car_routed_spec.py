"""The kernel paths of the car's routed solve (admpc_solve_batch_routed) and the inputs their tests share (TEST INFRASTRUCTURE).

PATHS names every launch regime a routed car solve takes: kernel F, kernel S, and kernel R (admpc_linearize_kernel + admpc_rowqp_kernel)
with one, two and four instances per wave, in two phases by default and on request, in chunks, at the GP default of N = 40, next to a
nominal cluster on kernel S, and in SQP mode with and without a tolerance.  car_kernel mirrors the dispatch of admpc_create / solve_impl
(its lines are in batch_regimes.LAUNCH_LINES); test_car_routed_paths_cpu.py holds the table against the source.  `scenario` draws the
inputs of one path: what tests/test_car_routed_paths.py solves on the device is what the CPU module checks, with the oracle alone, for
the conditions that keep a routed comparison from passing vacuously.

The K = 3 clusters are three GP sets of gp_structures.car_structures(), each with its own structure (n_gp 4 / 3 / 2, input features, 32
training points).  The route is the numpy nearest-centroid rule on v_x (feature 3) with centroids placed so that the cell boundaries
fall between the terciles of the batch: every cluster gets a third of it by construction.

The short horizon is N = 17.  At N = 13 the unconstrained trial solves 90 % of gp_structures.car_batch and every instance of the fastest
third, so a quarter of the batch would not iterate and a split batch would defer nothing of cluster 2; N = 17 is the first horizon at
which 30 % iterate on every batch used here (test_car_routed_paths_cpu.py asserts the floors).  The oracle solves the largest batch
(4261 instances at 256 CUs) in a tenth of a second either way."""
import numpy as np

import batch_regimes as R
import gp_structures as G
from ad_mpc_amd.config import default_config, NX, NU

K = 3
SETS = ("four_gps", "rotation_b", "inputs_alone")                  # cluster c runs the GPs of SETS[c]
FEATS = [3]                                                         # v_x
NC_CPU = 256                                                        # the CU count the CPU module draws the nc-sized batches for

# path: N, environment at the creation of the handles, batch (a number, or a key of batch_regimes.rowqp_sizes(num_cu)), clusters without
# GPs, (sqp_iters, sqp_tol), the kernel each cluster's handle runs, and for kernel R the regime: instances per wave of the (first) launch
# and whether it runs in two phases ("default": by batch size, "forced": ADMPC_ROWQP_SPLIT=1), the chunk cap
PATHS = {
    "R17_rows1": dict(N=17, env={}, B=96, kernels="RRR", rows=1, split=None),
    "R17_rows2": dict(N=17, env={}, B="rows2", kernels="RRR", rows=2, split=None),
    "R17_rows4": dict(N=17, env={}, B="rows4", kernels="RRR", rows=4, split=None),
    "R17_split": dict(N=17, env={}, B="split", kernels="RRR", rows=4, split="default"),
    "R17_forced_split": dict(N=17, env={"ADMPC_ROWQP_SPLIT": "1"}, B=97, kernels="RRR", rows=1, split="forced"),
    "R17_chunked": dict(N=17, env={"ADMPC_ROWQP_CHUNK": "40"}, B=97, kernels="RRR", rows=1, split=None, chunks=(40, 40, 17)),
    "R40": dict(N=40, env={}, B=96, kernels="RRR", rows=1, split=None),
    "S40_mixed": dict(N=40, env={}, B=96, nominal=(1,), kernels="RSR", rows=1, split=None),
    "F20_sqp3": dict(N=20, env={}, B=96, sqp=(3, 0.0), kernels="FFF"),
    "R20_sqp_tol": dict(N=20, env={}, B=96, sqp=(3, 1e-6), kernels="RRR", rows=1, split=None),
    "R17_sqp_tol_split": dict(N=17, env={"ADMPC_ROWQP_SPLIT": "1"}, B=97, sqp=(3, 1e-6), kernels="RRR", rows=1, split="forced"),
}
SQP_TOL_PATHS = [p for p, r in PATHS.items() if r.get("sqp", (1, 0.0))[1] > 0.0]
SQP_TOL = 1e-7                                                      # test_gp_structures.py::test_car_sqp_with_a_tolerance: |du|, |dx|
OFF = {5: 7, 6: -1, 11: K}                                          # instance: a route that names no cluster


def car_kernel(N, env, n_gp, sqp_iters=1, sqp_tol=0.0):
    """The kernel a handle created under `env` runs for a plain or routed fp64 solve without multiplier outputs: admpc_create's use_dense
    and use_seg, then solve_impl's `dense` and its use_seg branch."""
    qp = env.get("ADMPC_QP")
    use_dense = N == 20 and qp != "riccati"
    use_seg = N in (40, 60, 80) and (qp != "riccati" if n_gp == 0 else qp == "seg")
    tol_on = sqp_iters > 1 and sqp_tol > 0.0
    if use_seg and not tol_on:
        return "S"
    return "F" if use_dense and not tol_on else "R"


def split_mode(env):
    """admpc_create: -1 by batch size, 0 never, 1 always."""
    e = env.get("ADMPC_ROWQP_SPLIT", "")
    return 0 if e[:1] == "0" else (1 if e[:1] == "1" else -1)


def chunks(N, B, env, elem=8):
    """The chunk sizes solve_rows cuts a batch into (rowqp_chunk: 32-bit byte offsets, capped by ADMPC_ROWQP_CHUNK)."""
    m = min(((1 << 32) - 1) // ((N + 1) * 42 * elem), 0x7fffffff)
    c = int(env.get("ADMPC_ROWQP_CHUNK", "0") or 0)
    if 0 < c < m:
        m = c
    return tuple(min(m, B - off) for off in range(0, B, m))


def regime(path, nc):
    """(instances per wave, two phases?) of every chunk of the path's batch at `nc` CUs, by the mirrored launch plan."""
    r = PATHS[path]
    out = []
    for nb in chunks(r["N"], batch_size(path, nc), r["env"]):
        rows = R.rowqp_rows(nc, nb)
        mode = split_mode(r["env"])
        out.append((rows, mode == 1 or (mode == -1 and R.rowqp_splits(nc, nb, rows))))
    return out


def batch_size(path, nc):
    B = PATHS[path]["B"]
    return R.rowqp_sizes(nc)[B] if isinstance(B, str) else B


_GPS = {}


def clusters():
    if not _GPS:
        sets = dict(G.car_structures())
        _GPS["k"] = [sets[name] for name in SETS]
    return _GPS["k"]


def path_configs(path, sqp=None):
    """The K configs of a path: cluster c with the GPs of SETS[c] (or none, where the path names it nominal) and the path's SQP mode, or
    the mode (sqp_iters, sqp_tol) given: (1, 0.0) is the first QP of the path alone."""
    r = PATHS[path]
    it, tol = sqp if sqp is not None else r.get("sqp", (1, 0.0))
    kw = dict(sqp_iters=it, sqp_tol=tol) if it > 1 else {}
    return [default_config(N=r["N"], **kw) if c in r.get("nominal", ()) else G.car_cfg(gps, r["N"], **kw) for c, gps in enumerate(clusters())]


def select_numpy(xs, us, feats, cent):
    """admpc_select_cluster_batch in numpy: z = [x; u][feats]; per centroid the sum of the squared differences in feature order (no fused
    multiply-add), its square root, and the first strict minimum wins -- so a tie goes to the lower index, and a distance that is NaN or
    +inf for every centroid leaves cluster 0."""
    z = np.concatenate([np.asarray(xs, dtype=np.float64).reshape(-1, NX), np.asarray(us, dtype=np.float64).reshape(-1, NU)], axis=1)[:, list(feats)]
    cent = np.asarray(cent, dtype=np.float64).reshape(-1, len(feats))
    best = np.full(len(z), np.inf); route = np.zeros(len(z), dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(len(cent)):
            acc = np.zeros(len(z))
            for j in range(len(feats)):
                e = z[:, j] - cent[c, j]
                acc = acc + e * e
            dist = np.sqrt(acc)
            better = dist < best
            best[better] = dist[better]; route[better] = c
    return route


def tercile_centroids(v):
    """Three centroids on a line whose two cell boundaries lie half way between neighbouring values of v, a third of v on each side:
    c1 = median, c0 = 2 q33 - c1, c2 = 2 q67 - c1."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    n = len(s)
    q33, q67 = (0.5 * (s[k - 1] + s[k]) for k in (n // 3, n - n // 3))
    c1 = float(np.median(s))
    return np.array([[2.0 * q33 - c1], [c1], [2.0 * q67 - c1]])


def car_args(s):
    return tuple(s[k] for k in G.CAR_ARGS)


_SCEN = {}
WARM_QPS = 30                                                       # full steps that take the warm-started instances to convergence


def scenario(path, nc, oracle=None):
    """(configs, s, route, centroids) of one path at `nc` CUs.  The batch depends on (N, B) alone, the route on the batch: the paths of
    one horizon and size solve the same problems.  route: the numpy rule's, before the out-of-range entries of OFF go in.

    The paths with an SQP tolerance need `oracle`: three QPs from the cold iterate of car_batch end every instance at the QP limit
    (status 2), so every fourth instance starts from the iterate the oracle reaches after WARM_QPS full steps under its own cluster
    (where those converge), and stops on the tolerance in front of its second QP: converged and unconverged instances side by side."""
    N, B = PATHS[path]["N"], batch_size(path, nc)
    if (N, B) not in _SCEN:
        s = G.car_batch(N, B)
        cent = tercile_centroids(s["x0"][:, 3])
        route = select_numpy(s["x0"], s["ubar"][:, 0, :], FEATS, cent)
        d = np.sort(np.abs(s["x0"][:, 3:4] - cent[:, 0][None, :]), axis=1)
        assert (d[:, 1] - d[:, 0]).min() >= 1e-9, "a speed within 1e-9 of a cell boundary"
        _SCEN[N, B] = (s, route, cent)
    s, route, cent = _SCEN[N, B]
    if path in SQP_TOL_PATHS:
        if ("warm", path, B) not in _SCEN:
            assert oracle is not None, "the warm start of %s needs the oracle" % path
            _, o = oracle_routed(oracle, path_configs(path, sqp=(WARM_QPS, 0.0)), route, s)
            w = (np.arange(B) % 4 == 1) & (o[3] == 0) & (np.abs(o[0]).max(axis=(1, 2)) < 1e3) & (np.abs(o[1]).max(axis=(1, 2)) < 1e3)
            _SCEN["warm", path, B] = dict(s, xbar=np.where(w[:, None, None], o[0], s["xbar"]), ubar=np.where(w[:, None, None], o[1], s["ubar"]))
        s = _SCEN["warm", path, B]
    return path_configs(path), s, route, cent


def poisoned(s, route, rows=4):
    """(s with one non-finite entry in an instance of every cluster, those instances): NaN in x0 for cluster 0, +inf in yref for
    cluster 1, NaN in yref for cluster 2 -- each the first instance of its cluster that shares its wave of `rows` with another cluster."""
    route = np.asarray(route)
    bad = []
    for c in range(K):
        for b in np.flatnonzero(route == c):
            q = route[b - b % rows: b - b % rows + rows]
            if len(set(q[in_range(q)].tolist())) >= 2 and all(b // rows != x // rows for x in bad):
                bad.append(int(b)); break
    assert len(bad) == K
    x0, yref = s["x0"].copy(), s["yref"].copy()
    x0[bad[0], 1] = np.nan; yref[bad[1], 2, 3] = np.inf; yref[bad[2], 1, 0] = np.nan
    return dict(s, x0=x0, yref=yref), bad


def with_off(route):
    """The route with 7, -1 and K at three fixed places: instances no handle solves."""
    r = np.array(route, dtype=np.int32)
    for b, v in OFF.items():
        if b < len(r):
            r[b] = v
    return r


def in_range(route, k=K):
    route = np.asarray(route)
    return (route >= 0) & (route < k)


def oracle_routed(oracle, cfgs, route, s, idx=None, rotate=0, nthreads=16):
    """The oracle's solve of every in-range instance (of idx, when given) under the config of its own cluster -- of the cluster `rotate`
    places on, when given: (index array, results)."""
    route = np.asarray(route)
    idx = np.arange(len(route)) if idx is None else np.asarray(idx)
    idx = idx[in_range(route[idx], len(cfgs))]
    args = car_args(s)
    out = None
    for c in range(len(cfgs)):
        m = idx[route[idx] == c]
        if not len(m):
            continue
        o = oracle.solve_batch(cfgs[(c + rotate) % len(cfgs)], *(a[m] for a in args), nthreads=nthreads)
        if out is None:
            out = [np.zeros((len(route),) + a.shape[1:], dtype=a.dtype) for a in o]
        for a, b in zip(out, o):
            a[m] = b
    return idx, tuple(a[idx] for a in out)


def quadruple_mix(route, rows=4):
    """How many distinct in-range clusters each wave of `rows` consecutive instances holds: the set of counts over the batch."""
    route = np.asarray(route)
    return {len(set(route[i:i + rows][in_range(route[i:i + rows])].tolist())) for i in range(0, len(route), rows)}


def degenerate_routes(route):
    """The routes of the bit-for-bit test: the drawn one with its out-of-range entries; every instance to cluster 1 (handles 0 and 2 skip
    every wave); no instance to cluster 1; b % K (every quadruple mixed); blocks of four consecutive instances per cluster (whole waves
    skip at four instances per wave)."""
    B = len(route)
    b = np.arange(B)
    return {
        "drawn": with_off(route),
        "all to cluster 1": np.ones(B, dtype=np.int32),
        "none to cluster 1": np.where(np.asarray(route) == 1, (b % 2) * 2, route).astype(np.int32),
        "b % K": (b % K).astype(np.int32),
        "blocks of four": ((b // 4) % K).astype(np.int32),
    }
