"""The batches of the fp32-path tests and their CPU twin, shared by tests/test_fp32_path_cpu.py (no GPU) and tests/test_fp32_path.py
(-m gpu).  TEST INFRASTRUCTURE ONLY.

ROWS is the one table of solve batches.  Each row is solved by
  - the fp64 oracle at the tight stop levels (tight_ipm): the minimiser the float path is measured against.  The float path floors its
    own stop levels (rq_make_params), so the measured distance is the float path's alone;
  - the float emulator (tests/emu: the product's rowqp_core.h, T = float) fed the float oracle's linearisation (liboracle_f32.so) on
    the CPU, or the device's own float linearisation (admpc_shoot_batch_f32) on the GPU;
  - the device (admpc_solve_batch_f32), GPU only.
`stats` turns two results into the six figures the budgets are stated in: median, 99 % and max of the per-instance max |du|, |dx|.
"""
import numpy as np

from ad_mpc_amd.config import default_config, tight_ipm, set_gp
from ad_mpc_amd.scenarios import random_scenarios, grid_gp, assemble

B_ROW = 512
F32_BOUND = 2.5e-3            # the documented bound of the fp32 path on shipped weights
GP_MAX_N = 28                 # ADMPC_F32_GP_MAX_N (include/admpc.h): scripts/census_f32_gp.py
BUDGET_FACTOR = 4.0           # the convention of tests/test_accuracy_80bit.py
HORIZONS = (2, 3, 7, 13, 19, 21, 33, 40, 64, 65, 97, 128)
ARGS = ("x0", "yref", "yref_e", "p", "xbar", "ubar")

# name -> (kind, N, argument of the kind, seed).  Kinds: "shipped" (argument: blend or None for the generator's default, p = 0
# everywhere), "q7" (argument: draw d of tests/test_problem_data.py:_draw, even: iterate at x0 / blend (3, 5), odd: zero iterate),
# "q127" (all seven state weights, as test_all_state_weights_nonzero), "gp" (argument: "grid" or "multi"), "sqp3" (three passes).
ROWS = {}
for _N in HORIZONS:
    ROWS["N%d" % _N] = ("shipped", _N, (3.0, 5.0), 100)
ROWS["N40_kinematic"] = ("shipped", 40, None, 100)
for _N in (20, 40, 80):
    for _d in (0, 1):
        ROWS["q7_N%d_d%d" % (_N, _d)] = ("q7", _N, _d, None)
ROWS["q127_N20"] = ("q127", 20, None, 99)
ROWS["q127_N24"] = ("q127", 24, None, 99)
# GP residuals: both GPs of the suite at every horizon of HORIZONS that admpc_solve_batch_f32 allows for GP models, at the bound itself,
# and the grid GP at N = 20 (config 3) and 24 (the last horizon of the census whose states stay within 1e-1)
GP_HORIZONS = tuple(n for n in HORIZONS if n <= GP_MAX_N) + (GP_MAX_N,)
for _N in sorted(set(GP_HORIZONS + (20, 24))):
    ROWS["gp_grid_N%d" % _N] = ("gp", _N, "grid", 100)
for _N in sorted(set(GP_HORIZONS + (20,))):
    ROWS["gp_multi_N%d" % _N] = ("gp", _N, "multi", 77)
ROWS["sqp3_N20"] = ("sqp3", 20, (3.0, 5.0), 100)
# rows whose weights are the shipped ones: the device max |du| is held to F32_BOUND as well
SHIPPED = tuple(n for n, r in ROWS.items() if r[0] in ("shipped", "gp", "sqp3"))


def gp_model(name):
    if name == "grid":
        return grid_gp()
    from test_gpu_parity import _multi_feature_gps
    return _multi_feature_gps()


def row(name, B=B_ROW):
    """(cfg at the tight stop levels, scenarios) of a row."""
    kind, N, arg, seed = ROWS[name]
    if kind == "q7":
        from test_gpu_parity import random_q7_problem
        rng = np.random.default_rng([2026, N, arg])
        cfg = random_q7_problem(rng, N)
        kw = dict(blend=(3.0, 5.0), init="x0") if arg % 2 == 0 else dict(init="zeros")
        return tight_ipm(cfg), random_scenarios(B, N=N, Ts=cfg.Ts, seed=int(rng.integers(1 << 30)), **kw)
    if kind == "q127":
        return tight_ipm(default_config(N=N, q=(10.0, 10.0, 100.0, 1.0, 2.0, 3.0, 4.0))), random_scenarios(B, N=N, seed=seed, blend=(3.0, 5.0))
    if kind == "gp":
        cfg = set_gp(tight_ipm(default_config(N=N)), gp_model(arg))
        arg = None if arg == "grid" else (3.0, 5.0)
    else:
        cfg = tight_ipm(default_config(N=N, sqp_iters=3 if kind == "sqp3" else 1))
    s = random_scenarios(B, N=N, seed=seed, **({} if arg is None else dict(blend=arg)))
    if N < 19:
        # the generator's errors are too small to reach a bound within so few stages (the inequality-free trial solves nearly every
        # instance): the steering angle starts around its hard bound (0.52), inside and outside, with either sign
        rng = np.random.default_rng([seed, N])
        x0 = s["x0"].copy()
        x0[:, 6] = rng.uniform(0.4, 0.75, B) * rng.choice([-1.0, 1.0], B)
        s = assemble(x0, s["xref"], np.zeros((B, N, 2)), **({} if arg is None else dict(blend=arg)))
    return cfg, s


def args32(s):
    """The scenario arrays rounded to float once: what the device and the emulator receive, bit for bit."""
    return {k: np.ascontiguousarray(s[k], dtype=np.float32) for k in ARGS}


def oracle_solve(oracle, cfg, s, nthreads=8):
    """fp64 oracle on the unrounded inputs: the float path's distance includes the rounding of its inputs, as its documented bound does."""
    return oracle.solve_batch(cfg, *(s[k] for k in ARGS), nthreads=nthreads)


def emu_passes(emu, cfg, s, linearise, passes=None, want_pi=False):
    """The float emulator over cfg.sqp_iters passes (sqp_tol = 0) as admpc_solve_batch_f32 runs them: linearise at the float iterate,
    solve, and leave an instance alone once it has failed.  linearise(xbar32, ubar32, p32) -> (GT, bl) in float32."""
    a = args32(s)
    x, u = a["xbar"].copy(), a["ubar"].copy()
    B = len(x)
    st = np.zeros(B, dtype=np.int32); it = np.zeros(B, dtype=np.int32); cost = np.zeros(B, dtype=np.float32)
    extra = ()
    for _ in range(passes or max(1, int(cfg.sqp_iters))):
        GT, bl = linearise(x, u, a["p"])
        assert GT.dtype == np.float32 and bl.dtype == np.float32
        g = emu.solve(cfg, a["x0"], a["yref"], a["yref_e"], GT, bl, x, u, dtype=np.float32, want_pi=want_pi)
        live = st == 0
        x[live], u[live], cost[live], st[live], it[live] = g[0][live], g[1][live], g[2][live], g[3][live], g[4][live]
        extra = g[5:7] if want_pi else ()
    return (x, u, cost, st, it) + tuple(extra)


def cpu_lineariser(o32, cfg):
    from emu.emu import pack_linearisation
    return lambda x, u, p: pack_linearisation(o32, cfg, x, u, p, dtype=np.float32)


def stats(g, o):
    """Over the instances where the reference o has status 0: (|du| median, 99 %, max), (|dx| median, 99 %, max)."""
    ok = o[3] == 0
    B = len(ok)
    du = np.abs(g[1].astype(np.float64) - o[1]).reshape(B, -1).max(axis=1)[ok]
    dx = np.abs(g[0].astype(np.float64) - o[0]).reshape(B, -1).max(axis=1)[ok]
    q = lambda v: (float(np.median(v)), float(np.quantile(v, 0.99)), float(v.max()))
    return q(du), q(dx)


def round_up(v, digits=2):
    """v rounded up to `digits` significant digits (budgets are stated that way)."""
    if v <= 0:
        return 0.0
    e = int(np.floor(np.log10(v))) - (digits - 1)
    return float(np.ceil(v / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e)


def batch_conditions(o, g, cfg):
    """The conditions a chosen batch has to meet, on the CPU with the emulator's result g and on the GPU with the device's: statuses
    as the oracle's, >= 90 % status 0, >= a quarter with interior-point iterations, nobody at iter_max."""
    np.testing.assert_array_equal(g[3], o[3])
    ok = o[3] == 0
    assert ok.mean() >= 0.9, ok.mean()
    assert (g[4][ok] > 0).mean() >= 0.25, (g[4][ok] > 0).mean()
    assert g[4][ok].max() < cfg.ipm_iter_max, g[4][ok].max()


# ---- SQP with a tolerance (the only route into admpc_nlp_res_kernel<float>)
SQP_TOL = 1e-6
SQP_FLOORS = (1e-2, 1e-4, 1e-2, 1e-3)       # admpc_nlp_res_kernel<float>: res_stat, res_eq, res_ineq, res_comp


def sqp_tol_batch(oracle, N, B=B_ROW, passes=10, nthreads=8):
    """The first B scenarios of a seeded stream on which the fp64 oracle's SQP (tolerance 1e-6) converges within `passes` QPs, and the
    oracle's converged result on them.  The selection is the reference's alone."""
    cfg = tight_ipm(default_config(N=N, sqp_iters=passes, sqp_tol=SQP_TOL))
    s = random_scenarios(4 * B, N=N, seed=100, blend=(3.0, 5.0))            # kinematic, blended and dynamic instances in one batch
    o = oracle_solve(oracle, cfg, s, nthreads)
    keep = np.nonzero(o[3] == 0)[0][:B]
    assert len(keep) == B
    return {k: v[keep] for k, v in s.items()}, tuple(v[keep] for v in o)


def emu_sqp_tol(emu, o64, cfg, s, linearise):
    """CPU twin of an fp32 SQP solve with a tolerance: the float emulator per pass, and in front of every pass but the first the stopping
    test of admpc_nlp_res_kernel<float> -- evaluated by the fp64 oracle's restatement at the float iterate and multipliers against the
    float kernel's floored tolerances.  Returns (x, u, status, number of QPs per instance)."""
    a = args32(s)
    x, u = a["xbar"].copy(), a["ubar"].copy()
    B = len(x)
    d = lambda v: np.asarray(v, dtype=np.float64)
    tol = np.maximum(cfg.sqp_tol, SQP_FLOORS)
    done = np.zeros(B, dtype=bool); failed = np.zeros(B, dtype=bool); nqp = np.zeros(B, dtype=np.int32)
    pi = ineq = None
    for sq in range(int(cfg.sqp_iters)):
        if sq > 0:
            for b in np.nonzero(~done & ~failed)[0]:
                res = o64.nlp_residuals(cfg, d(a["x0"][b]), d(a["yref"][b]), d(a["yref_e"][b]), float(a["p"][b]), d(x[b]), d(u[b]), d(pi[b]), d(ineq[b]))
                done[b] = bool((res <= tol).all())
        GT, bl = linearise(x, u, a["p"])
        g = emu.solve(cfg, a["x0"], a["yref"], a["yref_e"], GT, bl, x, u, dtype=np.float32, want_pi=True)
        live = ~done & ~failed
        if pi is None:
            pi, ineq = g[5].copy(), g[6].copy()
        x[live], u[live], pi[live], ineq[live] = g[0][live], g[1][live], g[5][live], g[6][live]
        nqp[live] += 1
        failed |= live & (g[3] != 0)
    return x, u, np.where(failed, 4, np.where(done, 0, 2)).astype(np.int32), nqp
