"""CPU side of the fp32-path tests (tests/test_fp32_path.py runs the device): the float yardsticks themselves, the reference values the
GPU budgets are taken from, and the GP finding with its fix in the form a CPU can see.

  - The float oracle (liboracle_f32.so) is the model in float arithmetic: within float rounding of the 80-bit oracle, with the device's
    p == 0 rule.
  - Every batch of tests/fp32_path.py:ROWS meets, with the float emulator alone (fed the float oracle's linearisation), the conditions
    the GPU test places on it, and the committed BUDGET of that row is at most 4 x the emulator's distance from the fp64 oracle at the
    tight stop levels (rounded up to two digits).
  - GP models: at N = 40 the float algorithm returns status 0 on iterates far from the minimiser (the finding); at
    N = ADMPC_F32_GP_MAX_N it does not; admpc_solve_batch_f32 refuses everything beyond.
"""
import os
import re

import numpy as np
import pytest

import fp32_path as F
from ad_mpc_amd.config import default_config, tight_ipm, set_gp
from ad_mpc_amd.scenarios import random_scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    from emu.emu import Emu
    return Emu()


@pytest.fixture(scope="module")
def o32():
    from oracle.oracle import Oracle
    return Oracle(variant="f32")


@pytest.fixture(scope="module")
def o80():
    from oracle.oracle import Oracle
    return Oracle(variant="ld")


def test_float_oracle_is_the_model_in_float_arithmetic(o32, o80, oracle):
    """rk4_sens of the float build against 80-bit at float-rounded inputs: within 64 ulps of float per entry (scaled by the entry or 1),
    on every blend value; and not the fp64 build under another name (its error is float-sized, not double-sized)."""
    rng = np.random.default_rng(3)
    cfg = default_config(N=2)
    worst = 0.0
    for i in range(200):
        x = np.float32([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3, 3), rng.uniform(2, 15), rng.uniform(-0.3, 0.3),
                        rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5)]).astype(np.float64)
        u = np.float32([rng.uniform(-10, 5), rng.uniform(-3, 3)]).astype(np.float64)
        p = (0.0, 0.3, 1.0)[i % 3]
        for a, b in zip(o32.rk4_sens(cfg, x, u, p, cfg.Ts), o80.rk4_sens(cfg, x, u, p, cfg.Ts)):
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64))             # float values
            worst = max(worst, float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()))
    eps = float(np.finfo(np.float32).eps)
    assert eps / 16 < worst <= 64 * eps, worst


def test_float_oracle_drops_the_dynamic_terms_at_p_zero(o32, oracle):
    """v_x = 0, p = 0: finite (the fp64 build relies on 1e-99, which is 0 in float), equal to the fp64 kinematic model to float rounding,
    and independent of the tyre and inertia parameters bit for bit; with p > 0 they matter."""
    cfg = default_config(N=2)
    other = default_config(N=2); other.Cf *= 1.37; other.Cr /= 1.37; other.mass *= 1.37; other.Iz /= 1.37
    u = np.array([1.5, -0.25])
    for vx in (0.0, 6.5):
        x = np.array([1.0, 2.0, 0.3, vx, 0.1, 0.05, 0.1])
        a = o32.rk4_sens(cfg, x, u, 0.0, cfg.Ts); b = o32.rk4_sens(other, x, u, 0.0, cfg.Ts); c = oracle.rk4_sens(cfg, x, u, 0.0, cfg.Ts)
        for m, n, r in zip(a, b, c):
            assert np.isfinite(m).all() and np.array_equal(m, n)
            assert np.abs(m - r).max() <= 1e-5
    x = np.array([1.0, 2.0, 0.3, 6.5, 0.1, 0.05, 0.1])
    assert not np.array_equal(o32.rk4_sens(cfg, x, u, 0.3, cfg.Ts)[0], o32.rk4_sens(other, x, u, 0.3, cfg.Ts)[0])
    assert not np.isfinite(o32.f(cfg, np.array([1.0, 2.0, 0.3, 0.0, 0.1, 0.05, 0.1]), u, 0.3)).all()      # the blend keeps the reference's form


def test_float_linearisation_reaches_the_emulator_unchanged(o32, oracle):
    """pack_linearisation(dtype=float32) returns float arrays that Emu.solve passes on as they are, and pack_shooting packs shooting
    arrays exactly as pack_linearisation packs the oracle's."""
    from emu.emu import pack_linearisation, pack_shooting
    N = 5
    cfg = default_config(N=N)
    s = random_scenarios(3, N=N, seed=2, blend=(3.0, 5.0))
    GT, bl = pack_linearisation(o32, cfg, s["xbar"], s["ubar"], s["p"], dtype=np.float32)
    assert GT.dtype == np.float32 and bl.dtype == np.float32
    assert np.ascontiguousarray(GT, dtype=np.float32) is GT and np.ascontiguousarray(bl, dtype=np.float32) is bl
    phi = np.zeros((3, N, 7)); A = np.zeros((3, N, 7, 7)); Bm = np.zeros((3, N, 7, 2))
    for b in range(3):
        for k in range(N):
            phi[b, k], A[b, k], Bm[b, k] = oracle.rk4_sens(cfg, s["xbar"][b, k], s["ubar"][b, k], s["p"][b], cfg.Ts)
    G1, b1 = pack_linearisation(oracle, cfg, s["xbar"], s["ubar"], s["p"])
    G2, b2 = pack_shooting(phi, A, Bm, s["xbar"])
    assert np.array_equal(G1.reshape(G2.shape), G2) and np.array_equal(b1, b2)


@pytest.mark.parametrize("name", list(F.ROWS))
def test_row_batch_and_budget(name, emu, o32, oracle_omp):
    """The batch meets the GPU test's conditions with the emulator alone, and the committed budget is at most 4 x the emulator's value."""
    from test_fp32_path import BUDGET
    cfg, s = F.row(name)
    o = F.oracle_solve(oracle_omp, cfg, s)
    g = F.emu_passes(emu, cfg, s, F.cpu_lineariser(o32, cfg))
    F.batch_conditions(o, g, cfg)
    su, sx = F.stats(g, o)
    print("EMU %-14s |du| %.1e / %.1e / %.1e  |dx| %.1e / %.1e / %.1e" % ((name,) + su + sx))
    for got, lim in ((su, BUDGET[name][0]), (sx, BUDGET[name][1])):
        for v, l in zip(got, lim):
            assert l <= F.round_up(F.BUDGET_FACTOR * v) * (1 + 1e-9), (name, v, l)
    if name in F.SHIPPED:
        assert su[2] <= F.F32_BOUND


@pytest.mark.parametrize("N", [20, 40])
def test_sqp_tolerance_batch_and_budget(N, emu, o32, oracle, oracle_omp):
    """The batch of the GPU's SQP-with-tolerance test: the fp64 oracle converges within 10 passes on every instance (by selection), needs
    more than two on some; the CPU twin of the float solve converges on all of them with differing pass counts, and the committed
    budget is at most 4 x its distance from the oracle's converged solution."""
    from test_fp32_path import BUDGET
    s, ref = F.sqp_tol_batch(oracle_omp, N)
    assert (ref[3] == 0).all()
    cfg = tight_ipm(default_config(N=N, sqp_iters=20, sqp_tol=F.SQP_TOL))
    x, u, st, nqp = F.emu_sqp_tol(emu, oracle, cfg, s, F.cpu_lineariser(o32, cfg))
    assert (st == 0).all() and nqp.max() < 20 and len(np.unique(nqp)) > 1 and (nqp > 1).any(), np.bincount(nqp)
    su, sx = F.stats((x, u), ref)
    print("EMU sqp_tol_N%d passes %s |du| %.1e / %.1e / %.1e  |dx| %.1e / %.1e / %.1e" % ((N, np.bincount(nqp)) + su + sx))
    for got, lim in ((su, BUDGET["sqp_tol_N%d" % N][0]), (sx, BUDGET["sqp_tol_N%d" % N][1])):
        for v, l in zip(got, lim):
            assert l <= F.round_up(F.BUDGET_FACTOR * v) * (1 + 1e-9), (N, v, l)


def _gp_census(emu, o32, oracle, gp, N, B=256, seed=8):
    cfg = set_gp(tight_ipm(default_config(N=N)), F.gp_model(gp))
    s = random_scenarios(B, N=N, seed=seed)
    o = F.oracle_solve(oracle, cfg, s)
    g = F.emu_passes(emu, cfg, s, F.cpu_lineariser(o32, cfg))
    ok = (g[3] == 0) & (o[3] == 0)
    du = np.abs(g[1] - o[1]).reshape(B, -1).max(axis=1)
    return ok, du, g[4]


def test_gp_finding_and_bound(emu, o32, oracle_omp):
    """The finding: at N = 40 with the grid GP the float algorithm reports status 0 on instances more than 2.5e-3 (up to O(1)) from the
    fp64 minimiser, most of them solved by the inequality-free trial (iters == 0: the float Riccati recursion alone).  At the bound
    (N = 28) and below, none -- on a slice of the census of scripts/census_f32_gp.py.  Emulator values."""
    ok, du, it = _gp_census(emu, o32, oracle_omp, "grid", 40)
    bad = ok & (du > F.F32_BOUND)
    assert bad.sum() >= 10 and du[bad].max() > 0.1 and (it[bad] == 0).any(), (bad.sum(), du[ok].max())
    for gp, N in (("grid", F.GP_MAX_N), ("grid", 24), ("multi", F.GP_MAX_N)):
        ok, du, it = _gp_census(emu, o32, oracle_omp, gp, N)
        assert ok.all() and du.max() <= F.F32_BOUND, (gp, N, du.max())


def test_every_budget_row_states_its_emulator_and_device_values():
    """Under each BUDGET row: the emulator's six figures and the device's (or the words `not measured`), the device's within the budget
    unless the row is named in KNOWN_WEAK.  scripts/fp32_budget_table.py writes the block and keeps the device lines."""
    import test_fp32_path as T
    src = open(os.path.join(ROOT, "tests", "test_fp32_path.py")).read()
    blk = src[src.index("# BUDGET-BEGIN"):src.index("# BUDGET-END")]
    num = r"([0-9.e+-]+)"
    six = r"\|du\| %s / %s / %s; \|dx\| %s / %s / %s" % ((num,) * 6)
    rows = re.findall(r'"(\S+)": \(\(.*\n    #   emulator \(CPU\): ' + six + r"\n    #   device \(MI355X\): (?:not measured|" + six + r")\n", blk)
    assert [r[0] for r in rows] == list(T.BUDGET)
    for r in rows:
        lim = T.BUDGET[r[0]][0] + T.BUDGET[r[0]][1]
        assert all(float(v) <= l for v, l in zip(r[1:7], lim)), r[0]
        if r[7] and r[0] not in T.KNOWN_WEAK:
            assert all(float(v) <= l for v, l in zip(r[7:13], lim)), r[0]


def test_gp_bound_is_the_librarys():
    """The bound the tests use is the header's, and admpc_solve_batch_f32 refuses GP models beyond it before it launches anything."""
    hdr = open(os.path.join(ROOT, "include", "admpc.h")).read()
    assert int(re.search(r"#define\s+ADMPC_F32_GP_MAX_N\s+(\d+)", hdr).group(1)) == F.GP_MAX_N
    src = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "admpc_kernels.hip")).read()
    body = src[src.index("int admpc_solve_batch_f32("):]
    body = body[:body.index("\n}")]
    refuse = body.index("if (s->cfg.n_gp > 0 && s->cfg.N > ADMPC_F32_GP_MAX_N)")
    assert "return fail(ADMPC_EINVAL" in body[refuse:refuse + 200]
    assert refuse < body.index("solve_rows<float>") and refuse < body.index("ensure_status")
