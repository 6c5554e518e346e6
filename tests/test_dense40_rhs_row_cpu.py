"""dense40.h, dense40_factorise with a right-hand-side row: the right-hand side y of the first solve behind a factorisation rides
through the right-looking LDL' as row 40 of the matrix (lane 40) and comes out as D^-1 L^-1 y, so that solve needs no forward
substitution.  Two CPU checks:
  (a) a numpy restatement of the factorisation with and without the row: the factor does not notice the row, and the row is as close
      to an 80-bit forward solve as the substitution it replaces (both distances are measured here, on the same systems);
  (b) the generated 41-row Newton-row build (gen_subst_asm.py rowbuild(..., nrows=41)) on the lane interpreter: lane 40 receives its
      whole buffer, the lanes behind it nothing, the matrix lanes exactly what the 40-row build gives them.
"""
import importlib.util
import os

import numpy as np
import pytest

from asm_emu import Wave, WAVE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_subst_asm", os.path.join(ROOT, "ad_mpc_amd", "csrc", "gen_subst_asm.py"))
gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)

N = 40


def ldl_right_looking(M, y=None):
    """The factorisation as dense40_factorise runs it: row i in "lane" i (lower triangle, the rest zero), column j final when the
    rank-1 updates of columns < j are in; pivot chain dinv = 1 / a[j][j], lu = a[:, j] * dinv; update a[:, jj] += a[jj][j] * (-lu) on
    EVERY lane.  With y: one more lane whose row is y.  Returns L (strictly lower), d, and the extra lane's lu per column."""
    rows = N + (y is not None)
    a = np.zeros((rows, N))
    a[:N] = np.tril(M)
    if y is not None:
        a[N] = y
    L = np.zeros((N, N)); d = np.zeros(N); w = np.zeros(N)
    for j in range(N):
        d[j] = a[j, j]
        dinv = 1.0 / d[j]
        lu = a[:, j] * dinv
        L[j + 1:, j] = lu[j + 1:N]
        if y is not None:
            w[j] = lu[N]
        nl = -lu
        for jj in range(j + 1, N):
            a[:, jj] = a[:, jj] + a[jj, j] * nl
    return L, d, (w if y is not None else None)


def forward_substitution(L, d, y):
    """fwd_subst_40 and the scaling behind it: z_j final, then y_i -= L_ij z_j for the rows below; z * (1 / d)."""
    z = y.copy()
    for j in range(N):
        z[j + 1:] = z[j + 1:] - L[j + 1:, j] * z[j]
    return z * (1.0 / d)


def forward_80bit(L, d, y):
    Lq = L.astype(np.longdouble); z = y.astype(np.longdouble)
    for j in range(N):
        z[j + 1:] = z[j + 1:] - Lq[j + 1:, j] * z[j]
    return z / d.astype(np.longdouble)


def _systems():
    """H = G'G scaled to a unit largest diagonal entry, plus barrier diagonals from 1e-3 to 1e10 (every third system: up to 1 only, so
    that the factor stays far from the identity in every row); right-hand sides from 1e-3 to 1e3."""
    rng = np.random.default_rng(20)
    for k in range(60):
        G = rng.normal(size=(N, N))
        H = G.T @ G
        H /= H.diagonal().max()
        M = H + np.diag(10.0 ** rng.uniform(-3, 0 if k % 3 == 0 else 10, size=N))
        y = rng.normal(size=N) * 10.0 ** rng.uniform(-3, 3, size=N)
        yield k, M, y


def test_rhs_row_leaves_the_factor_alone_and_matches_the_substitution():
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an 80-bit type on this platform"
    for k, M, y in _systems():
        L0, d0, _ = ldl_right_looking(M)
        L1, d1, w = ldl_right_looking(M, y)
        assert np.array_equal(L0, L1) and np.array_equal(d0, d1), "system %d: the factor changed with the row" % k
        ref = forward_80bit(L0, d0, y)
        dist = lambda v: float(np.sqrt(((v.astype(np.longdouble) - ref) ** 2).sum() / (ref ** 2).sum()))       # relative, 2-norm over the 40 entries
        e_row = dist(w)
        e_sub = dist(forward_substitution(L0, d0, y))
        print("system %2d: row form %.2e, substitution form %.2e (relative 2-norm distance from the 80-bit solve)" % (k, e_row, e_sub))
        assert e_sub > 0.0
        assert e_row <= 4.0 * e_sub, "system %d: row form %.3e, substitution form %.3e" % (k, e_row, e_sub)


LP, LB = 0, 8 * 1000           # byte addresses: packed rows of H, the right-hand-side buffer [40]


def _rowbuild(nrows, H, yb, dbar, sodd):
    w = Wave()
    for i in range(N):
        for j in range(i + 1):
            w.lds[LP + 8 * (i * (i + 1) // 2 + j)] = H[i, j]
    for j in range(N):
        w.lds[LB + 8 * j] = yb[j]
    lane = np.arange(WAVE)
    row = np.zeros((WAVE, N))
    for lo, hi in ((0, N // 2), (N // 2, N)):
        cnt = hi - lo
        ops = ["v[%d:%d]" % (2 * q, 2 * q + 1) for q in range(cnt)] + ["v200", "v[202:203]", "v[204:205]"]
        w.v[200] = np.where(lane < N, LP + 8 * (lane * (lane + 1) // 2), np.where(lane == N, LB, LP))
        w.v[202] = dbar.copy(); w.v[204] = sodd.copy()
        w.run(gen.rowbuild(N, lo, hi, nrows), ops)
        for q in range(cnt):
            row[:, lo + q] = w.v[2 * q]
    assert w.exec.all()
    return row


def test_row_build_with_41_rows_on_the_lane_interpreter():
    rng = np.random.default_rng(41)
    H = rng.normal(size=(N, N)); H = H + H.T
    yb = rng.normal(size=N)
    lane = np.arange(WAVE)
    dbar = rng.normal(size=WAVE)                                      # also on lanes >= 40: it must not reach any of them
    sodd = np.where(lane < N, rng.normal(size=WAVE), 0.0)             # the callers pass 0 on the lanes behind the matrix
    r41 = _rowbuild(N + 1, H, yb, dbar, sodd)
    r40 = _rowbuild(None, H, yb, dbar, sodd)
    assert np.array_equal(r41[N], yb)                                 # all 40 entries of the buffer, no diagonal term, no s_odd
    assert np.abs(r41[N + 1:]).max() == 0.0
    assert np.abs(r40[N:]).max() == 0.0
    assert np.array_equal(r41[:N], r40[:N])
    for i in range(N):
        for c in range(N):
            want = (H[i, c] if c <= i else 0.0) + (sodd[i] if c & 1 else 0.0) + (dbar[i] if c == i else 0.0)
            assert abs(r41[i, c] - want) < 1e-13, (i, c)


def test_generated_include_holds_the_41_row_build():
    txt = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "subst_asm.inc")).read()
    for half, (lo, hi) in (("A", (0, N // 2)), ("B", (N // 2, N))):
        assert gen.emit("ADMPC_ROWBUILD_ASM_%d_%s_R%d" % (N, half, N + 1), gen.rowbuild(N, lo, hi, N + 1)) in txt
