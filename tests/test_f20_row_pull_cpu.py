"""Kernel F pulls H into registers without masks and presets, votes on its two threshold-only stop tests and scans its per-stage
quantities in five steps (gen_subst_asm.py rowpull / symrow(preset=False), dense40.h, cond_common.h wave_scan_incl32).  CPU checks:
  (a) the unmasked row build on the lane interpreter against the masked 41-row build, bit for bit on every entry the factorisation reads
      (at or below the diagonal of lanes 0..39, all of lane 40), the rest of LDS holding NaN; with the diagonal term added in registers
      and with the diagonal slots rewritten in LDS, s_odd zero and non-zero, odd and even lanes apart;
  (b) the symmetric row without presets against the one with them, lanes 0..39;
  (c) the right-looking LDL' with a right-hand-side row (the model of test_dense40_rhs_row_cpu.py, restated on 64 lanes) with NaN in every
      entry the unmasked build leaves undefined: same L, pivots and right-hand-side row, byte for byte -- a leak would show as NaN;
  (d) all(!(x > tol)) against max-ignoring-NaN(x) <= tol, and the five-step scan against the six-step one;
  (e) subst_asm.inc holds the emitted text of every new macro.
"""
import importlib.util
import os

import numpy as np
import pytest

from asm_emu import Wave, WAVE
from test_dense40_rhs_row_cpu import ldl_right_looking, _systems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_subst_asm", os.path.join(ROOT, "ad_mpc_amd", "csrc", "gen_subst_asm.py"))
gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)

N = 40
LP, LB = 0, 8 * 1000           # byte addresses: packed rows of H, the right-hand-side buffer [40]; everything else reads as NaN
HALVES = ((0, N // 2), (N // 2, N))
LANE = np.arange(WAVE)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _wave(H, yb):
    w = Wave()
    for i in range(N):
        for j in range(i + 1):
            w.lds[LP + 8 * (i * (i + 1) // 2 + j)] = H[i, j]
    for j in range(N):
        w.lds[LB + 8 * j] = yb[j]
    return w


def _run_rows(w, lines_of, dbar, sodd):
    row = np.full((WAVE, N), np.nan)
    for lo, hi in HALVES:
        cnt = hi - lo
        ops = ["v[%d:%d]" % (2 * q, 2 * q + 1) for q in range(cnt)] + ["v200", "v[202:203]", "v[204:205]"]
        for q in range(cnt):
            w.v[2 * q] = np.full(WAVE, np.nan)                          # no presets: stale registers
        w.v[200] = np.where(LANE < N, LP + 8 * (LANE * (LANE + 1) // 2), np.where(LANE == N, LB, LP))      # lanes 41..63 parked on row 0
        w.v[202] = dbar.copy(); w.v[204] = sodd.copy()
        w.run(lines_of(lo, hi), ops)
        for q in range(cnt):
            row[:, lo + q] = w.v[2 * q]
    assert w.exec.all()
    return row


# (diag = "none" is the form of a caller whose s_odd is 0.0 in every lane: it has no s_odd adds to run with a non-zero one)
@pytest.mark.parametrize("diag,sodd_zero", [("all", True), ("all", False), ("odd", True), ("odd", False), ("none", True)],
                         ids=["registers-sodd0", "registers-sodd", "lds_even-sodd0", "lds_even-sodd", "lds_all-sodd0"])
def test_unmasked_row_build_against_the_masked_one(diag, sodd_zero):
    rng = np.random.default_rng(7)
    H = rng.normal(size=(N, N)); H = H + H.T
    yb = rng.normal(size=N)
    dbar = rng.normal(size=WAVE)                                          # also on lanes >= 40: it must not reach lane 40
    sodd = np.zeros(WAVE)
    if not sodd_zero:
        sodd = np.where(LANE < N, rng.normal(size=WAVE), 0.0)
        if diag == "odd":
            sodd[0:N:2] = 0.0                                           # the contract of the LDS rewrite: even lanes carry no s_odd
    want = _run_rows(_wave(H, yb), lambda lo, hi: gen.rowbuild(N, lo, hi, N + 1), dbar, sodd)
    w = _wave(H, yb)
    rewritten = [i for i in range(N) if diag == "none" or (diag == "odd" and i % 2 == 0)]
    for i in rewritten:                                                  # what dense40_factorise does in front of the row reads
        a = LP + 8 * (i * (i + 1) // 2 + i)
        w.lds[a] = float(np.float64(w.lds[a]) + np.float64(dbar[i]))
    got = _run_rows(w, lambda lo, hi: gen.rowpull(N, lo, hi, sodd=(diag != "none"), diag=diag), dbar, sodd)
    text = [l for lo, hi in HALVES for l in gen.rowpull(N, lo, hi, sodd=(diag != "none"), diag=diag)]
    assert not any(l.startswith("v_mov") for l in text)                  # no presets
    assert sum(l.startswith("ds_read_b64") for l in text) == N
    assert sum(l.startswith("s_bfm_b64") for l in text) == {"all": N, "odd": N // 2, "none": 0}[diag]      # only the diagonal adds are masked
    for parity in (0, 1):                                                # even and odd lanes apart
        for i in range(parity, N, 2):
            assert np.array_equal(_bits(got[i, :i + 1]), _bits(want[i, :i + 1])), (diag, "lane", i)
    assert np.array_equal(_bits(got[N]), _bits(want[N])) and np.array_equal(got[N], yb)      # the right-hand-side row: its whole buffer
    assert np.isfinite(got[:N + 1][np.tril_indices(N + 1, 0, N)]).all()


def test_symmetric_row_without_presets():
    rng = np.random.default_rng(12)
    H = rng.normal(size=(N, N)); H = H + H.T
    rows = []
    for preset in (True, False):
        w = _wave(H, np.zeros(N))
        row = np.full((WAVE, N), np.nan)
        for lo, hi in HALVES:
            cnt = hi - lo
            ops = ["v[%d:%d]" % (2 * q, 2 * q + 1) for q in range(cnt)] + ["v200", "v201"]
            for q in range(cnt):
                w.v[2 * q] = np.full(WAVE, np.nan)
            w.v[200] = np.where(LANE < N, LP + 8 * (LANE * (LANE + 1) // 2), LP)
            w.v[201] = np.where(LANE < N, LP + 8 * LANE, LP)
            lines = gen.symrow(N, lo, hi, preset=preset)
            assert any(l.startswith("v_mov_b64") for l in lines) == preset
            w.run(lines, ops)
            for q in range(cnt):
                row[:, lo + q] = w.v[2 * q]
        assert w.exec.all()
        rows.append(row)
    assert np.array_equal(_bits(rows[0][:N]), _bits(rows[1][:N])) and np.array_equal(rows[1][:N], H)
    assert (rows[0][N:] == 0.0).all() and np.isnan(rows[1][N:]).all()    # lanes >= 40: zeros with presets, stale registers without
    assert gen.symrow(N, 0, N // 2) == gen.symrow(N, 0, N // 2, preset=True)


def _ldl_64_lanes(a):
    """ldl_right_looking of test_dense40_rhs_row_cpu.py on all 64 lanes of a wave, from the registers as a row build left them
    (a [64][40]): every rank-1 update on EVERY lane, the pivot of column j from lane j, the factor column from lanes j + 1 .. 40."""
    a = a.copy()
    L = np.zeros((N, N)); d = np.zeros(N); w = np.zeros(N)
    for j in range(N):
        d[j] = a[j, j]
        dinv = 1.0 / d[j]
        lu = a[:, j] * dinv
        L[j + 1:, j] = lu[j + 1:N]
        w[j] = lu[N]
        nl = -lu
        for jj in range(j + 1, N):
            a[:, jj] = a[:, jj] + a[jj, j] * nl
    return L, d, w


def test_factorisation_never_reads_what_the_unmasked_build_leaves_undefined():
    for k, M, y in list(_systems())[::6]:
        clean = np.zeros((WAVE, N)); clean[:N] = np.tril(M); clean[N] = y
        dirty = np.full((WAVE, N), np.nan); dirty[:N][np.tril_indices(N)] = M[np.tril_indices(N)]; dirty[N] = y
        assert np.isnan(dirty[:N][np.triu_indices(N, 1)]).all() and np.isnan(dirty[N + 1:]).all()
        with np.errstate(invalid="ignore"):
            L0, d0, w0 = _ldl_64_lanes(clean)
            L1, d1, w1 = _ldl_64_lanes(dirty)
        Lm, dm, wm = ldl_right_looking(M, y)                             # the 64-lane restatement is the pinned model
        for a, b, c, what in ((L0, L1, Lm, "L"), (1.0 / d0, 1.0 / d1, 1.0 / dm, "invd"), (w0, w1, wm, "right-hand-side row")):
            assert np.array_equal(_bits(a), _bits(c)), "system %d: %s, 64-lane model against the imported one" % (k, what)
            assert np.array_equal(_bits(a), _bits(b)), "system %d: %s changes with NaN in the undefined entries" % (k, what)


def _max0_ignoring_nan(x):
    m = 0.0                                                              # the DPP reduction's identity (OpMax0, bound_ctrl zeros)
    for v in x:
        m = np.fmax(m, v)
    return m


def test_vote_equals_the_max_reduction_compared_with_its_tolerance():
    rng = np.random.default_rng(5)
    for tol in (1e-8, 1e-6, 0.0, 1e300, -1.0):
        up, dn = np.nextafter(tol, np.inf), np.nextafter(tol, -np.inf)
        pools = [[0.0], [0.0, tol], [0.0, dn, tol], [0.0, tol, up], [0.0, np.nan], [np.nan], [np.nan, tol], [np.nan, up], [1e300], [0.0, 1e300, np.nan],
                 [0.0, 1e-12, 1e-9, np.nan], [tol, np.nan, 0.0], [np.inf, 0.0], [np.nan, np.inf]]
        for pool in pools:
            for _ in range(8):
                x = rng.choice(np.array(pool), size=WAVE)
                x[N:] = 0.0                                              # the idle lanes vote with 0.0 (1e300 in all 64 lanes: next case)
                assert bool(np.all(~(x > tol))) == bool(_max0_ignoring_nan(x) <= tol), (tol, x)
        x = np.full(WAVE, 1e300)                                         # the first iteration's step, every lane
        assert bool(np.all(~(x > tol))) == bool(_max0_ignoring_nan(x) <= tol)


def _scan(v, steps):
    """wave_scan_incl<OpSum> (steps = 6) / wave_scan_incl32 (5) on 64 lanes: row_shr:1,2,4,8 with zeros shifted in, row_bcast:15 into rows
    1 and 3, row_bcast:31 into rows 2 and 3."""
    v = v.copy()
    for sh in (1, 2, 4, 8):
        src = np.zeros(WAVE)
        for l in range(WAVE):
            if (l & 15) >= sh:
                src[l] = v[l - sh]
        v = v + src
    src = np.zeros(WAVE)
    for l in range(WAVE):
        if (l >> 4) in (1, 3):
            src[l] = v[(l & ~15) - 1]
    v = v + src
    if steps == 6:
        src = np.zeros(WAVE)
        src[32:] = v[31]
        v = v + src
    return v


def test_five_step_scan_on_operands_that_end_at_lane_20():
    rng = np.random.default_rng(6)
    for rep in range(20):
        v = np.zeros(WAVE); v[:20] = rng.normal(size=20) * 10.0 ** rng.uniform(-6, 6, size=20)
        if rep % 4 == 0:
            v[0] = 0.0                                                   # stage 0 carries no steering bound
        s6, s5 = _scan(v, 6), _scan(v, 5)
        assert np.array_equal(_bits(s6[:32]), _bits(s5[:32]))
        assert _bits(s6[63:]) == _bits(s5[31:32])                        # the total: lane 63 of the six-step scan, lane 31 of the five-step one
        ref = np.cumsum(v)
        assert np.abs(s5[:32] - ref[:32]).max() <= 1e-9 * np.abs(v).max()


def test_generated_include_holds_the_new_macros():
    txt = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "subst_asm.inc")).read()
    for half, (lo, hi) in zip("AB", HALVES):
        assert gen.emit("ADMPC_ROWPULL_ASM_%d_%s_I" % (N, half), gen.rowpull(N, lo, hi, True, "odd")) in txt
        assert gen.emit("ADMPC_ROWPULL_ASM_%d_%s_T" % (N, half), gen.rowpull(N, lo, hi, False, "none")) in txt
        assert gen.emit("ADMPC_SYMROW_ASM_%d_%s_NP" % (N, half), gen.symrow(N, lo, hi, preset=False)) in txt
