"""The GP fit (csrc/gp_fit_dev.h: gp_points, gp_fit_body), the NLL of the search (csrc/gp_search_dev.h: gp_nll_body) and the ensemble's
kernels that run the same bodies by pointer (admpc_quad_hyper.hip), on the cases of tests/gp_fit_cases.py: every point count 0 .. 32,
the patterns at the edges of the compaction, statistics behind a smaller grid, every failure site, and hard kernel matrices.

tests/test_gp_fit_cases_cpu.py holds what these tests rely on, on the numpy spec alone.  The checks are those of the tests whose
helpers run here: test_learn_gpu._fit and _check_fit for the fit, test_hyper_gpu._search, _check_round, _device_exp and _refit for the
search, the sentinels of test_quad_hyper_gpu for the ensemble.  What a case must give -- its points, n, info -- comes from the table.

Measured on the MI355X, the worst over the cases (the float64 spec's own figure from the CPU test in brackets): the residual over its
bound 3.6e-3 on the sweep and the patterns (3.6e-3) and 3.0e-4 on the hard matrices (3.3e-4); max |alpha - alpha_longdouble| over its
bound 1.8e-2 (1.8e-2); the NLL error over its bound 1.8e-2, the largest |dNLL| 1.3e-12; the mean within 4.4 yardsticks where it is held.
DESIGN.md has the table and the mean gaps that are recorded only.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import gp_fit_cases as GC
import hyper_spec as HS
import learn_spec as LS
import test_gp_fit_cases_cpu as TC
import test_hyper_gpu as TH
import test_lane_gpu as TL
import test_learn_gpu as TG
import test_quad_hyper_gpu as TQ

pytestmark = pytest.mark.gpu

_bits = TL._bits
HEALTHY = GC.BY_NAME["sweep1-n17"]                     # the live regressor that shares a launch with failing ones
SENT_HY = TQ.SENT_HY


def _launch(cases):
    """(obs, stats [4,32,5], min_count) of up to four cases as the regressors of one call."""
    assert 1 <= len(cases) <= 4 and len({c.min_count for c in cases}) == 1
    obs = TG._obs([GC.learn(c.reg, 3 + g % 3) for g, c in enumerate(cases)])
    stats = np.zeros((4, 32, 5))
    for g, c in enumerate(cases):
        stats[g] = c.stats
    return obs, stats, cases[0].min_count


@functools.lru_cache(maxsize=None)
def _fitted(names, zeroed=False):
    """admpc_gp_fit of the named cases in one call, once per module: (obs, stats, min_count, records, info)."""
    cases = [GC.BY_NAME[k] for k in names]
    obs, stats, m = _launch(cases)
    if zeroed:
        for g, c in enumerate(cases):
            stats[g] = c.zeroed
    gps, info = TG._fit(TL._lib(), obs, stats, m)
    return obs, stats, m, gps, info


def _names(chunk):
    return tuple(c.name for c in chunk)


def _with_healthy(dead):
    """Launches of three failing cases and the healthy one, which takes another slot in each."""
    out = []
    for i in range(0, len(dead), 3):
        chunk = list(dead[i:i + 3])
        chunk.insert((i // 3) % (len(chunk) + 1), HEALTHY)
        out.append(chunk)
    return out


def _head(G, gp, what):
    """The head of a record under the given regressor, bit for bit; returns (Z [32,3], alpha [32])."""
    nf = int(G.n_feat)
    assert gp.n_feat == nf and gp.out == G.out and [gp.feat[d] for d in range(3)] == [G.feat[d] if d < nf else 0 for d in range(3)], what
    assert gp.sigma_f == G.sigma_f, what
    _bits(np.array([gp.inv_l2[d] for d in range(3)]), np.concatenate([LS.inv_l2(G), np.zeros(3 - nf)]), what + ": inv_l2")
    return np.array([[gp.Z[d][i] for d in range(3)] for i in range(32)]), np.array([gp.alpha[i] for i in range(32)])


def _is_empty(G, gp, what):
    Z, alpha = _head(G, gp, what)
    assert gp.n_points == 0 and gp.ymean == 0.0 and not Z.any() and not alpha.any() and LS.install_ok(gp), what


def _points_are_the_tables(gp, case, what):
    """Z of the record is sum z / count of the rows the table names, in their order."""
    nf = len(case.reg["bins"])
    Z = np.array([[gp.Z[d][i] for d in range(nf)] for i in range(case.n)], dtype=np.float64).reshape(case.n, nf)
    want = case.stats[case.rows]
    _bits(Z, (want[:, 1:1 + nf] / want[:, 0:1]).reshape(case.n, nf), what + ": the points are the table's rows")


# ---- 1. the fit: every point count, every pattern ---------------------------------------------------------------------------------------

SWEEP1 = [c for c in GC.of_kind("sweep") if len(c.reg["bins"]) == 1]
SWEEP3 = [c for c in GC.of_kind("sweep") if len(c.reg["bins"]) == 3]
EASY = dict(sweep1=SWEEP1, sweep3=SWEEP3, pattern=GC.of_kind("pattern"))


@pytest.mark.parametrize("family", list(EASY))
def test_the_fit_on_every_point_count_and_pattern(family):
    """Four regressors a call through test_learn_gpu._check_fit as it stands: info, n_points, Z, ymean and inv_l2 bit for bit, the
    residual under its bound, the mean within ten yardsticks, zeros past n, the buffer 0x5A before the call.  info and the points are
    the table's."""
    for chunk in GC.chunks(EASY[family]):
        obs, stats, m, gps, info = _fitted(_names(chunk))
        for g, c in enumerate(chunk):
            assert info[g] == c.info == c.n and gps[g].n_points == c.n, (c.name, info[g], c.info)
            _points_are_the_tables(gps[g], c, c.name)
            TG._check_fit(obs.gp[g], gps[g], info[g], stats[g], m, c.name)


def test_statistics_past_the_product_of_bins_are_not_read_by_the_fit():
    """A grid of 8 bins ([8] and [4, 2, 1]) whose rows 8 .. 31 hold statistics a larger grid left behind: the record equals, byte for
    byte, the fit of the same statistics with those rows zeroed."""
    stale = [c for c in GC.CASES if c.zeroed is not None]
    assert len(stale) == 6
    for chunk in GC.chunks(stale):
        _, stats, _, gps, info = _fitted(_names(chunk))
        _, clean, _, want, winfo = _fitted(_names(chunk), zeroed=True)
        assert stats[:len(chunk), 8:, 0].all() and not clean[:, 8:].any()
        for g, c in enumerate(chunk):
            assert info[g] == winfo[g] == c.n and bytes(gps[g]) == bytes(want[g]), c.name


# ---- 2. the fit: failure sites ----------------------------------------------------------------------------------------------------------

def test_the_fit_fails_at_every_site_with_the_specs_info_and_the_empty_gp():
    """The twin at step 1, 16 and 31 of 32; a +inf and a NaN target at point 0, 8 and 16 of 17; a NaN feature sum at the first and the
    last point; sigma_f + noise = +inf.  info is the table's and the spec's, the record the empty GP under the given head, and the
    healthy regressor of the same launch is fitted as if alone."""
    dead = GC.of_kind("failure")
    assert len(dead) == 12
    alone = _fitted((HEALTHY.name,))
    for chunk in _with_healthy(dead):
        obs, stats, m, gps, info = _fitted(_names(chunk))
        for g, c in enumerate(chunk):
            G = obs.gp[g]
            want = LS.fit(G, stats[g], m)
            assert info[g] == c.info == want["info"], (c.name, info[g], c.info, want["info"])
            if c is HEALTHY:
                TG._check_fit(G, gps[g], info[g], stats[g], m, "%s next to %s" % (c.name, _names(chunk)))
                a, b = gps[g], alone[3][0]
                assert a.ymean == b.ymean and a.alpha[:] == b.alpha[:] and [list(r) for r in a.Z] == [list(r) for r in b.Z], "the healthy regressor is undisturbed"
            else:
                assert c.info < 0
                _is_empty(G, gps[g], c.name)


# ---- 3. the fit: hard kernel matrices ---------------------------------------------------------------------------------------------------

FIGURES = {}


def test_the_fit_on_hard_kernel_matrices():
    """32 points each; cond2(K) from 1 to 3.2e9.  Head, Z and ymean bit for bit; the residual under the bound of _check_fit, which does not
    depend on conditioning; max |alpha - alpha_longdouble| <= 64 cond2(K) eps max |alpha_longdouble|, the form of
    test_learn_cpu.test_the_specs_fit_solves_what_numpy_solves.  The float64 spec meets both within a tenth (the CPU test).  The gap of
    the mean over the 200 probes of _check_fit is held to ten yardsticks where the yardstick is below the ceiling of 1e-11, and printed
    where it is not."""
    hard = GC.of_kind("hard")
    for chunk in GC.chunks(hard):
        obs, stats, m, gps, info = _fitted(_names(chunk))
        for g, c in enumerate(chunk):
            G = obs.gp[g]
            want = LS.fit(G, stats[g], m)
            Z, alpha = _head(G, gps[g], c.name)
            nf = int(G.n_feat)
            assert info[g] == c.info == 32 and gps[g].n_points == 32, (c.name, info[g])
            _bits(Z[:, :nf], want["Z"], c.name + ": Z"); _bits(np.float64(gps[g].ymean), np.float64(want["ymean"]), c.name + ": ymean")
            assert not Z[:, nf:].any()
            res, gap, cond = TC.fit_figures(G, c, alpha)
            probes = TC.probes_of(G, 32)
            yard = LS.yardstick(G, stats[g], probes, m)
            mean = float(np.abs(LS.gp_mean(G, dict(Z=Z[:, :nf], alpha=alpha, ymean=gps[g].ymean), probes) - LS.gp_mean(G, want, probes)).max())
            held = yard < 1e-11
            print("%s: cond2(K) %.3g, residual over its bound %.3g, |alpha - alpha_ld| over its bound %.3g, mean gap %.3g (yardstick %.3g, %s)"
                  % (c.name, cond, res, gap, mean, yard, "held to ten" if held else "recorded only"))
            FIGURES[c.name] = (res, gap, mean, yard)
            assert np.isfinite(alpha).all() and res <= 1.0 and gap <= 1.0, (c.name, res, gap)
            assert not held or mean <= 10.0 * yard, (c.name, mean, yard)
    print("worst over the hard cases: residual %.3g, alpha %.3g of their bounds" % (max(f[0] for f in FIGURES.values()), max(f[1] for f in FIGURES.values())))


# ---- 4. the re-fit ----------------------------------------------------------------------------------------------------------------------

def _given(obs):
    """hyper [4,16] with the natural values of the regressors as given."""
    hy = np.zeros((4, 16))
    for g in range(4):
        G = obs.gp[g]
        hy[g, 10:15] = [G.length[d] if d < G.n_feat else 1.0 for d in range(3)] + [G.sigma_f, G.noise]
        with np.errstate(divide="ignore"):
            hy[g, 0:5], hy[g, 5:10] = np.log(hy[g, 10:15]), 0.125
    return hy


@pytest.mark.parametrize("kinds", [("sweep",), ("pattern", "failure", "hard")])
def test_the_refit_at_the_given_values_is_the_fit_byte_for_byte(kinds):
    """admpc_gp_refit at hyper[10 .. 14] = the given values against admpc_gp_fit, on every case: records and info."""
    lib = TL._lib()
    launches = GC.chunks(GC.of_kind(*[k for k in kinds if k != "failure"]))
    if "failure" in kinds:
        launches += _with_healthy(GC.of_kind("failure"))
    for chunk in launches:
        obs, stats, m, want, winfo = _fitted(_names(chunk))
        hy = _given(obs)
        got, ginfo = TH._refit(lib, obs, stats, hy, m)
        assert ginfo.tolist() == winfo.tolist() == [c.info for c in chunk], _names(chunk)
        for g, c in enumerate(chunk):
            assert bytes(got[g]) == bytes(want[g]), c.name


def test_the_refit_without_an_optimum_gives_the_empty_gp_at_every_point_count():
    """hyper[15] +inf, NaN or -inf: ADMPC_GP_NO_OPTIMUM and the empty GP under the given head, whatever n; a regressor of the same launch
    whose hyper[15] is finite is fitted."""
    lib = TL._lib()
    for i, chunk in enumerate(GC.chunks(SWEEP1 + SWEEP3)):
        obs, stats, m, want, winfo = _fitted(_names(chunk))
        for keep in (None, i % len(chunk)):                                       # nobody, then one regressor, keeps a finite best
            hy = _given(obs)
            for g in range(len(chunk)):
                if g != keep:
                    hy[g, 15] = (np.inf, np.nan, -np.inf)[(i + g) % 3]
            got, ginfo = TH._refit(lib, obs, stats, hy, m)
            for g, c in enumerate(chunk):
                if g == keep:
                    assert ginfo[g] == c.n and bytes(got[g]) == bytes(want[g]), c.name
                else:
                    assert ginfo[g] == HS.NO_OPTIMUM, (c.name, ginfo[g])
                    _is_empty(obs.gp[g], got[g], c.name)


# ---- 5. the NLL -------------------------------------------------------------------------------------------------------------------------

def _round_inputs(cases, boxes=None):
    """(obs, sp, stats, min_count, start states, (free, loglo, loghi) per regressor) of one round of up to four cases."""
    obs, stats, m = _launch(cases)
    gps = [GC.learn(c.reg, 3 + g % 3) for g, c in enumerate(cases)]
    sp = TH._params(gps, boxes or [c.box for c in cases], grid=5, shrink=0.5)
    starts = [HS.init_state(list(sp.box[g].lo), list(sp.box[g].hi), int(obs.gp[g].n_feat), 5) for g in range(len(cases))]
    frees = [HS.box_logs(list(sp.box[g].lo), list(sp.box[g].hi), int(obs.gp[g].n_feat)) for g in range(len(cases))]
    return obs, sp, stats, m, starts, frees


_EXPS = {}


def _exps(lib, starts, frees):
    """The device's exp of every theta of these rounds; a value is asked for once per module."""
    need = np.unique(np.concatenate([HS.thetas(s, *f, 5).reshape(-1) for s, f in zip(starts, frees)]))
    new = [t for t in need.tolist() if t not in _EXPS]
    if new:
        _EXPS.update(TH._device_exp(lib, new))
    return _EXPS


def _one_round(lib, cases, boxes=None, stats=None):
    obs, sp, own, m, starts, frees = _round_inputs(cases, boxes)
    stats = own if stats is None else stats
    up = np.full((4, 16), SENT_HY)
    up[:len(cases)] = np.stack(starts)
    hy, nll, info = TH._search(lib, obs, sp, stats, up, min_count=m, resume=1)
    _bits(hy[len(cases):], up[len(cases):], "the state past n_gp is not touched")
    assert (nll[len(cases):] == 7.0).all() and (info[len(cases):] == -9).all()
    return obs, sp, stats, m, starts, frees, (hy, nll, info)


@pytest.mark.parametrize("family", list(EASY))
def test_one_round_of_the_nll_on_every_point_count_and_pattern(family):
    """resume = 1 from the start state, 25 candidates (grid 5, sigma_f fixed; two of three length scales fixed too), every case through
    test_hyper_gpu._check_round, not exempt; the sentinel 7.0 past C is checked there.  No candidate is left out: the CPU test holds that
    float64 and longdouble agree on all of them."""
    lib = TL._lib()
    for chunk in GC.chunks(EASY[family]):
        obs, sp, stats, m, starts, frees, (hy, nll, info) = _one_round(lib, chunk)
        exps = _exps(lib, starts, frees)
        for g, c in enumerate(chunk):
            TH._check_round(obs.gp[g], stats[g], sp.box[g], 5, 0.5, starts[g], exps, (hy[g], nll[g], info[g]), c.name, False, m)
            assert info[g, 1] == 25 and np.isfinite(nll[g, :25]).all(), (c.name, info[g])
            if c.n == 0:
                assert (nll[g, :25] == 0.0).all() and info[g, 0] == 0


def test_statistics_past_the_product_of_bins_are_not_read_by_the_nll():
    lib = TL._lib()
    stale = [c for c in GC.CASES if c.zeroed is not None]
    for chunk in GC.chunks(stale):
        clean = np.zeros((4, 32, 5))
        for g, c in enumerate(chunk):
            clean[g] = c.zeroed
        got, want = _one_round(lib, chunk)[6], _one_round(lib, chunk, stats=clean)[6]
        for a, b, what in zip(got, want, ("hyper", "nll", "search_info")):
            _bits(a, b, "%s: %s of the round on the zeroed statistics" % (_names(chunk), what))


def test_every_failure_site_kills_every_candidate_and_no_other_regressor():
    """Each failing case under a box that keeps K exact (length scale 1e-4 .. 1e-3, sigma_f 1, noise 1e-300 .. 1e-200; the overflow under
    its own sigma_f and noise): every candidate +inf, search_info [-1, 0], the centre kept, the step shrunk, the best still +inf.  The
    healthy regressor of the same launch matches its spec."""
    lib = TL._lib()
    for chunk in _with_healthy(GC.of_kind("failure")):
        obs, sp, stats, m, starts, frees, (hy, nll, info) = _one_round(lib, chunk)
        exps = _exps(lib, starts, frees)
        for g, c in enumerate(chunk):
            what = "%s in %s" % (c.name, _names(chunk))
            if c is HEALTHY:
                TH._check_round(obs.gp[g], stats[g], sp.box[g], 5, 0.5, starts[g], exps, (hy[g], nll[g], info[g]), what, False, m)
                assert info[g, 1] == 25
                continue
            Cn = 5 if c.name == "overflowing-pivot" else 25
            th = HS.thetas(starts[g], *frees[g], 5)
            V = np.array([[exps[t] for t in row] for row in th.tolist()])
            assert len(th) == Cn and np.isposinf(HS.nll(obs.gp[g], stats[g], m, V)[0]).all(), what + ": the spec fails everywhere"
            assert np.isposinf(nll[g, :Cn]).all() and (nll[g, Cn:] == 7.0).all() and info[g].tolist() == [-1, 0], (what, info[g])
            _bits(hy[g, 0:5], starts[g][0:5], what + ": the centre is kept"); _bits(hy[g, 5:10], starts[g][5:10] * 0.5, what + ": the step is shrunk")
            _bits(hy[g, 10:16], starts[g][10:16], what + ": the natural values and the best are kept")


def test_the_twin_under_a_free_noise_has_finite_and_failing_halves_in_one_wave():
    """Noise free in [1e-300, 1e-2]: the candidates with noise 1e-2 (c = 4 mod 5) are finite, the others +inf; candidates 4 and 5 are the
    halves of one wave.  Through _check_round, not exempt, nothing left out."""
    lib = TL._lib()
    chunk = [GC.BY_NAME["twin-at-01"], GC.BY_NAME["twin-at-16"], HEALTHY, GC.BY_NAME["twin-at-31"]]
    boxes = [GC.TWIN_FREE if c is not HEALTHY else c.box for c in chunk]
    obs, sp, stats, m, starts, frees, (hy, nll, info) = _one_round(lib, chunk, boxes)
    exps = _exps(lib, starts, frees)
    for g, c in enumerate(chunk):
        TH._check_round(obs.gp[g], stats[g], sp.box[g], 5, 0.5, starts[g], exps, (hy[g], nll[g], info[g]), c.name + ", noise free", False, m)
        if c is not HEALTHY:
            assert np.isfinite(nll[g, :25]).tolist() == [k % 5 == 4 for k in range(25)] and np.isposinf(nll[g, :25][~np.isfinite(nll[g, :25])]).all()
            assert info[g, 1] == 5 and info[g, 0] % 5 == 4


# ---- 6. the ensemble's kernels, which run the same bodies by pointer --------------------------------------------------------------------

def test_the_ensemble_chain_equals_a_single_call_per_cluster_on_these_cases():
    """K = 8, n_gp = 3 as test_quad_hyper_gpu._ensemble builds its fleet: the 24 regressors carry n = 0, 1, 2, 3, 15, 16, 17, 31, 32, the
    patterns with the rows past a smaller grid filled, and three failure sites.  One chain of admpc_quad_ensemble_search (resume 0, two
    rounds) and admpc_quad_ensemble_refit against admpc_quad_gp_search and admpc_quad_gp_refit of each cluster alone: hyper, nll up to C,
    search_info, the records and their info bit for bit; sentinels past C and in the statistics.  No tolerance."""
    import torch
    from ad_mpc_amd.config import AdmpcGp, AdmpcGpSearchParams
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    K, n_gp, size, m = 8, 3, C.sizeof(AdmpcGp), 4
    table = [[GC.BY_NAME[k] for k in names] for names in GC.ENSEMBLE]
    learn = [[dict(c.reg, feat=GC.ENSEMBLE_FEAT[g], out=7 + g) for g, c in enumerate(row)] for row in table]
    fl = QuadEnsembleFleet(4, quad=SimQuad(drag=True), n_nodes=10, centroids=np.linspace(-3.0, 3.0, K).reshape(K, 1), feats=[7], learn=learn)
    L = fl.lib
    _host, _dev, _p = TQ._host, TQ._dev, TQ._p
    try:
        stats = np.stack([np.stack([c.stats for c in row]) for row in table])
        sp = (AdmpcGpSearchParams * K)()
        for c in range(K):
            sp[c] = TQ._params(fl._learn[c], [case.box for case in table[c]], rounds=2)
        assert L.admpc_quad_ensemble_set_search(fl._ens, sp) == 0, L.admpc_last_error()
        bins = _dev(stats)
        hy = torch.full((K, 3, 16), TQ.SENT_HY, dtype=torch.float64, device="cuda:0")
        nll = torch.full((K, 3, HS.SEARCH_MAX), TQ.SENT_NLL, dtype=torch.float64, device="cuda:0")
        info = torch.full((K, 3, 2), TQ.SENT_INFO, dtype=torch.int32, device="cuda:0")
        assert L.admpc_quad_ensemble_search(fl._ens, m, 0, _p(bins), _p(hy), _p(nll), _p(info), None) == 0, L.admpc_last_error()
        out = torch.full((K * 3 * size,), TQ.SENT_BYTE, dtype=torch.uint8, device="cuda:0")
        finfo = torch.full((K, 3), 77, dtype=torch.int32, device="cuda:0")
        assert L.admpc_quad_ensemble_refit(fl._ens, m, _p(bins), _p(hy), _p(out), _p(finfo), None) == 0, L.admpc_last_error()
        hy, nll, info, raw, finfo = _host(hy), _host(nll), _host(info), _host(out).tobytes(), _host(finfo)
        _bits(_host(bins), stats, "the statistics are read-only")
        for c in range(K):
            junk = np.full((3, 16), np.nan)
            w_hy, w_nll, w_info = TQ._search(L.admpc_quad_gp_search, fl._obs[c], sp[c], stats[c], junk, 3, min_count=m, resume=0)
            w_raw, w_finfo = TQ._refit(L.admpc_quad_gp_refit, fl._obs[c], stats[c], w_hy, 3, min_count=m)
            for g, case in enumerate(table[c]):
                what = "cluster %d, regressor %d (%s)" % (c, g, case.name)
                _bits(hy[c, g], w_hy[g], what + ": hyper")
                _bits(nll[c, g, :25], w_nll[g, :25], what + ": nll up to C")
                assert (nll[c, g, 25:] == TQ.SENT_NLL).all() and (w_nll[g, 25:] == TQ.SENT_NLL).all(), what + ": nothing past C"
                _bits(info[c, g], w_info[g], what + ": search_info")
                assert raw[(c * 3 + g) * size:(c * 3 + g + 1) * size] == w_raw[g * size:(g + 1) * size], what + ": the record of the re-fit"
                assert finfo[c, g] == w_finfo[g], what
                # what the table says of the case, so that the two sides cannot be wrong together
                rec = AdmpcGp.from_buffer_copy(raw, (c * 3 + g) * size)
                if case.info < 0:
                    assert np.isposinf(nll[c, g, :25]).all() and info[c, g].tolist() == [-1, 0] and hy[c, g, 15] == np.inf and finfo[c, g] == HS.NO_OPTIMUM, what
                    assert rec.n_points == 0 and rec.ymean == 0.0 and not any(rec.alpha[:]), what
                else:
                    assert finfo[c, g] == case.n == rec.n_points and info[c, g, 1] == 25 and np.isfinite(hy[c, g, 15]), (what, finfo[c, g], case.n)
                    _points_are_the_tables(rec, case, what)
        assert sorted(case.n for row in table for case in row[:2] if case.kind == "sweep") == [0, 1, 2, 3, 15, 16, 17, 31, 32]
        assert sum(case.zeroed is not None for row in table for case in row) == 4 and sum(case.info < 0 for row in table for case in row) == 3
    finally:
        fl.close()
