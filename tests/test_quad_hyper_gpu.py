"""The search of the quadrotor's GP hyperparameters on the device (include/admpc_quad_hyper.h; ad_mpc_amd/learning.py, quad_fleet.py:
search_gp, learned_hyper; quad_ensemble_fleet.py: the same for all clusters at once).

Nothing here needs a tolerance but the experiment: the routed single-handle entries are the car's kernels, so they are held against
admpc_gp_search and admpc_gp_refit bit for bit (tests/test_hyper_gpu.py holds those against the numpy spec); the ensemble's kernels run the
same bodies by pointer, so cluster c, regressor g of one chain of launches is held against admpc_quad_gp_search of that cluster alone,
bit for bit, with sentinels around everything a launch must not write.  Then resume, set_search again and a captured graph, the Python
surface of both fleets by the solve of a fresh handle, the learning experiment with a wrong length scale, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import hyper_spec as HS
import learn_spec as LS
import quad_learn_spec as QL
import test_quad_fleet_gpu as TQ
import test_quad_learn_gpu as TL

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _lib = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._lib
BOX = dict(length_scale=(1e-2, 1e2), sigma_f=(1e-3, 1e2), noise=(1e-8, 1.0))         # the box of the searches (tests 5 to 7), the car's
ROUND = dict(length_scale=(1e-2, 1e2), sigma_f=(0.25, 4.0), noise=(0.04, 1.0))       # the box of the rounds of tests/test_hyper_gpu.py
FIXED = dict(length_scale=(1.5, 1.5), sigma_f=(0.8, 0.8), noise=(0.05, 0.05))
SENT_NLL, SENT_INFO, SENT_HY, SENT_BYTE = 7.0, -9, 3.25, 0x5A
VX = lambda lo, hi, **kw: dict(dict(feat=7, out=7, lo=[lo], hi=[hi], bins=[32], length_scale=2.0, noise=1e-4, count_noise=1e-2), **kw)


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def quad_oracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


def _params(gps, bounds, grid=5, rounds=1, shrink=0.5):
    from ad_mpc_amd.config import AdmpcGpSearchParams, search_boxes
    return AdmpcGpSearchParams(grid=grid, rounds=rounds, shrink=shrink, box=search_boxes(gps, bounds))


def _search(entry, obs, sp, stats, hyper, rows, min_count=1, resume=1):
    """A single-handle search entry on uploaded statistics and state, `rows` regressors wide: (hyper, nll, search_info) afterwards."""
    import torch
    bins, hy = _dev(np.ascontiguousarray(stats[:rows])), _dev(np.ascontiguousarray(np.asarray(hyper, dtype=np.float64)[:rows]))
    nll = torch.full((rows, HS.SEARCH_MAX), SENT_NLL, dtype=torch.float64, device="cuda:0")
    info = torch.full((rows, 2), SENT_INFO, dtype=torch.int32, device="cuda:0")
    rc = entry(0, C.byref(obs), C.byref(sp), min_count, resume, _p(bins), _p(hy), _p(nll), _p(info), None)
    assert rc == 0, _lib().admpc_last_error()
    got = _host(hy), _host(nll), _host(info)
    _bits(_host(bins), np.ascontiguousarray(stats[:rows]), "the statistics are read-only")
    return got


def _refit(entry, obs, stats, hyper, rows, min_count=1):
    import torch
    from ad_mpc_amd.config import AdmpcGp
    bins, hy = _dev(np.ascontiguousarray(stats[:rows])), _dev(np.ascontiguousarray(hyper[:rows]))
    out = torch.full((rows * C.sizeof(AdmpcGp),), SENT_BYTE, dtype=torch.uint8, device="cuda:0")
    info = torch.full((rows,), 77, dtype=torch.int32, device="cuda:0")
    assert entry(0, C.byref(obs), min_count, _p(bins), _p(hy), _p(out), _p(info), None) == 0, _lib().admpc_last_error()
    return _host(out).tobytes(), _host(info)


def _late(st, box, best):
    """test_hyper_gpu._late: a state late in a search whose upper candidates are clamped onto the box's upper end."""
    free, loglo, loghi = box
    late = st.copy()
    late[0:5] = st[0:5] + np.where(free, 0.425 * (loghi - loglo), 0.0)
    late[5:10], late[15] = np.where(free, 0.15 * (loghi - loglo), 0.0), best
    late[10:15] = np.exp(late[0:5])
    return late


# ---- 1. the routed entries are the car's ----------------------------------------------------------------------------------------------

def test_the_routed_entries_equal_the_cars_bit_for_bit():
    """n_gp = 3, 8 / 20 / 32 bins filled, C = 125 / 625 / 3125: one round from the start of a search and one from a late, clamped state
    through admpc_quad_gp_search (feat 7, [7, 8], [7, 8, 9]; out 7, 8, 9) and through admpc_gp_search (feat 3, [3, 4], [3, 4, 5]; out 3, 4,
    5) with equal n_feat, nb, box and statistics: hyper, nll and search_info bit for bit; the re-fits byte for byte but feat and out."""
    from ad_mpc_amd.config import AdmpcGp, AdmpcObserveParams, learn_bins
    L = _lib()
    quad = [dict(feat=7, out=7, lo=[-4.0], hi=[4.0], bins=[8], length_scale=2.0),
            dict(feat=[7, 8], out=8, lo=[-4.0, -1.5], hi=[4.0, 1.5], bins=[8, 4], length_scale=[2.0, 1.0], noise=1e-4),
            dict(feat=[7, 8, 9], out=9, lo=[-6.0, 0.0, 0.0], hi=[6.0, 1.0, 1.0], bins=[4, 2, 4], length_scale=[3.0, 0.5, 0.5], noise=1e-4, count_noise=0.01)]
    car = [dict(d, feat=[f - 4 for f in np.atleast_1d(d["feat"])], out=d["out"] - 4) for d in quad]
    qobs = TL._obs(quad)
    cbins, n = learn_bins(car)
    cobs = AdmpcObserveParams(dt=TL.DT, blend_min=3.0, blend_max=5.0, substeps=1, n_gp=n, gp=cbins)
    qsp, csp = _params(quad, [ROUND] * 3), _params(car, [ROUND] * 3)
    assert bytes(qsp) == bytes(csp)
    rng = np.random.default_rng(41)
    stats = np.zeros((4, 32, 5))
    for g, fill in enumerate((8, 20, 32)):
        stats[g] = LS.hand_stats(qobs.gp[g], rng, fill)
    starts = [HS.init_state(list(qsp.box[g].lo), list(qsp.box[g].hi), int(qobs.gp[g].n_feat), 5) for g in range(3)]
    boxes = [HS.box_logs(list(qsp.box[g].lo), list(qsp.box[g].hi), int(qobs.gp[g].n_feat)) for g in range(3)]
    for label, sts in (("start", starts), ("late", [_late(s, b, np.inf) for s, b in zip(starts, boxes)])):
        up = np.full((4, 16), SENT_HY)
        up[:3] = np.stack(sts)
        q = _search(L.admpc_quad_gp_search, qobs, qsp, stats, up, 3)
        c = _search(L.admpc_gp_search, cobs, csp, stats, up, 4)
        for a, b, what in zip(q, c, ("hyper", "nll", "search_info")):
            _bits(a, b[:3], "%s, %s: the quadrotor's entry against the car's" % (label, what))
        assert [int(np.isfinite(q[1][g, :Cg]).sum()) for g, Cg in enumerate((125, 625, 3125))] == q[2][:, 1].tolist() and (q[2][:, 0] >= 0).all()
        assert all((q[1][g, Cg:] == SENT_NLL).all() for g, Cg in enumerate((125, 625, 3125)))
        if label == "late":
            assert any(np.unique(q[1][g, :Cg]).size < Cg for g, Cg in enumerate((125, 625, 3125)))      # clamped candidates coincide
        qr, qi = _refit(L.admpc_quad_gp_refit, qobs, stats, q[0], 3)
        cr, ci = _refit(L.admpc_gp_refit, cobs, stats, c[0], 4)
        _bits(qi, ci[:3], "%s: info of the re-fits" % label)
        assert qi.tolist() == [8, 20, 32]
        for g in range(3):
            a, b = (AdmpcGp.from_buffer_copy(raw, g * C.sizeof(AdmpcGp)) for raw in (qr, cr))
            nf = int(qobs.gp[g].n_feat)
            assert [a.feat[d] for d in range(3)] == [7 + d if d < nf else 0 for d in range(3)] and a.out == 7 + g
            assert [b.feat[d] for d in range(3)] == [3 + d if d < nf else 0 for d in range(3)] and b.out == 3 + g
            for r in (a, b):
                r.feat[0] = r.feat[1] = r.feat[2] = r.out = 0
            assert bytes(a) == bytes(b), "%s, regressor %d: the record of the quadrotor's re-fit is the car's but for feat and out" % (label, g)


# ---- 2. one chain of launches for all clusters ----------------------------------------------------------------------------------------

# the boxes of a cluster's three regressors, by the cluster's index: C = 125 / 625 / 3125, 1 / 125 / 125, 25 / 125 / 625
PATTERNS = ([ROUND, ROUND, ROUND],
            [FIXED, dict(ROUND, noise=(0.1, 0.1)), dict(ROUND, sigma_f=(0.7, 0.7), noise=(0.1, 0.1))],
            [dict(ROUND, sigma_f=(0.7, 0.7)), dict(ROUND, length_scale=[(2.0, 2.0), (0.1, 10.0)]), dict(ROUND, noise=(0.1, 0.1))])
COUNTS = ([125, 625, 3125], [1, 125, 125], [25, 125, 625])


def _ensemble(K, n_gp, B=4):
    """A fleet that learns K clusters of n_gp regressors whose boxes, bins and given values differ per cluster."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    learn = [([VX(-4.0 + 0.5 * c, 4.0 + 0.5 * c, length_scale=1.0 + c)] + [dict(TL.THREE[1], noise=1e-4 * (c + 1)), dict(TL.THREE[2])])[:n_gp] for c in range(K)]
    cent = np.linspace(-3.0, 3.0, K).reshape(K, 1) if K > 1 else np.zeros((1, 1))
    return QuadEnsembleFleet(B, quad=SimQuad(drag=True), n_nodes=10, centroids=cent, feats=[7], learn=learn)


def _ensemble_stats(fl, seed, empty=None, nan=None):
    """Hand-made statistics [K,3,32,5]: regressor 0 with 31 (even clusters) or 32 (odd clusters) of its 32 bins filled, 20 and 27 for the
    others; cluster `empty` without a sample; (c, g) = `nan` with one target that is not a number."""
    rng = np.random.default_rng(seed)
    stats = np.zeros((fl.K, 3, 32, 5))
    for c in range(fl.K):
        for g in range(fl.n_learn):
            stats[c, g] = LS.hand_stats(fl._obs[c].gp[g], rng, (31 + c % 2, 20, 27)[g])
    if empty is not None:
        stats[empty] = 0.0
    if nan is not None:
        stats[nan[0], nan[1], np.flatnonzero(stats[nan[0], nan[1], :, 0])[3], 4] = np.nan
    return stats


@pytest.mark.parametrize("K,n_gp", [(2, 3), (2, 2), (8, 3)])
def test_the_ensemble_search_equals_a_single_call_per_cluster_bit_for_bit(K, n_gp):
    """resume = 0, two rounds, all K * n_gp regressors in one chain (K = 8: 24 regressors, which no longer fit the kernel arguments)
    against admpc_quad_gp_search of bins[c] under block c and box c; then the re-fit against admpc_quad_gp_refit.  C takes the values 1,
    25, 125, 625 and 3125 within one launch; at K = 8 the last cluster holds no sample (n = 0: every NLL 0, candidate 0 picked, then
    none); regressor 1 of cluster 0 has a NaN target: every candidate +inf, none picked, ADMPC_GP_NO_OPTIMUM and the empty GP at the
    re-fit, there alone; regressor 0 has 31 points in the even clusters and 32 in the odd.
    Sentinels: nothing is written past C, past n_gp, or into bins."""
    import torch
    from ad_mpc_amd.config import AdmpcGp, AdmpcGpSearchParams
    fl = _ensemble(K, n_gp)
    L, size = fl.lib, C.sizeof(AdmpcGp)
    try:
        last = K - 1 if K > 2 else None
        stats = _ensemble_stats(fl, 5 + K, empty=last, nan=(0, 1))
        sp = (AdmpcGpSearchParams * K)()
        for c in range(K):
            sp[c] = _params(fl._learn[c], PATTERNS[c % 3][:n_gp], rounds=2)
        assert L.admpc_quad_ensemble_set_search(fl._ens, sp) == 0, L.admpc_last_error()
        bins = _dev(stats)
        hy = torch.full((K, 3, 16), SENT_HY, dtype=torch.float64, device="cuda:0")
        nll = torch.full((K, 3, HS.SEARCH_MAX), SENT_NLL, dtype=torch.float64, device="cuda:0")
        info = torch.full((K, 3, 2), SENT_INFO, dtype=torch.int32, device="cuda:0")
        assert L.admpc_quad_ensemble_search(fl._ens, 1, 0, _p(bins), _p(hy), _p(nll), _p(info), None) == 0, L.admpc_last_error()
        out = torch.full((K * 3 * size,), SENT_BYTE, dtype=torch.uint8, device="cuda:0")
        finfo = torch.full((K, 3), 77, dtype=torch.int32, device="cuda:0")
        assert L.admpc_quad_ensemble_refit(fl._ens, 1, _p(bins), _p(hy), _p(out), _p(finfo), None) == 0, L.admpc_last_error()
        hy, nll, info, raw, finfo = _host(hy), _host(nll), _host(info), _host(out).tobytes(), _host(finfo)
        _bits(_host(bins), stats, "the statistics are read-only")
        seen = set()
        for c in range(K):
            junk = np.full((3, 16), np.nan)
            w_hy, w_nll, w_info = _search(L.admpc_quad_gp_search, fl._obs[c], sp[c], stats[c], junk, 3, resume=0)
            w_raw, w_finfo = _refit(L.admpc_quad_gp_refit, fl._obs[c], stats[c], w_hy, 3)
            for g in range(3):
                what = "K = %d, cluster %d, regressor %d" % (K, c, g)
                if g >= n_gp:                                                                    # past n_gp: nothing is written
                    assert (hy[c, g] == SENT_HY).all() and (nll[c, g] == SENT_NLL).all() and (info[c, g] == SENT_INFO).all(), what
                    assert finfo[c, g] == 77 and raw[(c * 3 + g) * size:(c * 3 + g + 1) * size] == bytes([SENT_BYTE]) * size, what
                    continue
                Cg = COUNTS[c % 3][g]
                seen.add(Cg)
                _bits(hy[c, g], w_hy[g], what + ": hyper")
                _bits(nll[c, g, :Cg], w_nll[g, :Cg], what + ": nll up to C")
                assert (nll[c, g, Cg:] == SENT_NLL).all() and (w_nll[g, Cg:] == SENT_NLL).all(), what + ": nothing past C"
                _bits(info[c, g], w_info[g], what + ": search_info")
                assert raw[(c * 3 + g) * size:(c * 3 + g + 1) * size] == w_raw[g * size:(g + 1) * size], what + ": the record of the re-fit"
                assert finfo[c, g] == w_finfo[g], what
        assert seen >= ({1, 125, 625, 3125} if n_gp == 3 else {1, 125, 625})
        points = [[int((stats[c, g, :, 0] > 0).sum()) for g in range(n_gp)] for c in range(K)]
        assert points[0][0] == 31 and points[1][0] == 32 and (last is None or points[last] == [0] * n_gp)
        # the NaN target: +inf everywhere, nothing picked in either round, no optimum at the re-fit -- in that regressor alone
        assert (nll[0, 1, :COUNTS[0][1]] == np.inf).all() and info[0, 1].tolist() == [-1, 0] and hy[0, 1, 15] == np.inf
        want = np.array(points)
        want[0, 1] = HS.NO_OPTIMUM
        assert finfo[:, :n_gp].tolist() == want.tolist()
        e = AdmpcGp.from_buffer_copy(raw, size)
        assert (e.n_points, e.ymean, e.n_feat, e.out) == (0, 0.0, 2, 8) and QL.install_ok(e) and not any(e.alpha[:])
        # the cluster without a sample: every NLL 0, all finite; candidate 0 picked in the first round, none in the second
        for g in range(n_gp if last is not None else 0):
            Cg = COUNTS[last % 3][g]
            assert (nll[last, g, :Cg] == 0.0).all() and info[last, g].tolist() == [-1, Cg] and hy[last, g, 15] == 0.0
        assert np.isfinite(hy[:, :n_gp, 15]).sum() == K * n_gp - 1
    finally:
        fl.close()


# ---- 3. resume ------------------------------------------------------------------------------------------------------------------------

def test_four_rounds_equal_one_round_and_three_resumed():
    """K = 3: search_gp(rounds=4) against search_gp(rounds=1) and three calls with resume=True, bit for bit in hyper, search_info, the
    re-fitted records and their info."""
    fl = _ensemble(3, 3)
    try:
        fl.bins.copy_(_dev(_ensemble_stats(fl, 9)))
        bounds = [PATTERNS[c] for c in range(3)]
        fl.search_gp(rounds=4, bounds=bounds, install=False)
        whole = {k: _host(getattr(fl, k)).copy() for k in ("hyper", "search_info", "_gp_dev", "fit_info")}
        fl.hyper.fill_(np.nan)
        fl.search_gp(rounds=1, bounds=bounds, install=False)
        first = _host(fl.hyper).copy()
        for _ in range(3):
            fl.search_gp(rounds=1, bounds=bounds, resume=True, install=False)
        for k, v in whole.items():
            _bits(_host(getattr(fl, k)), v, k + ": 1 + 3 calls against one")
        assert np.isfinite(whole["hyper"]).all() and not np.array_equal(first[:, :, 0:5], whole["hyper"][:, :, 0:5])      # the later rounds moved on
        assert (whole["hyper"][:, :, 5:10] <= first[:, :, 5:10]).all() and (whole["fit_info"] > 0).all()
    finally:
        fl.close()


# ---- 4. set_search again, and a captured graph ----------------------------------------------------------------------------------------

def test_a_captured_search_follows_new_boxes_and_new_bins_at_replay():
    """K = 2.  search_gp under boxes A captured after one eager run (the second call with the same parameters does not call set_search,
    which synchronises); then admpc_quad_ensemble_set_search with boxes B, whose length scales exclude A's, other bins, a replay: hyper,
    the records, the install's flags and the counts equal those of an eager fleet under B on the same bins bit for bit.  The eager
    fleet itself searched under A first: its second set_search is followed by the next search."""
    import torch
    fls = [_ensemble(2, 3) for _ in range(2)]
    eager, graphed = fls
    A = [[dict(BOX, length_scale=(1e-2, 1.0))] * 3] * 2
    Bb = [[dict(BOX, length_scale=(2.0, 1e2))] * 3, [dict(BOX, length_scale=(3.0, 50.0))] * 3]
    try:
        first, second = _ensemble_stats(graphed, 1), _ensemble_stats(graphed, 2)
        graphed.bins.copy_(_dev(first))
        graphed.search_gp(rounds=3, bounds=A)                                      # every kernel has run once before the capture
        torch.cuda.synchronize()
        before = _host(graphed.hyper).copy()
        assert (before[:, :, 10] <= 1.0).all()
        held = graphed._search_set
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.search_gp(rounds=3, bounds=A)
        assert graphed._search_set == held                                         # no set_search inside the capture
        eager.bins.copy_(_dev(second))
        eager.search_gp(rounds=3, bounds=A)
        under_a = _host(eager.hyper).copy()
        info, installed, _ = eager.search_gp(rounds=3, bounds=Bb)                 # set_search again: the next search follows it
        torch.cuda.synchronize()
        assert graphed.lib.admpc_quad_ensemble_set_search(graphed._ens, graphed_params(graphed, Bb, 3)) == 0, graphed.lib.admpc_last_error()
        graphed.bins.copy_(_dev(second))
        g.replay()
        torch.cuda.synchronize()
        for k in ("hyper", "_gp_dev", "installed", "fit_info", "search_info"):
            _bits(_host(getattr(graphed, k)), _host(getattr(eager, k)), k + " after the replay")
        hy = _host(graphed.hyper)
        assert (hy[0, :, 10] >= 2.0).all() and (hy[1, :, 10] >= 3.0).all() and (under_a[:, :, 10] <= 1.0).all()      # the new boxes, per cluster
        assert (_host(installed) == 1).all() and _host(info)[:, 0].tolist() == [31, 32]
    finally:
        for fl in fls:
            fl.close()


def graphed_params(fl, bounds, rounds):
    from ad_mpc_amd.config import AdmpcGpSearchParams
    sp = (AdmpcGpSearchParams * fl.K)()
    for c in range(fl.K):
        sp[c] = _params(fl._learn[c], bounds[c], rounds=rounds)
    return sp


# ---- 5. the Python surface: a searched GP solves as a handle created with it ----------------------------------------------------------

def test_a_searched_gp_solves_as_a_handle_created_with_it():
    """N = 10, B = 5: QuadFleet.search_gp on hand-made bins installs what a fresh QuadBatchSolver created from learned_gps() solves with;
    learned_hyper() is hyper[:, 10:16]; a later fit_gp reports the given values again."""
    from ad_mpc_amd.config import AdmpcGp
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import SimQuad, set_quad_gp
    from ad_mpc_amd.quad_fleet import QuadFleet
    from ad_mpc_amd.quad_scenarios import random_quad_scenarios
    N, B = 10, 5
    fl = QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, learn=TL.THREE)
    fresh = None
    try:
        s = random_quad_scenarios(B, fl.cfg, seed=N)
        base = TL._solve(fl._eng, s)
        assert [h["nll"] for h in fl.learned_hyper()] == [np.inf] * 3 and fl.learned_hyper()[1]["length_scale"] == [2.0, 1.0]
        rng = np.random.default_rng(N)
        stats = np.zeros((3, 32, 5))
        for g, fill in enumerate((12, 20, 27)):
            stats[g] = LS.hand_stats(fl._obs.gp[g], rng, fill)
        fl.bins.copy_(_dev(stats))
        info, installed, hyper = fl.search_gp(rounds=4, bounds=[BOX] * 3)
        got = TL._solve(fl._eng, s)
        assert _host(info).tolist() == [12, 20, 27] and _host(installed).tolist() == [1, 1, 1] and tuple(hyper.shape) == (3, 16)
        hy = _host(hyper)
        gps, found = fl.learned_gps(), fl.learned_hyper()
        raw = _host(fl._gp_dev).tobytes()
        for g in range(3):
            rec = AdmpcGp.from_buffer_copy(raw, g * C.sizeof(AdmpcGp))
            nf = rec.n_feat
            assert list(gps[g]["length_scale"]) == found[g]["length_scale"] == hy[g, 10:10 + nf].tolist() and gps[g]["sigma_f"] == hy[g, 13] == rec.sigma_f
            assert [found[g]["sigma_f"], found[g]["noise"], found[g]["nll"]] == hy[g, 13:16].tolist() and np.isfinite(hy[g, 15])
            assert [1.0 / l ** 2 for l in gps[g]["length_scale"]] == [rec.inv_l2[d] for d in range(nf)]      # set_quad_gp forms what was installed
        fresh = QuadBatchSolver(set_quad_gp(fl._eng.cfg.copy(), gps), device=0)
        want = TL._solve(fresh, s)
        for a, b, what in zip(got, want, ("x", "u", "cost", "status", "iters")):
            _bits(a, b, "%s of the handle after search_gp against the fresh one" % what)
        assert np.nanmax(np.abs(got[1] - base[1])) > 1e-6                          # not the placeholder
        info, installed = fl.fit_gp()                                              # a fit_gp afterwards: the given values again
        assert [g["length_scale"] for g in fl.learned_gps()] == [d["length_scale"] for d in TL.THREE] and _host(info).tolist() == [12, 20, 27]
    finally:
        fl.close()
        if fresh is not None:
            fresh.close()


def test_a_searched_ensemble_solves_as_an_ensemble_created_with_it():
    """The same per cluster, K = 2, through solve_routed: the fleet after search_gp against QuadEnsembleFleet(ensemble=learned_gps())."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    from ad_mpc_amd.quad_scenarios import random_quad_scenarios
    B = 5
    fl, fresh = _ensemble(2, 3, B=B), None
    try:
        s = random_quad_scenarios(B, fl.cfg, seed=2)
        route = _dev((np.arange(B) % 2).astype(np.int32))

        def solve(f):
            for t, k in ((f.x, "x0"), (f.yref, "yref"), (f.yref_e, "yref_e"), (f.x_opt, "xbar"), (f.w_opt, "ubar")):
                t.copy_(_dev(s[k]))
            f.solve_routed(route)
            return [_host(t).copy() for t in (f.x_opt, f.w_opt, f.cost, f.status, f.iters)]

        base = solve(fl)
        given = fl.learned_hyper()
        assert [[h["nll"] for h in cl] for cl in given] == [[np.inf] * 3] * 2 and [cl[0]["length_scale"] for cl in given] == [[1.0], [2.0]]
        fl.bins.copy_(_dev(_ensemble_stats(fl, 4)))
        info, installed, hyper = fl.search_gp(rounds=4, bounds=[[BOX] * 3, [dict(BOX, length_scale=(0.5, 20.0))] * 3])
        assert _host(info).tolist() == [[31, 20, 27], [32, 20, 27]] and (_host(installed) == 1).all() and tuple(hyper.shape) == (2, 3, 16)
        got, hy = solve(fl), _host(hyper)
        learned, found = fl.learned_gps(), fl.learned_hyper()
        for c in range(2):
            for g in range(3):
                nf = int(fl._obs[c].gp[g].n_feat)
                assert list(learned.clusters[c][g]["length_scale"]) == found[c][g]["length_scale"] == hy[c, g, 10:10 + nf].tolist()
                assert [found[c][g]["sigma_f"], found[c][g]["noise"], found[c][g]["nll"]] == hy[c, g, 13:16].tolist() and np.isfinite(hy[c, g, 15])
                assert learned.clusters[c][g]["sigma_f"] == hy[c, g, 13]
        assert (hy[1, :, 10] >= 0.5).all() and (hy[1, :, 10] <= 20.0).all()         # cluster 1 under its own box
        fresh = QuadEnsembleFleet(B, quad=SimQuad(drag=True), n_nodes=10, ensemble=learned)
        want = solve(fresh)
        for a, b, what in zip(got, want, ("x", "u", "cost", "status", "iters")):
            _bits(a, b, "%s of the fleet after search_gp against the fleet created with what it learned" % what)
        assert np.nanmax(np.abs(got[1] - base[1])) > 1e-6
        fl.fit_gp()                                                                # a fit_gp afterwards: the given values again
        assert [[g["length_scale"] for g in cl] for cl in fl.learned_gps().clusters] == [[d["length_scale"] for d in cl] for cl in fl._learn]
    finally:
        fl.close()
        if fresh is not None:
            fresh.close()


# ---- 6. the experiment on the device --------------------------------------------------------------------------------------------------

def test_the_search_mends_a_wrong_length_scale_on_the_device(quad_oracle):
    """The loop of test_quad_learn_gpu.test_the_learning_experiment_on_the_device with every length scale given as 0.3: the held-out
    ratios RMS(y_after) / RMS(y_before) per axis after fit_gp, and after search_gp on the same bins.  The device's final NLL per
    regressor lies within hyper_spec.gaps of the spec's at the device's own values; a regressor whose every pick the spec's gap rule
    forces has the spec's centre and steps bit for bit, and where that holds for all three the ratios are the spec's to 1e-6 (the rules
    of the car's test); searched < given per axis in any case.  The ratios are printed.  Measured on the MI355X: given 0.168801 /
    0.142839 / 0.303258, searched 0.0105533 / 0.0158449 / 0.120125 (found length scales 3.619 / 6.321 / 6.208); every pick of every
    axis forced, the NLLs within 1e-10 of the spec's."""
    from ad_mpc_amd.config import search_boxes
    from ad_mpc_amd.quad_config import SimQuad, set_quad_gp
    from ad_mpc_amd.quad_fleet import QuadFleet
    learn = [dict(d, length_scale=0.3) for d in QL.EXP_LEARN]
    fl = QuadFleet(QL.EXP_B, quad=SimQuad(drag=True), n_nodes=10, learn=learn)
    try:
        trans, S = {}, {}
        X, U = QL.experiment_inputs("before")
        u = _dev(U)
        fl.x.copy_(_dev(X))
        fl.observe_latch(); fl.plant_step(u); fl.observe(u)
        trans["before"] = (X, U, _host(fl.x))
        bins = fl.bins.clone()
        info, installed = fl.fit_gp(min_count=QL.EXP_MIN_COUNT)
        points = _host(info).tolist()
        assert min(points) >= 20 and _host(installed).tolist() == [1, 1, 1]
        X, U = QL.experiment_inputs("after")
        u = _dev(U)
        fl.x.copy_(_dev(X))
        fl.observe_latch(); fl.plant_step(u); fl.observe(u)
        trans["after"] = (X, U, _host(fl.x))
        S["nominal"] = _host(fl.samples)

        def learned():
            fl._prev.copy_(_dev(X))
            fl.set_observer(learned=True)
            fl.observe(u)
            out = _host(fl.samples)
            assert (out[:, 13] == 1.0).all()
            return QL.rms(out) / QL.rms(S["nominal"])

        given = learned()
        fl.bins.copy_(bins)                                                        # the statistics of the first set alone
        info, installed, hyper = fl.search_gp(min_count=QL.EXP_MIN_COUNT, bounds=[BOX] * 3)
        searched = learned()
        assert _host(info).tolist() == points and _host(installed).tolist() == [1, 1, 1]
        hy, stats = _host(hyper), _host(bins)
        exp = QL.experiment(quad_oracle, transitions=trans)
        box = search_boxes(learn, [BOX] * 3)
        every, found = [], []
        for g in range(3):
            G = fl._obs.gp[g]
            v64, size = HS.nll(G, stats[g], QL.EXP_MIN_COUNT, hy[g, 10:15])
            vld, _ = HS.nll(G, stats[g], QL.EXP_MIN_COUNT, hy[g, 10:15], np.longdouble)
            bound = HS.gaps(v64.astype(np.float64), size.astype(np.float64), vld, points[g])[0]
            # the spec's own search on the spec's statistics, and whether the gap rule forces every pick of it
            free, loglo, loghi = HS.box_logs(list(box[g].lo), list(box[g].hi), 1)
            st, forced = HS.init_state(list(box[g].lo), list(box[g].hi), 1, 5), True
            for _ in range(10):
                th = HS.thetas(st, free, loglo, loghi, 5)
                V = HS.natural(th)
                a64, asize = HS.nll(G, exp["bins"][g], QL.EXP_MIN_COUNT, V)
                ald, _ = HS.nll(G, exp["bins"][g], QL.EXP_MIN_COUNT, V, np.longdouble)
                a64 = a64.astype(np.float64)
                forced = forced and HS.forced(a64, HS.gaps(a64, asize.astype(np.float64), ald, points[g]))[1]
                st, _, _ = HS.pick(st, th, V, a64, 0.5)
            print("axis %d: ratio on the device given %.6g, searched %.6g (length %.6g, sigma_f %.6g, noise %.6g); NLL %.12g, the spec's there %.12g "
                  "(bound %.3g); every pick forced: %s" % (g, given[g], searched[g], hy[g, 10], hy[g, 13], hy[g, 14], hy[g, 15], v64[0], bound, forced))
            assert abs(hy[g, 15] - float(v64[0])) <= bound, g
            if forced:
                _bits(hy[g, 0:10], st[0:10], "axis %d: the centre and the steps of the spec's search" % g)
            every.append(forced)
            found.append(HS.with_hyper(G, st[10:15]))
        assert (searched < given).all(), (searched, given)
        if all(every):
            nominal, plant, obs = QL.experiment_params()
            model = set_quad_gp(nominal.copy(), [QL.as_set_gp(H, LS.fit(H, exp["bins"][g], QL.EXP_MIN_COUNT)) for g, H in enumerate(found)])
            a = exp["after"]
            Sw = np.stack([QL.record(quad_oracle, model, plant, obs, a["X"][b], a["now"][b], a["U"][b])[0] for b in range(QL.EXP_B)])
            want = QL.rms(Sw) / exp["before_rms"]
            print("ratios by the spec %s" % np.array2string(want, precision=9))
            assert (np.abs(searched - want) <= 1e-6 * want).all(), (searched, want)
    finally:
        fl.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------

def test_argument_errors():
    """The Python refusals of both fleets, and the refusals of the ensemble entries that need a live ensemble, in their order."""
    import torch
    from ad_mpc_amd._lib import AdmpcError
    from ad_mpc_amd.config import AdmpcGpSearchParams
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    from ad_mpc_amd.quad_fleet import QuadFleet, QuadLearningFleet
    # a QuadFleet that does not learn is a plain QuadFleet, which has no search at all; one that learns is created as a QuadLearningFleet;
    # a QuadLearningFleet created without learn refuses as the car's controller does
    nosearch, fl = QuadFleet(4, quad=SimQuad(drag=True), n_nodes=10), QuadFleet(4, quad=SimQuad(drag=True), n_nodes=10, learn=TL.THREE)
    plain = QuadLearningFleet(4, quad=SimQuad(drag=True), n_nodes=10)
    assert type(nosearch) is QuadFleet and type(fl) is QuadLearningFleet and isinstance(fl, QuadFleet)
    assert not hasattr(nosearch, "search_gp") and not hasattr(nosearch, "learned_hyper")
    flies = QuadEnsembleFleet(4, quad=SimQuad(drag=True), n_nodes=10, ensemble=QuadGPEnsemble([[], []], [[-1.0], [1.0]], [7]))
    ens = _ensemble(2, 3)
    try:
        # the C entries behind a live ensemble
        L = ens.lib
        buf = torch.full((2, 3, 16), SENT_HY, dtype=torch.float64, device="cuda:0")
        idx = torch.full((2, 3, 2), SENT_INFO, dtype=torch.int32, device="cuda:0")

        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        ok = graphed_params(ens, [[{}] * 3] * 2, 2)
        for e in (flies._ens,):                                                    # created without observe parameters: in front of everything else
            refused(L.admpc_quad_ensemble_set_search(e, None), "admpc_quad_ensemble_set_search: the ensemble was created without observe parameters")
            refused(L.admpc_quad_ensemble_search(e, 0, 2, None, None, None, None, None), "admpc_quad_ensemble_search: the ensemble was created without")
            refused(L.admpc_quad_ensemble_refit(e, 0, None, None, None, None, None), "admpc_quad_ensemble_refit: the ensemble was created without")
        refused(L.admpc_quad_ensemble_search(ens._ens, 0, 2, None, None, None, None, None), "no search parameters yet")      # in front of min_count
        refused(L.admpc_quad_ensemble_set_search(ens._ens, None), "the search parameters are not set")
        bad = graphed_params(ens, [[{}] * 3] * 2, 2)
        bad[0].rounds, bad[1].grid = 3, 4                                          # cluster 1's grid in front of the blocks that differ
        refused(L.admpc_quad_ensemble_set_search(ens._ens, bad), "grid must be 3, 5, 7 or 9")
        bad[1].grid = 5
        bad[1].box[2].lo[4] = 0.0                                                  # cluster 1's box in front of the blocks that differ
        refused(L.admpc_quad_ensemble_set_search(ens._ens, bad), "regressor 2: slot 4 of the box")
        bad[0].grid, bad[0].box[0].hi[3] = 7, -1.0                                 # the clusters in their order
        refused(L.admpc_quad_ensemble_set_search(ens._ens, bad), "regressor 0: slot 3 of the box")
        for field, value in (("grid", 3), ("rounds", 3), ("shrink", 0.25)):
            bad = graphed_params(ens, [[{}] * 3] * 2, 2)
            setattr(bad[1], field, value)
            refused(L.admpc_quad_ensemble_set_search(ens._ens, bad), "must share grid, rounds and shrink")
        refused(L.admpc_quad_ensemble_search(ens._ens, 1, 0, _p(buf), _p(buf), _p(buf), _p(idx), None), "no search parameters yet")      # every refused set_search left it so
        assert L.admpc_quad_ensemble_set_search(ens._ens, ok) == 0, L.admpc_last_error()
        args = dict(bins=_p(buf), hyper=_p(buf), nll=_p(buf), info=_p(idx))
        search = lambda min_count=1, resume=0, **kw: L.admpc_quad_ensemble_search(ens._ens, min_count, resume, *[dict(args, **kw)[k] for k in ("bins", "hyper", "nll", "info")], None)
        refused(search(min_count=0, resume=2, bins=None), "admpc_quad_ensemble_search: min_count must be at least 1")
        refused(search(resume=2, bins=None), "admpc_quad_ensemble_search: resume must be 0 or 1")
        for k in args:
            refused(search(**{k: None}), "admpc_quad_ensemble_search: null array")
        refit = lambda min_count=1, **kw: L.admpc_quad_ensemble_refit(ens._ens, min_count, *[dict(args, **kw)[k] for k in ("bins", "hyper", "nll", "info")], None)
        refused(refit(min_count=0, bins=None), "admpc_quad_ensemble_refit: min_count must be at least 1")
        for k in args:
            refused(refit(**{k: None}), "admpc_quad_ensemble_refit: null array")
        assert (_host(buf) == SENT_HY).all() and (_host(idx) == SENT_INFO).all()    # a refused call writes nothing
        for call in (lambda: plain.search_gp(), lambda: plain.learned_hyper(), lambda: flies.search_gp(), lambda: flies.learned_hyper()):
            with pytest.raises(ValueError, match="does not learn"):
                call()
        for f in (fl, ens):
            for kw, words in ((dict(grid=4), "grid must be"), (dict(grid=7), "16807 candidates"), (dict(shrink=1.0), "shrink must be"),
                              (dict(rounds=0), "rounds must be"), (dict(min_count=0), "min_count must be"), (dict(grid=6, shrink=2.0), "grid must be")):
                with pytest.raises(AdmpcError, match=words):
                    f.search_gp(**kw)
        for bounds in ([dict(sigma_f=(2.0, 1.0)), {}, {}], [{}, dict(length_scale=(0.0, 1.0)), {}], [{}]):
            with pytest.raises(ValueError, match="bound"):
                fl.search_gp(bounds=bounds)
        for bounds in ([[{}] * 3], [[{}] * 3] * 3, [[{}] * 3, {}], [[{}] * 2, [{}] * 3], [[{}] * 3, [dict(noise=(1.0, 0.5)), {}, {}]], [{}, {}]):
            with pytest.raises(ValueError, match="bound"):
                ens.search_gp(bounds=bounds)
        found = fl.learned_hyper()                                                 # no search yet: the given values
        assert found[0] == dict(length_scale=[2.0], sigma_f=fl._obs.gp[0].sigma_f, noise=fl._obs.gp[0].noise, nll=np.inf) and found[2]["length_scale"] == [3.0, 0.5, 0.5]
        assert not _host(fl.hyper).any() and not _host(ens.hyper).any() and [len(g["alpha"]) for g in fl.learned_gps()] == [0, 0, 0]
        fl.search_gp(grid=7, rounds=1, bounds=[{}, dict(noise=(1e-4, 1e-4)), dict(sigma_f=(1.0, 1.0), noise=(1e-4, 1e-4))])      # 7^3, 7^3 and 7^3 candidates pass
        assert np.isfinite(fl.learned_hyper()[0]["nll"])
    finally:
        for f in (nosearch, plain, fl, flies, ens):
            f.close()
