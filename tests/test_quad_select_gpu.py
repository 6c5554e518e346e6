"""The selection of the GP training points from the log on the device (include/admpc_quad_select.h; csrc/admpc_quad_select.hip;
QuadEnsembleFleet.select_points / selected_points) against the numpy spec, tests/quad_select_spec.py, which
tests/test_quad_select_cpu.py pins to the reference's distance_maximizing_points_1d.

The selection is a rule of decisions, so everything is held EXACTLY: ``sel`` and ``info`` integer for integer, the rows of ``bins``
bit for bit the records' own z and y.  Logs are written straight into the log tensor of a small fleet (B = 64, K = 1, 2, 3, one-feature
regressors on the body axes 7, 8, 9, the clusters on feature 10 so that the route of a record does not depend on what is selected);
no flight is needed but for the closing experiment."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import quad_learn_spec as QL
import quad_select_spec as SS
import test_quad_ensemble_gpu as TE
import test_quad_fleet_gpu as TQ

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _stream = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._stream
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 64, 1094                                    # 1094 * 64 = 70 016 records: more than 256 blocks of 256 threads
REGS = [(7, 7), (8, 9), (9, 8)]                        # (feature, output): the second and the third regressor cross their outputs
CENT = {1: [[0.0]], 2: [[-5.0], [5.0]], 3: [[-5.0], [0.0], [5.0]]}
ROUTE = 3                                              # the record's entry of the clustering feature 10
_FLEETS = {}


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module", autouse=True)
def _close_the_fleets():
    yield
    for fl in _FLEETS.values():
        fl.close()
    _FLEETS.clear()


def _learn(K, bins=(32, 32, 32)):
    return [[dict(QL.EXP_LEARN[g], feat=f, out=o, bins=[bins[g]]) for g, (f, o) in enumerate(REGS)] for _ in range(K)]


def _make(K, steps=STEPS, **kw):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    kw.setdefault("learn", _learn(K))
    return QuadEnsembleFleet(B, quad=SimQuad(drag=True), n_nodes=10, centroids=CENT[K], feats=[10], log_steps=steps, **kw)


def _fleet(K):
    """One fleet per K for the whole module: a selection leaves nothing behind that the next one reads."""
    if K not in _FLEETS:
        _FLEETS[K] = _make(K)
    return _FLEETS[K]


def _records(M, seed, route=None):
    """M valid records of normal data whose target follows the feature; ``route``: the clustering feature per record (default 0)."""
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(M, SS.REC))
    S[:, 10:13] = np.sin(S[:, [0, 2, 1]]) + 0.05 * S[:, 10:13]
    S[:, ROUTE] = 0.0 if route is None else route
    S[:, 13] = 1.0
    return S


def _load(fl, S):
    """S [M, 14] into the log, padded to whole steps with records that are not valid; returns the padded log [M', 14]."""
    steps = -(-S.shape[0] // B)
    full = np.full((steps * B, SS.REC), -7.5)
    full[:, 13] = 0.0
    full[:S.shape[0]] = S
    fl.log[:steps].copy_(_dev(full.reshape(steps, B, SS.REC)))
    fl.log_count = steps
    return full


def _select(fl, n_points):
    """select_points() over poisoned outputs: (bins, sel, info) on the host, the whole tensors."""
    fl.bins.fill_(7.0); fl.sel.fill_(7); fl.select_info.fill_(7)
    sel, info = fl.select_points(n_points)
    assert sel.shape == (fl.K, 3, 32) and info.shape == (fl.K, 3, 4)
    return _host(fl.bins).copy(), _host(fl.sel).copy(), _host(fl.select_info).copy()


def _check(fl, S, n_points, what):
    full = _load(fl, S)
    got = _select(fl, n_points)
    want = SS.select_log(full, CENT[fl.K], [10], REGS, np.broadcast_to(n_points, 3))
    _bits(got[1], want[1], what + ": sel"); _bits(got[2], want[2], what + ": info"); _bits(got[0], want[0], what + ": bins")
    return got, want, full


# ---- 1. every fixture of the reference's cases, as the data of cluster 0 ------------------------------------------------------------------------

with open(os.path.join(ROOT, "tests", "golden", "quad_select_vectors.json")) as _f:
    _GOLDEN = json.load(_f)["cases"]


@pytest.mark.parametrize("case", _GOLDEN, ids=["%s-%d-%d" % (c["kind"], c["N"], c["n_points"]) for c in _GOLDEN])
def test_fixtures_equal_the_spec_and_the_reference(case):
    N, n = case["N"], case["n_points"]
    S = _records(N, case["seed"])
    S[:, 0] = SS.values(case["kind"], N, case["seed"])
    got, want, _ = _check(_fleet(1), S, [n, 20, 32], "fixture")
    assert got[1][0, 0, :n].tolist() == case["index"]                              # the reference's own indices: the records are in log order
    assert got[2][0, 0, 1] == N and got[2][0, 0, 3] == 0


# ---- 2. clusters ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [2, 3])
def test_interleaved_clusters(K):
    M = 3000
    route = np.asarray(CENT[K]).ravel()[np.random.default_rng(K).integers(0, K, size=M)] + np.random.default_rng(9).uniform(-1.0, 1.0, size=M)
    got, want, _ = _check(_fleet(K), _records(M, 20 + K, route), [20, 7, 32], "interleaved")
    assert (want[2][:, :, 0] >= 5).all() and want[2][:, 0, 1].sum() == M and (want[2][:, :, 3] == 0).all()


def test_a_cluster_without_a_record_and_one_with_a_single_record():
    M = 1000
    route = np.full(M, -5.0)
    route[617] = 5.0                                                               # cluster 2 holds one record, cluster 1 none
    got, want, full = _check(_fleet(3), _records(M, 31, route), [20, 20, 20], "empty and single")
    assert want[2][1].tolist() == [[0, 0, 20, SS.ENOVALID]] * 3 and not got[0][1].any() and (got[1][1] == -1).all()
    # the single record: lo - 0.5 .. hi + 0.5 in 20 bins, the record on the middle edge as it is rounded: in bin 10, or in bin 9
    assert want[2][2].tolist() == [[1, 1, 19, 0]] * 3 and (got[1][2] >= 0).sum() == 3
    assert all(sorted(got[1][2, g, 9:11].tolist()) == [-1, 617] for g in range(3))
    assert got[0][2, 1, 0].tolist() == [1.0, full[617, 1], 0.0, 0.0, full[617, 12]]
    assert want[2][0, 0, 1] == M - 1 and want[2][0, 0, 0] >= 15


# ---- 3, 4. the pick by hand: bins of 1, 2, 3 and 4 members, the member set aside, the point equal to hi -----------------------------------------

def test_the_pick_by_hand():
    fl = _fleet(1)
    for z, n, sel in (([0.0, 1.5, 1.25, 2.5, 2.0, 2.75, 3.5, 3.25, 3.5, 3.0, 4.0], 4, [0, 1, 3, 6]),
                      ([0.0, 4.0, 3.25, 3.75, 3.5, 3.1, 3.9, 3.5], 4, [0, -1, -1, 4]),
                      ([0.0, 4.0, 3.5, 3.25, 3.75, 3.5], 4, [0, -1, -1, 2]),         # the member set aside equals the median; the lowest index wins
                      ([0.0, 4.0, 3.25, 3.5], 4, [0, -1, -1, 2]),
                      ([-1.0, -0.0, 0.0, 0.0, 1.0], 1, [1]),                         # -0.0 == 0.0, and the row holds the record's own -0.0
                      ([0.5, -1.25], 1, [1]), ([0.5, -1.25, 0.75], 2, [1, 0])):
        S = _records(len(z), 40)
        S[:, 0] = z
        got, want, full = _check(fl, S, [n, 1, 1], "by hand %s" % (z,))
        assert got[1][0, 0, :n].tolist() == sel and (got[1][0, 0, n:] == -1).all(), (z, got[1][0, 0, :n].tolist())
        hi = int(np.argmax(z))
        assert hi not in got[1][0, 0] and got[2][0, 0, 1] == len(z)                # the point equal to hi takes part and is in no bin
        rows = [i for i in sel if i >= 0]
        _bits(got[0][0, 0, :len(rows), 1], np.asarray(z, dtype=np.float64)[rows], "the records' own bits")


# ---- 5. records that do not take part ------------------------------------------------------------------------------------------------------------------

def test_flags_and_values_that_are_not_finite_are_skipped():
    M = 4001
    S = _records(M, 50)
    S[::5, 13], S[3::17, 13], S[7::29, 13] = 0.0, 2.0, np.nan
    S[11::31, 0], S[13::37, 10], S[2::41, 1], S[9::43, 12], S[23::47, 2] = np.nan, np.inf, -np.inf, np.nan, np.inf
    got, want, full = _check(_fleet(1), S, [32, 20, 7], "dirty")
    took = want[2][0, :, 1]
    assert len(set(took.tolist())) == 3 and (took < (S[:, 13] == 1.0).sum()).all()  # every regressor lost records of its own
    for g, (f, o) in enumerate(REGS):
        idx = got[1][0, g][got[1][0, g] >= 0]
        assert (full[idx, 13] == 1.0).all() and np.isfinite(full[idx, f - 7]).all() and np.isfinite(full[idx, 3 + o]).all()
        _bits(got[0][0, g, :idx.size, 1], full[idx, f - 7], "z at the log's positions"); _bits(got[0][0, g, :idx.size, 4], full[idx, 3 + o], "y")


# ---- 6. past the grid ----------------------------------------------------------------------------------------------------------------------------------

def test_a_log_past_the_grid_with_medians_decided_in_the_second_stride():
    M = STEPS * B
    assert M == 70016 > 256 * 256
    rng = np.random.default_rng(60)
    route = np.where(rng.integers(0, 4, size=M) == 0, 5.0, -5.0)
    S = _records(M, 61, route)
    # feature 8 of cluster 0 over [0, 10] in ten bins; bins 3, 5 and 7 hold records past index 65 536 alone
    z = rng.uniform(0.0, 10.0, size=M)
    early = np.arange(M) < 65536
    hole = early & np.isin(np.floor(z).astype(int), (3, 5, 7))
    z[hole] = z[hole] - 1.0
    mine = np.flatnonzero(route < 0)
    z[mine[0]], z[mine[1]] = 0.0, 10.0
    S[:, 1] = z
    got, want, full = _check(_fleet(2), S, [32, 10, 20], "70 016 records")
    late = got[1][0, 1, [3, 5, 7]]
    assert (late >= 65536).all() and (got[1][0, 1, :10] >= 0).all(), got[1][0, 1, :10]


# ---- 7. n_points per regressor -------------------------------------------------------------------------------------------------------------------------

def test_n_points_per_regressor_and_the_rows_behind_them():
    S = _records(2500, 70)
    fl = _fleet(1)
    for n in ([1, 2, 32], [32, 1, 7], 20):
        got, want, _ = _check(fl, S, n, "n_points %s" % (n,))
        for g, k in enumerate(np.broadcast_to(n, 3)):
            assert (got[1][0, g, k:] == -1).all() and not got[0][0, g, k:].any() and got[2][0, g, 0] + got[2][0, g, 2] == k
    full = _load(fl, S)
    got = _select(fl, None)                                                        # None: each regressor's nbins
    want = SS.select_log(full, CENT[1], [10], REGS, [32, 32, 32])
    _bits(got[1], want[1], "n_points None: sel"); _bits(got[2], want[2], "n_points None: info"); _bits(got[0], want[0], "n_points None: bins")
    pts = fl.selected_points()
    assert len(pts) == 1 and len(pts[0]) == 3
    for g, (f, o) in enumerate(REGS):
        p = pts[0][g]
        assert np.array_equal(p["index"], got[1][0, g][got[1][0, g] >= 0]) and np.array_equal(p["z"], S[p["index"], f - 7])
        assert np.array_equal(p["y"], S[p["index"], 3 + o]) and p["status"] == 0 and p["took_part"] == 2500 and p["empty"] == 32 - p["index"].size


# ---- 8. the same bits twice, and a captured chain under new centroids ---------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits_and_a_replay_follows_new_centroids():
    import torch
    fl = _make(3, steps=48)
    try:
        M = 48 * B
        route = np.random.default_rng(80).uniform(-8.0, 8.0, size=M)
        full = _load(fl, _records(M, 81, route))
        first = _select(fl, [20, 32, 7])
        work = _host(fl._select_work).copy()
        second = _select(fl, [20, 32, 7])
        for a, b, name in zip(first, second, ("bins", "sel", "info")):
            _bits(a, b, "the second run: " + name)
        _bits(_host(fl._select_work), work, "the second run: the work area")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fl.select_points([20, 32, 7])
        moved = [[-2.0], [1.0], [2.5]]
        fl.set_centroids(moved)
        fl.bins.fill_(7.0); fl.sel.fill_(7); fl.select_info.fill_(7)
        g.replay()
        got = (_host(fl.bins).copy(), _host(fl.sel).copy(), _host(fl.select_info).copy())
        want = SS.select_log(full, moved, [10], REGS, [20, 32, 7])
        _bits(got[1], want[1], "the replay: sel"); _bits(got[2], want[2], "the replay: info"); _bits(got[0], want[0], "the replay: bins")
        assert not np.array_equal(got[1], first[1]) and not np.array_equal(got[2][:, 0, 1], first[2][:, 0, 1])
    finally:
        fl.close()


# ---- 9. the fit reads the selected rows, and the re-bin restores the means -----------------------------------------------------------------------------

def test_fit_gp_fits_the_selected_rows_and_rebin_restores_the_bins():
    import torch
    from ad_mpc_amd.config import AdmpcGp
    fl = _make(2, steps=40)
    try:
        M = 40 * B
        route = np.random.default_rng(90).uniform(-8.0, 8.0, size=M)
        _load(fl, _records(M, 91, route))
        fl.rebin()
        parent, parent_dropped = _host(fl.bins).copy(), _host(fl.dropped).copy()
        assert parent[..., 0].max() > 1.0
        got = _select(fl, 20)
        info, installed = fl.fit_gp(min_count=1)
        assert _host(info).tolist() == got[2][:, :, 0].tolist() and (_host(info) >= 10).all() and (_host(installed) == 1).all()
        fitted = _host(fl._gp_dev).copy().reshape(2, 3, C.sizeof(AdmpcGp))
        out = torch.zeros(3 * C.sizeof(AdmpcGp), dtype=torch.uint8, device="cuda:0")
        oinfo = torch.zeros(3, dtype=torch.int32, device="cuda:0")
        for c in range(2):
            rows = _dev(got[0][c])
            rc = fl.lib.admpc_quad_gp_fit(0, C.byref(fl._obs[c]), 1, _p(rows), _p(out), _p(oinfo), _stream())
            assert rc == 0, fl.lib.admpc_last_error()
            _bits(fitted[c], _host(out).reshape(3, -1), "cluster %d: the GP of the rows handed over directly" % c)
            assert _host(oinfo).tolist() == got[2][c, :, 0].tolist()
        fl.rebin()
        _bits(_host(fl.bins), parent, "rebin() after a selection: the bin means again"); _bits(_host(fl.dropped), parent_dropped, "dropped")
    finally:
        fl.close()


# ---- 10. refusals, each in front of any device work -----------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_no_ops():
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    from ad_mpc_amd.quad_config import SimQuad
    fl = _make(2, steps=4, learn=_learn(2, bins=(32, 8, 32)))
    two = QuadEnsembleFleet(B, quad=SimQuad(drag=True), n_nodes=10, centroids=[[0.0]], feats=[10], log_steps=4,
                            learn=[[dict(QL.EXP_LEARN[0], feat=[7, 8], lo=[-9.0, -9.0], hi=[9.0, 9.0], bins=[4, 4], length_scale=[2.0, 2.0])]])
    nolog = _make(1, steps=0)
    try:
        L = fl.lib
        full = _load(fl, _records(4 * B, 95))
        fl.bins.fill_(4.0); fl.sel.fill_(4); fl.select_info.fill_(4); fl._select_work.fill_(4); fl._select_code.fill_(4); fl.select_edges.fill_(4.0)
        arrays = lambda: [_p(fl._select_code), _p(fl.select_edges), _p(fl._select_work), _p(fl.bins), _p(fl.sel), _p(fl.select_info)]
        n3 = lambda *v: (C.c_int32 * 3)(*v)
        call = lambda ens, M, n, log=True, arrs=None: L.admpc_quad_ensemble_select_points(ens, M, _p(fl.log) if log else None, n, *(arrs or arrays()), _stream())
        err = lambda: L.admpc_last_error().decode()
        # everything from refusal i on is wrong: i is reported
        assert call(None, -1, None, log=False, arrs=[None] * 6) == -1 and "null ensemble" in err()
        assert call(two._ens, -1, None, log=False, arrs=[None] * 6) == -1 and "number of records" in err()
        assert call(two._ens, 2 ** 31, None, log=False, arrs=[None] * 6) == -1 and "number of records" in err()
        assert call(two._ens, 4 * B, None, log=False, arrs=[None] * 6) == -1 and "more than one feature" in err()
        assert call(fl._ens, 4 * B, None, log=False, arrs=[None] * 6) == -1 and "null n_points" in err()
        for bad in (n3(0, 8, 20), n3(33, 8, 20), n3(20, 9, 20), n3(20, 8, -1)):       # regressor 1 has 8 bins
            assert call(fl._ens, 4 * B, bad, log=False, arrs=[None] * 6) == -1 and "n_points must be" in err()
        assert call(fl._ens, 4 * B, n3(20, 8, 20), log=False) == -1 and "null array" in err()
        for k in range(6):
            arrs = arrays(); arrs[k] = None
            assert call(fl._ens, 4 * B, n3(20, 8, 20), arrs=arrs) == -1 and "null array" in err()
        # the no-op: M == 0 with every array null, and with arrays that must stay as they are
        assert call(fl._ens, 0, n3(20, 8, 20), log=False, arrs=[None] * 6) == 0 and call(fl._ens, 0, n3(32, 8, 32)) == 0
        assert (_host(fl.bins) == 4.0).all() and (_host(fl.sel) == 4).all() and (_host(fl.select_info) == 4).all()
        assert (_host(fl._select_work) == 4).all() and (_host(fl._select_code) == 4).all() and (_host(fl.select_edges) == 4.0).all()
        _bits(_host(fl.log).reshape(-1, SS.REC), full, "the log after the refusals and the no-ops")
        # the fleet refuses before a launch
        for kw, words in ((dict(n_points=9), "regressor 1 must be in 1 .. 8"), (dict(n_points=[20, 8]), "one value per regressor"), (dict(n_points=0), "must be in")):
            with pytest.raises(ValueError, match=words):
                fl.select_points(**kw)
        with pytest.raises(ValueError, match="more than one feature"):
            two.select_points(4)
        with pytest.raises(ValueError, match="nothing selected yet"):
            fl.selected_points()
        fl.log_count = 0
        with pytest.raises(ValueError, match="the log is empty"):
            fl.select_points([20, 8, 20])
        with pytest.raises(ValueError, match="keeps no log"):
            nolog.select_points()
        assert (_host(fl.sel) == 4).all()
        # and the call that is not refused works on this fleet: regressor 1 at its 8 bins
        fl.log_count = 4
        sel, info = fl.select_points()
        want = SS.select_log(full, CENT[2], [10], REGS, [32, 8, 32])
        _bits(_host(sel), want[1], "sel at each regressor's nbins"); _bits(_host(info), want[2], "info")
    finally:
        fl.close(); two.close(); nolog.close()


# ---- 11. the experiment ------------------------------------------------------------------------------------------------------------------------------------

def test_a_closed_loop_trained_on_selected_records_flies_better_than_the_nominal_model():
    """The 64-vehicle closed loop of tests/test_quad_clusters_gpu.py (circles of 5 m at 2, 3, 4 and 5 m/s, drag on, 60 observed and
    logged steps, K = 3 on v_x): prune_log -> fit_clusters -> select_points(20) -> search_gp(factor=True) -> evaluate_log, then the second
    pass.  Only learned < nominal is asserted; the figures are printed: the summed position error of this route and of the binned one
    (the same chain with rebin() in place of select_points), the augmented / nominal RMS of both, and the largest distance between the
    mean of the selected targets and the mean of all targets of a cluster, relative to the range of the targets.
    Measured on the MI355X: nominal 532.879 m; selected 120.336 m with 20 20 15 / 20 20 20 / 20 19 20 points per cluster and axis,
    augmented / nominal RMS 0.0106 / 0.0078 / 0.3891; binned 120.262 m with 8 6 3 / 10 6 5 / 9 7 4 points, RMS 0.0044 / 0.0036 / 0.1037;
    the largest distance of the two means 0.2707 of the range; 5 + 1 empty bins of 180."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, T = 10, 60
    dt = 1.0 / (N * 5)
    trajs = [circle_reference(T + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
    traj_of = (np.arange(B) % 4).astype(np.int32)
    idx0 = (np.arange(B) // 4).astype(np.int32)
    ref = np.concatenate([[QL.body_velocity(trajs[k][0][i + t])[0] for t in range(T)] for k, i in zip(traj_of, idx0)])
    poor = np.quantile(ref, [0.05, 0.15, 0.9]).reshape(3, 1)
    learn = [[TE.VX(ref.min() - 0.5, ref.max() + 0.5)] + [dict(d) for d in QL.EXP_LEARN[1:]] for _ in range(3)]
    fl = TE._fleet(B, N, trajs, traj_of, idx0, None, centroids=poor, feats=[7], learn=learn, log_steps=T)
    try:
        fl.rollout(T, observe=True, log=True)
        nominal = float(_host(fl.tally)[:, 0].sum())
        fl.prune_log()
        fl.fit_clusters()
        flown = {}
        for route in ("selected", "binned"):
            if route == "selected":
                sel, info = fl.select_points(20)
            else:
                fl.rebin()
            fit_info, installed, hyper = fl.search_gp(factor=True)
            fl.evaluate_log()
            ev = fl.evaluation()
            ratio = ev.total.augmented_rms / ev.total.nominal_rms
            fl.reset(traj_of, idx0)
            fl.rollout(T)
            flown[route] = float(_host(fl.tally)[:, 0].sum())
            assert (_host(fl.counts) == [T, 0, 0]).all() and (_host(installed) == 1).all()
            print("%s: summed position error %.6g m (nominal %.6g m), points %s, augmented / nominal RMS per axis %s"
                  % (route, flown[route], nominal, _host(fit_info).tolist(), np.round(ratio, 4).tolist()))
        log = _host(fl.log).reshape(-1, SS.REC)
        cent = fl._device_centroids()
        want = SS.select_log(log, cent, [7], [(7, 7), (8, 8), (9, 9)], [20, 20, 20])
        _bits(_host(sel), want[1], "the selection of the flight"); _bits(_host(info), want[2], "info")
        valid = log[log[:, 13] == 1.0]
        from quad_ensemble_spec import route_records
        where = route_records(valid, [7], cent)
        gap = max(abs(want[0][c, g, :want[2][c, g, 0], 4].mean() - valid[where == c, 10 + g].mean()) / np.ptp(valid[where == c, 10 + g])
                  for c in range(3) for g in range(3))
        print("largest |mean of the selected targets - mean of all targets of the cluster| / range of the targets: %.4f; empty bins %s"
              % (gap, want[2][:, :, 2].tolist()))
        assert np.isfinite([nominal, flown["selected"], flown["binned"]]).all() and flown["selected"] < nominal
    finally:
        fl.close()
