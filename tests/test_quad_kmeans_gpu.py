"""The k-means start of the Gaussian-mixture EM (include/admpc_quad_kmeans.h; ad_mpc_amd/quad_ensemble_fleet.py) on the GPU, against the
numpy spec of tests/quad_kmeans_spec.py, which tests/test_quad_kmeans_cpu.py pins to scikit-learn's _kmeans_plusplus and KMeans: the raw
C ABI on every M, K and d at which the kernels take another path, the failures, determinism and the captured graph, the n_init rule, and
the fleet's chain k-means -> EM -> install -> re-bin in a short closed loop whose initial centroids are useless.

idx, labels, iterations and converged must equal the float64 spec exactly: tests/test_quad_kmeans_cpu.py holds every case used here to a
margin of 1e-9, so a correct kernel cannot decide otherwise.  The centres, the inertia and tol_abs are held to the spec in
numpy.longdouble within the forward error bounds of the header (quad_kmeans_spec.bounds); the fraction of the bound is printed."""
import ctypes as C
import functools

import numpy as np
import pytest

import quad_clusters_spec as CS
import quad_kmeans_spec as KS
import quad_learn_spec as QL
import test_quad_clusters_gpu as TC
import test_quad_ensemble_gpu as TE
import test_quad_fleet_gpu as TQ

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _stream = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._stream
LD = np.longdouble
PAD = 8


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


handle = TC.handle


class KM:
    """The scratch and the results of admpc_quad_kmeans_fit for up to M records over an ensemble of test_quad_clusters_gpu.Ens, with PAD
    poisoned entries behind every array that no kernel may touch."""

    def __init__(self, ens, M):
        import torch
        self.e, self.M = ens, M
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda:0")
        self.dist, self.labels, self.work = z(M + PAD), z(M + PAD, dtype=torch.int32), z(KS.work_doubles(M) + PAD)
        self.centers, self.idx, self.stats, self.info = z(ens.K * ens.d + PAD), z(ens.K + PAD, dtype=torch.int64), z(4 + PAD), z(4 + PAD, dtype=torch.int32)

    def fit(self, rec, seed, draw=0, max_iter=300, tol=1e-4):
        M = self.M
        for t, v in ((self.dist, float("nan")), (self.labels, 77), (self.work, float("nan")), (self.centers, float("nan")), (self.idx, 77),
                     (self.stats, float("nan")), (self.info, 77)):
            t.fill_(v)
        self.e.packed[M:].fill_(float("nan"))
        self.launch(rec, seed, draw, max_iter, tol)
        K, d = self.e.K, self.e.d
        out = dict(centers=_host(self.centers)[:K * d].reshape(K, d).copy(), idx=_host(self.idx)[:K].copy(), labels=_host(self.labels)[:M].copy(),
                   stats=_host(self.stats)[:4].copy(), info=_host(self.info)[:4].copy(), dist=_host(self.dist)[:M].copy())
        assert np.isnan(_host(self.dist)[M:]).all() and (_host(self.labels)[M:] == 77).all() and np.isnan(_host(self.work)[KS.work_doubles(M):]).all()
        assert np.isnan(_host(self.centers)[K * d:]).all() and (_host(self.idx)[K:] == 77).all() and np.isnan(_host(self.stats)[4:]).all()
        assert (_host(self.info)[4:] == 77).all() and np.isnan(_host(self.e.packed)[M:]).all()
        return out

    def launch(self, rec, seed, draw=0, max_iter=300, tol=1e-4):
        rc = self.e.L.admpc_quad_kmeans_fit(self.e.h, seed, draw, max_iter, tol, self.M, _p(rec), _p(self.e.packed), _p(self.dist), _p(self.labels),
                                            _p(self.work), _p(self.centers), _p(self.idx), _p(self.stats), _p(self.info), _stream())
        assert rc == 0, self.e.L.admpc_last_error()


@functools.lru_cache(maxsize=None)
def _spec(M, K, d, seed):
    """The records of a case and its spec in float64 and in longdouble, computed once and shared."""
    rec = KS.gpu_case(M, K, d, seed)
    lo, hi = (KS.fit(rec, KS.FEATS[d], K, seed=seed, dtype=t) for t in (np.float64, LD))
    assert hi["info"].tolist() == lo["info"].tolist() and np.array_equal(hi["labels"], lo["labels"]) and hi["idx"].tolist() == lo["idx"].tolist()
    return rec, lo, hi


def _held(got, lo, hi, K, d, tol, what):
    """The decisions exactly, the values within the header's bounds of the longdouble spec; returns the fractions of the bounds."""
    assert got["idx"].tolist() == lo["idx"].tolist(), what
    assert got["info"].tolist() == lo["info"].tolist(), (what, got["info"], lo["info"])
    assert np.array_equal(got["labels"], lo["labels"]), (what, int((got["labels"] != lo["labels"]).sum()))
    bc, bi, bt = KS.bounds(hi, K, d, tol)
    fc = float((np.abs(got["centers"] - hi["centers"]).max(axis=1) / bc).max())
    fi = abs(float(got["stats"][0] - hi["stats"][0])) / bi if bi > 0 else 0.0
    ft = abs(float(got["stats"][1] - hi["stats"][1])) / bt if bt > 0 else 0.0
    n = int(lo["info"][3])
    fp = abs(float(got["stats"][3] - hi["stats"][3])) / ((n + 4) * 2.0 ** -53 * float(hi["stats"][3])) if hi["stats"][3] > 0 else 0.0
    print("%s: fractions of the bounds: centres %.3f inertia %.3f tol_abs %.3f potential %.3f; %d iterations, converged %d, margin %.1e"
          % (what, fc, fi, ft, fp, lo["info"][0], lo["info"][1], lo["margin"]))
    assert fc <= 1.0 and fi <= 1.0 and ft <= 1.0 and fp <= 1.0, (what, fc, fi, ft, fp)
    assert abs(float(got["stats"][2] - hi["stats"][2])) <= 1e-12 * (1.0 + float(hi["stats"][2])), what
    return fc, fi, ft


# ---- 1. the device against the spec ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,d,seed", KS.GPU_CASES)
def test_the_fit_equals_the_spec(handle, M, K, d, seed):
    """M: less than a wave, exactly one tile, one record over a tile, a stride loop past the grid's first pass (4097 records are 17 tiles;
    65 793 are 258 tiles on a grid of 256 blocks, and more tiles than the one-wave scan has lanes).  Records that do not count at index 0,
    at M - 1, across a tile boundary and filling a tile."""
    rec, lo, hi = _spec(M, K, d, seed)
    e = TC.Ens(handle, K, KS.FEATS[d], np.full((K, d), 9.0), M)
    try:
        got = KM(e, M).fit(_dev(rec), seed)
        _held(got, lo, hi, K, d, 1e-4, "M %d K %d d %d" % (M, K, d))
        ok = CS.pack(rec, KS.FEATS[d])[:, 3] == 1.0
        assert (got["dist"][~ok] == 0.0).all() or K == 1
    finally:
        e.close()


def test_candidates_from_the_first_and_the_last_tile(handle):
    rec = KS.edges()
    lo, hi = (KS.fit(rec, [7], 3, seed=KS.EDGE_SEED, dtype=t) for t in (np.float64, LD))
    assert lo["idx"].min() < 256 and lo["idx"].max() >= 768
    e = TC.Ens(handle, 3, [7], [[9.0], [9.0], [9.0]], rec.shape[0])
    try:
        _held(KM(e, rec.shape[0]).fit(_dev(rec), KS.EDGE_SEED), lo, hi, 3, 1, 1e-4, "edges")
    finally:
        e.close()


def test_the_stops_by_tolerance_and_at_max_iter(handle):
    """A tolerance that the first shift below it stops (converged 1) and a max_iter that ends the run (converged 0): both label once more,
    so that the labels are those of the final centres."""
    M, K, d, seed = 4097, 3, 2, 1
    rec = KS.gpu_case(M, K, d, seed)
    e = TC.Ens(handle, K, KS.FEATS[d], np.full((K, d), 9.0), M)
    try:
        km, seen = KM(e, M), set()
        for kw in (dict(tol=1e-2), dict(max_iter=2), dict(max_iter=1, tol=0.0)):
            lo, hi = (KS.fit(rec, KS.FEATS[d], K, seed=seed, dtype=t, **kw) for t in (np.float64, LD))
            assert lo["margin"] >= 1e-9 and hi["info"].tolist() == lo["info"].tolist() and np.array_equal(hi["labels"], lo["labels"])
            assert abs(float(hi["stats"][2] - hi["stats"][1])) > 1e-6 * float(hi["stats"][1])      # the shift is not at the tolerance
            _held(km.fit(_dev(rec), seed, **kw), lo, hi, K, d, kw.get("tol", 1e-4), str(kw))
            seen.add(int(lo["info"][1]))
        assert seen == {0, 1}
    finally:
        e.close()


# ---- 2. failures -------------------------------------------------------------------------------------------------------------------------------

def test_failures_give_their_status_and_the_present_centroids(handle):
    cent = np.array([[4.0, -1.0], [2.0, 0.5], [7.0, 3.0]])
    rng = np.random.default_rng(3)
    none = KS.cloud(300, 3, 2, 0); none[:, 13] = 0.0
    few = none.copy(); few[[5, 299], 13] = 1.0
    twins = KS.cloud(300, 3, 2, 0); twins[:, :2] = np.where(rng.random((300, 1)) < 0.5, [1.0, 2.0], [-3.0, 0.25])
    e = TC.Ens(handle, 3, [7, 8], cent, 300)
    try:
        km = KM(e, 300)
        for what, rec, status, n in (("no valid record", none, KS.ENOVALID, 0), ("n_valid < K", few, KS.EFEW, 2), ("two distinct points", twins, KS.EFEW, 300)):
            want = KS.fit(rec, [7, 8], 3, seed=4)
            assert want["info"].tolist() == [0, 0, status, n], (what, want["info"])
            got = km.fit(_dev(rec), 4)
            assert got["info"].tolist() == [0, 0, status, n], (what, got["info"])
            _bits(got["centers"], cent, what + ": centers are the present centroids")
            assert (got["stats"] == 0.0).all(), what
            # an EM chained behind it starts where it would have started without the k-means
            e.gmm.fill_(0.0); e.info.fill_(0)
            e.fit(_dev(rec), km.centers, max_iter=2)
            chained = e.state()
            e.gmm.fill_(0.0); e.info.fill_(0)
            e.fit(_dev(rec), None, max_iter=2)
            _bits(chained[0], e.state()[0], what + ": the chained EM"); assert chained[1].tolist() == e.state()[1].tolist()
    finally:
        e.close()


@pytest.mark.parametrize("seed,status", KS.EMPTY_SEEDS)
def test_an_empty_cluster_is_a_failure(handle, seed, status):
    """A labelling pass that leaves cluster k empty ends the fit with status -(k + 1), where scikit-learn would relocate the centre: the
    seeding of quad_kmeans_spec.empties() under these seeds puts centres at 6, 10 and 31, and the second pass takes every record from the
    one at 10, which is cluster 0, 1 or 2.  info[0] counts the iteration before the empty pass, stats stay 0, centers are the present
    centroids bit for bit, and an EM chained behind it runs as without the k-means."""
    rec, cent = KS.empties(), np.array([[4.0], [2.0], [7.0]])
    want = KS.fit(rec, [7], 3, seed=seed)
    assert want["info"].tolist() == [1, 0, status, 23] and want["margin"] >= 1e-9
    e = TC.Ens(handle, 3, [7], cent, 23)
    try:
        km = KM(e, 23)
        got = km.fit(_dev(rec), seed)
        assert got["info"].tolist() == want["info"].tolist(), (got["info"], want["info"])
        assert got["idx"].tolist() == want["idx"].tolist()
        _bits(got["centers"], cent, "centers are the present centroids")
        assert (got["stats"] == 0.0).all()
        e.gmm.fill_(0.0); e.info.fill_(0)
        e.fit(_dev(rec), km.centers, max_iter=2)
        chained = e.state()
        e.gmm.fill_(0.0); e.info.fill_(0)
        e.fit(_dev(rec), None, max_iter=2)
        _bits(chained[0], e.state()[0], "the chained EM"); assert chained[1].tolist() == e.state()[1].tolist()
        # launches behind the failure change nothing
        again = km.fit(_dev(rec), seed, max_iter=20)
        for name in ("info", "idx", "centers", "stats"):
            _bits(again[name], got[name], "launches behind the failure: " + name)
    finally:
        e.close()


# ---- 3. invariants -------------------------------------------------------------------------------------------------------------------------------

def test_two_runs_and_a_captured_graph_give_the_same_bits(handle):
    import torch
    M, K, d, seed = 65793, 8, 2, 1
    rec, lo, _ = _spec(M, K, d, seed)
    e = TC.Ens(handle, K, KS.FEATS[d], np.full((K, d), 9.0), M)
    try:
        km, drec = KM(e, M), _dev(rec)
        first, again = km.fit(drec, seed), km.fit(drec, seed)
        for name in first:
            _bits(again[name], first[name], "two runs: " + name)
        assert first["info"].tolist() == lo["info"].tolist()
        # iterations behind the stop change nothing: the launches read the flag and return
        longer = km.fit(drec, seed, max_iter=int(lo["info"][0]) + 40)
        for name in first:
            _bits(longer[name], first[name], "launches behind the stop: " + name)
        other = km.fit(drec, seed, draw=1)
        assert other["idx"].tolist() != first["idx"].tolist()                                     # another draw is another seeding
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            km.launch(drec, seed)
        for t in (km.centers, km.stats, km.dist):
            t.fill_(0.0)
        km.labels.fill_(5); km.idx.fill_(5); km.info.fill_(5)
        g.replay()
        K_, d_ = K, d
        got = dict(centers=_host(km.centers)[:K_ * d_].reshape(K_, d_), idx=_host(km.idx)[:K_], labels=_host(km.labels)[:M], stats=_host(km.stats)[:4],
                   info=_host(km.info)[:4], dist=_host(km.dist)[:M])
        for name in first:
            _bits(got[name], first[name], "the replay: " + name)
    finally:
        e.close()


def test_refusals_in_their_order_and_the_no_op(handle):
    e = TC.Ens(handle, 2, [7], [[0.0], [1.0]], 64)
    low = TC.Ens(handle, 2, [3], [[0.0], [1.0]], 64)
    try:
        L, km = e.L, KM(e, 64)
        rec = _dev(KS.cloud(64, 2, 1, 0))
        a = lambda: [_p(rec), _p(e.packed), _p(km.dist), _p(km.labels), _p(km.work), _p(km.centers), _p(km.idx), _p(km.stats), _p(km.info)]

        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        refused(L.admpc_quad_kmeans_fit(low.h, 0, 0, 0, -1.0, -1, *([None] * 9), _stream()), "clustering features must lie in [7, 16]")
        refused(L.admpc_quad_kmeans_fit(e.h, 0, 0, 0, -1.0, -1, *([None] * 9), _stream()), "max_iter must be in [1, 1000]")
        refused(L.admpc_quad_kmeans_fit(e.h, 0, 0, 1001, -1.0, -1, *([None] * 9), _stream()), "max_iter must be in [1, 1000]")
        for bad in (-1.0, float("nan"), float("inf")):
            refused(L.admpc_quad_kmeans_fit(e.h, 0, 0, 5, bad, -1, *([None] * 9), _stream()), "tol must be finite and not negative")
        refused(L.admpc_quad_kmeans_fit(e.h, 0, 0, 5, 0.0, -1, *([None] * 9), _stream()), "negative number of records")
        assert L.admpc_quad_kmeans_fit(e.h, 0, 0, 5, 0.0, 0, *([None] * 9), _stream()) == 0        # M == 0: a no-op, nothing is read
        for i in range(9):
            args = a(); args[i] = None
            refused(L.admpc_quad_kmeans_fit(e.h, 0, 0, 5, 0.0, 64, *args, _stream()), "null array argument")
        refused(L.admpc_quad_kmeans_keep(e.h, -1, -1, *([None] * 11), _stream()), "negative draw")
        refused(L.admpc_quad_kmeans_keep(e.h, 0, -1, *([None] * 11), _stream()), "negative number of records")
        assert L.admpc_quad_kmeans_keep(e.h, 0, 0, *([None] * 11), _stream()) == 0
        refused(L.admpc_quad_kmeans_keep(e.h, 0, 64, *([None] * 11), _stream()), "null array argument")
        refused(L.admpc_quad_clusters_keep(e.h, -1, None, None, None, None, None, _stream()), "negative draw")
        refused(L.admpc_quad_clusters_keep(e.h, 0, _p(e.gmm), _p(e.info), _p(e.gmm), None, _p(e.perm), _stream()), "null array argument")
    finally:
        e.close(); low.close()


def test_keep_is_the_n_init_rule(handle):
    """The try replaces the best if its status is 0 and its bound finite, and the best holds nothing or the try's bound is strictly
    larger; draw 0 starts a series."""
    import torch
    K = 2
    e = TC.Ens(handle, K, [7], [[0.0], [1.0]], 8)
    try:
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda:0")
        best, binfo, kept = z(1 + K, CS.ROW), z(4, dtype=torch.int32), z(1, dtype=torch.int32)
        best.fill_(-7.0); binfo.fill_(9); kept.fill_(5)

        def tried(draw, bound, status):
            g = np.full((1 + K, CS.ROW), float(draw + 10)); g[0, 0] = bound
            assert e.L.admpc_quad_clusters_keep(e.h, draw, _p(_dev(g)), _p(_dev(np.array([draw, 1, status, 8], dtype=np.int32))), _p(best), _p(binfo), _p(kept),
                                                _stream()) == 0
            return int(_host(kept)[0]), float(_host(best)[1, 0]) - 10.0, _host(binfo).tolist()

        assert tried(0, -1.5, -2) == (-1, 0.0, [0, 1, -2, 8])                  # a failed first try is carried, and nothing is held
        assert tried(1, float("-inf"), 0)[:2] == (-1, 0.0)                     # a bound that is not finite
        assert tried(2, -1.5, 0) == (2, 2.0, [2, 1, 0, 8])                     # the first good one
        assert tried(3, -1.5, 0)[:2] == (2, 2.0)                               # an equal bound does not replace
        assert tried(4, -1.25, -1)[:2] == (2, 2.0)                             # a larger bound of a failed fit
        assert tried(5, -1.25, 0) == (5, 5.0, [5, 1, 0, 8])
        assert tried(6, float("nan"), 0)[:2] == (5, 5.0)
        assert tried(0, -9.0, 0) == (0, 0.0, [0, 1, 0, 8])                     # draw 0 starts afresh
        # the k-means results follow: copied where the rule has just kept that draw or started a series, else left
        M, d = 600, 1
        mk = lambda v: (z(K, d) + v, z(K, dtype=torch.int64) + int(v), z(M, dtype=torch.int32) + int(v), z(4) + v, z(4, dtype=torch.int32) + int(v))
        best5 = mk(-1.0)
        for draw, held, copied in ((3, 2, False), (3, 3, True), (0, -1, True), (1, 0, False)):
            kept.fill_(held)
            before = [_host(t).copy() for t in best5]
            try5 = mk(float(draw + 20))
            assert e.L.admpc_quad_kmeans_keep(e.h, draw, M, _p(kept), *[_p(t) for t in try5], *[_p(t) for t in best5], _stream()) == 0
            for t, b, w in zip(best5, before, try5):
                _bits(_host(t), _host(w) if copied else b, "draw %d kept %d" % (draw, held))
    finally:
        e.close()


# ---- 4. the fleet: init= an array as before, n_init, and the chain in a closed loop ---------------------------------------------------------------

@pytest.fixture(scope="module")
def flight():
    """The flight of tests/test_quad_clusters_gpu.py's closing test (B = 64, N = 10, circles of 5 m at 2, 3, 4 and 5 m/s, 60 observed and
    logged steps, K = 3 on the body-frame v_x), but ALL initial centroids useless: 50, 60 and 70 m/s, where no record lies."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, B, T = 10, 64, 60
    dt = 1.0 / (N * 5)
    trajs = [circle_reference(T + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
    traj_of = (np.arange(B) % 4).astype(np.int32)
    idx0 = (np.arange(B) // 4).astype(np.int32)
    ref = np.concatenate([[QL.body_velocity(trajs[k][0][i + t])[0] for t in range(T)] for k, i in zip(traj_of, idx0)])
    useless = np.array([[50.0], [60.0], [70.0]])
    learn = [[TE.VX(ref.min() - 0.5, ref.max() + 0.5)] + [dict(d) for d in QL.EXP_LEARN[1:]] for _ in range(3)]
    fl = TE._fleet(B, N, trajs, traj_of, idx0, None, centroids=useless, feats=[7], learn=learn, log_steps=T)
    fl.rollout(T, observe=True, log=True)
    nominal = float(_host(fl.tally)[:, 0].sum())
    yield dict(fl=fl, T=T, B=B, traj_of=traj_of, idx0=idx0, useless=useless, nominal=nominal, log=_host(fl.log).reshape(-1, 14).copy())
    fl.close()


def test_init_an_array_is_the_existing_entry_bit_for_bit(flight):
    """fit_clusters(init=<array>) launches what it launched before the k-means came: the state equals the existing entry's, called
    directly over the same log with scratch of its own; so it does with init=None, from the present centroids."""
    import torch
    fl, M = flight["fl"], flight["T"] * flight["B"]
    z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device=fl.device)
    packed, partial, gmm, info = z(M, 4), z(CS.BLOCKS_MAX, CS.PARTIAL), z(4, CS.ROW), z(4, dtype=torch.int32)
    for init in (np.array([[-4.5], [-3.4], [-0.4]]), None):
        start = None if init is None else torch.as_tensor(init).to(fl.device)
        assert fl.lib.admpc_quad_clusters_fit(fl._ens, 100, 1e-3, 1e-6, 0, M, _p(fl.log), _p(start), _p(packed), _p(partial), _p(gmm), _p(info), _stream()) == 0
        fl.gmm.fill_(0.0); fl.gmm_info.fill_(0)
        got = fl.fit_clusters(init=init, install=False, rebin=False)
        assert got[1] is None and got[2] is None
        _bits(_host(fl.gmm), _host(gmm), "gmm"); _bits(_host(fl.gmm_info), _host(info), "info"); _bits(_host(fl._packed)[:M], _host(packed), "packed")
    # from the useless centroids every record is nearest to the first: the EM keeps one component on the data and two on nothing
    assert _host(info)[2] == 0 and (_host(gmm)[2:, 17] < 1.0).all()
    for kw in (dict(seed=1), dict(n_init=2), dict(init="random")):
        with pytest.raises(ValueError):
            fl.fit_clusters(install=False, rebin=False, **kw)
    with pytest.raises(ValueError, match="needs a seed"):
        fl.fit_clusters(init="kmeans", install=False, rebin=False)


def test_n_init_keeps_the_fit_with_the_largest_bound(flight):
    """n_init = 3 against three single runs of the raw entries under draw = 0, 1, 2 over the same log."""
    import torch
    fl, M, K = flight["fl"], flight["T"] * flight["B"], 3
    z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device=fl.device)
    packed, partial, dist, labels, work = z(M, 4), z(CS.BLOCKS_MAX, CS.PARTIAL), z(M), z(M, dtype=torch.int32), z(KS.work_doubles(M))
    centers, idx, stats, kinfo = z(K, 1), z(K, dtype=torch.int64), z(4), z(4, dtype=torch.int32)
    runs = []
    for draw in range(3):
        gmm, info = z(1 + K, CS.ROW), z(4, dtype=torch.int32)
        assert fl.lib.admpc_quad_kmeans_fit(fl._ens, 7, draw, 300, 1e-4, M, _p(fl.log), _p(packed), _p(dist), _p(labels), _p(work), _p(centers), _p(idx),
                                            _p(stats), _p(kinfo), _stream()) == 0
        assert fl.lib.admpc_quad_clusters_fit(fl._ens, 100, 1e-3, 1e-6, 0, M, _p(fl.log), _p(centers), _p(packed), _p(partial), _p(gmm), _p(info), _stream()) == 0
        runs.append((_host(gmm).copy(), _host(info).copy(), _host(idx).copy(), _host(labels).copy(), _host(centers).copy(), _host(stats).copy(),
                     _host(kinfo).copy()))
    bounds = [r[0][0, 0] if r[1][2] == 0 and np.isfinite(r[0][0, 0]) else -np.inf for r in runs]
    best = int(np.argmax(bounds))                                                                # the first largest: a later equal one does not replace
    print("bounds of draw 0, 1, 2: %s; seeded records %s" % (bounds, [r[2].tolist() for r in runs]))
    assert np.isfinite(bounds[best]) and len({tuple(r[2].tolist()) for r in runs}) > 1
    info, perm, installed = fl.fit_clusters(init="kmeans", seed=7, n_init=3, install=False, rebin=False)
    assert perm is None and installed is None and info is fl.gmm_info
    _bits(_host(fl.gmm), runs[best][0], "the kept mixture"); _bits(_host(fl.gmm_info), runs[best][1], "its info")
    km = fl.learned_kmeans()
    # the k-means results are those of the kept draw
    assert km.kept == best and km.idx.tolist() == runs[best][2].tolist() and km.status == 0
    _bits(km.labels, runs[best][3], "labels of the kept draw"); _bits(km.centers, runs[best][4], "centres of the kept draw")
    _bits(_host(fl.km_stats), runs[best][5], "stats"); _bits(_host(fl.km_info), runs[best][6], "info")
    # n_init = 1 is draw 0 and launches no keep
    fl.fit_clusters(init="kmeans", seed=7, install=False, rebin=False)
    _bits(_host(fl.gmm), runs[0][0], "n_init = 1: draw 0"); assert fl.learned_kmeans().kept == 0


def test_the_chain_finds_the_clusters_of_a_flight_nobody_described(flight):
    """fit_clusters(init="kmeans", seed=0) from useless centroids: the k-means equals the spec on the downloaded log (the decisions exactly,
    given the margin of this flight's log, which is asserted; the values within the header's bounds), the centroids equal the numpy
    chain (k-means spec, then quad_clusters_spec.fit) within the 1e-10 x range of tests/test_quad_clusters_gpu.py, and the second pass's
    summed position error lies below the nominal model's measured in the same test.
    Measured on the MI355X: the k-means seeds the records 3300 / 2395 / 2014 and stops by tolerance after 5 iterations at -0.668 /
    -3.463 / -1.904; the EM ends after 5 iterations at the centroids -3.324 / -1.800 / -0.658; summed position error 532.879 m with
    the nominal model, 120.389 m with the clusters found from useless centroids and learned from the first pass (120.158 m with the
    EM from hand-placed poor centroids in tests/test_quad_clusters_gpu.py, 120.602 m with centroids given at the terciles of the
    reference).  Only learned < nominal is asserted."""
    fl, T, B, log = flight["fl"], flight["T"], flight["B"], flight["log"]
    lo, hi = (KS.fit(log, [7], 3, seed=0, dtype=t) for t in (np.float64, LD))
    assert lo["margin"] >= 1e-9 and hi["info"].tolist() == lo["info"].tolist() and np.array_equal(hi["labels"], lo["labels"]), lo["margin"]
    info, perm, installed = fl.fit_clusters(init="kmeans", seed=0)
    fit_info, gp_installed = fl.fit_gp(min_count=2)
    km, got = fl.learned_kmeans(), fl.learned_clusters()
    dev = dict(idx=km.idx, labels=km.labels, centers=km.centers, info=np.array([km.n_iter, km.converged, km.status, km.n_valid], dtype=np.int32),
               stats=np.array([km.inertia, km.tol_abs, km.shift, km.potential]))
    _held(dev, lo, hi, 3, 1, 1e-4, "the flight's k-means")
    span = np.ptp(log[log[:, 13] == 1.0, 0])
    gmm, winfo = np.zeros((4, CS.ROW)), np.zeros(4, dtype=np.int32)
    packed, changes = CS.pack(log, [7]), []
    assert CS.start(packed, lo["centers"], 1, 1e-6, gmm, winfo)
    for _ in range(100):
        if CS.iterate(packed, 1, 1e-3, 1e-6, gmm, winfo):
            changes.append(abs(gmm[0, 1]))
    assert min(abs(ch - 1e-3) for ch in changes) > 1e-8, changes
    cent, wperm, ok = CS.install(gmm, winfo, flight["useless"])
    print("k-means centres %s (records %s, %d iterations, converged %d), centroids %s after %d EM iterations" % (km.centers.ravel().tolist(), km.idx.tolist(), km.n_iter,
                                                                                                          km.converged, fl.centroids.ravel().tolist(), got.n_iter))
    assert ok == 1 and _host(installed).tolist() == [1] and got.status == 0 and _host(info).tolist() == winfo.tolist()
    assert got.perm.tolist() == wperm.tolist()
    assert np.abs(fl.centroids - cent).max() <= 1e-10 * span and np.abs(got.means - gmm[1:, 1:2]).max() <= 1e-10 * span
    assert (np.diff(fl.centroids[:, 0]) > 0).all() and fl.centroids.max() < 10.0
    bins, dropped = _host(fl.bins), _host(fl.dropped)
    wb, wd = np.zeros((3, 3, 32, 5)), np.zeros((3, 4), dtype=np.int32)
    CS.rebin(list(fl._obs), [7], fl.centroids, log.reshape(T, B, 14), wb, wd)
    _bits(bins, wb, "the bins the GPs were fitted to: the log under the found centroids"); _bits(dropped, wd, "dropped")
    assert _host(fit_info).min() >= 2 and (_host(gp_installed) == 1).all()
    fl.reset(flight["traj_of"], flight["idx0"])
    fl.rollout(T)
    learned = float(_host(fl.tally)[:, 0].sum())
    print("sum of |e| over %d steps of %d vehicles: nominal %.6g m, with K = 3 clusters found from useless centroids and learned from the first pass %.6g m"
          % (T, B, flight["nominal"], learned))
    assert (_host(fl.counts) == [T, 0, 0]).all() and np.isfinite([flight["nominal"], learned]).all() and learned < flight["nominal"]
