"""The centroids of a clustered GP ensemble found on the device (include/admpc_quad_clusters.h; ad_mpc_amd/quad_ensemble_fleet.py) without
a GPU: the header, the prototype table and the library agree; the refusals that need no handle come back in their order; the Python layer
refuses before a handle is asked for; and the numpy spec (tests/quad_clusters_spec.py), which the GPU tests hold the kernels against, is
pinned to sklearn.mixture.GaussianMixture -- the class the reference calls (gp_common.py:224-271).  The refusals behind a live handle are
in tests/test_quad_clusters_gpu.py."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import quad_clusters_spec as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"admpc_quad_ensemble_rollout_log_batch": 31, "admpc_quad_clusters_fit": 13, "admpc_quad_clusters_install": 6,
         "admpc_quad_ensemble_centroids_set": 4, "admpc_quad_ensemble_centroids_get": 3, "admpc_quad_clusters_rebin": 7}
VX = lambda lo, hi, **kw: dict(dict(feat=7, out=7, lo=[lo], hi=[hi], bins=[32], length_scale=2.0, noise=1e-4), **kw)


@pytest.fixture(scope="module")
def lib():
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- 1. the header, the table and the library -----------------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from ad_mpc_amd import _lib, quad_ensemble_fleet as F
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_clusters.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_CLUSTERS_EXPORTS, tuple) and list(_lib.QUAD_CLUSTERS_EXPORTS) == list(ARITY)
    # a fourth registry, which load() walks too; the three existing ones are what they were
    assert list(_lib.CLUSTER_TABLES) == ["admpc_quad_clusters.h"] and tuple(_lib.CLUSTER_TABLES["admpc_quad_clusters.h"]) == _lib.QUAD_CLUSTERS_EXPORTS
    assert len(_lib.TABLES) == 9 and list(_lib.MORE_TABLES) == ["admpc_quad_noise.h"] and list(_lib.ENSEMBLE_TABLES) == ["admpc_quad_ensemble.h"]
    others = {n for reg in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES) for t in reg.values() for n in t}
    assert not set(_lib.QUAD_CLUSTERS_EXPORTS) & others
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n and fn.restype is C.c_int, name
    # the logged rollout takes the ensemble rollout's arguments, then log, then the stream
    logged, plain = lib.admpc_quad_ensemble_rollout_log_batch.argtypes, lib.admpc_quad_ensemble_rollout_batch.argtypes
    assert list(logged[:29]) == list(plain[:29]) and logged[30] is plain[29]
    for name, val, py in (("ADMPC_GMM_BLOCKS_MAX", "256", F.GMM_BLOCKS_MAX), ("ADMPC_GMM_ROW", "18", F.GMM_ROW), ("ADMPC_GMM_PARTIAL", "81", F.GMM_PARTIAL),
                          ("ADMPC_GMM_ENOVALID", r"\(-100\)", F.GMM_ENOVALID)):
        assert re.search(r"#define\s+%s\s+%s" % (name, val), hdr), name
        assert py == int(val.strip("\\()")) == getattr(CS, name[len("ADMPC_GMM_"):]), name
    for cite in ("gp_common.py:224-271", "gp_fitting.py:190", "gp.py:592-596", "reference call site", "replaced by", "GaussianMixture"):
        assert cite in hdr, cite
    offered = hdr[hdr.index("NOT offered"):]
    for words in ("k-means++", "n_init", "covariance types", "choosing K", "top-2", "gp_common.py:253-262", "PCA", "gp_fitting.py:237-240",
                  "search of the hyperparameters", "SQP mode"):
        assert words in offered, words
    for words in ("CLUSTER c KEEPS BLOCK c", "DETERMINISM", "No floating-point atomics", "function of M alone", "bit for bit", "10 * 2^-52"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_clusters\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_clusters\.h", mk, flags=re.M)
    assert re.search(r"^#\s+admpc_quad_clusters\.hip\s", mk, flags=re.M)
    # the ensemble's header points here and keeps the phrases tests/test_quad_ensemble_cpu.py greps for
    ens = open(os.path.join(ROOT, "include", "admpc_quad_ensemble.h")).read()
    assert "admpc_quad_clusters.h" in ens[ens.index("NOT offered"):] and "centroids are GIVEN" in ens


# ---- 2. the refusals that need no handle ------------------------------------------------------------------------------------------------

def test_refusals_without_a_handle(lib):
    """The null ensemble, which every entry refuses first, whatever else is wrong with the call.  No device is touched."""
    L = lib

    def refused(rc, words):
        assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

    refused(L.admpc_quad_ensemble_rollout_log_batch(None, None, None, 0, -1, -1, *([None] * 23), None, None), "admpc_quad_ensemble_rollout_batch: null ensemble")
    refused(L.admpc_quad_clusters_fit(None, 0, -1.0, -1.0, 2, -1, None, None, None, None, None, None, None), "admpc_quad_clusters_fit: null ensemble")
    refused(L.admpc_quad_clusters_install(None, None, None, None, None, None), "admpc_quad_clusters_install: null ensemble")
    refused(L.admpc_quad_ensemble_centroids_set(None, None, None, None), "admpc_quad_ensemble_centroids_set: null ensemble")
    refused(L.admpc_quad_ensemble_centroids_get(None, None, None), "admpc_quad_ensemble_centroids_get: null ensemble")
    refused(L.admpc_quad_clusters_rebin(None, -1, -1, None, None, None, None), "admpc_quad_clusters_rebin: null ensemble")


# ---- 3. the Python layer refuses before a handle is asked for ---------------------------------------------------------------------------

def test_python_refusals_come_before_a_handle():
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet, centroid_block, clusters_request, log_layout
    two, cent = [[VX(0.0, 3.0)], [VX(2.0, 6.0, length_scale=1.0)]], [[1.5], [4.0]]
    with pytest.raises(ValueError, match="log_steps must be"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=two, log_steps=-1)
    with pytest.raises(ValueError, match="log_steps must be"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=two, log_steps=2.5)
    with pytest.raises(ValueError, match="needs a fleet that learns"):
        QuadEnsembleFleet(4, ensemble=QuadGPEnsemble([[], []], cent, [7]), log_steps=8)
    with pytest.raises(ValueError, match="features in 7 .. 16"):                                # a fleet that logs learns: the constructor's own refusal
        QuadEnsembleFleet(4, centroids=cent, feats=[2], learn=two, log_steps=8)
    assert log_layout(0, False) == 0 and log_layout(60, True) == 60
    # fit_clusters' arguments, in admpc_quad_clusters_fit's order
    ask = lambda **kw: clusters_request(2, kw.pop("feats", [7]), kw.pop("steps", 5), **kw)
    with pytest.raises(ValueError, match="features must lie in 7 .. 16"):
        ask(feats=[7, 2], steps=0, max_iter=0)
    with pytest.raises(ValueError, match="the log is empty"):
        ask(steps=0, max_iter=0)
    for bad in (0, 1001, -3, 2.5):
        with pytest.raises(ValueError, match="max_iter must be in 1 .. 1000"):
            ask(max_iter=bad, tol=-1.0)
    for bad in (-1e-9, np.nan):
        with pytest.raises(ValueError, match="tol must not be negative"):
            ask(tol=bad, reg_covar=-1.0)
    for bad in (-1e-9, np.nan, np.inf):
        with pytest.raises(ValueError, match="reg_covar must be finite"):
            ask(reg_covar=bad, init=[[0.0]])
    with pytest.raises(ValueError, match="init must be K x len"):
        ask(init=[[0.0], [1.0], [2.0]])
    with pytest.raises(ValueError, match="init must be K x len"):
        ask(feats=[7, 8], init=[0.0, 1.0])
    with pytest.raises(ValueError, match="init: a centroid is not finite"):
        ask(init=[[0.0], [np.inf]])
    assert ask() == (100, 1e-3, 1e-6, None) and ask(tol=0, max_iter=1000, reg_covar=0)[:3] == (1000, 0.0, 0.0)      # sklearn's defaults
    got = ask(init=[0.5, 2.0])[3]
    assert got.shape == (2, 1) and got.dtype == np.float64
    with pytest.raises(ValueError, match="set_centroids: c must be K x len"):
        centroid_block("set_centroids: c", [[1.0, 2.0]], 2, 1)
    with pytest.raises(ValueError, match="not finite"):
        centroid_block("set_centroids: c", [[1.0], [np.nan]], 2, 1)


# ---- 4. the spec is the reference's algorithm ---------------------------------------------------------------------------------------------

def _sklearn_from(spec_start, d, K, X, **kw):
    """GaussianMixture started where the spec's start step stands: with the three *_init its _initialize ignores its own k-means."""
    from sklearn.mixture import GaussianMixture
    w, m, c, P = CS.unpack(spec_start, d)
    prec = np.array([p @ p.T for p in P])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                          # tol = 0 never converges: that is the point
        return GaussianMixture(K, covariance_type="full", weights_init=w / w.sum(), means_init=m, precisions_init=prec, random_state=0, **kw).fit(X)


@pytest.mark.parametrize("d,K", CS.FIXTURES)
def test_spec_is_sklearns_em(d, K):
    """30 iterations at tol = 0: means, covariances and weights within 1e-12 of sklearn's (measured when this was written: 7.2e-15,
    2.8e-16, 5e-16, the scale of the data being a few units); at sklearn's default tol = 1e-3 the same number of iterations, and no change
    of the lower bound within [0.8 tol, 1.25 tol], so that an implementation a few units in the last place away stops at the same one."""
    rec, init = CS.blobs(d, K)
    feats, X = CS.FIXTURE_FEATS[d], rec[:, :d]
    packed = CS.pack(rec, feats)
    first, info0 = np.zeros((1 + K, CS.ROW)), np.zeros(4, dtype=np.int32)
    assert CS.start(packed, init, d, 1e-6, first, info0) and info0.tolist() == [0, 0, 0, K * 400] and first[0, 0] == -np.inf
    sk = _sklearn_from(first, d, K, X, tol=0.0, max_iter=30)
    gmm, info = CS.fit(rec, feats, init, max_iter=30, tol=0.0)
    w, m, c, _ = CS.unpack(gmm, d)
    print("d %d K %d: |means| %.2e |cov| %.2e |weights| %.2e |bound| %.2e" % (d, K, np.abs(m - sk.means_).max(), np.abs(c - sk.covariances_).max(),
                                                                             np.abs(w - sk.weights_).max(), abs(gmm[0, 0] - sk.lower_bound_)))
    assert info.tolist() == [30, 0, 0, K * 400] and sk.n_iter_ == 30
    assert np.abs(m - sk.means_).max() <= 1e-12 and np.abs(c - sk.covariances_).max() <= 1e-12 and np.abs(w - sk.weights_).max() <= 1e-12
    assert abs(gmm[0, 0] - sk.lower_bound_) <= 1e-12
    # the default tolerance: the same stop
    tol = 1e-3
    sk = _sklearn_from(first, d, K, X, tol=tol, max_iter=100)
    gmm, info = first.copy(), info0.copy()
    changes = []
    for _ in range(100):
        if CS.iterate(packed, d, tol, 1e-6, gmm, info):
            changes.append(abs(gmm[0, 1]))
    assert sk.converged_ and info[1] == 1 and info[0] == sk.n_iter_ == len(changes) and 2 <= info[0] < 30, (info, sk.n_iter_)
    assert not any(0.8 * tol <= ch <= 1.25 * tol for ch in changes), changes
    assert np.abs(CS.unpack(gmm, d)[1] - sk.means_).max() <= 1e-12
    # what the fit is for: the means find the blobs, 2.5 apart on the first feature, whatever the poor start
    cent, perm, installed = CS.install(gmm, info, init)
    assert installed == 1 and np.abs(cent[:, 0] - 2.5 * np.arange(K)).max() < 0.15 and sorted(perm.tolist()) == list(range(K))


def test_spec_resume_failures_and_install():
    rec, init = CS.blobs(2, 3)
    feats = CS.FIXTURE_FEATS[2]
    whole, winfo = CS.fit(rec, feats, init, max_iter=4, tol=0.0)
    gmm, info = CS.fit(rec, feats, init, max_iter=1, tol=0.0)
    for _ in range(3):
        CS.fit(rec, feats, None, max_iter=1, tol=0.0, gmm=gmm, info=info, resume=True)
    assert np.array_equal(gmm.view(np.uint64), whole.view(np.uint64)) and info.tolist() == winfo.tolist() == [4, 0, 0, 1200]
    # records that do not count: a cleared flag, a feature that is not finite (one the clustering does not read does not matter)
    bad = rec.copy()
    bad[5, 13], bad[9, 0], bad[11, 1], bad[12, 5] = 0.0, np.nan, np.inf, np.nan
    assert CS.pack(bad, feats)[:, 3].sum() == 1197 and not CS.pack(bad, feats)[[5, 9, 11]].any() and CS.pack(bad, feats)[12, 3] == 1.0
    assert CS.fit(bad, feats, init, max_iter=2)[1][3] == 1197
    # identical points under identical means, no regularisation: component 0 takes them all and its covariance is zero
    same = np.zeros((50, 14)); same[:, 0], same[:, 13] = 1.25, 1.0
    keep = np.full((3, CS.ROW), 7.0)
    gmm, info = CS.fit(same, [7], [[1.0], [1.0]], max_iter=3, reg_covar=0.0, gmm=keep.copy(), info=np.full(4, 9, dtype=np.int32))
    assert info.tolist() == [0, 0, -1, 50] and np.array_equal(gmm, keep)
    cent, perm, installed = CS.install(gmm, info, [[4.0], [2.0]])
    assert installed == 0 and cent.tolist() == [[4.0], [2.0]] and perm.tolist() == [0, 1]
    same[:, 13] = 0.0
    assert CS.fit(same, [7], [[1.0], [1.0]], max_iter=3)[1].tolist() == [0, 0, CS.ENOVALID, 0]
    # the install sorts along the first feature, ties to the lower component
    g = np.zeros((4, CS.ROW)); g[1:, 1], g[1:, 2] = [3.0, -1.0, 3.0], [0.1, 0.2, 0.3]
    cent, perm, installed = CS.install(g, np.zeros(4, dtype=np.int32), np.zeros((3, 2)))
    assert installed == 1 and perm.tolist() == [1, 0, 2] and cent.tolist() == [[-1.0, 0.2], [3.0, 0.1], [3.0, 0.3]]
    g[2, 2] = np.nan
    assert CS.install(g, np.zeros(4, dtype=np.int32), np.zeros((3, 2)))[2] == 0
