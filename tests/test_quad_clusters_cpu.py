"""The centroids of a clustered GP ensemble found on the device (include/admpc_quad_clusters.h; ad_mpc_amd/quad_ensemble_fleet.py) without
a GPU: the header, the prototype table and the library agree; the refusals that need no handle come back in their order; the Python layer
refuses before a handle is asked for; and the numpy spec (tests/quad_clusters_spec.py), which the GPU tests hold the kernels against, is
pinned to sklearn.mixture.GaussianMixture -- the class the reference calls (gp_common.py:224-271).  The spec runs in float64 and in
numpy.longdouble: its float64 path is held to the bits it returned before it took the arithmetic as an argument, and the fixtures that
are not easy (quad_clusters_spec.hard) are held to the conditions the GPU tests rely on, in both.  The refusals behind a live handle are
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


# ---- 5. the spec in two precisions ----------------------------------------------------------------------------------------------------------

class Was:
    """The spec as it stood before it took the arithmetic as an argument: float64 throughout, formulas unchanged.  Kept to hold the
    float64 path of tests/quad_clusters_spec.py to the bits it returned then; nothing else may use it."""

    @staticmethod
    def pack(records, feats):
        S = np.asarray(records, dtype=np.float64).reshape(-1, CS.REC)
        out = np.zeros((S.shape[0], 4))
        z = S[:, [f - CS.QL.FEAT0 for f in feats]]
        ok = (S[:, CS.REC - 1] == 1.0) & np.isfinite(z).all(axis=1)
        out[ok, :len(feats)] = z[ok]
        out[ok, 3] = 1.0
        return out

    @staticmethod
    def moments(x, r, means):
        K = means.shape[0]
        S = np.zeros((K, 10))
        for k in range(K):
            D = x - means[k]
            rD = r[:, k, None] * D
            S[k, 0], S[k, 1:4] = r[:, k].sum(), rD.sum(axis=0)
            S[k, 4:10] = [(rD[:, i] * D[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        return S

    @staticmethod
    def m_step(gmm, info, S, lse_sum, means, d, n_valid, tol, reg, start):
        K = S.shape[0]
        rows, bad = np.zeros((K, CS.ROW)), []
        with np.errstate(all="ignore"):
            for k in range(K):
                N = S[k, 0] + CS.TINY
                s = S[k, 1:4] / N
                m = means[k] + s
                c = S[k, 4:10] / N - np.array([s[0] * s[0], s[0] * s[1], s[0] * s[2], s[1] * s[1], s[1] * s[2], s[2] * s[2]])
                c[[0, 3, 5]] += reg
                if d < 2:
                    m[1], c[1], c[3], c[4] = 0.0, 0.0, 1.0, 0.0
                if d < 3:
                    m[2], c[2], c[4], c[5] = 0.0, 0.0, 0.0, 1.0
                p0 = c[0]; l00 = np.sqrt(p0); l10 = c[1] / l00; l20 = c[2] / l00
                p1 = c[3] - l10 * l10; l11 = np.sqrt(p1); l21 = (c[4] - l20 * l10) / l11
                p2 = c[5] - l20 * l20 - l21 * l21; l22 = np.sqrt(p2)
                if not all(p > 0.0 and np.isfinite(p) for p in (p0, p1, p2)):
                    bad.append(k)
                    continue
                P00, P11, P22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
                P01 = -(l10 * P00) / l11; P12 = -(l21 * P11) / l22; P02 = -(l20 * P00 + l21 * P01) / l22
                rows[k, 0], rows[k, 1:4], rows[k, 4:10] = N / n_valid, m, c
                rows[k, 10:16] = [P00, P01, P02, P11, P12, P22]
                rows[k, 16], rows[k, 17] = np.log(P00) + np.log(P11) + np.log(P22), N
        if bad:
            info[2] = -(bad[0] + 1)
            if start:
                info[0], info[1], info[3] = 0, 0, int(n_valid)
            return False
        lb, change = -np.inf, np.inf
        if not start:
            lb = lse_sum / n_valid
            change = lb - gmm[0, 0]
        gmm[1:] = rows
        gmm[0] = 0.0
        gmm[0, :3] = lb, change, n_valid
        info[0] = 0 if start else info[0] + 1
        info[1] = int((not start) and abs(change) < tol)
        info[2], info[3] = 0, int(n_valid)
        return True

    @staticmethod
    def start(packed, init, d, reg_covar, gmm, info):
        init = np.asarray(init, dtype=np.float64).reshape(-1, d)
        K = init.shape[0]
        x = packed[packed[:, 3] == 1.0, :3]
        if x.shape[0] == 0:
            info[:] = 0, 0, CS.ENOVALID, 0
            return False
        means = np.zeros((K, 3)); means[:, :d] = init
        r = np.zeros((x.shape[0], K))
        r[np.arange(x.shape[0]), CS.nearest_rows(x[:, :d], init)[0]] = 1.0
        return Was.m_step(gmm, info, Was.moments(x, r, means), 0.0, means, d, float(x.shape[0]), 0.0, reg_covar, True)

    @staticmethod
    def iterate(packed, d, tol, reg_covar, gmm, info):
        if info[1] or info[2]:
            return False
        x = packed[packed[:, 3] == 1.0, :3]
        K = gmm.shape[0] - 1
        means = gmm[1:, 1:4].copy()
        lp = np.zeros((x.shape[0], K))
        with np.errstate(all="ignore"):
            for k in range(K):
                P = gmm[1 + k, 10:16][CS.TRI] * np.triu(np.ones((3, 3)))
                y = (x - means[k]) @ P
                lp[:, k] = (np.log(gmm[1 + k, 0]) + gmm[1 + k, 16] - 0.5 * d * CS.LOG_2PI) - 0.5 * (y * y).sum(axis=1)
            mx = lp.max(axis=1)
            lse = mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1))
            r = np.exp(lp - lse[:, None])
        return Was.m_step(gmm, info, Was.moments(x, r, means), lse.sum(), means, d, gmm[0, 2], tol, reg_covar, False)

    @staticmethod
    def fit(records, feats, init, max_iter, tol, reg_covar):
        d = len(feats)
        packed = Was.pack(records, feats)
        gmm, info = np.zeros((1 + np.asarray(init).reshape(-1, d).shape[0], CS.ROW)), np.zeros(4, dtype=np.int32)
        Was.start(packed, init, d, reg_covar, gmm, info)
        for _ in range(int(max_iter)):
            Was.iterate(packed, d, tol, reg_covar, gmm, info)
        return gmm, info


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("d,K", CS.FIXTURES)
def test_float64_path_returns_the_bits_it_returned_and_longdouble_agrees(d, K):
    """The float64 path against the formulas as they stood (class Was), bit for bit: the packed records, the start, every one of 30
    iterations at tol = 0, and the fit at the defaults.  The longdouble path returns arrays of that type and lies within the sklearn
    pin's own figure, 1e-12, of the float64 path (measured when this was written: below 1e-14); same iteration count at the default tol."""
    LD = np.longdouble
    rec, init = CS.blobs(d, K)
    feats = CS.FIXTURE_FEATS[d]
    assert _same_bits(CS.pack(rec, feats), Was.pack(rec, feats))
    packed = CS.pack(rec, feats)
    now, was = (np.zeros((1 + K, CS.ROW)), np.zeros(4, dtype=np.int32)), (np.zeros((1 + K, CS.ROW)), np.zeros(4, dtype=np.int32))
    assert CS.start(packed, init, d, 1e-6, *now) and Was.start(packed, init, d, 1e-6, *was)
    for it in range(31):
        assert _same_bits(now[0], was[0]) and now[1].tolist() == was[1].tolist(), it
        assert CS.iterate(packed, d, 0.0, 1e-6, *now) and Was.iterate(packed, d, 0.0, 1e-6, *was)
    whole, old = CS.fit(rec, feats, init), Was.fit(rec, feats, init, 100, 1e-3, 1e-6)
    assert _same_bits(whole[0], old[0]) and whole[1].tolist() == old[1].tolist() and whole[1][1] == 1
    # the same lines in 80-bit arithmetic
    assert CS.pack(rec, feats, LD).dtype == LD and np.array_equal(CS.pack(rec, feats, LD), packed)
    for kw in (dict(max_iter=30, tol=0.0), dict()):
        lo, hi = CS.fit(rec, feats, init, **kw), CS.fit(rec, feats, init, dtype=LD, **kw)
        assert hi[0].dtype == LD and lo[0].dtype == np.float64 and hi[1].dtype == np.int32 and hi[1].tolist() == lo[1].tolist()
        (lw, lm, lc, _), (hw, hm, hc, _) = CS.unpack(lo[0], d), CS.unpack(hi[0], d)
        assert hm.dtype == LD and hc.dtype == LD and hw.dtype == LD
        gaps = [float(np.abs(a - b).max()) for a, b in ((lm, hm), (lc, hc), (lw, hw))] + [float(abs(lo[0][0, 0] - hi[0][0, 0]))]
        print("d %d K %d %s: float64 against longdouble |means| %.2e |cov| %.2e |weights| %.2e |bound| %.2e" % ((d, K, kw) + tuple(gaps)))
        assert max(gaps) <= 1e-12
        assert np.abs(hi[0] - hi[0].astype(np.float64)).max() > 0.0                              # it is not float64 carried in a wider type


# ---- 6. the hard fixtures keep the conditions the GPU tests rely on -------------------------------------------------------------------------

@pytest.mark.parametrize("name,reg", CS.HARD_CASES + (CS.HARD_FAILS,))
def test_hard_fixtures_hold_what_the_gpu_tests_rely_on(name, reg):
    """For every hard fixture, in float64 and in longdouble, at tol = 1e-3: the fit does not fail (but `starved` at reg_covar = 0, whose
    start fails with info[2] = -3 and leaves the state as it was); both arithmetics converge, in the same number of iterations; no
    iteration's |change| lies within 1e-6 of tol, nor within 100 x the largest gap in `change` between the two arithmetics, so the
    device's iteration count cannot differ for a correct kernel; at the start every record's nearest-mean margin is at least 1e-9.  The
    gap between the two arithmetics, which the GPU tests scale their tolerance with, is printed in their scaling."""
    tol, LD = 1e-3, np.longdouble
    d, K, regs = CS.HARD[name]
    lo, hi = CS.hard_run(name, reg, np.float64, tol), CS.hard_run(name, reg, LD, tol)
    assert lo["rec"].shape[0] <= 4000 and lo["init"].shape == (K, d) and hi["whole"][0].dtype == LD
    assert lo["margin"] >= 1e-9 and np.isfinite(lo["rec"][:, :d]).all()
    if (name, reg) == CS.HARD_FAILS:
        keep = np.full((1 + K, CS.ROW), 7.0)
        for dtype in (np.float64, LD):
            gmm, info = CS.fit(lo["rec"], lo["feats"], lo["init"], max_iter=3, reg_covar=reg, gmm=keep.astype(dtype), info=np.full(4, 9, dtype=np.int32),
                               dtype=dtype)
            assert info.tolist() == [0, 0, -3, lo["rec"].shape[0]] and np.array_equal(gmm, keep)
        assert lo["one"] is None and hi["one"] is None and CS.install(gmm, info, lo["init"])[2] == 0
        assert reg not in regs and any(n == name for n, _ in CS.HARD_CASES)                      # the same data is fitted at the default
        return
    n = lo["rec"].shape[0]
    for run in (lo, hi):
        assert run["one"][1].tolist() == [1, 0, 0, n] and run["whole"][1][1:].tolist() == [1, 0, n], (name, reg, run["whole"][1])
        assert 2 <= run["whole"][1][0] < CS.HARD_MAX_ITER and len(run["changes"]) == run["whole"][1][0] - 1
    near = min(abs(abs(float(ch)) - tol) for run in (lo, hi) for ch in run["changes"])
    assert near >= 1e-6, (lo["changes"], hi["changes"])
    assert lo["whole"][1].tolist() == hi["whole"][1].tolist()
    dch = max(abs(float(a - b)) for a, b in zip(lo["changes"], hi["changes"]))
    one, whole = CS.scaled_gap(lo["one"][0], hi["one"][0], d, lo["span"]), CS.scaled_gap(lo["whole"][0], hi["whole"][0], d, lo["span"])
    print("%s reg %g: %d iterations; float64 against longdouble (means, covariances, weights, bound) one iteration %s, whole fit %s; change %.1e"
          % (name, reg, lo["whole"][1][0], ["%.1e" % g for g in one], ["%.1e" % g for g in whole], dch))
    # the device's change may differ from the float64 spec's by twice the tolerance of the bound, 10 x the gap each: the nearest change
    # of this fixture keeps five times that from tol
    assert near >= 100.0 * dch, (near, dch)
    if name == "starved":
        assert lo["given"][0][3, 17] == CS.TINY and lo["whole"][0][3, 17] == CS.TINY            # the third component has no record, then and later


@pytest.mark.parametrize("name", ["anisotropic", "overlap"])
def test_without_a_regulariser_the_bound_of_the_spec_does_not_decrease(name):
    """EM's bound is monotone; at reg_covar = 0 the M step is the exact maximiser, so what decrease there is is rounding.  40 iterations at
    tol = 0: the longdouble run's change is never below -1e-15 (1 + |bound|).  The float64 run's lies within the gap between the two,
    which is what the GPU test allows the device ten times of."""
    lo, hi = CS.hard_run(name, 0.0, np.float64, 0.0, 40), CS.hard_run(name, 0.0, np.longdouble, 0.0, 40)
    assert lo["whole"][1].tolist() == hi["whole"][1].tolist() == [40, 0, 0, lo["rec"].shape[0]] and len(hi["changes"]) == 39
    bound = float(hi["whole"][0][0, 0])
    gap = max(abs(float(a - b)) for a, b in zip(lo["changes"], hi["changes"]))
    print("%s: bound %.6f, smallest change longdouble %.2e float64 %.2e, largest gap in change %.2e" % (name, bound, float(min(hi["changes"])), min(lo["changes"]), gap))
    floor = -1e-15 * (1.0 + abs(bound))
    assert float(min(hi["changes"])) >= floor
    assert min(lo["changes"]) >= floor - gap and 0.0 < gap < 1e-12


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
