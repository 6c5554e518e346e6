"""The k-means start of the Gaussian-mixture EM (include/admpc_quad_kmeans.h; ad_mpc_amd/quad_ensemble_fleet.py) without a GPU: the
header, the prototype table, the Makefile and the library agree; the refusals that need no handle; the Python layer's refusals; and the
numpy spec (tests/quad_kmeans_spec.py), which the GPU tests hold the kernels against, pinned to scikit-learn -- the seeding to
sklearn.cluster._kmeans._kmeans_plusplus through a stub random_state that hands out the spec's uniforms, the Lloyd run to
KMeans(init=<those points>, n_init=1, algorithm="lloyd") -- and held to the margin the GPU tests rely on for every case they use."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import quad_clusters_spec as CS
import quad_kmeans_spec as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "admpc_quad_kmeans.h"
ARITY = {"admpc_quad_kmeans_fit": 16, "admpc_quad_clusters_keep": 8, "admpc_quad_kmeans_keep": 15}
LD = np.longdouble
# (n, K, d, seed): K = 1, 2, 3, 8 and d = 1, 2, 3 twice each, 50 .. 3000 points
CPU_CASES = tuple((n, K, d, s) for s, sizes in enumerate(((50, 400, 3000), (120, 1000, 2000)))
                  for K in (1, 2, 3, 8) for d, n in zip((1, 2, 3), sizes))


@pytest.fixture(scope="module")
def lib():
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---- 1. the header, the table, the Makefile and the library -------------------------------------------------------------------------------

def test_header_table_makefile_and_library_agree(lib):
    from ad_mpc_amd import _lib, quad_ensemble_fleet as F
    hdr = open(os.path.join(ROOT, "include", HEADER)).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: len(p.split(",")) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert list(_lib.KMEANS_TABLES) == [HEADER] and tuple(_lib.KMEANS_TABLES[HEADER]) == _lib.QUAD_KMEANS_EXPORTS == tuple(ARITY)
    known = [t for group in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES, _lib.TARGET_TABLES,
                             _lib.PRUNE_TABLES, _lib.EVAL_TABLES, _lib.TRAJ_TABLES, _lib.POLY_TRAJ_TABLES, _lib.SELECT_TABLES, _lib.SQP_TABLES)
             for t in group.values()]
    assert not set(ARITY) & {n for t in known for n in t}                          # no name is declared by two headers
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n == len(_lib.KMEANS_TABLES[HEADER][name][1]) and fn.restype is C.c_int, name
    assert lib.admpc_quad_kmeans_fit.argtypes[1] is C.c_uint64 and lib.admpc_quad_kmeans_fit.argtypes[2] is C.c_uint32
    for name, val, py, spec in (("ADMPC_KMEANS_PHILOX_WORD", "0x4B4D2B2Bu", 0x4B4D2B2B, KS.WORD), ("ADMPC_KMEANS_PARTIAL", "33", F.KMEANS_PARTIAL, KS.PARTIAL),
                                ("ADMPC_KMEANS_STATE", "48", F.KMEANS_STATE, KS.STATE), ("ADMPC_KMEANS_EFEW", r"\(-101\)", F.KMEANS_EFEW, KS.EFEW)):
        assert re.search(r"#define\s+%s\s+%s" % (name, val), hdr), name
        assert py == spec, name
    assert "2 * (((M) + 255) / 256) + ADMPC_GMM_BLOCKS_MAX * ADMPC_KMEANS_PARTIAL + ADMPC_KMEANS_STATE" in hdr
    for M in (1, 256, 257, 65793):
        assert F.kmeans_work(M) == KS.work_doubles(M) == 2 * math.ceil(M / 256) + 256 * 33 + 48
    for cite in ("gp_common.py:242", "reference call site", "replaced by", "_kmeans_plusplus", "_kmeans_single_lloyd", "KMeans(n_clusters, n_init=1)",
                 "GaussianMixture"):
        assert cite in hdr, cite
    for words in ("NOT offered", "AN EMPTY CLUSTER IS A FAILURE", "deliberate difference", "THE RANDOM NUMBERS", "word t % 2 of call t / 2",
                  "Round 0 uses word 0 of call 0", "DETERMINISM", "No floating-point atomics", "function of M alone", "function of K and max_iter alone",
                  "the smallest wins, ties to the lower", "PRESENT device centroids", "((x0 - c0)^2 + (x1 - c1)^2) + (x2 - c2)^2", "ACCURACY"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*[:+]?=.*\badmpc_quad_kmeans\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_kmeans\.h", mk, flags=re.M)
    assert re.search(r"^#\s+admpc_quad_kmeans\.hip\s", mk, flags=re.M)
    # the EM's header points here from the entry that said the start is not offered
    cl = open(os.path.join(ROOT, "include", "admpc_quad_clusters.h")).read()
    assert HEADER in cl[cl.index("NOT offered"):cl.index("covariance types")]
    # the unit launches the EM's pack kernel and does not carry a copy of it
    src = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "admpc_quad_kmeans.hip")).read()
    assert "hipLaunchKernelGGL(admpc_quad_gmm_pack_kernel" in src and "atomicAdd(w.changed" in src and src.count("atomicAdd") == 1
    for doc in ("README.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc


def test_refusals_without_a_handle(lib):
    """The null ensemble, which both entries refuse first, whatever else is wrong with the call.  No device is touched."""
    for call, words in ((lambda: lib.admpc_quad_kmeans_fit(None, 0, 0, 0, -1.0, -1, *([None] * 9), None), "admpc_quad_kmeans_fit: null ensemble"),
                        (lambda: lib.admpc_quad_clusters_keep(None, -1, None, None, None, None, None, None), "admpc_quad_clusters_keep: null ensemble"),
                        (lambda: lib.admpc_quad_kmeans_keep(None, -1, -1, *([None] * 11), None), "admpc_quad_kmeans_keep: null ensemble")):
        rc = call()
        assert rc == -1 and words in lib.admpc_last_error().decode(), (rc, lib.admpc_last_error())


def test_python_refusals_come_before_a_handle():
    from ad_mpc_amd.quad_ensemble_fleet import KMEANS_N_INIT_MAX, clusters_request, kmeans_request
    with pytest.raises(ValueError, match="needs a seed"):
        kmeans_request(None, n_init=0)
    for bad in (-1, 2 ** 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="seed must be a whole number"):
            kmeans_request(bad, n_init=0)
    for bad in (0, -2, 1.5, KMEANS_N_INIT_MAX + 1, True):
        with pytest.raises(ValueError, match="n_init must be in 1"):
            kmeans_request(3, n_init=bad, km_max_iter=0)
    for bad in (0, 1001, 2.5):
        with pytest.raises(ValueError, match="km_max_iter must be in 1 .. 1000"):
            kmeans_request(3, km_max_iter=bad, km_tol=-1.0)
    for bad in (-1e-9, np.nan, np.inf):
        with pytest.raises(ValueError, match="km_tol must be finite"):
            kmeans_request(3, km_tol=bad, resume=True)
    with pytest.raises(ValueError, match="resume=True goes on"):
        kmeans_request(3, resume=True)
    assert kmeans_request(0) == (0, 1, 300, 1e-4) and kmeans_request(np.int64(5), 3, 10, 0) == (5, 3, 10, 0.0)      # scikit-learn's defaults
    assert kmeans_request(2 ** 64 - 1)[0] == 2 ** 64 - 1
    assert clusters_request(2, [7], 5) == (100, 1e-3, 1e-6, None)                                # the EM's request is what it was


# ---- 2. the spec is scikit-learn's algorithm ------------------------------------------------------------------------------------------------

class Handout:
    """A random_state for _kmeans_plusplus that hands out the spec's uniforms: choice() the record of round 0, uniform() the trials of
    the next round."""

    def __init__(self, seed, draw):
        self.seed, self.draw, self.round = seed, draw, 0

    def choice(self, n, p=None):
        assert p is not None and np.allclose(p, 1.0 / n)
        u = KS.uniforms(self.seed, self.draw, 0, 1)[0]
        return min(int(math.floor(u * n)), n - 1)

    def uniform(self, size=None):
        self.round += 1
        return np.array(KS.uniforms(self.seed, self.draw, self.round, int(size)))


def test_the_uniforms_are_the_headers():
    """Philox4x32-10 under (round, draw, call, WORD): the known-answer vector of the generator, and the assignment of words to trials."""
    import quad_noise_spec as NS
    o = NS.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in o] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]                # Random123's kat_vectors, all zero
    u = KS.uniforms(11, 2, 3, 4)
    for j in range(2):
        o = NS.philox4x32_10((3, 2, j, KS.WORD), (11, 0))
        w = [int(o[0]) | int(o[1]) << 32, int(o[2]) | int(o[3]) << 32]
        assert u[2 * j:2 * j + 2] == [(float(v >> 11) + 0.5) * 2.0 ** -53 for v in w]
    assert KS.uniforms(11, 2, 3, 3) == u[:3] and all(0.0 < v < 1.0 for v in u) and KS.uniforms(2 ** 40 + 11, 2, 3, 4) != u
    assert [KS.trials(K) for K in range(1, 9)] == [2, 2, 3, 3, 3, 3, 3, 4]


@pytest.mark.parametrize("n,K,d,seed", CPU_CASES)
def test_spec_is_sklearns_kmeans(n, K, d, seed):
    """The seeded indices integer for integer, the labels and n_iter_ equal, the centres of scikit-learn within 1e-10, and the float64
    centres, inertia and tol_abs within the header's bounds of the longdouble run, which takes the same decisions."""
    from sklearn.cluster import KMeans
    from sklearn.cluster._kmeans import _kmeans_plusplus
    from sklearn.utils.extmath import row_norms
    rec = KS.cloud(n, K, d, seed)
    X = np.ascontiguousarray(rec[:, :d])
    lo, hi = (KS.fit(rec, KS.FEATS[d], K, seed=seed + 5, draw=seed, dtype=t) for t in (np.float64, LD))
    _, sk_idx = _kmeans_plusplus(X, K, row_norms(X, squared=True), np.ones(n), Handout(seed + 5, seed))
    assert lo["idx"].tolist() == sk_idx.tolist() == hi["idx"].tolist()
    km = KMeans(K, init=X[sk_idx], n_init=1, algorithm="lloyd").fit(X)
    assert lo["info"].tolist() == [km.n_iter_, lo["info"][1], 0, n] and lo["info"][1] in (1, 2)
    assert np.array_equal(lo["labels"], km.labels_)
    assert np.abs(lo["centers"] - km.cluster_centers_).max() <= 1e-10 and abs(float(lo["stats"][0]) - km.inertia_) <= 1e-10 * (1.0 + km.inertia_)
    assert abs(float(lo["stats"][1]) - 1e-4 * X.var(axis=0).mean()) <= 1e-14 * float(lo["stats"][1])
    # the yardstick
    assert hi["centers"].dtype == LD and hi["info"].tolist() == lo["info"].tolist() and np.array_equal(hi["labels"], lo["labels"])
    bc, bi, bt = KS.bounds(hi, K, d, 1e-4)
    print("n %d K %d d %d: margin %.1e, float64 against longdouble as fractions of the bounds: centres %.2f inertia %.2f tol_abs %.2f"
          % (n, K, d, lo["margin"], float((np.abs(lo["centers"] - hi["centers"]).max(axis=1) / bc).max()),
             abs(float(lo["stats"][0] - hi["stats"][0])) / bi, abs(float(lo["stats"][1] - hi["stats"][1])) / bt))
    assert (np.abs(lo["centers"] - hi["centers"]).max(axis=1) <= bc).all()
    assert abs(float(lo["stats"][0] - hi["stats"][0])) <= bi and abs(float(lo["stats"][1] - hi["stats"][1])) <= bt
    assert lo["margin"] >= 1e-9


# ---- 3. the cases of the GPU tests ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,d,seed", KS.GPU_CASES)
def test_gpu_cases_keep_the_margin(M, K, d, seed):
    """A condition on the inputs, not a measurement: no threshold within 1e-9 of the potential of a cumulative sum, no two candidate
    potentials and no two centre distances of a record that close.  The float64 and the longdouble run then take the same decisions,
    and so does a correct kernel."""
    rec = KS.gpu_case(M, K, d, seed)
    lo = KS.fit(rec, KS.FEATS[d], K, seed=seed, dtype=np.float64)
    assert lo["margin"] >= 1e-9, lo["margin"]
    assert lo["info"][2] == 0 and lo["info"][1] in (1, 2) and lo["info"][3] == int((CS.pack(rec, KS.FEATS[d])[:, 3] == 1.0).sum()) < M
    assert (lo["labels"][[0, M - 1]] == -1).all()
    if M <= 4097:
        hi = KS.fit(rec, KS.FEATS[d], K, seed=seed, dtype=LD)
        assert hi["info"].tolist() == lo["info"].tolist() and np.array_equal(hi["labels"], lo["labels"]) and hi["idx"].tolist() == lo["idx"].tolist()


def test_the_edge_case_draws_from_the_first_and_the_last_tile():
    rec = KS.edges()
    run = KS.fit(rec, [7], 3, seed=KS.EDGE_SEED)
    assert run["margin"] >= 1e-9 and run["info"][2] == 0
    assert run["idx"].min() < 256 and run["idx"].max() >= 256 * ((rec.shape[0] - 1) // 256)


@pytest.mark.parametrize("seed,status", KS.EMPTY_SEEDS)
def test_the_empty_cluster_cases_keep_the_margin(seed, status):
    """The second labelling pass leaves the cluster that was seeded at 10 empty, whichever index it has; the margin of the seeding and of
    both passes is 1e-9 or more, and the longdouble run decides the same."""
    rec = KS.empties()
    lo, hi = (KS.fit(rec, [7], 3, seed=seed, dtype=t) for t in (np.float64, LD))
    assert lo["info"].tolist() == hi["info"].tolist() == [1, 0, status, 23] and lo["margin"] >= 1e-9, (lo["info"], lo["margin"])
    assert lo["idx"].tolist() == hi["idx"].tolist() and sorted(np.round(rec[lo["idx"], 0]).tolist()) == [6.0, 10.0, 31.0]
    assert round(rec[lo["idx"][-status - 1], 0]) == 10 and lo["centers"] is None and (lo["stats"] == 0).all() and (lo["labels"] == -1).all()
    assert {st for _, st in KS.EMPTY_SEEDS} == {-1, -2, -3}
