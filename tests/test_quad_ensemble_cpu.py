"""A clustered GP ensemble in the quadrotor's closed loop (include/admpc_quad_ensemble.h; ad_mpc_amd/quad_ensemble_fleet.py) without a
GPU: the header, the prototype table and the library agree; the refusals that need no handle come back in their order; the Python layer
refuses before a handle is asked for; the numpy spec (tests/quad_ensemble_spec.py) routes as QuadGPEnsemble.select_gp does and bins as
the masking identity says.  The refusals behind a live handle are in tests/test_quad_ensemble_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import quad_ensemble_spec as ES
import quad_learn_spec as QL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"admpc_quad_ensemble_create": 7, "admpc_quad_ensemble_destroy": 1, "admpc_quad_ensemble_route_batch": 5,
         "admpc_quad_ensemble_observe_batch": 12, "admpc_quad_ensemble_fit": 6, "admpc_quad_ensemble_install": 4,
         "admpc_quad_ensemble_rollout_batch": 30}
VX = lambda lo, hi, **kw: dict(dict(feat=7, out=7, lo=[lo], hi=[hi], bins=[32], length_scale=2.0, noise=1e-4), **kw)


@pytest.fixture(scope="module")
def lib():
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _blocks(learn, dt=0.02, substeps=1):
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, quad_learn_bins
    out = []
    for cluster in learn:
        bins, n = quad_learn_bins(cluster)
        out.append(AdmpcQuadObserveParams(dt=dt, substeps=substeps, n_gp=n, gp=bins))
    return out


# ---- 1. the header, the table and the library ---------------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from ad_mpc_amd import _lib, quad_ensemble_fleet
    from ad_mpc_amd.config import AdmpcGpBins
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_ensemble.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_ENSEMBLE_EXPORTS, tuple) and list(_lib.QUAD_ENSEMBLE_EXPORTS) == list(ARITY)
    # a third registry, which load() walks too; the two existing ones are what they were
    assert list(_lib.ENSEMBLE_TABLES) == ["admpc_quad_ensemble.h"] and tuple(_lib.ENSEMBLE_TABLES["admpc_quad_ensemble.h"]) == _lib.QUAD_ENSEMBLE_EXPORTS
    assert len(_lib.TABLES) == 9 and list(_lib.MORE_TABLES) == ["admpc_quad_noise.h"]
    others = {n for t in list(_lib.TABLES.values()) + list(_lib.MORE_TABLES.values()) for n in t}
    assert not set(_lib.QUAD_ENSEMBLE_EXPORTS) & others
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n and fn.restype is (None if name.endswith("destroy") else C.c_int), name
    assert C.sizeof(AdmpcQuadObserveParams) == 400 and C.sizeof(AdmpcGpBins) == 128
    assert re.search(r"#define\s+ADMPC_QUAD_CLUSTERS_MAX\s+8\b", hdr) and quad_ensemble_fleet.CLUSTERS_MAX == ES.CLUSTERS_MAX == 8
    # the rollout takes the plain rollout's arguments up to u_out, then route, route_out, the watch block without obs, noise, noise_step, stream
    roll, plain, noisy = (getattr(lib, n).argtypes for n in ("admpc_quad_ensemble_rollout_batch", "admpc_quad_rollout_batch", "admpc_quad_rollout_noise_batch"))
    assert list(roll[:20]) == list(plain[:20]) and list(roll[-3:]) == list(noisy[-3:])
    for cite in ("quad_3d_optimizer.py:207", "quad_3d_optimizer.py:485-491", "gp.py:738-770", "gp_fitting.py", "reference call site", "replaced by"):
        assert cite in hdr, cite
    offered = hdr[hdr.index("NOT offered"):]
    for words in ("GMM", "centroids are GIVEN", "search of the hyperparameters", "SQP mode"):
        assert words in offered, words
    for words in ("ONE ITERATE PER VEHICLE", "The reference keeps an iterate per solver", "device copy"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_ensemble\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_ensemble\.h", mk, flags=re.M)
    assert re.search(r"^HDRS\s*=.*\bquad_route_dev\.h", mk, flags=re.M) and re.search(r"^#\s+admpc_quad_ensemble\.hip\s", mk, flags=re.M)
    # the headers that said "not served" point here, and the phrase tests/test_quad_learn_cpu.py greps for stays
    for name in ("admpc_quad_fleet.h", "admpc_quad_learn.h"):
        other = open(os.path.join(ROOT, "include", name)).read()
        assert "admpc_quad_ensemble.h" in other and "clustered GP ensembles" in other, name


# ---- 2. the refusals that need no handle ----------------------------------------------------------------------------------------------

def test_refusals_without_a_handle_in_their_order(lib):
    """admpc_quad_ensemble_create up to its second rule, and the null ensemble that every other entry refuses first, whatever else
    is wrong with the call.  No device is touched (this machine has none)."""
    L = lib

    def refused(rc, words):
        assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

    feats = (C.c_int32 * 3)(7, 8, 9)
    cent = (C.c_double * 24)()
    out = C.c_void_p(0)
    nine = (C.c_void_p * 9)()
    create = lambda h=nine, K=2, nf=1, f=feats, c=cent, o=C.byref(out): L.admpc_quad_ensemble_create(h, K, nf, f, c, None, o)
    refused(create(h=None, K=0), "null argument")                                                # 1: a null before K
    refused(create(f=None, K=9), "null argument")
    refused(create(c=None), "null argument")
    refused(create(o=None), "null argument")
    for K in (0, -1, 9):
        refused(create(K=K, nf=0), "K must be in [1, 8]")                                        # 1 before 5
    refused(create(K=1, nf=0), "null solver")                                                    # 2 before 5
    refused(create(K=8, nf=4), "null solver")
    assert out.value is None
    L.admpc_quad_ensemble_destroy(None)                                                          # a no-op

    x = (C.c_double * 17)()
    r = (C.c_int32 * 1)()
    refused(L.admpc_quad_ensemble_route_batch(None, -1, None, None, None), "admpc_quad_ensemble_route_batch: null ensemble")
    refused(L.admpc_quad_ensemble_observe_batch(None, None, None, -1, None, 3, None, None, None, None, None, None),
            "admpc_quad_ensemble_observe_batch: null ensemble")
    refused(L.admpc_quad_ensemble_fit(None, 0, None, None, None, None), "admpc_quad_ensemble_fit: null ensemble")
    refused(L.admpc_quad_ensemble_install(None, None, None, None), "admpc_quad_ensemble_install: null ensemble")
    refused(L.admpc_quad_ensemble_rollout_batch(None, None, None, 0, -1, -1, *([None] * 23), None), "admpc_quad_ensemble_rollout_batch: null ensemble")
    assert x[0] == 0.0 and r[0] == 0


# ---- 3. the Python layer refuses before a handle is asked for -------------------------------------------------------------------------

def test_python_refusals_come_before_a_handle():
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet, ensemble_layout
    from ad_mpc_amd.quad_fleet import fleet_quad_config
    two = [[VX(0.0, 3.0)], [VX(2.0, 6.0, length_scale=1.0)]]
    cent = [[1.5], [4.0]]
    with pytest.raises(ValueError, match="agree in every regressor's feat and out"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=[[VX(0.0, 3.0)], [VX(2.0, 6.0, feat=8)]])
    with pytest.raises(ValueError, match="agree in every regressor's feat and out"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=[[VX(0.0, 3.0)], [VX(2.0, 6.0, out=8)]])
    with pytest.raises(ValueError, match="agree in every regressor's feat and out"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=[[VX(0.0, 3.0)], [VX(2.0, 6.0), VX(2.0, 6.0, feat=8, out=8)]])
    with pytest.raises(ValueError, match="features in 7 .. 16"):
        QuadEnsembleFleet(4, centroids=cent, feats=[2], learn=two)                               # a position: the sample record does not hold it
    with pytest.raises(ValueError, match="1 to 8 clusters"):
        QuadEnsembleFleet(4, centroids=np.arange(9.0)[:, None], feats=[7], learn=[[VX(0.0, 3.0)]] * 9)
    with pytest.raises(ValueError, match="1 to 8 clusters"):
        QuadEnsembleFleet(4, ensemble=QuadGPEnsemble([[]] * 9, np.arange(9.0)[:, None], [7]))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            QuadEnsembleFleet(4, centroids=[[1.5], [bad]], feats=[7], learn=two)
        with pytest.raises(ValueError, match="not finite"):
            QuadEnsembleFleet(4, ensemble=QuadGPEnsemble([[], []], [[1.5], [bad]], [7]))
    with pytest.raises(ValueError, match="one list of regressors per cluster"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=two[:1])
    with pytest.raises(ValueError, match="clustering features in 0 .. 16"):
        QuadEnsembleFleet(4, centroids=cent, feats=[17], learn=two)
    with pytest.raises(ValueError, match="K x len"):
        QuadEnsembleFleet(4, centroids=[[1.5, 0.0], [4.0, 0.0]], feats=[7], learn=two)
    with pytest.raises(ValueError, match="either ensemble"):
        QuadEnsembleFleet(4)
    with pytest.raises(ValueError, match="either ensemble"):
        QuadEnsembleFleet(4, ensemble=QuadGPEnsemble([[], []], cent, [7]), centroids=cent, feats=[7], learn=two)
    with pytest.raises(ValueError, match="observe_substeps"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=two, observe_substeps=65)
    with pytest.raises(ValueError, match="bad bins"):
        QuadEnsembleFleet(4, centroids=cent, feats=[7], learn=[[VX(0.0, 3.0)], [VX(6.0, 2.0)]])
    # the box, the bins and the hyperparameters may differ per cluster
    c, f, blocks = ensemble_layout(cent, 7, [[VX(0.0, 3.0)], [VX(2.0, 6.0, bins=[16], length_scale=0.5, noise=1e-3)]])
    assert c.shape == (2, 1) and f == [7] and [n for _, n in blocks] == [1, 1] and blocks[1][0][0].nb[0] == 16 and blocks[0][0][0].hi[0] == 3.0
    # the single-handle configuration goes on refusing K > 1, and says where to go
    with pytest.raises(NotImplementedError, match="clustered.*QuadEnsembleFleet"):
        fleet_quad_config(gp_regressors=QuadGPEnsemble([[], []], cent, [7]))


# ---- 4. the spec's routing ------------------------------------------------------------------------------------------------------------

def test_spec_routing_is_select_gp_and_ties_go_to_the_lower_index():
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    rng = np.random.default_rng(3)
    hit = set()
    for feats, K in (([7], 3), ([7, 13], 4), ([8, 11, 16], 8), ([0, 9], 2)):
        cent = rng.normal(size=(K, len(feats))) * 2.0
        ens = QuadGPEnsemble([[]] * K, cent, feats)
        for _ in range(200):
            row = rng.normal(size=17) * 2.0
            row[3:7] /= np.linalg.norm(row[3:7])
            z = ES.z_of_row(row)
            assert ES.margin(z[feats], cent) >= 1e-9                                             # far from a tie: the two orders of summation agree on the winner
            got = ES.nearest(z[feats], cent)
            assert got == ens.select_gp(z) == ES.route_window(np.tile(row, (1, 3, 1)), feats, cent)[0]
            hit.add((K, got))
    assert {k for K, k in hit if K == 3} == {0, 1, 2}
    # constructed ties, on exactly representable numbers: the lower index
    level = np.zeros(17); level[3] = 1.0
    assert ES.nearest([0.0], np.array([[1.0], [-1.0]])) == 0 and ES.nearest([0.0], np.array([[-1.0], [1.0]])) == 0
    assert ES.nearest([0.0], np.array([[2.0], [-1.0], [1.0]])) == 1
    assert ES.route_window(level[None, None, :], [7], np.array([[1.0], [-1.0]]))[0] == 0 and ES.margin([0.0], np.array([[1.0], [-1.0]])) == 0.0
    row = level.copy(); row[7], row[13] = -0.25, 0.375                                           # the tie of tests/test_quad_gpu.py
    assert ES.route_window(row[None, None, :], [7, 13], np.array([[0.5, 0.5], [-1.0, 0.25], [2.0, 0.75]]))[0] == 0
    # a feature that is not finite: cluster 0, where numpy.argmin of NaN distances points too
    for bad in (np.nan, np.inf, -np.inf):
        assert ES.nearest([bad], np.array([[5.0], [0.0]])) == 0
    # the body-frame rotation acts: a quarter turn about z carries the world's v_y into the body's v_x
    turned = np.zeros(17); turned[3], turned[6], turned[8] = np.sqrt(0.5), np.sqrt(0.5), 3.0
    assert abs(ES.z_of_row(turned)[7] - 3.0) < 1e-15 and ES.route_window(turned[None, None, :], [7], np.array([[0.0], [3.0]]))[0] == 1
    # the record's own features: feature f reads entry f - 7
    rec = np.zeros((2, 14)); rec[0, 0], rec[1, 6] = 2.9, 0.9
    assert ES.route_records(rec, [7], np.array([[0.0], [3.0]])).tolist() == [1, 0] and ES.route_records(rec, [13], np.array([[0.0], [1.0]])).tolist() == [0, 1]


# ---- 5. the spec's cluster binning ----------------------------------------------------------------------------------------------------

def test_spec_cluster_binning_is_the_masking_identity():
    """Hand-made records, 200 of them (more than three rounds of the 64 lanes), two accumulating calls: the spec written from the contract
    equals, bit for bit, quad_learn_spec.accumulate under each cluster's block of the records with the other clusters' flags cleared."""
    rng = np.random.default_rng(8)
    learn = [[VX(-1.0, 2.5), dict(feat=[8, 12], out=8, lo=[-4.0, -1.5], hi=[4.0, 1.5], bins=[8, 4], length_scale=[2.0, 1.0])],
             [VX(2.0, 4.5, bins=[16]), dict(feat=[8, 12], out=8, lo=[-2.0, -1.0], hi=[2.0, 1.0], bins=[4, 8], length_scale=[1.0, 1.0])],
             [VX(4.0, 7.0, bins=[8]), dict(feat=[8, 12], out=8, lo=[-4.0, -1.5], hi=[4.0, 1.5], bins=[2, 2], length_scale=[2.0, 1.0])]]
    blocks, feats, cent = _blocks(learn), [7], np.array([[1.0], [3.25], [5.5]])
    bins, dropped = np.zeros((3, 3, 32, 5)), np.zeros((3, 4), dtype=np.int32)
    wb, wd = bins.copy(), dropped.copy()
    total = 0
    for call in range(2):
        S = rng.normal(size=(200, 14)) * 1.5
        S[:, 0] = rng.uniform(-1.5, 7.5, 200)
        S[:, 13] = 1.0
        S[[3, 77, 130], 13] = 0.0                                                                # not valid, one of them far out as well
        S[77, 0] = 100.0
        route = ES.route_records(S, feats, cent)
        assert min(ES.margin(r[[0]], cent) for r in S) >= 1e-9 and set(route.tolist()) == {0, 1, 2}
        ES.accumulate(blocks, feats, cent, S, bins, dropped)
        ES.accumulate_masked(blocks, feats, cent, S, wb, wd)
        total += 200
        assert np.array_equal(bins.view(np.uint64), wb.view(np.uint64)) and np.array_equal(dropped, wd), call
    assert dropped[0, 3] == 6 and not dropped[1:, 3].any() and not bins[:, 2].any() and not dropped[:, 2].any()
    for g in range(2):                                                                           # every record exactly once per regressor
        assert bins[:, g, :, 0].sum() + dropped[:, g].sum() + dropped[0, 3] == total
    assert (bins[:, 0, :, 0].sum(axis=1) > 40).all() and (dropped[:, :2] > 0).any()
