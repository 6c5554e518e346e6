"""The search of the quadrotor's GP hyperparameters (include/admpc_quad_hyper.h; ad_mpc_amd/learning.py, quad_fleet.py,
quad_ensemble_fleet.py) without a GPU: the header declares exactly the five entry points with the arities of the prototype table and
admpc_hyper.h still its two; the three older headers keep "search of the hyperparameters" under NOT offered and name this header there;
every refusal that stands in front of the first device call is reachable in the stated order and writes nothing; the numpy restatement
of the car's search (tests/hyper_spec.py, as it stands) mends the quadrotor's learning experiment (tests/quad_learn_spec.py) when the
length scale given to it is wrong.  The refusals of the ensemble entries behind a live ensemble are in tests/test_quad_hyper_gpu.py: an
ensemble cannot be created without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hyper_spec as HS
import learn_spec as LS
import quad_learn_spec as QL
from ad_mpc_amd import _lib
from ad_mpc_amd.config import AdmpcGpSearchParams, search_boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"admpc_quad_gp_search": 10, "admpc_quad_gp_refit": 8, "admpc_quad_ensemble_set_search": 2, "admpc_quad_ensemble_search": 8,
         "admpc_quad_ensemble_refit": 7}
BOX = dict(length_scale=(1e-2, 1e2), sigma_f=(1e-3, 1e2), noise=(1e-8, 1.0))        # the box of the car's experiment (tests/test_hyper_cpu.py)


def _declared(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return {fn: len(params.split(",")) for fn, params in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def quad_oracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


def _gp(feat=7, bins=8, out=7, lo=None, hi=None, **kw):
    rng = {7: (-4.0, 4.0), 8: (-4.0, 4.0), 9: (-6.0, 6.0), 12: (-1.5, 1.5), 13: (0.0, 1.0), 16: (0.0, 1.0)}
    feat = list(np.atleast_1d(feat))
    d = dict(feat=feat, out=out, lo=lo or [rng[f][0] for f in feat], hi=hi or [rng[f][1] for f in feat], bins=list(np.atleast_1d(bins)),
             length_scale=1.0, sigma_f=1.0, noise=1e-4, count_noise=0.0)
    d.update(kw)
    return d


def _obs(gps):
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, quad_learn_bins
    bins, n = quad_learn_bins(gps)
    return AdmpcQuadObserveParams(dt=0.02, substeps=1, n_gp=n, gp=bins)


def _params(gps, bounds=None, grid=5, rounds=10, shrink=0.5):
    return AdmpcGpSearchParams(grid=grid, rounds=rounds, shrink=shrink, box=search_boxes(gps, bounds))


# ---- the interface ------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_exactly_the_five_functions(lib):
    assert _declared("admpc_quad_hyper.h") == ARITY
    assert _declared("admpc_hyper.h") == {"admpc_gp_search": 10, "admpc_gp_refit": 8}             # the car's header keeps exactly its two
    assert isinstance(_lib.QUAD_HYPER_EXPORTS, tuple) and list(_lib.QUAD_HYPER_EXPORTS) == list(ARITY)
    # a register of its own, which load() walks; the existing ones are what they were
    assert list(_lib.HYPER_TABLES) == ["admpc_quad_hyper.h"] and tuple(_lib.HYPER_TABLES["admpc_quad_hyper.h"]) == _lib.QUAD_HYPER_EXPORTS
    assert len(_lib.TABLES) == 9 and list(_lib.CLUSTER_TABLES) == ["admpc_quad_clusters.h"] and list(_lib.ENSEMBLE_TABLES) == ["admpc_quad_ensemble.h"]
    others = {n for reg in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES) for t in reg.values() for n in t}
    assert not set(ARITY) & others
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n == len(_lib.HYPER_TABLES["admpc_quad_hyper.h"][name][1]) and fn.restype is C.c_int, name
    # the routed entries take the car's arguments with the quadrotor's parameter block in the second place
    for quad, car in (("admpc_quad_gp_search", "admpc_gp_search"), ("admpc_quad_gp_refit", "admpc_gp_refit")):
        q, c = getattr(lib, quad).argtypes, getattr(lib, car).argtypes
        assert list(q[:1]) + list(q[2:]) == list(c[:1]) + list(c[2:]) and q[1] is not c[1]
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_hyper.h")).read()
    for words in ("reference call site", "replaced by", "gp.py:278-316", "gp.py:318-323, 337-352", "gp.py:354-363", "gp_fitting.py", "NOT offered",
                  "BIT FOR BIT", "byte for byte", "4 KB", "by pointer", "SYNCHRONOUS"):
        assert words in hdr, words
    offered = hdr[hdr.index("NOT offered"):hdr.index("WHY THE ENSEMBLE")]
    for words in ("L-BFGS-B", "random restarts", "warm start", "K chosen", "SQP mode"):
        assert words in offered, words
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_hyper\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_hyper\.h", mk, flags=re.M)
    assert re.search(r"^HDRS\s*=.*\bgp_search_dev\.h", mk, flags=re.M) and re.search(r"^#\s+admpc_quad_hyper\.hip\s", mk, flags=re.M)


@pytest.mark.parametrize("name", ["admpc_quad_learn.h", "admpc_quad_ensemble.h", "admpc_quad_clusters.h"])
def test_the_older_headers_keep_the_phrase_and_point_here(name):
    hdr = open(os.path.join(ROOT, "include", name)).read()
    offered = hdr[hdr.index("NOT offered"):]
    item = offered[offered.index("search of the hyperparameters"):]
    item = re.split(r";\n|\.\n \*\n", item)[0]                                            # the item of the list that holds the phrase
    assert "by THESE entries" in item and "admpc_quad_hyper.h" in item, item
    assert "is not routed" not in hdr and "a later change can route it" not in hdr


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------

def test_host_side_refusals_need_no_device(lib):
    """The checks in front of the first device call, in the stated order; nothing is written.  The single-handle entries have the car's
    refusals behind the quadrotor's check of the observe parameters; of the ensemble entries the null ensemble comes first, whatever else
    is wrong with the call."""
    buf = (C.c_double * 64)(*([2.5] * 64))
    idx = (C.c_int32 * 8)(*([-7] * 8))
    bp, ip = C.cast(buf, C.c_void_p), C.cast(idx, C.c_void_p)
    one, three = [_gp()], [_gp([9, 13, 16], [4, 2, 4], out=9)]

    def search(obs, sp, min_count=1, resume=0, bins=bp, hyper=bp, nll=bp, info=ip):
        return lib.admpc_quad_gp_search(0, obs, sp, min_count, resume, bins, hyper, nll, info, None)

    def refused(rc, words):
        assert rc == -1 and words in lib.admpc_last_error().decode(), (rc, lib.admpc_last_error())

    ok_obs, ok = _obs(one), _params(one)
    bad_obs = _obs(one); bad_obs.dt = 0.0
    refused(search(None, None), "admpc_quad_gp_search: the observe parameters are not set")
    refused(search(C.byref(bad_obs), C.byref(_params(one, grid=4)), min_count=0), "admpc_quad_gp_search: dt must be")      # obs in front of everything else
    bad_obs = _obs(one); bad_obs.substeps = 65
    refused(search(C.byref(bad_obs), None), "admpc_quad_gp_search: substeps must be")
    # the quadrotor's ranges: the car's features and rows are refused here, as admpc_quad_learn.h refuses them
    for field, value, words in (("feat", 3, "regressor 0: feat"), ("feat", 17, "regressor 0: feat"), ("out", 3, "regressor 0: out"), ("out", 10, "regressor 0: out")):
        bad_obs = _obs(one)
        if field == "feat":
            bad_obs.gp[0].feat[0] = value
        else:
            bad_obs.gp[0].out = value
        refused(search(C.byref(bad_obs), None), words)
    bad_obs = _obs(one); bad_obs.n_gp = 4                                                  # ADMPC_QUAD_GP_MAX is 3
    refused(search(C.byref(bad_obs), None), "admpc_quad_gp_search: n_gp")
    bad_obs = _obs(one); bad_obs.gp[0].noise = 0.0                                         # (the given values are checked, though not read)
    refused(search(C.byref(bad_obs), C.byref(ok)), "admpc_quad_gp_search: regressor 0: noise must be")
    refused(search(C.byref(ok_obs), None), "admpc_quad_gp_search: the search parameters are not set")
    for grid in (1, 2, 4, 6, 8, 10, 11, -3):
        refused(search(C.byref(ok_obs), C.byref(_params(one, grid=grid, rounds=0))), "grid must be 3, 5, 7 or 9")
    for rounds in (0, 65, -1):
        refused(search(C.byref(ok_obs), C.byref(_params(one, rounds=rounds, shrink=1.0))), "rounds must be in [1, 64]")
    for shrink in (0.0, 1.0, -0.5, 1.5, np.nan, np.inf):
        sp = _params(one, shrink=shrink)
        sp.box[0].lo[0] = -1.0
        refused(search(C.byref(ok_obs), C.byref(sp)), "shrink must be in (0, 1)")
    for slot, lo, hi in ((0, 0.0, 1.0), (0, -1.0, 1.0), (3, 2.0, 1.0), (4, np.nan, 1.0), (4, 1e-3, np.inf), (3, np.inf, np.inf)):
        sp = _params(one)
        sp.box[0].lo[slot], sp.box[0].hi[slot] = lo, hi
        refused(search(C.byref(ok_obs), C.byref(sp), min_count=0), "regressor 0: slot %d of the box" % slot)
    sp = _params(one)                                                                      # the slots of unused features are not read
    sp.box[0].lo[1], sp.box[0].hi[2] = np.nan, -1.0
    refused(search(C.byref(ok_obs), C.byref(sp), min_count=0), "min_count must be at least 1")
    two = [_gp(), _gp(8, out=8)]
    sp = _params(two)
    sp.box[1].hi[4] = 0.0
    refused(search(C.byref(_obs(two)), C.byref(sp)), "regressor 1: slot 4 of the box")
    sp.box[1].lo[4] = 5.0                                                                  # of the boxes the first n_gp are read
    refused(search(C.byref(ok_obs), C.byref(sp), resume=2), "resume must be 0 or 1")
    # the candidate count: 5^5 and 7^4 pass, 7^5 does not; every regressor's slots in front of any count
    refused(search(C.byref(_obs(three)), C.byref(_params(three, grid=7)), min_count=0), "regressor 0: 16807 candidates per round, at most 4096")
    refused(search(C.byref(_obs(three)), C.byref(_params(three, grid=5)), min_count=0), "min_count must be at least 1")
    refused(search(C.byref(_obs(three)), C.byref(_params(three, [dict(noise=(1e-4, 1e-4))], grid=7)), min_count=0), "min_count must be at least 1")
    back = [_gp([9, 13, 16], [4, 2, 4], out=9), _gp()]
    sp = _params(back, grid=7)
    sp.box[1].lo[3] = 0.0
    refused(search(C.byref(_obs(back)), C.byref(sp)), "regressor 1: slot 3 of the box")
    # min_count, resume, the arrays
    refused(search(C.byref(ok_obs), C.byref(ok), min_count=0, resume=5), "admpc_quad_gp_search: min_count must be at least 1")
    refused(search(C.byref(ok_obs), C.byref(ok), resume=-1, bins=None), "admpc_quad_gp_search: resume must be 0 or 1")
    for kw in (dict(bins=None), dict(hyper=None), dict(nll=None), dict(info=None)):
        refused(search(C.byref(ok_obs), C.byref(ok), **kw), "admpc_quad_gp_search: null array")

    def refit(obs, min_count=1, bins=bp, hyper=bp, out=bp, info=ip):
        return lib.admpc_quad_gp_refit(0, obs, min_count, bins, hyper, out, info, None)

    refused(refit(None), "admpc_quad_gp_refit: the observe parameters are not set")
    refused(refit(C.byref(bad_obs), min_count=0), "admpc_quad_gp_refit: regressor 0: noise must be")
    refused(refit(C.byref(ok_obs), min_count=0, bins=None), "admpc_quad_gp_refit: min_count must be at least 1")
    for kw in (dict(bins=None), dict(hyper=None), dict(out=None), dict(info=None)):
        refused(refit(C.byref(ok_obs), **kw), "admpc_quad_gp_refit: null array")
    # the ensemble entries: the null ensemble in front of everything else
    refused(lib.admpc_quad_ensemble_set_search(None, None), "admpc_quad_ensemble_set_search: null ensemble")
    refused(lib.admpc_quad_ensemble_set_search(None, C.byref(_params(one, grid=4))), "admpc_quad_ensemble_set_search: null ensemble")
    refused(lib.admpc_quad_ensemble_search(None, 0, 2, None, bp, bp, ip, None), "admpc_quad_ensemble_search: null ensemble")
    refused(lib.admpc_quad_ensemble_refit(None, 0, None, bp, bp, ip, None), "admpc_quad_ensemble_refit: null ensemble")
    assert list(buf) == [2.5] * 64 and list(idx) == [-7] * 8


def test_python_refusals_need_no_device():
    """What the Python layer refuses of ``bounds`` before anything is sent: the shapes of the ensemble's three forms."""
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    fl = QuadEnsembleFleet.__new__(QuadEnsembleFleet)
    fl.K = 2
    assert fl._cluster_bounds(None) == [None, None]
    assert fl._cluster_bounds([BOX, {}]) == [[BOX, {}], [BOX, {}]]                          # one list per regressor: every cluster
    assert fl._cluster_bounds([[BOX], None]) == [[BOX], None]                               # one list per cluster
    for bad in ([[BOX]], [[BOX], [BOX], [BOX]], [[BOX], BOX], [3.0, [BOX]], []):
        with pytest.raises(ValueError, match="bounds"):
            fl._cluster_bounds(bad)


def test_a_quadfleet_that_learns_is_created_with_the_search():
    """QuadFleet(learn=...) creates a QuadLearningFleet, whose search_gp and learned_hyper are the car's own methods (learning.py's
    FleetSearch) keyed by the quadrotor's entries; QuadFleet itself and FleetLearning stay without them, as tests/test_learning_cpu.py
    holds.  The class is chosen before anything touches a device."""
    from ad_mpc_amd.fleet import FleetController
    from ad_mpc_amd.learning import FleetLearning, FleetSearch
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    from ad_mpc_amd.quad_fleet import QuadFleet, QuadLearningFleet
    for name in ("search_gp", "learned_hyper", "_head", "_fitted", "_alloc_learning"):
        assert getattr(QuadLearningFleet, name) is getattr(FleetController, name) is getattr(FleetSearch, name), name
    assert issubclass(QuadLearningFleet, QuadFleet) and issubclass(FleetSearch, FleetLearning)
    assert (FleetController._SEARCH, FleetController._REFIT) == ("admpc_gp_search", "admpc_gp_refit")
    assert (QuadLearningFleet._SEARCH, QuadLearningFleet._REFIT) == ("admpc_quad_gp_search", "admpc_quad_gp_refit")
    assert (QuadLearningFleet._FIT, QuadLearningFleet._INSTALL, QuadLearningFleet._EMPTY) == ("admpc_quad_gp_fit", "admpc_quad_gp_install", 7)
    learn = [_gp()]
    new = lambda cls, *a, **kw: type(cls.__new__(cls, *a, **kw))
    assert new(QuadFleet, 4, learn=learn) is QuadLearningFleet and new(QuadFleet, 4) is QuadFleet and new(QuadFleet, 4, learn=None) is QuadFleet
    assert new(QuadFleet, 4, None, 1.0, 10, None, None, 5e-4, 5, None, None, 0, learn) is QuadLearningFleet      # learn given by position
    assert new(QuadLearningFleet, 4) is QuadLearningFleet and new(QuadEnsembleFleet, 4, learn=[learn]) is QuadEnsembleFleet
    for name in ("search_gp", "learned_hyper", "learned_gps", "fit_gp"):
        assert name in vars(QuadEnsembleFleet), name                                        # the ensemble's own, over all clusters
    import inspect
    assert inspect.signature(QuadEnsembleFleet.search_gp) == inspect.signature(FleetSearch.search_gp)


# ---- the experiment with a wrong length scale -----------------------------------------------------------------------------------------

def test_the_search_mends_a_wrong_length_scale(quad_oracle):
    """The quadrotor's experiment of quad_learn_spec.py (512 periods of the drag plant, EXP_LEARN: a regressor per body axis on 32 bins)
    with every length scale given as 0.3 where 2.0 serves: RMS(y_after) / RMS(y_before) per axis on the held-out set after a fit at the
    given values, and after the spec's search (tests/hyper_spec.py as it stands, the car's box, 10 rounds of grid 5) and a fit at what it
    found.  Measured with the oracle: given 0.1688 / 0.1428 / 0.3033, searched 0.01055 / 0.01584 / 0.1201 (found lengths 3.62 / 6.32 /
    6.21), so searched / given = 0.0625 / 0.1109 / 0.3961; every axis improves.  Asserted with the car's margin, twice the measured
    value: searched < 0.125 / 0.222 / 0.792 of given.  (Given 0.1: 0.676 / 0.625 / 0.634; given 20: 0.153 / 0.146 / 0.268 -- the search
    does not read the given values and finds the same.)"""
    from ad_mpc_amd.quad_config import set_quad_gp
    exp = QL.experiment(quad_oracle)
    nominal, plant, obs = QL.experiment_params()
    box = search_boxes(QL.EXP_LEARN, [BOX] * 3)

    def ratio(Gs):
        gps = [LS.fit(G, exp["bins"][g], QL.EXP_MIN_COUNT) for g, G in enumerate(Gs)]
        learned = set_quad_gp(nominal.copy(), [QL.as_set_gp(G, gp) for G, gp in zip(Gs, gps)])
        a = exp["after"]
        S = np.stack([QL.record(quad_oracle, learned, plant, obs, a["X"][b], a["now"][b], a["U"][b])[0] for b in range(QL.EXP_B)])
        return QL.rms(S) / exp["before_rms"]

    given = [HS.with_hyper(obs.gp[g], [0.3, 1.0, 1.0, obs.gp[g].sigma_f, obs.gp[g].noise]) for g in range(3)]
    found, states = [], []
    for g in range(3):
        st, _ = HS.search(given[g], exp["bins"][g], list(box[g].lo), list(box[g].hi), min_count=QL.EXP_MIN_COUNT)
        states.append(st)
        found.append(HS.with_hyper(given[g], st[10:15]))
    rg, rs = ratio(given), ratio(found)
    print("ratios with length 0.3 given %s, searched %s, searched / given %s; found length, sigma_f, noise, NLL %s"
          % (np.array2string(rg, precision=4), np.array2string(rs, precision=4), np.array2string(rs / rg, precision=4),
             [["%.4g" % v for v in st[[10, 13, 14, 15]]] for st in states]))
    assert np.isfinite([st[15] for st in states]).all()
    assert (rs < np.array([0.125, 0.222, 0.792]) * rg).all(), (rs, rg)
