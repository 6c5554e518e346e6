"""Learning the quadrotor's body-frame residual GPs (include/admpc_quad_learn.h) without a GPU: the header, the structs and the
prototype table; the refusals that need no device; the refusals of QuadFleet(learn=...) that come before a handle exists; and the
learning experiment in the numpy spec alone (tests/quad_learn_spec.py), with the real oracle as the model and tests/quad_plant_spec.py
as the plant."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import learn_spec as LS
import quad_learn_spec as QL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"admpc_quad_observe_latch_batch": 5, "admpc_quad_observe_batch": 12, "admpc_quad_gp_fit": 7, "admpc_quad_gp_install": 5,
         "admpc_quad_rollout_observe_batch": 27}


def _obs(learn=None, dt=0.02, substeps=1):
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, quad_learn_bins
    bins, n = quad_learn_bins(QL.EXP_LEARN if learn is None else learn)
    return AdmpcQuadObserveParams(dt=dt, substeps=substeps, n_gp=n, gp=bins)


def test_header_structs_and_library_agree():
    from ad_mpc_amd import _lib
    from ad_mpc_amd.config import AdmpcGp, AdmpcGpBins
    from ad_mpc_amd.quad_config import QUAD_GP_MAX, QUAD_REC, AdmpcQuadConfig, AdmpcQuadObserveParams
    raw = open(os.path.join(ROOT, "include", "admpc_quad_learn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decl = {n: len(p.split(",")) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_LEARN_EXPORTS, tuple) and list(_lib.QUAD_LEARN_EXPORTS) == list(ARITY)
    others = _lib.EXPORTS + _lib.QUAD_EXPORTS + _lib.FLEET_EXPORTS + _lib.LANE_EXPORTS + _lib.PLANT_EXPORTS + _lib.LEARN_EXPORTS + \
        _lib.HYPER_EXPORTS + _lib.QUAD_FLEET_EXPORTS
    assert not set(_lib.QUAD_LEARN_EXPORTS) & set(others)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    for name, n in ARITY.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == n and fn.restype is C.c_int, name
    # the struct as the header declares it: double dt; int32_t substeps, n_gp; AdmpcGpBins gp[ADMPC_QUAD_GP_MAX]
    body = re.search(r"typedef struct AdmpcQuadObserveParams \{(.*?)\} AdmpcQuadObserveParams;", txt, flags=re.S).group(1)
    assert [f.strip() for f in body.split(";") if f.strip()] == ["double  dt", "int32_t substeps, n_gp", "AdmpcGpBins gp[ADMPC_QUAD_GP_MAX]"]
    assert "400 bytes" in raw and C.sizeof(AdmpcQuadObserveParams) == 400 and C.sizeof(AdmpcGpBins) == 128 and QUAD_GP_MAX == 3 and QUAD_REC == 14
    P = AdmpcQuadObserveParams
    assert (P.dt.offset, P.substeps.offset, P.n_gp.offset, P.gp.offset) == (0, 8, 12, 16)
    assert AdmpcQuadConfig.gp.offset % 8 == 0 and C.sizeof(AdmpcGp) % 8 == 0          # the install copies 8-byte words
    for cite in ("gp_common.py:68-99", "gp_common.py:101-112", "model_fitting/gp.py", "point_tracking_and_record.py:215-265",
                 "quad_3d_optimizer.py:289-327"):
        assert cite in raw, cite
    for word in ("NOT offered", "search of the hyperparameters", "clustered GP ensembles", "random disturbances", "SQP mode", "velocity cap"):
        assert word in raw, word
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_learn\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_learn\.h", mk, flags=re.M)
    assert re.search(r"^HDRS\s*=.*\bquad_model_dev\.h", mk, flags=re.M)
    assert "The quadrotor is not touched" not in open(os.path.join(ROOT, "include", "admpc_learn.h")).read()


def test_refusals_in_front_of_the_device():
    """The refusals of the observe parameters in their stated order, and those of every entry that need no handle."""
    from ad_mpc_amd import _lib
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    L = _lib.load()

    def refused(rc, words):
        assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

    x = (C.c_double * 64)()
    i4 = (C.c_int32 * 4)()
    fit = lambda o, mc=1, b=x, g=x, i=i4: L.admpc_quad_gp_fit(0, None if o is None else C.byref(o), mc, b, g, i, None)
    refused(fit(None), "observe parameters are not set")
    for kw, words in ((dict(dt=0.0), "dt must be"), (dict(dt=float("inf")), "dt must be"), (dict(substeps=0), "substeps must be in [1, 64]"),
                      (dict(substeps=65), "substeps must be in [1, 64]"), (dict(n_gp=0), "n_gp must be in [1, 3]"), (dict(n_gp=4), "n_gp must be in [1, 3]")):
        o = _obs()
        for k, v in kw.items():
            setattr(o, k, v)
        refused(fit(o), words)
    o = _obs()
    o.dt, o.substeps, o.n_gp = -1.0, 0, 9                         # the order: dt, substeps, n_gp
    refused(fit(o), "dt must be")
    o.dt = 0.02
    refused(fit(o), "substeps")
    per_gp = (("n_feat", 0, "n_feat must be in [1, 3]"), ("feat", 6, "feat must be in [7, 16]"), ("feat", 17, "feat must be in [7, 16]"),
              ("out", 6, "out must be in [7, 9]"), ("out", 10, "out must be in [7, 9]"), ("nb", 33, "the product of nb"), ("nb", 0, "nb must be >= 1"),
              ("hi", -9.0, "lo and hi"), ("sigma_f", 0.0, "sigma_f must be"), ("length", 0.0, "length must be"), ("noise", 0.0, "noise must be"),
              ("count_noise", -1.0, "count_noise must not"))
    for field, value, words in per_gp:
        o = _obs()
        g = o.gp[1]
        if field in ("feat", "nb", "hi", "length"):
            getattr(g, field)[0] = value
        else:
            setattr(g, field, value)
        refused(fit(o), "regressor 1: " + words)
    o = _obs()
    o.gp[0].out, o.gp[0].noise, o.gp[0].feat[0] = 3, 0.0, 3       # the order within a regressor: feat, out, ..., noise
    refused(fit(o), "regressor 0: feat")
    o.gp[0].feat[0] = 7
    refused(fit(o), "regressor 0: out")
    o = _obs()
    refused(fit(o, mc=0), "min_count must be at least 1")
    refused(fit(o, b=None), "null array")
    o.dt = 0.0
    refused(fit(o, mc=0, b=None), "dt must be")                   # obs before min_count before the arrays

    refused(L.admpc_quad_observe_latch_batch(0, -1, x, x, None), "negative batch")
    assert L.admpc_quad_observe_latch_batch(0, 0, None, None, None) == 0
    refused(L.admpc_quad_observe_latch_batch(0, 1, None, x, None), "null array")

    plant, o = quad_plant_params(SimQuad(drag=True), 5e-4, 0.02), _obs()
    observe = lambda m, p, ob, B=1: L.admpc_quad_observe_batch(m, None if p is None else C.byref(p), None if ob is None else C.byref(ob), B, x, 4, x, x, x, x,
                                                               i4, None)
    refused(observe(None, None, None), "observe parameters are not set")
    refused(observe(None, None, o), "plant parameters are not set")
    bad = quad_plant_params(SimQuad(drag=True), 5e-4, 0.02)
    bad.u_min = 2.0
    refused(observe(None, bad, o), "u_min <= u_max")
    refused(observe(None, plant, o), "null model")
    refused(observe(None, plant, o, B=-1), "null model")

    refused(L.admpc_quad_gp_install(None, 1, x, i4, None), "null solver")
    roll = lambda ob, model=None: L.admpc_quad_rollout_observe_batch(None, None, C.byref(plant), 5, 1, 1, *([None] * 14), model,
                                                                     None if ob is None else C.byref(ob), None, None, None, None, None)
    refused(roll(None), "observe parameters are not set")
    refused(roll(o), "null model")


def test_learn_refusals_before_a_handle_exists():
    """Every ValueError of QuadFleet(learn=...) is raised on a machine without a GPU: before QuadBatchSolver is reached (which raises
    AdmpcError there)."""
    import torch
    from ad_mpc_amd.quad_config import quad_learn_bins
    from ad_mpc_amd.quad_fleet import QuadFleet
    good = dict(QL.EXP_LEARN[0])
    for change, words in ((dict(feat=6), "features in 7 .. 16, out in 7 .. 9"), (dict(feat=17), "features in 7 .. 16"), (dict(out=10), "out in 7 .. 9"),
                          (dict(out=3), "out in 7 .. 9"), (dict(bins=[33]), "bad bins"), (dict(hi=[-9.0]), "bad bins"), (dict(noise=0.0), "positive and finite"),
                          (dict(length_scale=[1.0, 2.0]), "one entry per feature")):
        with pytest.raises(ValueError, match=words):
            QuadFleet(4, learn=[dict(good, **change)])
    with pytest.raises(ValueError, match="1 to 3 regressors"):
        QuadFleet(4, learn=[good] * 4)
    with pytest.raises(ValueError, match="1 to 3 regressors"):
        QuadFleet(4, learn=[])
    with pytest.raises(ValueError, match="exclude each other"):
        QuadFleet(4, learn=[good], gp_regressors=[dict(feat=7, out=7, Z=[], alpha=[], length_scale=1.0)])
    with pytest.raises(ValueError, match="observe_substeps"):
        QuadFleet(4, learn=[good], observe_substeps=65)
    bins, n = quad_learn_bins([dict(good, feat=[7, 13, 16], lo=[-9, 0, 0], hi=[9, 1, 1], bins=[4, 2, 4], length_scale=[2.0, 0.5, 0.5])])
    assert n == 1 and list(bins[0].feat) == [7, 13, 16] and list(bins[0].nb) == [4, 2, 4] and len(bins) == 3
    # the car's ranges are untouched
    from ad_mpc_amd.config import learn_bins
    with pytest.raises(ValueError, match="features in 3 .. 8, out in 3 .. 5"):
        learn_bins([dict(good)])
    if not torch.cuda.is_available():
        from ad_mpc_amd._lib import AdmpcError
        with pytest.raises(AdmpcError):
            QuadFleet(4, learn=[good])


def test_the_spec_bins_as_the_car_spec_does():
    """quad_learn_spec.accumulate presents the quadrotor's record to learn_spec.accumulate; here it is held against a direct count."""
    rng = np.random.default_rng(3)
    learn = [dict(feat=[7, 12], out=8, lo=[-2.0, -1.0], hi=[2.0, 1.0], bins=[4, 4], length_scale=1.0), dict(feat=16, out=9, lo=[0.0], hi=[1.0], bins=[8], length_scale=1.0)]
    obs = _obs(learn)
    S = rng.uniform(-2.5, 2.5, (150, 14))
    S[:, 6:10] = rng.uniform(-0.1, 1.1, (150, 4))
    S[:, 13] = 1.0
    S[5, 13], S[77, 13], S[9, 0] = 0.0, 0.0, np.nan
    bins, dropped = np.zeros((3, 32, 5)), np.zeros(4, dtype=np.int32)
    QL.accumulate(obs, S, bins, dropped)
    ok = S[:, 13] == 1.0
    in0 = ok & (S[:, 0] >= -2) & (S[:, 0] < 2) & (S[:, 5] >= -1) & (S[:, 5] < 1)
    in1 = ok & (S[:, 9] >= 0) & (S[:, 9] < 1)
    assert dropped.tolist() == [int((ok & ~in0).sum()), int((ok & ~in1).sum()), 0, 2]
    assert bins[0, :, 0].sum() == in0.sum() and bins[1, :, 0].sum() == in1.sum() and not bins[2].any() and not bins[1, 8:].any()
    np.testing.assert_allclose(bins[0, :, 4].sum(), S[in0, 11].sum(), rtol=1e-13)
    np.testing.assert_allclose(bins[1, :, 4].sum(), S[in1, 12].sum(), rtol=1e-13)
    np.testing.assert_allclose(bins[0, :, 2].sum(), S[in0, 5].sum(), rtol=1e-13)
    QL.accumulate(obs, S, bins, dropped)                                      # a second call accumulates
    assert bins[0, :, 0].sum() == 2 * in0.sum() and dropped[3] == 4


@pytest.fixture(scope="module")
def quad_oracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


def test_the_learning_experiment_in_the_spec(quad_oracle):
    """512 periods of 20 ms of the drag plant (0.3 rotor drag, 0.08 aerodynamic drag) against the nominal model; one feature per
    regressor, its own body-frame velocity component, on 32 bins over [-9, 9); min_count 2.  Three conditions: at least 20 points per
    regressor; no sample outside the box; the residual of the held-out set falls to 0.15 of its size or below on every axis."""
    exp = QL.experiment(quad_oracle)
    n = [g["n_points"] for g in exp["gps"]]
    print("points per regressor %s, dropped %s, cond(K) %s" % (n, exp["dropped"].tolist(), ["%.3g" % c for c in exp["cond"]]))
    print("held-out RMS residual before %s, after %s m/s^2" % (np.array2string(exp["before_rms"], precision=4), np.array2string(exp["after_rms"], precision=4)))
    print("ratios %s" % np.array2string(exp["ratio"], precision=4))
    assert (exp["before"]["samples"][:, 13] == 1.0).all() and (exp["after"]["samples"][:, 13] == 1.0).all()
    assert min(n) >= 20 and [g["info"] for g in exp["gps"]] == n
    assert exp["dropped"].tolist() == [0, 0, 0, 0]
    assert (exp["bins"][:, :, 0].sum(axis=1) == QL.EXP_B).all()
    assert (exp["ratio"] <= 0.15).all(), exp["ratio"]
    assert max(exp["cond"]) < 1e6
    probes = np.linspace(-8.9, 8.9, 200)[:, None]
    _, _, obs = QL.experiment_params()
    yard = max(LS.yardstick(obs.gp[g], exp["bins"][g], probes, QL.EXP_MIN_COUNT) for g in range(3))
    print("longdouble yardstick of the three fits: %.3g" % yard)
    assert yard < 1e-9
