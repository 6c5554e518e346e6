"""The evaluation of the learned GPs on a flight log (include/admpc_quad_eval.h; ad_mpc_amd/quad_ensemble_fleet.py) without a GPU: the
header, the prototype table, the Makefile and the library agree; the refusals that need no device come back under the entry's name; the
Python layer refuses before a handle is asked for; and the numpy spec (tests/quad_eval_spec.py), which the GPU tests hold the kernels
against, is pinned to the reference's own CustomGPRegression.predict and GPEnsemble.select_gp through
tests/golden/quad_eval_vectors.json (tests/gen_quad_eval_golden.py writes it where the reference tree is present, and is run live there).

THE BOUNDS (u = 2^-53; `_bounds` below).  They are forward bounds, not measured tolerances.
  mean    mu = ymean + sum_i k_i alpha_i is a sum of n + 1 terms.  Computed in any order from the SAME k and alpha it is off by at most
          n u (|ymean| + sum |k_i alpha_i|) to first order; a k_i carries the rounding of its exponent and of exp (a few u, relative),
          which makes each term off by a further (3 + 5) u or so.  Doubled for the second-order terms and for the side it is compared
          with: 4 (n + 8) u (|ymean| + sum |k_i alpha_i|).  This is the bound where both sides read the same alpha -- the device against
          the spec evaluated from the device's own factor (tests/test_quad_eval_gpu.py).
          Where the two sides SOLVE for alpha on their own -- the reference through inv(K), the spec through a Cholesky factor, in
          float64 or in longdouble -- each alpha is off by up to c u cond_2(K) |alpha|_2 (the backward stability of the solve), and the
          dot product with k by |k|_2 times that.  With the constant of the variance bound: + 64 u cond_2(K) |k|_2 |alpha|_2.
          Measured worst ratio to this bound: 0.034 (float64 spec against the reference), 0.024 (longdouble); without the second term
          the reference misses the first by a factor 5.9, its alpha being inv(K) y.
  std^2   var = k_ss - k' K^-1 k through an explicit inverse (the reference's inv(K), here W'W with W = L^-1): the inverse is off by
          c u cond_2(K) relative, the quadratic form is at most k_ss = sigma_f + 1e-8 (the posterior variance is not negative), so
          64 u cond_2(K) (sigma_f + 1e-8).  Measured worst ratio: 0.073.
The fixtures keep 64 u cond_2(K) <= 1e-6 and have no clipped variance: with sigma_f = 0.5, sigma_n = 0.01 and n <= 32 the condition
number is at most n sigma_f / sigma_n^2 = 1.6e5 (measured: 1.18e5)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import quad_ensemble_spec as ES
import quad_eval_spec as EV
import quad_learn_spec as QL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "quad_eval_vectors.json")
ARITY = {"admpc_quad_ensemble_factor": 7, "admpc_quad_ensemble_evaluate": 11}
EINVAL = -1
U, LD = EV.U, np.longdouble


@pytest.fixture(scope="module")
def lib():
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def last(lib):
    return lib.admpc_last_error().decode()


def _bounds(n, ymean, absdot, cond, knorm=None, sigma_f=EV.SIGMA_F):
    """(the bound of the mean, the bound of std^2) of the module's docstring; knorm: |k|_2 |alpha|_2 where the sides solve on their own."""
    mean = 4.0 * (n + 8) * U * (abs(ymean) + absdot)
    if knorm is not None:
        mean = mean + 64.0 * U * cond * knorm
    return mean, 64.0 * U * cond * (sigma_f + EV.JITTER)


# ---- 1. the header, the table, the Makefile and the library ------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from ad_mpc_amd import _lib, quad_ensemble_fleet as F
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_eval.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_EVAL_EXPORTS, tuple) and list(_lib.QUAD_EVAL_EXPORTS) == list(ARITY)
    assert list(_lib.EVAL_TABLES) == ["admpc_quad_eval.h"] and tuple(_lib.EVAL_TABLES["admpc_quad_eval.h"]) == _lib.QUAD_EVAL_EXPORTS
    known = [t for group in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES, _lib.TARGET_TABLES,
                             _lib.PRUNE_TABLES) for t in group.values()]
    assert len(known) == 15 and not set(ARITY) & {n for t in known for n in t}
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n == len(_lib.EVAL_TABLES["admpc_quad_eval.h"][name][1]) and fn.restype is C.c_int, name
    for name, val, py, spec in (("ADMPC_EVAL_FACTOR", "672", F.EVAL_FACTOR, EV.FACTOR), ("ADMPC_EVAL_STATS", "8", F.EVAL_STATS, EV.STATS),
                                ("ADMPC_EVAL_ENOVALID", r"\(-100\)", F.EVAL_ENOVALID, EV.ENOVALID)):
        assert re.search(r"#define\s+%s\s+%s" % (name, val), hdr), name
        assert py == int(val.strip("\\()")) == spec, name
    assert EV.F_W + 32 * 33 // 2 == EV.FACTOR
    for cite in ("gp_fitting.py:304-311, 314-348", "gp_visualization.py:74-93", "gp.py:632-736", "gp.py:738-770", "gp.py:403-444", "gp.py:361-363",
                 "reference call site", "replaced by"):
        assert cite in hdr, cite
    offered = hdr[hdr.index("NOT offered"):]
    for words in ("NaN standard deviation", "CLIPPED", "NotImplementedError", "sample_y", "distance_maximizing_points", "QuadFleet", "the car"):
        assert words in offered, words
    for words in ("THE FACTOR", "WHICH RECORDS TAKE PART", "PER RECORD", "THE STATISTICS", "DETERMINISM", "No floating-point atomics",
                  "function of M alone", "THE KERNEL", "v_mfma_f64_16x16x4_f64", "Measured on one MI355X"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_eval\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_eval\.h", mk, flags=re.M)
    assert re.search(r"^#\s+admpc_quad_eval\.hip\s", mk, flags=re.M)
    # the headers that spoke of evaluation as missing point here
    for other in ("admpc_quad_learn.h", "admpc_quad_hyper.h", "admpc_quad_prune.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "admpc_quad_eval.h" in text[text.index("NOT offered"):], other


# ---- 2. the refusals that need no device, and the Python layer -------------------------------------------------------------------------------

def test_null_ensemble_is_refused_first(lib):
    one = C.c_void_p(8)                                  # never dereferenced: the call is refused
    assert lib.admpc_quad_ensemble_factor(None, 0, None, None, None, None, None) == EINVAL
    assert last(lib) == "admpc_quad_ensemble_factor: null ensemble"
    assert lib.admpc_quad_ensemble_factor(None, 1, one, one, one, one, None) == EINVAL and "null ensemble" in last(lib)
    assert lib.admpc_quad_ensemble_evaluate(None, -1, None, 5, None, None, None, None, None, None, None) == EINVAL
    assert last(lib) == "admpc_quad_ensemble_evaluate: null ensemble"
    assert lib.admpc_quad_ensemble_evaluate(None, 0, None, 0, None, None, None, None, None, None, None) == EINVAL      # in front of the M == 0 no-op


def test_python_layer_refuses_without_a_gpu():
    from ad_mpc_amd import quad_ensemble_fleet as F
    assert F.eval_request(60, 60, True) == (0, False, False)
    assert F.eval_request(60, 1, True, True, True, True, True) == (1, True, True)
    for kw, words in ((dict(log_steps=0, steps=0, has_factor=True), "keeps no log"), (dict(log_steps=60, steps=0, has_factor=True), "the log is empty"),
                      (dict(log_steps=60, steps=3, has_factor=False), "no factor yet"),
                      (dict(log_steps=60, steps=3, has_factor=True, drag=True, has_rdrv=False), "fit_rdrv"),
                      (dict(log_steps=60, steps=3, has_factor=True, include_pruned=2), "include_pruned"),
                      (dict(log_steps=60, steps=3, has_factor=True, per_record="yes"), "per_record")):
        with pytest.raises(ValueError, match=words):
            F.eval_request(**kw)
    # the order: no log, an empty log, no factor, no drag
    with pytest.raises(ValueError, match="keeps no log"):
        F.eval_request(0, 0, False, drag=True)
    with pytest.raises(ValueError, match="the log is empty"):
        F.eval_request(5, 0, False, drag=True)
    with pytest.raises(ValueError, match="no factor yet"):
        F.eval_request(5, 2, False, drag=True)
    # the table of an evaluation from its sums
    s = np.zeros((2, 3, 8))
    s[0, 0] = [4, 8.0, 36.0, 2.0, 4.0, 1.0, 3, 1]
    s[1, 0] = [12, 8.0, 12.0, 6.0, 12.0, 3.0, 12, 0]
    e = F.evaluation_table(s, 2)
    assert e.count.tolist() == [[4, 0], [12, 0]] and e.nominal_mae[0, 0] == 2.0 and e.augmented_mae[0, 0] == 0.5 and e.nominal_rms[0, 0] == 3.0
    assert e.augmented_rms[1, 0] == 1.0 and e.mean_std[:, 0].tolist() == [0.25, 0.25] and e.within_3std[:, 0].tolist() == [0.75, 1.0]
    assert e.clipped.tolist() == [[1, 0], [0, 0]] and np.isnan(e.nominal_mae[:, 1]).all()
    assert e.total.count.tolist() == [16, 0] and e.total.nominal_mae[0] == 1.0 and e.total.augmented_rms[0] == 1.0 and e.total.total is None
    v = F.evaluation_table(s, 2, dt=0.02)
    assert v.nominal_mae[0, 0] == 0.04 and v.within_3std[0, 0] == 0.75 and v.mean_std[0, 0] == 0.005 and v.total.augmented_rms[0] == 0.02


# ---- 3. the spec against the reference (through the golden file) --------------------------------------------------------------------------------

def test_golden_file_is_what_the_spec_lists(golden):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert [(c["seed"], c["n_feat"], c["n"], c["K"]) for c in golden] == [tuple(c) for c in EV.GOLDEN_CASES]
    assert all(set(c) == {"seed", "n_feat", "n", "K", "sigma_f", "sigma_n", "idx", "mu", "std"} and len(c["mu"]) == EV.QUERIES for c in golden)
    assert {c["n_feat"] for c in golden} == {1, 2, 3} and {c["n"] for c in golden} == {1, 2, 31, 32} and {c["K"] for c in golden} == {1, 3}
    assert len(golden) >= 16 and all(c["sigma_f"] == EV.SIGMA_F and c["sigma_n"] == EV.SIGMA_N for c in golden)
    assert all(np.isfinite(c["std"]).all() for c in golden)          # the reference took no root of a negative variance here


def _against(golden, dtype):
    """The spec in `dtype` against the golden file: the worst ratios (mean, std^2) to their bounds, and the share of excluded routes."""
    worst_mean = worst_var = 0.0
    excluded = total = 0
    for c in golden:
        feats, cent, clusters, z = EV.golden_fixture(c["seed"], c["n_feat"], c["n"], c["K"])
        factors = EV.golden_factors(clusters, feats, dtype)
        S = np.zeros((len(z), EV.REC))
        S[:, :c["n_feat"]], S[:, 13] = z, 1.0
        ev = EV.evaluate(S, feats, cent, factors, dtype=dtype)
        # the condition on the fixtures, on the spec alone
        assert all(64.0 * U * f[0]["cond"] <= 1e-6 and f[0]["info"] == c["n"] for f in factors) and not ev["clipped"].any() and ev["part"].all()
        ok = ev["gap"] >= 1e-9
        excluded, total = excluded + int((~ok).sum()), total + len(z)
        assert np.array_equal(ev["route"][ok], np.array(c["idx"])[ok]), c["seed"]
        assert np.array_equal(ev["route"][:40], ES.route_records(S[:40], feats, cent))       # the vectorised routing is the ensemble spec's
        for k in range(c["K"]):
            at = ok & (np.array(c["idx"]) == k)
            f = factors[k][0]
            bm, bv = _bounds(f["n"], f["ymean"], ev["absdot"][at, 0], f["cond"], ev["knorm"][at, 0])
            em = np.abs(ev["mu"][at, 0] - np.array(c["mu"], dtype=dtype)[at])
            evar = np.abs(ev["var"][at, 0] - np.array(c["std"], dtype=dtype)[at] ** 2)
            assert (em <= bm).all() and (evar <= bv).all(), (c["seed"], k, float((em / bm).max()), float((evar / bv).max()))
            if at.any():
                worst_mean, worst_var = max(worst_mean, float((em / bm).max())), max(worst_var, float((evar / bv).max()))
    assert excluded <= 0.01 * total
    return worst_mean, worst_var, excluded / total


def test_spec_predicts_what_the_reference_predicts(golden):
    wm, wv, share = _against(golden, np.float64)
    print("float64 spec against the reference: worst ratio to the bound, mean %.3g, std^2 %.3g; excluded routes %.4f" % (wm, wv, share))
    wm, wv, share = _against(golden, LD)
    print("longdouble spec against the reference: mean %.3g, std^2 %.3g" % (wm, wv))


def test_golden_is_what_the_reference_gives_now(golden):
    """Where the reference tree is present: its functions, taken live, give the committed file."""
    import gen_quad_eval_golden as G
    if not G.reference_present():
        pytest.skip("no reference tree on this machine: tests/golden/quad_eval_vectors.json stands in")
    ref = G.load_reference()
    for c in golden:
        idx, mu, std = G.run_case(ref, c["seed"], c["n_feat"], c["n"], c["K"])
        assert idx == c["idx"] and mu == c["mu"] and std == c["std"], c["seed"]


# ---- 4. the spec in float64 against the spec in longdouble ------------------------------------------------------------------------------------

def _blocks(K, n_feat, n_gp=3, bins=32, noise=1e-4, count_noise=0.0, sigma_f=None):
    """K observe blocks of n_gp regressors on features 7 .. 7 + n_feat - 1, `bins` bins along the first feature."""
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, quad_learn_bins
    feats = [7, 8, 9][:n_feat]
    obs = []
    for c in range(K):
        learn = [dict(feat=feats, out=7 + g, lo=[-9.0] * n_feat, hi=[9.0] * n_feat, bins=[bins] + [1] * (n_feat - 1),
                      length_scale=[1.5 + 0.25 * c + 0.1 * g] * n_feat, sigma_f=0.5 + 0.1 * g if sigma_f is None else sigma_f, noise=noise, count_noise=count_noise) for g in range(n_gp)]
        b, n = quad_learn_bins(learn)
        obs.append(AdmpcQuadObserveParams(dt=0.02, substeps=1, n_gp=n, gp=b))
    return feats, obs


def _log(M, seed, K=3, dirty=True):
    """Records with v_b in the boxes of _blocks, y a smooth function of it plus noise; with `dirty` all three flag values, a fourth, and
    entries that are not finite."""
    rng = np.random.default_rng(seed)
    S = rng.uniform(-8.5, 8.5, (M, EV.REC))
    S[:, 10:13] = np.sin(S[:, 0:3]) - 0.3 * S[:, 0:3] + 0.05 * rng.standard_normal((M, 3))
    S[:, 13] = 1.0
    if dirty and M >= 8:
        S[::7, 13], S[3::11, 13], S[5::13, 13] = 0.0, EV.PRUNED, 3.0
        S[2::17, rng.integers(0, 13)] = np.nan
        S[4::19, 11] = np.inf
    return S


def _fixture(K=3, n_feat=1, seed=1, M=600, count_noise=0.0):
    feats, obs = _blocks(K, n_feat, count_noise=count_noise)
    cent = np.linspace(-5.0, 5.0, K).reshape(K, 1) * np.ones((1, n_feat)) if K > 1 else np.zeros((1, n_feat))
    S = _log(M, seed)
    bins, dropped = np.zeros((K, 3, 32, 5)), np.zeros((K, 4), dtype=np.int32)
    ES.accumulate_masked(obs, feats, cent, _log(M, seed + 100, dirty=False), bins, dropped)      # fitted to one flight, evaluated on another
    return feats, obs, cent, S, bins


def test_float64_spec_is_the_longdouble_spec_within_the_bounds():
    worst = [0.0, 0.0]
    for K, n_feat, seed in ((1, 1, 1), (3, 1, 2), (3, 2, 3), (2, 3, 4)):
        feats, obs, cent, S, bins = _fixture(K, n_feat, seed, count_noise=1e-3)
        fs = {dt: [[EV.factor_from_bins(obs[c].gp[g], bins[c, g], 1, None, dt) for g in range(3)] for c in range(K)] for dt in (np.float64, LD)}
        a, b = EV.evaluate(S, feats, cent, fs[np.float64]), EV.evaluate(S, feats, cent, fs[LD], dtype=LD)
        assert np.array_equal(a["route"], b["route"]) and np.array_equal(a["info"], b["info"]) and a["info"][1] > 300 and a["info"][2] > 0 < a["info"][3]
        for c in range(K):
            for g in range(3):
                f = fs[LD][c][g]
                at = a["part"] & (a["route"] == c)
                assert f["n"] == fs[np.float64][c][g]["n"] > 0 and 64.0 * U * f["cond"] <= 1e-6
                bm, bv = _bounds(f["n"], f["ymean"], b["absdot"][at, g], f["cond"], b["knorm"][at, g], float(f["sigma_f"]))
                em, evar = np.abs(a["mu"][at, g] - b["mu"][at, g]), np.abs(a["var"][at, g] - b["var"][at, g])
                assert (em <= bm).all() and (evar <= bv).all(), (K, n_feat, c, g)
                worst = [max(worst[0], float((em / bm).max())), max(worst[1], float((evar / bv).max()))]
        # the sums: M u sum |terms| and the summed per-record bounds are far above what float64 loses here; the counts are exact
        assert np.array_equal(a["stats"][..., [0, 6, 7]], b["stats"][..., [0, 6, 7]].astype(np.float64)) or (b["margin"][a["part"]] < 1e-9).any()
    print("float64 against longdouble: worst ratio to the bound, mean %.3g, std^2 %.3g" % tuple(worst))


# ---- 5. the empty factor, a failed pivot, take_pruned, the drag term, the statistics --------------------------------------------------------

def test_empty_factor_failed_pivot_and_no_optimum():
    feats, obs, cent, S, bins = _fixture(1, 1, 5)
    G = obs[0].gp[0]
    empty = EV.factor_from_bins(G, np.zeros((32, 5)), 1)
    assert empty["n"] == 0 and empty["info"] == 0 and empty["ymean"] == 0.0
    mu, var, absdot, _ = EV.predict(empty, S[:50, 0:1])
    assert (mu == 0.0).all() and (var == G.sigma_f + EV.JITTER).all() and not absdot.any()
    assert EV.factor_from_bins(G, bins[0, 0], 10 ** 6)["n"] == 0                     # no bin has that many samples
    # a failed pivot: two bins with the same mean under sigma_f = 1 and a noise that 1 swallows make the second pivot exactly 0
    _, obs0 = _blocks(1, 1, noise=1e-300, sigma_f=1.0)
    twin = np.zeros((32, 5))
    twin[3], twin[9] = [2.0, 1.0, 0.0, 0.0, 0.4], [4.0, 2.0, 0.0, 0.0, 0.9]
    failed = EV.factor_from_bins(obs0[0].gp[0], twin, 1)
    assert failed["n"] == 0 and failed["info"] == -2 and failed["W"].size == 0
    nan_target = bins[0, 0].copy()
    nan_target[np.nonzero(nan_target[:, 0])[0][2], 4] = np.nan
    assert EV.factor_from_bins(G, nan_target, 1)["info"] == -3
    # a search without an optimum; and one with: the hyperparameters are the search's
    hy = np.zeros(16)
    hy[10:15], hy[15] = [0.7, 1.0, 1.0, 0.8, 1e-3], np.inf
    none = EV.factor_from_bins(G, bins[0, 0], 1, hy)
    assert none["n"] == 0 and none["info"] == EV.NO_OPTIMUM and none["sigma_f"] == 0.8
    hy[15] = 12.5
    found = EV.factor_from_bins(G, bins[0, 0], 1, hy)
    assert found["n"] > 20 and found["sigma_f"] == 0.8 and found["inv_l2"][0] == 1.0 / (0.7 * 0.7) and found["inv_l2"][1] == 0.0
    # W is the inverse of L, and the packed block round-trips
    assert np.abs(found["W"] @ found["L"] - np.eye(found["n"])).max() <= 64.0 * U * found["cond"]
    back = EV.unpack(EV.pack(found))
    assert all(np.array_equal(back[k], found[k]) for k in ("Z", "alpha", "W", "inv_l2")) and back["n"] == found["n"] and back["out"] == found["out"]
    # every record of an evaluation under empty factors has r = y
    ev = EV.evaluate(S, feats, cent, [[empty] * 3])
    p = ev["part"]
    assert np.array_equal(ev["res"][p], ev["y"][p]) and np.array_equal(ev["stats"][0, :, 1], ev["stats"][0, :, 3]) and ev["stats"][0, 0, 6] < p.sum()


def test_take_pruned_the_drag_term_and_the_statistics():
    feats, obs, cent, S, bins = _fixture(3, 1, 6)
    fs = [[EV.factor_from_bins(obs[c].gp[g], bins[c, g], 1) for g in range(3)] for c in range(3)]
    kept, whole = EV.evaluate(S, feats, cent, fs, 0), EV.evaluate(S, feats, cent, fs, 1)
    pruned = (S[:, 13] == EV.PRUNED) & np.isfinite(S[:, :13]).all(axis=1)
    assert pruned.sum() > 10 and np.array_equal(whole["part"], kept["part"] | pruned) and not (kept["part"] & pruned).any()
    assert whole["info"][1] == kept["info"][1] + pruned.sum() and whole["info"][2] == kept["info"][2] - (S[:, 13] == EV.PRUNED).sum()
    assert kept["info"].sum() - kept["info"][0] == len(S) == whole["info"][1:].sum()
    assert np.array_equal(whole["mu"][kept["part"]], kept["mu"][kept["part"]]) and np.isnan(kept["mu"][~kept["part"]]).all()
    # the drag term: mu moves by D_a v_b,a, the residual the other way, std stays
    D = np.array([-0.3, 0.2, -0.1])
    drag = EV.evaluate(S, feats, cent, fs, 0, D)
    p = kept["part"]
    assert np.allclose(drag["mu"][p], kept["mu"][p] + D * S[p, 0:3], rtol=0, atol=1e-15) and np.array_equal(drag["std"][p], kept["std"][p])
    assert np.array_equal(drag["res"][p], drag["y"][p] - drag["mu"][p]) and np.array_equal(drag["stats"][..., :3], kept["stats"][..., :3])
    # a drag alone: empty factors leave r = y - D v
    e = EV.empty_factor([7], 7, 0.5, [1.0])
    alone = EV.evaluate(S, feats, cent, [[dict(e, out=7 + g) for g in range(3)]] * 3, 0, D)
    assert np.array_equal(alone["res"][p], S[p, 10:13] - D * S[p, 0:3])
    # the statistics are the sums of the per-record outputs; empty clusters stay 0
    for ev in (kept, whole, drag):
        again = EV.stats_of(ev, 3)
        assert np.array_equal(again[..., [0, 6, 7]], ev["stats"][..., [0, 6, 7]]) and np.allclose(again, ev["stats"], rtol=1e-13, atol=0)
        assert ev["stats"][:, :, 0].sum(axis=0).tolist() == [ev["info"][1]] * 3
    far = EV.evaluate(S, feats, np.array([[0.0], [100.0], [200.0]]), fs, 0)
    assert not far["stats"][1:].any() and far["stats"][0, 0, 0] == far["info"][1]
    nobody = S.copy()
    nobody[:, 13] = 0.0
    z = EV.evaluate(nobody, feats, cent, fs)
    assert z["info"].tolist() == [EV.ENOVALID, 0, len(S), 0] and not z["stats"].any() and np.isnan(z["mu"]).all()
