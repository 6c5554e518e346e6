"""Flying to random targets (include/admpc_quad_targets.h) without a GPU: the numpy spec's sampler and reach test
(tests/quad_targets_spec.py) against the reference's own `sample_random_target` and `euclidean_dist`, live where the reference tree is
present and through the golden vectors everywhere; the generator's counter against the disturbances'; the scenario of the plant test
(tests/test_quad_targets_gpu.py) with its margins; the header, the prototype table and the refusals of the C ABI in their order; the
Python layer's refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gen_quad_targets_golden as TG
import quad_noise_spec as NS
import quad_plant_spec as QS
import quad_targets_spec as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"admpc_quad_target_draw_batch": 9, "admpc_quad_targets_reset_batch": 11, "admpc_quad_target_window_batch": 14,
         "admpc_quad_plant_target_step_batch": 18, "admpc_quad_observe_var_batch": 13, "admpc_quad_rollout_targets_batch": 33}


def _rel(got, want):
    return float((np.abs(np.asarray(got) - np.asarray(want)) / np.maximum(1.0, np.abs(want))).max())


def _tp(**kw):
    from ad_mpc_amd.quad_config import quad_target_params
    kw.setdefault("seed", TG.SEED)
    return quad_target_params(**kw)


# ---- the sampler and the reach test against the reference ---------------------------------------------------------------------------

@pytest.mark.skipif(not TG.reference_present(), reason="the reference tree is not on this machine")
def test_spec_equals_the_live_reference_functions():
    """sample_random_target and euclidean_dist, taken out of the reference's files at run time, fed with the spec's uniforms in place of
    np.random.uniform's: 1e-15 * max(1, |value|)."""
    sample, euclid, rnd = TG.load_reference()
    P, no = TG.inputs()
    U = TS.uniforms(TS.words(TG.SEED, np.arange(TG.B), no))
    for mode, aggressive in ((1, True), (2, False)):
        want = TG.run_reference(sample, rnd, aggressive, P, U)
        got = TS.sample(mode, TG.R, P, U)
        print("mode %d: largest relative difference %.3g" % (mode, _rel(got, want)))
        assert _rel(got, want) <= 1e-15
        if mode == 1:
            r = np.linalg.norm(want - P, axis=1)
            assert (r >= 0.5 * TG.R - 1e-12).all() and (r <= 1.5 * TG.R + 1e-12).all()
        else:
            assert (np.abs(want) <= TG.R).all()
    t, p = TG.pairs()
    for i in range(len(t)):
        d = euclid(t[i], p[i])
        assert abs(TS.dist(t[i], p[i]) - d) <= 1e-15 * max(1.0, d)
        assert bool(euclid(t[i], p[i], thresh=0.05)) == bool(TS.dist(t[i], p[i]) < 0.05)


def test_spec_equals_the_golden_vectors():
    with open(TG.OUT) as f:
        doc = json.load(f)
    P, no = TG.inputs()
    assert doc["seed"] == TG.SEED and doc["world_radius"] == TG.R and np.array_equal(np.array(doc["positions"]), P)
    assert doc["target_no"] == [int(v) for v in no] and doc["target_no"][2] == 2 ** 32
    U = TS.uniforms(TS.words(TG.SEED, np.arange(TG.B), no))
    assert np.array_equal(np.array(doc["uniforms"]), U) and (U > 0).all() and (U < 1).all()
    for mode, key in ((1, "aggressive"), (2, "uniform")):
        assert _rel(TS.sample(mode, TG.R, P, U), np.array(doc[key])) <= 1e-15
    tp = _tp(mode="aggressive", world_radius=TG.R)
    assert _rel(np.stack([TS.draw(tp, b, no[b], P[b]) for b in range(TG.B)]), np.array(doc["aggressive"])) <= 1e-15
    t, p = np.array(doc["pair_t"]), np.array(doc["pair_p"])
    assert np.array_equal(t, TG.pairs()[0])
    for i in range(len(t)):
        assert abs(TS.dist(t[i], p[i]) - doc["dist"][i]) <= 1e-15 and bool(TS.dist(t[i], p[i]) < 0.05) == doc["within_0.05"][i]
    assert True in doc["within_0.05"] and False in doc["within_0.05"]


def test_the_targets_counter_words_do_not_meet_the_disturbances():
    """The disturbances' fourth counter word is 8 m + j with m < substeps <= 1024 and j < 5; a target's is 0xffffffff - j, j < 2."""
    noise_words = {8 * m + j for m in range(1024) for j in range(5)}
    assert max(noise_words) == 8188 and not noise_words & {TS.LAST, TS.LAST - 1}
    # ... and under one seed, vehicle and period / target number the words differ
    w = TS.words(5, 3, 7)
    n = NS.words(5, 3, 7, np.arange(4))
    assert not set(int(v) for v in w.ravel()) & set(int(v) for v in n.ravel())
    # the known answer of Philox4x32-10 at the all-ones counter, through the target's construction: b, t and the word of call 0 all ones
    raw = TS.words(0xffffffff_ffffffff, 0xffffffff, 0xffffffff_ffffffff)
    assert (int(raw[0]), int(raw[1])) == (0x41c83b0e_408f276d, 0x6d5451fd_a20bc7c6)
    assert not np.array_equal(TS.words(5, 3, 7), TS.words(5, 3, 7 + 2 ** 32)) and not np.array_equal(TS.words(5, 3, 7), TS.words(6, 3, 7))


def test_distribution_of_the_targets():
    """4096 targets per mode: the uniform mode fills the box evenly (means and variances within 4 standard errors); the aggressive
    mode's distance from the position is uniform in [R / 2, 3 R / 2]."""
    n, R = 4096, 3.0
    U = TS.uniforms(TS.words(9, np.arange(n), 0))
    box = TS.sample(2, R, np.zeros((n, 3)), U)
    assert (np.abs(box.mean(0)) <= 4 * (2 * R / np.sqrt(12)) / np.sqrt(n)).all() and (np.abs(box) < R).all()
    assert (np.abs(box.var(0) - (2 * R) ** 2 / 12) <= 4 * (2 * R) ** 2 / 12 * np.sqrt(0.8 / n) * 1.5).all()
    P = np.tile([1.0, -2.0, 0.5], (n, 1))
    r = np.linalg.norm(TS.sample(1, R, P, U) - P, axis=1)
    assert r.min() >= 0.5 * R - 1e-12 and r.max() <= 1.5 * R + 1e-12 and abs(r.mean() - R) <= 4 * (R / np.sqrt(12)) / np.sqrt(n)


# ---- the rules in the spec ----------------------------------------------------------------------------------------------------------

def test_fast_is_signed_and_a_nan_compares_false():
    x = np.zeros(13)
    for v, want in (([14.0, 0, 0], 0), ([14.000001, 0, 0], 1), ([-20.0, 0, 0], 0), ([0, np.nan, 0], 0), ([np.nan, 0, 15.0], 1), ([0, np.inf, 0], 1)):
        x[7:10] = v
        assert TS.too_fast(x, 14.0) == want, v


def test_the_plant_scenario_keeps_its_margins():
    """The scenario of the GPU plant test, every case of it: vehicles reach at sub-step 1, at a middle one, at the last one and never,
    and |d - thresh| >= 1e-9 behind every sub-step of every vehicle, so that a device that agrees with the spec to 1e-12 decides alike."""
    import test_quad_targets_gpu as TT
    for drag in (False, True):
        for noisy, motor_noise in TT.SWITCHES:
            sc = TT.plant_scenario(drag, noisy, motor_noise)
            margins = np.array([abs(m) for row in sc["margins"] for m in row])
            nsub, reached = sc["nsub"], sc["reached"]
            print("drag=%s noisy=%s motor_noise=%s: smallest |d - thresh| %.3g, nsub %s" % (drag, noisy, motor_noise, margins.min(), np.bincount(nsub, minlength=41)[[1, 40]]))
            assert len(sc["margins"]) == 67 and all(len(row) == n for row, n in zip(sc["margins"], nsub))
            assert margins.min() >= 1e-9
            assert (reached & (nsub == 1)).sum() >= 5 and (reached & (nsub > 1) & (nsub < 40)).sum() >= 5
            assert (reached & (nsub == 40)).sum() >= 5 and (~reached).sum() >= 5 and (nsub[~reached] == 40).all()
            assert reached[9] and sc["state"]["tcounts"][9, 4] == sc["st0"]["tcounts"][9, 4] + 1                               # the NaN activation's vehicle reaches, and is counted


def test_presets_end_in_done():
    """Two presets placed on the flown path: the second one reached, then the vehicle is done: full periods, nothing counted."""
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    plant = quad_plant_params(SimQuad(drag=True), 5e-4, 5e-4)
    plant.substeps = 8
    X, U = QS.fleet67()
    X, U = X[:3].copy(), U[:3].copy()
    import test_quad_targets_gpu as TT
    tp = _tp(mode="preset", thresh=1e-4, n_preset=2, seed=None)
    free = TT._free_flight(plant, None, X, U, None)
    # under one input the flight goes on along the free path: behind sub-step 3 of the first period, behind sub-step 2 of the second
    presets = np.stack([np.stack([free[b][2], free[b][4]]) for b in range(3)])
    st, x = TS.reset(tp, X, presets), X.copy()
    seen = []
    for _ in range(4):
        nsub, _, _ = TS.plant_step(plant, tp, None, st, x, U, presets=presets)
        seen.append((nsub.tolist(), st["target_no"].tolist(), st["tcounts"][:, 0].tolist(), st["tcounts"][:, 2].tolist(), st["n_iter"].tolist()))
    assert seen[0] == ([3] * 3, [1] * 3, [1] * 3, [1] * 3, [1] * 3)
    assert seen[1] == ([2] * 3, [2] * 3, [2] * 3, [2] * 3, [1] * 3)
    assert seen[2] == ([8] * 3, [2] * 3, [2] * 3, [2] * 3, [1] * 3) and seen[3] == seen[2]      # done


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_table_and_library_agree(lib):
    from ad_mpc_amd import _lib
    from ad_mpc_amd.quad_config import AdmpcQuadTargetParams
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_targets.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert list(_lib.QUAD_TARGETS_EXPORTS) == list(ARITY) and list(_lib.TARGET_TABLES) == ["admpc_quad_targets.h"]
    known = [t for group in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES) for t in group.values()]
    assert not set(ARITY) & {n for t in known for n in t}
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n and fn.restype is C.c_int, name
    assert C.sizeof(AdmpcQuadTargetParams) == 48 and "48 bytes" in hdr
    m = re.search(r"typedef struct AdmpcQuadTargetParams \{(.*?)\} AdmpcQuadTargetParams;", txt, flags=re.S)
    fields = re.findall(r"\b(?:uint64_t|int32_t|double)\s+(\w+)\s*;", m.group(1))
    assert fields == [f[0] for f in AdmpcQuadTargetParams._fields_]
    for cite in ("point_tracking_and_record.py:82-107", "point_tracking_and_record.py:204-206", "utils/utils.py:262-281", "quad_3d_optimizer.py:429-462",
                 "0xffffffff - j", "6.283185307179586", "NOT offered", "bit for bit", "simulation_time"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_targets\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_targets\.h", mk, flags=re.M)
    assert re.search(r"^HDRS\s*=.*\bquad_noise_dev\.h", mk, flags=re.M) and re.search(r"^HDRS\s*=.*\bquad_observe_dev\.h", mk, flags=re.M)


def test_refusals_in_front_of_the_device_in_their_order(lib):
    """Every refusal of include/admpc_quad_targets.h comes back without a device (this machine has none), and a call that breaks two
    rules is refused for the first."""
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, SimQuad, quad_learn_bins, quad_noise_params, quad_plant_params
    import quad_learn_spec as QL
    L = lib

    def refused(rc, words):
        assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

    def plant(**kw):
        p = quad_plant_params(SimQuad(drag=True), 5e-4, 0.02)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def tp(**kw):
        t = _tp()
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    a = (C.c_double * 64)()
    i = (C.c_int32 * 16)()
    q = (C.c_uint64 * 4)()
    inf, nan = float("inf"), float("nan")
    bad_tp = [(None, "target parameters are not set"), (tp(mode=3, world_radius=0.0), "mode must be"), (tp(mode=-1), "mode must be"),
              (tp(world_radius=0.0, thresh=0.0), "world_radius"), (tp(world_radius=inf), "world_radius"), (tp(world_radius=nan), "world_radius"),
              (tp(thresh=0.0, v_max=nan), "thresh"), (tp(thresh=inf), "thresh"), (tp(v_max=nan, max_iters=-1), "v_max"),
              (tp(max_iters=-1, mode=0, n_preset=0), "max_iters"), (tp(mode=0, n_preset=0), "n_preset >= 1")]
    ref = lambda t: None if t is None else C.byref(t)

    def draw(t=tp(), B=1, x=a, stride=13, no=q, out=a):
        return L.admpc_quad_target_draw_batch(ref(t), 0, B, x, stride, no, out, None, None)

    def reset(t=tp(), B=1, x=a, presets=None, target=a, no=q, n_iter=i, fast=i, tc=i):
        return L.admpc_quad_targets_reset_batch(ref(t), 0, B, x, presets, target, no, n_iter, fast, tc, None)

    def window(t=tp(), B=1, N=10, x=a, target=a, no=None, n_iter=i, fast=i, tc=i, yref=a, yref_e=a):
        return L.admpc_quad_target_window_batch(ref(t), 0, B, N, x, target, no, n_iter, fast, tc, None, yref, yref_e, None)

    def step(p=plant(), t=tp(), n=None, B=1, u=a, stride=4, x=a, presets=None, target=a, no=q, nsub=i, ns=None):
        return L.admpc_quad_plant_target_step_batch(ref(p), ref(t), ref(n), 0, B, u, stride, x, None, presets, target, no, i, i, i, nsub, ns, None)

    def roll(p=plant(), t=tp(), n=None, s=None, B=1, T=1, model=None, obs=None):
        return L.admpc_quad_rollout_targets_batch(s, ref(p), ref(t), B, T, *([None] * 19), model, ref(obs), *([None] * 4), ref(n), None, None)

    for t, words in bad_tp:
        for call in (draw, reset, window):
            refused(call(t=t, B=-1), words)
        refused(step(t=t, B=-1), words); refused(roll(t=t, B=-1), words)
    for call in (step, roll):
        refused(call(p=None, t=None), "plant parameters are not set")                            # the plant before the targets
        refused(call(p=plant(substeps=0), t=None), "substeps must be in [1, 1024]")
        noise = quad_noise_params(SimQuad(noisy=True, motor_noise=True), 5e-4, 1)
        noise.noisy = 2
        refused(call(t=tp(mode=3), n=noise), "mode must be")                                     # the targets before the noise
        refused(call(n=noise, B=-1), "must be 0 or 1")                                           # the noise before the batch
        noise.noisy = 1
        refused(call(p=plant(u_min=-0.5), n=noise, B=-1), "motor_noise needs u_min >= 0")
    preset = tp(mode=0, n_preset=2)
    refused(draw(t=preset, B=-1), "presets are not drawn")
    refused(draw(B=-1, x=None), "negative batch")
    for kw in (dict(x=None), dict(no=None), dict(out=None)):
        refused(draw(stride=2, **kw), "null array")
    refused(draw(stride=2), "x_stride must be at least 3")
    assert draw(B=0, x=None) == 0
    refused(reset(B=-1, x=None), "negative batch")
    for kw in (dict(x=None), dict(target=None), dict(no=None), dict(n_iter=None), dict(fast=None), dict(tc=None)):
        refused(reset(t=preset, **kw), "null array")
    refused(reset(t=preset), "mode 0 needs the presets")
    assert reset(B=0, x=None) == 0
    refused(window(B=-1, N=1), "negative batch")
    for N in (1, 25):
        refused(window(N=N, x=None), "N must be in [2, 24]")
    for kw in (dict(x=None), dict(target=None), dict(n_iter=None), dict(fast=None), dict(tc=None), dict(yref=None), dict(yref_e=None)):
        refused(window(t=preset, **kw), "null array")
    refused(window(t=preset), "mode 0 needs target_no")
    assert window(B=0, x=None) == 0
    refused(step(B=-1, u=None), "negative batch")
    for kw in (dict(u=None), dict(x=None), dict(target=None), dict(no=None), dict(nsub=None)):
        refused(step(stride=3, **kw), "null array")
    refused(step(stride=3, t=preset), "u_stride must be at least 4")
    refused(step(t=preset, n=noise), "mode 0 needs the presets")
    refused(step(n=noise), "null noise_step")
    assert step(B=0, u=None) == 0
    # the rollout: the observe parameters with a model, then the solver, before the batch
    bins, n_gp = quad_learn_bins(QL.EXP_LEARN)
    obs = AdmpcQuadObserveParams(dt=0.02, substeps=1, n_gp=n_gp, gp=bins)
    refused(roll(model=C.c_void_p(1), obs=None), "observe parameters are not set")
    obs.substeps = 65
    refused(roll(model=C.c_void_p(1), obs=obs), "substeps must be in [1, 64]")
    refused(roll(B=-1, T=-1), "null solver")
    # the observation with a period per vehicle: admpc_quad_observe_batch's order
    obs.substeps = 1

    def watch(o=obs, p=plant(), model=C.c_void_p(1), B=1, u=a, stride=4, nsub=i):
        return L.admpc_quad_observe_var_batch(model, ref(p), ref(o), B, u, stride, a, a, nsub, a, a, i, None)

    refused(watch(o=None, p=None), "observe parameters are not set")
    refused(watch(p=None, model=None), "plant parameters are not set")
    refused(watch(model=None, B=-1), "null model")
    refused(watch(B=-1, u=None), "negative batch")
    refused(watch(u=None, stride=3), "null array")
    refused(watch(nsub=None, stride=3), "null array")
    assert watch(B=0, u=None) == 0


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------

def test_target_params_are_the_reference_constants_and_refuse():
    from ad_mpc_amd.quad_config import quad_target_params
    t = quad_target_params(seed=2 ** 64 - 1)
    assert (t.seed, t.mode, t.world_radius, t.thresh, t.v_max, t.max_iters) == (2 ** 64 - 1, 1, 3.0, 0.05, 14.0, 100)
    assert quad_target_params("uniform", seed=0).mode == 2 and quad_target_params("preset", n_preset=3).n_preset == 3
    for kw, words in ((dict(mode="random"), "mode"), (dict(world_radius=0.0), "world_radius"), (dict(world_radius=float("inf")), "world_radius"),
                      (dict(thresh=-1.0), "thresh"), (dict(thresh=float("nan")), "thresh"), (dict(v_max=float("nan")), "v_max"),
                      (dict(max_iters=-1), "max_iters"), (dict(max_iters=1.5), "max_iters"), (dict(seed=None), "needs a seed"),
                      (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(mode="preset", n_preset=0), "preset")):
        with pytest.raises(ValueError, match=words):
            quad_target_params(**dict(dict(seed=1), **kw))


def test_set_targets_refuses_before_any_device_call():
    """On a fleet that has no device at all: every refusal of set_targets, the order of the calls, and the ensemble's refusal."""
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    from ad_mpc_amd.quad_fleet import QuadFleet
    fl = object.__new__(QuadFleet)
    fl.B, fl._tp, fl._learn = 4, None, None
    for kw, words in ((dict(mode="fast"), "mode"), (dict(), "needs a seed"), (dict(seed=1, thresh=0.0), "thresh"), (dict(seed=1, world_radius=-3.0), "world_radius"),
                      (dict(seed=1, v_max=float("nan")), "v_max"), (dict(seed=1, max_iters=-2), "max_iters"), (dict(seed=2 ** 64), "seed"),
                      (dict(mode="preset"), "needs presets"), (dict(mode="preset", presets=np.zeros((3, 2, 3))), r"\[n,3\] or \[B,n,3\]"),
                      (dict(mode="preset", presets=np.zeros((0, 3))), r"\[n,3\] or \[B,n,3\]"), (dict(mode="preset", presets=np.zeros((2, 4))), r"\[n,3\]"),
                      (dict(seed=1, presets=np.zeros((2, 3))), "come with mode 'preset'")):
        with pytest.raises(ValueError, match=words):
            fl.set_targets(**kw)
    for call in (fl.reset_targets, fl.target_window, fl.plant_step_targets, fl.observe_targets, lambda: fl.rollout_targets(3)):
        with pytest.raises(ValueError, match="call set_targets first"):
            call()
    ens = object.__new__(QuadEnsembleFleet)
    for call in (lambda: ens.set_targets(seed=1), ens.reset_targets, ens.target_window, ens.plant_step_targets, lambda: ens.rollout_targets(3)):
        with pytest.raises(ValueError, match="clustered ensembles do not chase targets"):
            call()
    ens._ens, ens._solvers = None, []                                                        # nothing for __del__ to release
