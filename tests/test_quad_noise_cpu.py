"""The simulator's random disturbances (include/admpc_quad_noise.h) without a GPU: the generator's known answers and the distributions of
the numpy spec (tests/quad_noise_spec.py); the spec's noisy update against the reference's own `Quadrotor3D.update` fed with the spec's
draws, live where the reference tree is present and through the golden vectors everywhere; the header, the prototype table and every
refusal in its order; the Python layer's constants and refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gen_quad_noise_golden as NG
import gen_quad_plant_golden as GG
import quad_noise_spec as NS
import quad_plant_spec as QS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"admpc_quad_noise_draw_batch": 8, "admpc_quad_plant_step_noise_batch": 9, "admpc_quad_rollout_noise_batch": 29}


def _plant(drag=False, substeps=1, dt=GG.DT):
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    p = quad_plant_params(SimQuad(drag=drag), dt, dt)
    p.substeps = substeps
    return p


def _noise(noisy=True, motor_noise=True, seed=NG.SEED, dt=GG.DT):
    from ad_mpc_amd.quad_config import SimQuad, quad_noise_params
    return quad_noise_params(SimQuad(noisy=noisy, motor_noise=motor_noise), dt, seed)


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


# ---- the generator ------------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    """The known answers of Philox4x32-10 (Random123's kat_vectors)."""
    ones = 0xffffffff
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                               ((ones,) * 4, (ones, ones), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(o) for o in NS.philox4x32_10(counter, key)) == want
    # the counter and the key of the contract: (b, p low, p high, 8 m + j) under (seed low, seed high)
    seed, b, p, m = 0x299f31d0a4093822, 0x243f6a88, 0x1319_8a2e_85a3_08d3, 0x03707344 // 8
    assert 0x03707344 % 8 == 4
    w = NS.words(seed, b, p, m)
    assert (int(w[8]), int(w[9])) == (0x94fdcceb_d16cfe09, 0x24126ea1_5001e420)                  # j = 4: w0 = o0 | o1 << 32, w1 = o2 | o3 << 32


def test_uniforms_and_normals_are_finite_at_the_ends():
    raw = np.array([[0, 0] + [2 ** 64 - 1] * 2 + [0, 2 ** 64 - 1] + [1 << 11, 1 << 63] * 2], dtype=np.uint64)
    z, r = NS.normals(raw)
    assert np.isfinite(z).all() and r.max() == np.sqrt(-2.0 * np.log(2.0 ** -54)) and r.max() < 8.66 and r.min() == 0.0


def test_distribution_of_the_draws():
    """Seed 7, p = 0, B = 4096, 8 sub-steps: 32 768 rows of 10.  Means within 4 standard errors of 0, standard deviations within 4 of 1,
    off-diagonal correlations within 5 of 0; the mean of a - n at a = 0.5 within 4 standard errors of 0.5 - 0.1 * (0.5 / 1.3)^2."""
    B, S = 4096, 8
    Z = NS.draws(7, np.arange(B)[:, None], 0, np.arange(S)[None, :]).reshape(-1, 10)
    n = Z.shape[0]
    assert n == 32768
    mean = np.abs(Z.mean(0)) / (1 / np.sqrt(n))
    std = np.abs(Z.std(0, ddof=1) - 1) / (1 / np.sqrt(2 * (n - 1)))
    corr = np.corrcoef(Z.T)
    off = np.abs(corr[~np.eye(10, dtype=bool)]) / (1 / np.sqrt(n))
    print("worst mean %.2f, std %.2f, correlation %.2f standard errors" % (mean.max(), std.max(), off.max()))
    assert mean.max() <= 4 and std.max() <= 4 and off.max() <= 5
    noise = _noise()
    a = 0.5
    an = a - (noise.motor_bias * (a / noise.motor_ref) ** 2 + noise.motor_std * np.sqrt(a) * Z[:, 0:4])
    se = noise.motor_std * np.sqrt(a) / np.sqrt(n)
    assert (np.abs(an.mean(0) - (0.5 - 0.1 * (0.5 / 1.3) ** 2)) <= 4 * se).all()
    # a switch's numbers do not depend on the other switch, a vehicle's not on its neighbours: the draws are a function of (seed, b, p, m)
    assert np.array_equal(NS.draws(7, 5, 0, 3), Z.reshape(B, S, 10)[5, 3])
    assert not np.array_equal(NS.draws(8, 5, 0, 3), NS.draws(7, 5, 0, 3)) and not np.array_equal(NS.draws(7, 5, 1, 3), NS.draws(7, 5, 0, 3))
    assert not np.array_equal(NS.draws(7, 5, 2 ** 32, 3), NS.draws(7, 5, 0, 3))


# ---- the noisy update against the reference's simulator -----------------------------------------------------------------------------

@pytest.mark.skipif(not GG.reference_present(), reason="the reference tree is not on this machine")
def test_spec_equals_the_live_reference_simulator_under_noise():
    ref, rnd = NG.load_reference()
    X, U = GG.inputs()
    p = NG.periods(X.shape[0])
    worst = 0.0
    for noisy, motor_noise, drag, substeps in NG.CASES:
        want = NG.run_reference(ref, rnd, noisy, motor_noise, drag, substeps, X, U)
        got, replaced = NS.step_batch(_plant(drag, substeps), _noise(noisy, motor_noise), X, U, p)
        assert not replaced.any() and np.isfinite(want).all()
        worst = max(worst, _rel(got, want))
        if noisy or motor_noise:
            calm = QS.step_batch(_plant(drag, substeps), X, U)[0]
            assert np.abs(want - calm).max() > 1e-6                                             # the disturbances act
    print("noisy spec against Quadrotor3D.update: largest relative difference %.3g" % worst)
    assert worst <= 1e-15


def test_spec_equals_the_golden_vectors_under_noise():
    with open(NG.OUT) as f:
        doc = json.load(f)
    X, U = np.array(doc["x"]), np.array(doc["u"])
    Xg, Ug = GG.inputs()
    assert np.array_equal(X, Xg) and np.array_equal(U, Ug) and doc["dt"] == GG.DT and doc["seed"] == NG.SEED
    assert doc["periods"] == [int(v) for v in NG.periods(12)] and doc["periods"][2] == 2 ** 32
    assert [(c["noisy"], c["motor_noise"], c["drag"], c["substeps"]) for c in doc["cases"]] == NG.CASES
    p = np.array(doc["periods"], dtype=np.uint64)
    for c in doc["cases"]:
        got, _ = NS.step_batch(_plant(c["drag"], c["substeps"]), _noise(c["noisy"], c["motor_noise"]), X, U, p)
        assert _rel(got, np.array(c["result"])) <= 1e-15, c
    res = {(c["noisy"], c["motor_noise"], c["drag"], c["substeps"]): np.array(c["result"]) for c in doc["cases"]}
    calm = QS.step_batch(_plant(True, 40), X, U)[0]
    assert _rel(res[(False, False, True, 40)], calm) <= 1e-15                                   # both switches off: the deterministic plant
    assert np.abs(res[(True, False, True, 40)] - calm)[:, 10:13].max() > 1e-3                   # the torque acts on the rates
    assert np.abs(res[(False, True, True, 40)] - calm)[:, 9].max() > 1e-3                       # the rotors' bias acts on the climb


def test_vectorised_noisy_plant_agrees_with_the_spec():
    """step_fleet, the plant of the CPU closed loop in tests/test_quad_noise_gpu.py, against the spec in the reference's order."""
    X, U = QS.fleet67()
    p = np.arange(16, dtype=np.uint64) * np.uint64(2 ** 31)
    for noisy, motor_noise, drag, substeps in ((True, True, True, 40), (True, False, False, 1), (False, True, True, 3)):
        plant, noise = _plant(drag, substeps), _noise(noisy, motor_noise)
        want, rep = NS.step_batch(plant, noise, X[:16], U[:16], p)
        got, rep2 = NS.step_fleet(plant, noise, X[:16], U[:16], p)
        assert np.array_equal(rep, rep2) and rep[9] and _rel(got, want) <= 1e-13, _rel(got, want)


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
    from ad_mpc_amd.quad_config import AdmpcQuadNoiseParams
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_noise.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_NOISE_EXPORTS, tuple) and list(_lib.QUAD_NOISE_EXPORTS) == list(ARITY)
    assert list(_lib.MORE_TABLES) == ["admpc_quad_noise.h"] and tuple(_lib.MORE_TABLES["admpc_quad_noise.h"]) == _lib.QUAD_NOISE_EXPORTS
    assert not set(_lib.QUAD_NOISE_EXPORTS) & {n for t in _lib.TABLES.values() for n in t}
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n and fn.restype is C.c_int, name
    assert C.sizeof(AdmpcQuadNoiseParams) == 56
    roll, watch = lib.admpc_quad_rollout_noise_batch.argtypes, lib.admpc_quad_rollout_observe_batch.argtypes
    assert list(roll[:len(watch) - 1]) == list(watch[:-1])                                       # the observed rollout's arguments, then noise, noise_step, stream
    for cite in ("quad_3d.py:187-202", "quad_3d.py:207-215", "quad_3d.py:271", "quad_3d.py:284-286", "Philox4x32-10", "0xD2511F53", "0xCD9E8D57",
                 "0x9E3779B9", "0xBB67AE85", "6.283185307179586"):
        assert cite in hdr, cite
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_noise\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_noise\.h", mk, flags=re.M)
    assert re.search(r"^HDRS\s*=.*\bquad_sim_dev\.h", mk, flags=re.M)


def test_refusals_in_front_of_the_device_in_their_order(lib):
    """Every refusal of include/admpc_quad_noise.h comes back without a device (this machine has none), and a call that breaks two rules
    is refused for the first."""
    L = lib

    def refused(rc, words):
        assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

    x = (C.c_double * 13)()
    ns = (C.c_uint64 * 1)()

    def noise(**kw):
        n = _noise()
        for k, v in kw.items():
            setattr(n, k, v)
        return n

    def step(p=_plant(), n=_noise(), B=1, u=x, stride=4, xx=x, step_=ns):
        return L.admpc_quad_plant_step_noise_batch(None if p is None else C.byref(p), None if n is None else C.byref(n), 0, B, u, stride, xx, step_, None)

    def roll(p=_plant(), n=_noise(), **kw):
        return L.admpc_quad_rollout_noise_batch(None, None, None if p is None else C.byref(p), 5, 1, 1, *([None] * 20),
                                                None if n is None else C.byref(n), kw.get("step_", ns), None)

    def draw(n=_noise(), B=1, S=1, step_=ns, z=x):
        return L.admpc_quad_noise_draw_batch(None if n is None else C.byref(n), 0, B, S, step_, z, None, None)

    bad_plant = _plant(); bad_plant.substeps = 0
    neg = _plant(); neg.u_min = -0.5
    inf, nan = float("inf"), float("nan")
    for call in (step, roll):
        refused(call(p=None, n=None), "plant parameters are not set")                            # 1 before 2
        refused(call(p=bad_plant, n=None), "substeps must be in [1, 1024]")
        refused(call(n=None), "noise parameters are not set")                                    # 2
        refused(call(n=noise(noisy=2, motor_noise=0)), "must be 0 or 1")                         # 3 before 4
        refused(call(n=noise(motor_noise=-1)), "must be 0 or 1")
        refused(call(n=noise(noisy=0, motor_noise=0, force_std=-1.0)), "call admpc_quad_plant_step_batch")     # 4 before 5
        for k in ("force_std", "torque_std", "motor_std"):
            for v in (-1e-9, inf, nan):
                refused(call(n=noise(motor_ref=0.0, **{k: v})), "force_std, torque_std and motor_std")        # 5 before 6
        for kw in (dict(motor_ref=0.0), dict(motor_ref=-1.3), dict(motor_ref=inf), dict(motor_ref=nan), dict(motor_bias=nan), dict(motor_bias=inf)):
            refused(call(p=neg, n=noise(**kw)), "motor_ref must be positive and finite, motor_bias finite")    # 6 before 7
        refused(call(p=neg), "motor_noise needs u_min >= 0")                                     # 7
    refused(step(p=neg, B=-1), "motor_noise needs u_min >= 0")                                   # 7 before 8
    assert step(p=neg, n=noise(motor_noise=0), B=0) == 0                                         # without motor_noise a negative u_min is fine
    refused(step(B=-1, u=None), "negative batch")                                                # 8: the batch arguments of the plant step, in their order
    refused(step(u=None, stride=3), "null array")
    refused(step(xx=None, stride=3), "null array")
    refused(step(stride=3, step_=None), "u_stride must be at least 4")
    refused(step(step_=None), "null noise_step")                                                 # 9
    assert step(B=0, u=None, xx=None, step_=None) == 0
    refused(roll(step_=None), "admpc_quad_rollout_batch: null solver")                           # 8: the rollout's own refusals, under its name
    # the observed form: the observe parameters come first among the refusals of the entry it extends
    refused(L.admpc_quad_rollout_noise_batch(None, None, C.byref(_plant()), 5, 1, 1, *([None] * 14), C.c_void_p(1), None, *([None] * 4),
                                             C.byref(_noise()), ns, None), "admpc_quad_rollout_observe_batch: the observe parameters are not set")

    refused(draw(n=None, B=-1), "noise parameters are not set")
    refused(draw(n=noise(noisy=3), B=-1), "must be 0 or 1")
    refused(draw(n=noise(noisy=0, motor_noise=0), B=-1), "both 0")
    refused(draw(n=noise(torque_std=nan), B=-1), "force_std, torque_std and motor_std")
    refused(draw(n=noise(motor_ref=0.0), B=-1), "motor_ref must be positive")
    refused(draw(B=-1, S=0), "negative batch")
    refused(draw(S=0, z=None), "substeps must be in [1, 1024]")
    refused(draw(S=1025), "substeps must be in [1, 1024]")
    refused(draw(z=None), "null array")
    refused(draw(step_=None), "null array")
    assert draw(B=0, z=None, step_=None) == 0


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------

def test_noise_params_are_the_reference_constants():
    from ad_mpc_amd.quad_config import SimQuad, quad_noise_params, quad_plant_params
    n = quad_noise_params(SimQuad(noisy=True, motor_noise=True), 5e-4, 2 ** 64 - 1)
    assert (n.seed, n.noisy, n.motor_noise) == (2 ** 64 - 1, 1, 1)
    assert (n.force_std, n.torque_std, n.motor_bias, n.motor_ref, n.motor_std) == (10 * 5e-4, 10 * 5e-4, 0.1, 1.3, 0.02)
    m = quad_noise_params(SimQuad(motor_noise=True), 1e-3, 5)
    assert (m.noisy, m.motor_noise, m.force_std) == (0, 1, 10 * 1e-3)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="seed"):
            quad_noise_params(SimQuad(noisy=True), 5e-4, bad)
    quad = SimQuad(drag=True, noisy=True, motor_noise=True)
    with pytest.raises(NotImplementedError, match="random disturbances"):
        quad_plant_params(quad, 5e-4, 0.02)
    p, q = quad_plant_params(quad, 5e-4, 0.02, allow_noise=True), quad_plant_params(SimQuad(drag=True), 5e-4, 0.02)
    assert bytes(p) == bytes(q)                                                                  # the plant parameters know nothing of the switches


def test_noisy_fleet_without_a_seed_is_refused():
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    for kw in (dict(noisy=True), dict(motor_noise=True), dict(noisy=True, motor_noise=True)):
        with pytest.raises(NotImplementedError, match="random disturbances"):
            QuadFleet(4, quad=SimQuad(**kw))                                                     # refused before a handle (and so a GPU) is asked for
        with pytest.raises(ValueError, match="seed"):
            QuadFleet(4, quad=SimQuad(**kw), noise_seed=-1)                                      # ... and so is a key that does not fit
