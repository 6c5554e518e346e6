"""Flying to random targets on the device (include/admpc_quad_targets.h; ad_mpc_amd/quad_fleet.py: set_targets, rollout_targets).

The generator's words are compared bit for bit with the numpy spec (tests/quad_targets_spec.py) and the targets at a bound worked out
from the libraries' errors; the plant kernel with the reach test against the spec under given inputs, where every decision of the spec
keeps a margin that the plant's bound cannot cross; the window and the recovery bit for bit; the observation over the flown time against
the existing entry (full periods, bit for bit) and against tests/quad_learn_spec.py run at the vehicle's own period; the rollout bit for
bit against the loop of calls it replaces; a captured rollout; and the experiment end to end."""
import ctypes as C
import json

import numpy as np
import pytest

import gen_quad_plant_golden as GG
import gen_quad_targets_golden as TG
import quad_learn_spec as QL
import quad_noise_spec as NS
import quad_plant_spec as QS
import quad_targets_spec as TS
import test_quad_fleet_gpu as TQ
from test_quad_fleet_gpu import RTOL, _bits, _dev, _host, _p, _stream

pytestmark = pytest.mark.gpu

SEED = TG.SEED
NOISE_SEED = 0x5EEDF00D2024
SWITCHES = [(False, False), (True, False), (False, True), (True, True)]           # (noisy, motor_noise); the first: the deterministic kernel
THRESH = 1e-4                 # of the plant tests: below the 3 mm a vehicle at 6 m/s flies per sub-step, so that a reach at a chosen sub-step can be placed
ULP = 2.0 ** -52


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _plant(drag, substeps):
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    p = quad_plant_params(SimQuad(drag=drag), GG.DT, GG.DT)
    p.substeps = substeps
    return p


def _noise(noisy, motor_noise, seed=NOISE_SEED):
    from ad_mpc_amd.quad_config import SimQuad, quad_noise_params
    if not (noisy or motor_noise):
        return None
    return quad_noise_params(SimQuad(noisy=noisy, motor_noise=motor_noise), GG.DT, seed)


def _tp(**kw):
    from ad_mpc_amd.quad_config import quad_target_params
    kw.setdefault("seed", SEED)
    return quad_target_params(**kw)


def _numbers(B):
    return np.arange(B, dtype=np.uint64) * np.uint64(2 ** 31)


def target_bound(R, p):
    """What two IEEE implementations of a target may differ by: sin and cos are within 2 ulp in both libraries, so r sin(theta) agrees
    to 5 ulp and its product with cos(psi) or sin(psi) to 10 ulp of 1.5 R at most; the sum with p rounds once more.  16 ulp of
    max(1, 1.5 R + |p|_inf) has a margin of about 1.5, as the bound of the disturbances' normals has."""
    return 16 * ULP * np.maximum(1.0, 1.5 * R + np.abs(p).max(axis=-1))[..., None]


# ---- 1. the targets -----------------------------------------------------------------------------------------------------------------

def _draw(L, tp, P, no):
    import torch
    B = P.shape[0]
    x = torch.full((B, 13), float("nan"), dtype=torch.float64, device="cuda:0")
    x[:, :3] = _dev(P)
    out = torch.full((B, 3), float("nan"), dtype=torch.float64, device="cuda:0")
    raw = torch.zeros((B, 4), dtype=torch.int64, device="cuda:0")
    num = _dev(np.asarray(no, dtype=np.uint64).view(np.int64))
    assert L.admpc_quad_target_draw_batch(C.byref(tp), 0, B, _p(x), 13, _p(num), _p(out), _p(raw), _stream()) == 0, L.admpc_last_error()
    _bits(_host(num).view(np.uint64), np.asarray(no, dtype=np.uint64), "target_no is read-only")
    return _host(out), _host(raw).view(np.uint64)


@pytest.mark.parametrize("mode", ["aggressive", "uniform"])
def test_targets_equal_the_spec_and_the_golden_vectors(mode):
    """B = 67, target numbers arange(67) * 2^31, so that the high counter word is used.  The words bit for bit; the targets within
    target_bound.  Then the 24 golden targets the reference's own sample_random_target gave under the same uniforms."""
    L = TQ._lib()
    B, R = 67, 3.0
    tp = _tp(mode=mode, world_radius=R)
    P = QS.random_states(B, 41)[:, :3]
    no = _numbers(B)
    assert (no >> np.uint64(32)).max() > 0
    got, raw = _draw(L, tp, P, no)
    want_raw = TS.words(SEED, np.arange(B), no)
    _bits(raw, want_raw, "the generator's words")
    want = TS.sample(int(tp.mode), R, P, TS.uniforms(want_raw))
    ratio = np.abs(got - want) / target_bound(R, P)
    print("targets, %s: largest |t - spec| = %.3g, over its bound %.3g" % (mode, np.abs(got - want).max(), ratio.max()))
    assert np.isfinite(got).all() and ratio.max() <= 1.0
    with open(TG.OUT) as f:
        doc = json.load(f)
    Pg, ng = np.array(doc["positions"]), np.array(doc["target_no"], dtype=np.uint64)
    assert doc["seed"] == SEED and doc["world_radius"] == R
    gold, graw = _draw(L, tp, Pg, ng)
    _bits(TS.uniforms(graw), np.array(doc["uniforms"]), "the golden uniforms")
    ratio = np.abs(gold - np.array(doc[mode])) / target_bound(R, Pg)
    print("golden targets, %s: over the bound %.3g" % (mode, ratio.max()))
    assert ratio.max() <= 1.0


# ---- 2. the plant kernel against the spec -------------------------------------------------------------------------------------------

_SCENARIO = {}


def _free_flight(plant, noise, X, U, noise_step):
    """The positions behind every sub-step of a period that reaches nothing, by the spec: [B][substeps][3]."""
    B = X.shape[0]
    far = _tp(mode="aggressive", thresh=1e-12)
    st = dict(target=np.full((B, 3), 1e6), target_no=np.zeros(B, dtype=np.uint64), n_iter=np.zeros(B, dtype=np.int32),
              fast=np.zeros(B, dtype=np.int32), tcounts=np.zeros((B, 5), dtype=np.int32))
    step = None if noise is None else np.array(noise_step, dtype=np.uint64)
    return [np.stack(p) for p in TS.plant_step(plant, far, noise, st, X.copy(), U, noise_step=step)[2]]


def _initial_state(B, targets):
    """Counters away from zero, so that every update shows: target numbers with the high word in use."""
    return dict(target=np.array(targets, dtype=np.float64), target_no=_numbers(B), n_iter=(np.arange(B) % 5).astype(np.int32),
                fast=np.full(B, 7, dtype=np.int32), tcounts=(np.arange(B * 5).reshape(B, 5) % 11).astype(np.int32))


def plant_scenario(drag, noisy, motor_noise):
    """QS.fleet67 with its NaN activation, 40 sub-steps, vehicle b in noise period b * 2^31.  The targets lie on the spec's own flown
    positions: vehicle b with b % 4 == 0 on the position behind sub-step 1, == 1 behind a middle one (3 .. 38), == 2 behind sub-step 40,
    == 3 fifty metres away.  Returns the inputs, the state before, and the spec's period with its margins."""
    key = (drag, noisy, motor_noise)
    if key in _SCENARIO:
        return _SCENARIO[key]
    X, U = QS.fleet67()
    B, S = 67, 40
    plant, noise = _plant(drag, S), _noise(noisy, motor_noise)
    tp = _tp(mode="aggressive", thresh=THRESH)
    step0 = _numbers(B)
    free = _free_flight(plant, noise, X, U, step0)
    targets = np.zeros((B, 3))
    for b in range(B):
        kind = b % 4
        targets[b] = free[b][0] if kind == 0 else free[b][2 + (b * 7) % 36] if kind == 1 else free[b][S - 1] if kind == 2 else X[b, :3] + [50.0, 0.0, 0.0]
    st0 = _initial_state(B, targets)
    st, x, step = TS.copy_state(st0), X.copy(), step0.copy()
    status = (np.arange(B) % 3 == 0).astype(np.int32) * 4
    nsub, margins, _ = TS.plant_step(plant, tp, noise, st, x, U, status=status, noise_step=step if noise is not None else None)
    sc = dict(X=X, U=U, plant=plant, noise=noise, tp=tp, st0=st0, step0=step0, status=status, state=st, x=x, nsub=nsub, margins=margins,
              reached=st["target_no"] != st0["target_no"], step=step)
    _SCENARIO[key] = sc
    return sc


def _run_step(L, plant, tp, noise, X, U, st, noise_step=None, status=None, presets=None):
    """admpc_quad_plant_target_step_batch on copies: (x [B,13], the state afterwards, nsub [B], noise_step afterwards)."""
    import torch
    B = X.shape[0]
    x, u = _dev(X), _dev(U)
    d = {k: _dev(v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in st.items()}
    nsub = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    ns = _dev(np.asarray(noise_step, dtype=np.uint64).view(np.int64)) if noise is not None else None
    rc = L.admpc_quad_plant_target_step_batch(C.byref(plant), C.byref(tp), None if noise is None else C.byref(noise), 0, B, _p(u), 4, _p(x),
                                              _p(None if status is None else _dev(status)), _p(None if presets is None else _dev(presets)),
                                              _p(d["target"]), _p(d["target_no"]), _p(d["n_iter"]), _p(d["fast"]), _p(d["tcounts"]), _p(nsub), _p(ns),
                                              _stream())
    assert rc == 0, L.admpc_last_error()
    torch.cuda.synchronize()
    out = {k: _host(v) for k, v in d.items()}
    out["target_no"] = out["target_no"].view(np.uint64)
    return _host(x), out, _host(nsub), (_host(ns).view(np.uint64) if ns is not None else None)


def _same_period(got, want, nsub, R, what, rows=None):
    """The outcome of a period against the spec's: (x, state, nsub, noise_step) each.  The counters equal; the states within
    nsub * RTOL (nsub: the sub-steps flown since the device and the spec started from the same doubles); a next target within
    target_bound plus what the position at the reach, from which it is sampled, may differ by."""
    (gx, gs, gn, gstep), (wx, ws, wn, wstep) = got, want
    rows = slice(None) if rows is None else rows
    _bits(gn[rows], wn, "nsub, " + what)
    for k in ("target_no", "n_iter", "fast", "tcounts"):
        _bits(gs[k][rows], ws[k], "%s, %s" % (k, what))
    if wstep is not None:
        _bits(gstep[rows], wstep, "noise_step, " + what)
    ratio = np.abs(gx[rows] - wx) / (nsub[:, None] * RTOL * np.maximum(1.0, np.abs(wx)))
    print("%s: largest |x - spec| over nsub * RTOL * max(1, |x|): %.3g" % (what, ratio.max()))
    assert not np.isnan(gx[rows]).any() and ratio.max() <= 1.0
    bound = target_bound(R, wx[:, :3]) + nsub[:, None] * RTOL * np.maximum(1.0, np.abs(wx[:, :3]).max(axis=1))[:, None]
    ratio = np.abs(gs["target"][rows] - ws["target"]) / bound
    print("%s: largest |target - spec| over its bound: %.3g" % (what, ratio.max()))
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("drag", [False, True])
@pytest.mark.parametrize("noisy,motor_noise", SWITCHES)
def test_plant_target_kernel_matches_the_spec(noisy, motor_noise, drag):
    """The scenario above.  The test is valid only where the spec's |d - thresh| >= 1e-9 behind every sub-step of every vehicle (a state
    within 40 * 1e-12 of the spec's cannot decide otherwise); tests/test_quad_targets_cpu.py checks the classes of the scenario too."""
    L = TQ._lib()
    sc = plant_scenario(drag, noisy, motor_noise)
    margins = np.array([abs(m) for row in sc["margins"] for m in row])
    assert len(sc["margins"]) == 67 and margins.min() >= 1e-9, margins.min()
    nsub, reached = sc["nsub"], sc["reached"]
    assert (reached & (nsub == 1)).any() and (reached & (nsub > 1) & (nsub < 40)).any() and (reached & (nsub == 40)).any() and (~reached).any()
    got = _run_step(L, sc["plant"], sc["tp"], sc["noise"], sc["X"], sc["U"], sc["st0"], sc["step0"], status=sc["status"])
    what = "noisy=%s motor_noise=%s drag=%s" % (noisy, motor_noise, drag)
    _same_period(got, (sc["x"], sc["state"], nsub, sc["step"] if sc["noise"] is not None else None), nsub, sc["tp"].world_radius, what)
    st = got[1]
    assert (st["fast"] == 0).all() and (st["tcounts"][:, 0] - sc["st0"]["tcounts"][:, 0] == reached).all()
    assert (st["tcounts"][:, 3] - sc["st0"]["tcounts"][:, 3] == (sc["status"] != 0)).all() and st["tcounts"][9, 4] == sc["st0"]["tcounts"][9, 4] + 1
    _bits(st["target"][~reached], sc["st0"]["target"][~reached], "a vehicle that has not reached keeps its target")
    assert (np.linalg.norm(st["target"][reached] - got[0][reached, :3], axis=1) >= 1.5 - 1e-9).all()          # sampled away from the reach


def test_plant_target_kernel_with_one_vehicle_and_with_fast_ones():
    """B = 1 under both kernels; then `fast`: signed, a NaN compares false, from the state at the START of the period."""
    L = TQ._lib()
    for noisy in (False, True):
        sc = plant_scenario(True, noisy, noisy)
        one = {k: v[1:2].copy() for k, v in sc["st0"].items()}
        one["target_no"] = np.array([5], dtype=np.uint64)
        plant, tp, noise = sc["plant"], sc["tp"], sc["noise"]
        st, x, step = TS.copy_state(one), sc["X"][1:2].copy(), np.array([9], dtype=np.uint64)
        # vehicle 0 of a batch of one: its own draws and its own target stream, whatever it was in the fleet of 67
        free = _free_flight(plant, noise, x, sc["U"][1:2], step)
        one["target"][0] = st["target"][0] = free[0][10]
        nsub, margins, _ = TS.plant_step(plant, tp, noise, st, x, sc["U"][1:2], noise_step=step if noise is not None else None)
        assert nsub[0] == 11 and np.abs(margins[0]).min() >= 1e-9
        got = _run_step(L, plant, tp, noise, sc["X"][1:2], sc["U"][1:2], one, np.array([9], dtype=np.uint64))
        _same_period(got, (x, st, nsub, step if noise is not None else None), nsub, tp.world_radius, "B = 1, noisy=%s" % noisy)
    X, U = QS.fleet67()
    X, U = X[:8].copy(), U[:8].copy()
    X[:, 7:10] = [[14.5, 0, 0], [0, 14.0, 0], [0, 0, 14.0000001], [-30.0, 0, 0], [np.nan, 1.0, 1.0], [np.nan, 0, 20.0], [0, np.inf, 0], [1.0, 2.0, 3.0]]
    plant = _plant(False, 2)
    st0 = _initial_state(8, X[:, :3] + 50.0)
    st = _run_step(L, plant, _tp(thresh=THRESH), None, X, U, st0)[1]
    assert st["fast"].tolist() == [1, 0, 1, 0, 0, 1, 1, 0]


@pytest.mark.parametrize("noisy", [False, True])
def test_plant_target_kernel_past_the_grid(noisy):
    """B = 4096 * 64 + 301 with 2 sub-steps, drag on: one lane per vehicle in both kernels, the stride loop runs and the last wave is
    partial.  The targets lie on the deterministic flight of vehicle b mod 67 (b % 3: fifty metres away, behind sub-step 1, behind
    sub-step 2; the disturbances move a vehicle by 1e-7 m in two sub-steps, THRESH is 1e-4).  Held against the spec on the sample
    test_noisy_plant_past_the_grid takes: the last 301 vehicles and every 997th."""
    L = TQ._lib()
    B = QS.PAST_THE_GRID
    X, U = QS.fleet67()
    t = np.arange(B) % 67
    plant, noise, tp = _plant(True, 2), _noise(noisy, noisy), _tp(thresh=THRESH)
    free = np.stack(_free_flight(plant, None, X, U, None))                                      # [67, 2, 3]
    kind = np.arange(B) % 3
    targets = np.where((kind == 0)[:, None], X[t, :3] + 50.0, free[t, np.maximum(kind - 1, 0)])
    st0 = dict(target=targets, target_no=np.arange(B, dtype=np.uint64) % np.uint64(7), n_iter=(np.arange(B) % 5).astype(np.int32),
               fast=np.zeros(B, dtype=np.int32), tcounts=np.zeros((B, 5), dtype=np.int32))
    step0 = np.full(B, 5, dtype=np.uint64)
    got = _run_step(L, plant, tp, noise, X[t], U[t], st0, step0)
    sample = np.unique(np.concatenate([np.arange(0, B, 997), np.arange(B - 301, B)]))
    assert sample.max() == B - 1 and (sample >= 4096 * 64).sum() >= 301
    st = {k: v[sample].copy() for k, v in st0.items()}
    wx, wstep = X[sample % 67].copy(), step0[sample].copy()
    wn, margins, _ = TS.plant_step(plant, tp, noise, st, wx, U[sample % 67], noise_step=wstep if noise is not None else None, ids=sample)
    margins = [abs(v) for row in margins for v in row]
    assert min(margins) >= 1e-9
    assert {1, 2} <= set(wn.tolist()) and (st["target_no"] != st0["target_no"][sample]).sum() > 100
    want = (wx, st, wn, wstep if noise is not None else None)
    _same_period(got, want, wn, tp.world_radius, "past the grid, noisy=%s" % noisy, rows=sample)
    if noise is not None:
        assert (got[3] == 6).all()
    assert (got[2] >= 1).all() and (got[2] <= 2).all() and (got[1]["tcounts"][:, 2] == 1).all()


def _run_plain(L, plant, noise, X, U, noise_step):
    """admpc_quad_plant_step_batch or, with a noise, admpc_quad_plant_step_noise_batch on copies: (x [B,13], noise_step afterwards or None)."""
    x, u, ns = _dev(X), _dev(U), None
    if noise is None:
        rc = L.admpc_quad_plant_step_batch(C.byref(plant), 0, X.shape[0], _p(u), 4, _p(x), _stream())
    else:
        ns = _dev(np.asarray(noise_step, dtype=np.uint64).view(np.int64))
        rc = L.admpc_quad_plant_step_noise_batch(C.byref(plant), C.byref(noise), 0, X.shape[0], _p(u), 4, _p(x), _p(ns), _stream())
    assert rc == 0, L.admpc_last_error()
    return _host(x), (None if ns is None else _host(ns).view(np.uint64))


NO_TARGET_CASES = [(n, m, B, 13) for n, m in SWITCHES for B in (1, 67)] + [(True, True, NS.WIDE_MAX, 13), (True, True, NS.WIDE_MAX + 1, 5)]


@pytest.mark.parametrize("noisy,motor_noise,B,substeps", NO_TARGET_CASES)
def test_plant_where_no_target_can_matter_equals_the_plain_plant_bit_for_bit(noisy, motor_noise, B, substeps):
    """The plant towards targets and the noisy plant are one kernel text (TARGET on and off); the deterministic plant has its own.
    Where no target can be reached -- every vehicle DONE (mode 0, one preset, target number 1), or a threshold of 1e-300 -- the target
    step leaves x and noise_step as the plain step of the same inputs does, bit for bit, and nsub == substeps.  Device against device,
    drag on.  B = 1: vehicle 9 of QS.fleet67 alone, whose NaN activation is replaced; B = 67: five blocks of 16 vehicles with a partial
    last one under four lanes a vehicle, two waves under one; 13 sub-steps cross the chunk of 10 that four lanes have.  Under the
    disturbances also the largest fleet with four lanes a vehicle and the smallest with one (5 sub-steps: chunks of 2)."""
    L = TQ._lib()
    X67, U67 = QS.fleet67()
    t = np.array([9]) if B == 1 else np.arange(B) % 67
    X, U = X67[t].copy(), U67[t].copy()
    assert np.isnan(U).any()
    plant, noise, step0 = _plant(True, substeps), _noise(noisy, motor_noise), _numbers(B)
    wx, wstep = _run_plain(L, plant, noise, X, U, step0)
    assert not np.isnan(wx).any() and not np.array_equal(wx, X)
    presets = (X[:, None, :3] + 50.0).copy()
    done = dict(target=presets[:, 0].copy(), target_no=np.ones(B, dtype=np.uint64), n_iter=(np.arange(B) % 5).astype(np.int32),
                fast=np.full(B, 7, dtype=np.int32), tcounts=(np.arange(B * 5).reshape(B, 5) % 11).astype(np.int32))
    far = dict(done, target_no=_numbers(B))
    for what, tp, st0, pre in (("done", _tp(mode="preset", thresh=THRESH, n_preset=1, seed=None), done, presets),
                               ("thresh = 1e-300", _tp(mode="aggressive", thresh=1e-300), far, None)):
        gx, st, nsub, gstep = _run_step(L, plant, tp, noise, X, U, st0, step0, presets=pre)
        _bits(gx, wx, "x, " + what)
        assert (nsub == substeps).all()
        if noise is not None:
            _bits(gstep, wstep, "noise_step, " + what)
            _bits(gstep, step0 + np.uint64(1), "noise_step advanced by one, " + what)
        _bits(st["target"], st0["target"], "target, " + what); _bits(st["target_no"], st0["target_no"], "target_no, " + what)
        counted = 0 if what == "done" else 1                                                     # a DONE vehicle counts nothing any more
        want_tc = st0["tcounts"].copy()
        want_tc[:, 2] += counted
        want_tc[:, 4] += counted * np.isnan(U).any(axis=1)
        _bits(st["tcounts"], want_tc, "tcounts, " + what); _bits(st["n_iter"], st0["n_iter"] + np.int32(counted), "n_iter, " + what)
        assert (st["fast"] == 0).all()


def test_presets_the_last_one_reached_then_done():
    """Three vehicles with two presets each on their flown path (tests/test_quad_targets_cpu.py has the same flight in the spec): the
    first reached behind sub-step 3, the second behind sub-step 2 of the next period, then full periods and nothing counted."""
    L = TQ._lib()
    plant = _plant(True, 8)
    X, U = QS.fleet67()
    X, U = X[:3].copy(), U[:3].copy()
    tp = _tp(mode="preset", thresh=THRESH, n_preset=2, seed=None)
    free = _free_flight(plant, None, X, U, None)
    presets = np.stack([np.stack([free[b][2], free[b][4]]) for b in range(3)])
    st, x = TS.reset(tp, X, presets), X.copy()
    dst, dx = TS.copy_state(st), X.copy()
    for period, want_nsub in enumerate(([3] * 3, [2] * 3, [8] * 3, [8] * 3)):
        nsub, margins, _ = TS.plant_step(plant, tp, None, st, x, U, presets=presets)
        assert nsub.tolist() == want_nsub and min(abs(m) for row in margins for m in row) >= 1e-9
        dx, dst, dn, _ = _run_step(L, plant, tp, None, dx, U, dst, presets=presets)
        _same_period((dx, dst, dn, None), (x, st, nsub, None), np.full(3, 8 * (period + 1), dtype=np.int32), tp.world_radius, "presets, period %d" % period)
    assert dst["target_no"].tolist() == [2] * 3 and dst["tcounts"][:, [0, 2]].tolist() == [[2, 2]] * 3 and dst["n_iter"].tolist() == [1] * 3
    _bits(dst["target"], presets[:, 1], "a done vehicle keeps its last preset")


# ---- 3. the window and the recovery -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [10, 20])
def test_window_and_recovery_equal_the_spec_bit_for_bit(N):
    """B = 67.  Vehicle 0: fast set; 1: n_iter == max_iters (no recovery); 2: n_iter == max_iters + 1 (recovery); 3: a NaN velocity and
    fast 0 (no recovery); 4: fast and n_iter both; every other vehicle: neither.  Then with a latch: prev re-latched at a recovery only."""
    import torch
    L = TQ._lib()
    B = 67
    X = QS.random_states(B, 5)
    X[3, 8] = np.nan
    tp = _tp(max_iters=9)
    st0 = _initial_state(B, QS.random_states(B, 6)[:, :3])
    st0["fast"][:] = 0; st0["fast"][[0, 4]] = [1, -3]
    st0["n_iter"][:] = np.arange(B) % 9; st0["n_iter"][[1, 2, 4]] = [9, 10, 50]
    for with_prev in (False, True):
        prev0 = QS.random_states(B, 7)
        st, x, prev = TS.copy_state(st0), X.copy(), prev0.copy()
        yref, yref_e, rec = TS.window(tp, st, x, N, prev if with_prev else None)
        assert np.flatnonzero(rec).tolist() == [0, 2, 4]
        d = {k: _dev(v.view(np.int64) if v.dtype == np.uint64 else v) for k, v in st0.items()}
        dx, dprev = _dev(X), _dev(prev0)
        dy = torch.full((B, N, 17), float("nan"), dtype=torch.float64, device="cuda:0")
        dye = torch.full((B, 13), float("nan"), dtype=torch.float64, device="cuda:0")
        rc = L.admpc_quad_target_window_batch(C.byref(tp), 0, B, N, _p(dx), _p(d["target"]), None, _p(d["n_iter"]), _p(d["fast"]), _p(d["tcounts"]),
                                              _p(dprev if with_prev else None), _p(dy), _p(dye), _stream())
        assert rc == 0, L.admpc_last_error()
        _bits(_host(dy), yref, "yref"); _bits(_host(dye), yref_e, "yref_e")
        _bits(_host(dx), x, "x: the recovered vehicles on their targets, the others untouched")
        _bits(_host(dprev), prev if with_prev else prev0, "prev")
        for k in ("n_iter", "fast", "tcounts", "target"):
            _bits(_host(d[k]), st[k], k)
        assert (st["tcounts"][:, 1] - st0["tcounts"][:, 1] == rec).all() and (st["n_iter"][rec] == 0).all()
        assert np.array_equal(x[0], TS.row_of(st0["target"][0])) and np.isnan(_host(dx)[3, 8])


# ---- 4. the observation over the flown time -----------------------------------------------------------------------------------------

def _observe_var(eng, plant, obs, prev, now, U, nsub):
    import torch
    B = prev.shape[0]
    x, pv, u = _dev(now), _dev(prev), _dev(U)
    samples = torch.full((B, 14), 7.0, dtype=torch.float64, device="cuda:0")
    bn, dr = _dev(np.zeros((3, 32, 5))), _dev(np.zeros(4, dtype=np.int32))
    rc = eng.lib.admpc_quad_observe_var_batch(eng._h, C.byref(plant), C.byref(obs), B, _p(u), 4, _p(x), _p(pv), _p(_dev(np.asarray(nsub, dtype=np.int32))),
                                              _p(samples), _p(bn), _p(dr), _stream())
    assert rc == 0, eng.lib.admpc_last_error()
    return _host(samples), _host(pv), _host(bn), _host(dr)


@pytest.mark.parametrize("kind,M", [("nominal", 1), ("gp", 4)])
def test_observation_over_the_flown_time(kind, M):
    """B = 67 of tests/test_quad_learn_gpu.py's fleet (a NaN activation, a NaN in the state now and one in the state before).  With
    nsub == substeps everywhere: samples, prev, bins and dropped bit for bit admpc_quad_observe_batch's.  With mixed nsub: against
    tests/quad_learn_spec.py run at dt_b, at that file's bound with dt_b in dt's place.  nsub = 0 and -1: invalid, and counted."""
    import test_quad_learn_gpu as TL
    import plant_spec as PS_
    from ad_mpc_amd.engine import QuadBatchSolver
    from oracle.quad_oracle import QuadOracle
    oracle = QuadOracle()
    cfg = TL._model_cfg(kind)
    plant, obs = TL._plant(), TL._obs(TL.THREE, substeps=M)
    S = int(plant.substeps)
    assert S == 40
    eng = QuadBatchSolver(cfg)
    try:
        B = 67
        prev, now, U = TL._fleet(B)
        full = _observe_var(eng, plant, obs, prev, now, U, np.full(B, S))
        old = TL._observe(eng, plant, obs, prev, now, U)
        for g, w, what in zip(full, old, ("samples", "prev", "bins", "dropped")):
            _bits(g, w, "%s of full periods against admpc_quad_observe_batch" % what)
        nsub = 1 + (np.arange(B) * 7) % S
        nsub[[0, 20, 40]] = S
        nsub[[1, 2]] = [0, -1]
        got, latched, bins, dropped = _observe_var(eng, plant, obs, prev, now, U, nsub)
        spec = [TS.record(oracle, cfg, plant, obs, prev[b], now[b], U[b], nsub[b]) for b in range(B)]
        want = np.stack([s[0] for s in spec])
        _bits(latched, now, "the latch")
        _bits(got[:, :10], want[:, :10], "features and activations")
        _bits(got[:, 13], want[:, 13], "the flag")
        assert (want[[1, 2, 11, 12], 13] == 0.0).all() and (want[:, 13] == 0.0).sum() == 4
        ok = want[:, 13] == 1.0
        dtb = np.array([TS.period_of(plant, obs, n) for n in nsub])
        vh = np.stack([QL.body_velocity(s[1]) for s in spec])
        G = np.array([PS_.chain_gain(s[2]) for s in spec])
        bound = M * G[ok] * 1e-12 * np.maximum(1.0, np.linalg.norm(vh[ok], axis=1)) / dtb[ok]
        ratio = np.linalg.norm(got[ok, 10:13] - want[ok, 10:13], axis=1) / bound
        print("%s, M = %d: largest |dy| over its bound %.3g" % (kind, M, ratio.max()))
        assert ratio.max() <= 1.0
        wb, wd = np.zeros((3, 32, 5)), np.zeros(4, dtype=np.int32)
        QL.accumulate(obs, got, wb, wd)                              # the bin launch is the existing one: its sums of THESE samples
        _bits(bins, wb, "bins"); _bits(dropped, wd, "dropped")
        assert dropped[3] == 4
    finally:
        eng.close()


# ---- 5. the rollout against the loop it replaces ------------------------------------------------------------------------------------

TARGET_STATE = ("x", "x_opt", "w_opt", "status", "yref", "yref_e", "cost", "iters", "target", "target_no", "n_iter", "fast", "tcounts", "nsub")
ROLL = dict(mode="aggressive", world_radius=0.3, thresh=0.12, max_iters=15)


def _fleet(B, N, learn=None, noisy=False, seed=SEED, **kw):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    fl = QuadFleet(B, quad=SimQuad(drag=True, noisy=noisy, motor_noise=noisy), n_nodes=N, learn=learn, noise_seed=NOISE_SEED if noisy else None)
    fl.set_targets(seed=seed, **dict(ROLL, **kw))
    return fl


def _start(B, seed):
    x0 = np.tile(np.array([0.0, 0.0, 1.0, 1.0] + [0.0] * 9), (B, 1))
    x0[:, :3] += np.random.default_rng(seed).uniform(-0.5, 0.5, (B, 3))
    return x0


def _state(fl):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(fl, k).cpu().numpy() for k in TARGET_STATE}


def _loop(fl, T, observe):
    """The loop rollout_targets replaces, every step a call of its own: (traj [T+1,B,13], u, nsub, targets)."""
    traj, us, ns, tg = [], [], [], []
    if observe:
        fl.observe_latch()
    for t in range(T):
        fl.target_window()
        if t == 0:
            traj.append(_host(fl.x))
        tg.append(_host(fl.target))
        fl._eng.solve(fl.x, fl.yref, fl.yref_e, fl.x_opt, fl.w_opt, fl.cost, fl.status, fl.iters)
        us.append(_host(fl.w_opt)[:, 0, :].copy())
        fl.plant_step_targets()
        if observe:
            fl.observe_targets()
        traj.append(_host(fl.x)); ns.append(_host(fl.nsub))
    return np.stack(traj), np.stack(us), np.stack(ns), np.stack(tg)


@pytest.mark.parametrize("N,T,noisy,observe", [(10, 40, False, False), (10, 40, True, True), (20, 40, False, True), (20, 30, True, False)])
def test_rollout_targets_equals_the_loop_it_replaces(N, T, noisy, observe):
    """B = 5 from scattered starts, targets 0.15 .. 0.45 m away, reached within 12 cm, a recovery behind 15 periods on one target.
    Every record and every piece of state bit for bit, and in the run itself: a vehicle that reaches at least two targets, one that
    reaches mid-period, one that is recovered."""
    B = 5
    x0 = _start(B, N)
    learn = QL.EXP_LEARN if observe else None
    whole, loop = (_fleet(B, N, learn=learn, noisy=noisy) for _ in range(2))
    try:
        for fl in (whole, loop):
            fl.reset_targets(x0)
        out = whole.rollout_targets(T, record=True, observe=observe)
        traj, us, ns, tg = _loop(loop, T, observe)
        got, want = _state(whole), _state(loop)
        for k in TARGET_STATE:
            _bits(got[k], want[k], k)
        _bits(_host(out.traj), traj, "traj_out"); _bits(_host(out.u), us, "u_out")
        _bits(_host(out.nsub), ns, "nsub_out"); _bits(_host(out.targets), tg, "target_out")
        if noisy:
            _bits(_host(whole.noise_step), _host(loop.noise_step), "noise_step")
            assert (_host(whole.noise_step) == T).all()
        if observe:
            for k in ("samples", "bins", "dropped", "_prev"):
                _bits(_host(getattr(whole, k)), _host(getattr(loop, k)), k)
            bins, dropped = _host(whole.bins), _host(whole.dropped)
            assert (bins[:, :, 0].sum(axis=1) + dropped[:3] + dropped[3] == B * T).all()
        tc, S = got["tcounts"], int(whole._plant.substeps)
        print("N = %d noisy=%s: reached %s, recovered %s, nsub < substeps in %d periods, statuses != 0: %s"
              % (N, noisy, tc[:, 0].tolist(), tc[:, 1].tolist(), int((ns < S).sum()), tc[:, 3].tolist()))
        assert (tc[:, 2] == T).all() and (tc[:, 0] == got["target_no"].astype(np.int64)).all()
        assert tc[:, 0].max() >= 2, "a vehicle reaches at least two targets"
        assert ((ns > 0) & (ns < S)).any(), "a vehicle reaches mid-period"
        assert tc[:, 1].max() >= 1, "a vehicle is recovered"
        assert ((ns < S).sum(axis=0) <= tc[:, 0]).all()                                          # a period cut short is a reach
        assert (tc[:, 0] > tc[:, 1]).any(), "a vehicle reaches a target by flying, not only behind a recovery"
    finally:
        whole.close(); loop.close()


def test_rollout_targets_no_ops_and_refusals_in_their_order():
    """T = 0 changes nothing and returns the start in slot 0; then the refusals that need a handle, in the header's order."""
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config
    fl = _fleet(3, 10)
    sqp_cfg = default_quad_config(N=10)
    sqp_cfg.sqp_iters, sqp_cfg.sqp_tol = 5, 1e-6
    sqp = QuadBatchSolver(sqp_cfg)
    try:
        fl.reset_targets()
        before = _state(fl)
        out = fl.rollout_targets(0, record=True)
        after = _state(fl)
        for k in TARGET_STATE:
            _bits(after[k], before[k], "%s after T = 0" % k)
        assert out.traj.shape == (1, 3, 13) and out.nsub.shape == (0, 3) and np.array_equal(_host(out.traj)[0], before["x"])
        assert (before["x"] == [[0, 0, 0, 1] + [0] * 9] * 3).all() and (np.linalg.norm(before["target"], axis=1) >= 0.5 * ROLL["world_radius"] - 1e-12).all()
        L = fl.lib

        def roll(s=fl._eng._h, B=3, T=2, x=_p(fl.x), nsub=_p(fl.nsub), model=None, obs=None, tp=fl._tp):
            return L.admpc_quad_rollout_targets_batch(s, C.byref(fl._plant), C.byref(tp), B, T, x, _p(fl.x_opt), _p(fl.w_opt), _p(fl.yref), _p(fl.yref_e),
                                                      _p(fl.cost), _p(fl.status), _p(fl.iters), None, _p(fl.target), _p(fl.target_no), _p(fl.n_iter),
                                                      _p(fl.fast), _p(fl.tcounts), nsub, None, None, None, None, model, obs, None, None, None, None,
                                                      None, None, _stream())

        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        refused(roll(s=sqp._h, B=-1), "SQP mode")                                                # SQP before the batch
        refused(roll(B=-1, T=5000), "negative batch")
        refused(roll(T=4097, x=None), "T must be in [0, 4096]")
        refused(roll(T=-1, x=None), "T must be in [0, 4096]")
        refused(roll(x=None), "null array")
        refused(roll(nsub=None), "null array")
        assert roll(B=0, x=None) == 0 and roll(T=0, x=None) == 0
        with pytest.raises(ValueError, match="does not learn"):
            fl.rollout_targets(2, observe=True)
        with pytest.raises(ValueError, match="T must be in"):
            fl.rollout_targets(4097)
        other = _fleet(3, 10)
        try:
            with pytest.raises(ValueError, match="call reset_targets first"):
                other.rollout_targets(1)
        finally:
            other.close()
    finally:
        sqp.close(); fl.close()


# ---- 6. graph -----------------------------------------------------------------------------------------------------------------------

def test_captured_rollout_targets_advances_on_the_device():
    """rollout_targets(3) at B = 5 captured and replayed twice WITHOUT a reset in between equals six eager periods bit for bit: the
    targets, the counters and the noise counters live on the device."""
    import torch
    N, B, T = 10, 5, 3
    x0 = _start(B, 3)
    kw = dict(world_radius=0.3, thresh=0.15, max_iters=2)                                       # reaches and recoveries within six periods
    eager, graphed = (_fleet(B, N, noisy=True, **kw) for _ in range(2))
    try:
        graphed.reset_targets(x0)
        graphed.rollout_targets(T)                                   # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = graphed.rollout_targets(T, record=True)
        graphed.reset_targets(x0); graphed.reseed(step=0)
        eager.reset_targets(x0)
        ref = eager.rollout_targets(2 * T, record=True)
        rt, ru, rn, rg = _host(ref.traj), _host(ref.u), _host(ref.nsub), _host(ref.targets)
        for r in range(2):
            g.replay()
            _bits(_host(out.traj)[1:], rt[r * T + 1:(r + 1) * T + 1], "traj at replay %d" % r); _bits(_host(out.u), ru[r * T:(r + 1) * T], "u at replay %d" % r)
            _bits(_host(out.nsub), rn[r * T:(r + 1) * T], "nsub at replay %d" % r); _bits(_host(out.targets), rg[r * T:(r + 1) * T], "targets at replay %d" % r)
        want, got = _state(eager), _state(graphed)
        for k in TARGET_STATE:
            _bits(got[k], want[k], "%s after two replays" % k)
        assert (_host(graphed.noise_step) == 2 * T).all() and (got["tcounts"][:, 2] == 2 * T).all()
        assert got["tcounts"][:, 0].sum() >= 1 and got["tcounts"][:, 1].sum() >= 1
    finally:
        eager.close(); graphed.close()


# ---- 7. the experiment --------------------------------------------------------------------------------------------------------------

RATIO_MEASURED = dict(fit_gp=[0.151, 0.464, 0.089], search_gp=[0.073, 0.186, 0.071])         # per axis, measured on the MI355X


def _residual_rms(fl, model, out, T):
    """The RMS per axis of what `model` does not predict of the recorded flight `out`, all B * T periods observed in one call."""
    import torch
    B = fl.B
    traj = out.traj
    prev, now = traj[:-1].reshape(B * T, 13).clone(), traj[1:].reshape(B * T, 13).contiguous()
    u, nsub = out.u.reshape(B * T, 4).contiguous(), out.nsub.reshape(B * T).contiguous()
    samples = torch.zeros((B * T, 14), dtype=torch.float64, device=fl.device)
    bins, dropped = torch.zeros((3, 32, 5), dtype=torch.float64, device=fl.device), torch.zeros(4, dtype=torch.int32, device=fl.device)
    rc = fl.lib.admpc_quad_observe_var_batch(model._h, C.byref(fl._plant), C.byref(fl._obs), B * T, _p(u), 4, _p(now), _p(prev), _p(nsub),
                                                     _p(samples), _p(bins), _p(dropped), _stream())
    assert rc == 0, fl.lib.admpc_last_error()
    S = _host(samples)
    assert (S[:, 13] == 1.0).all()
    return QL.rms(S)


def test_the_experiment_flies_to_targets_learns_and_flies_again():
    """64 vehicles, the drag plant, three one-feature regressors on the body velocity: an observed target flight, fit_gp (and search_gp),
    then a second target flight under another seed.  Its residual under the learned GPs over that under the nominal model, per axis,
    is below 1 and below twice what was measured on the MI355X (fit_gp 0.151, 0.464, 0.089; search_gp 0.073, 0.186, 0.071; the circles
    122.6 m).  Then the 5 m circle flight of tests/test_quad_learn_gpu.py under the
    GPs learned from targets, next to that file's figures (532.9 m nominal, 120.6 m learned from circles): reported, not asserted."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, B, T = 10, 64, 60
    fl = _fleet(B, N, learn=QL.EXP_LEARN, world_radius=3.0, thresh=0.05, max_iters=100)
    try:
        fl.reset_targets()
        fl.rollout_targets(T, observe=True)
        bins, dropped, tc = _host(fl.bins), _host(fl.dropped), _host(fl.tcounts)
        assert (bins[:, :, 0].sum(axis=1) + dropped[:3] + dropped[3] == B * T).all() and dropped[3] == 0
        ratios = {}
        for how in ("fit_gp", "search_gp"):
            if how == "fit_gp":
                info, installed = fl.fit_gp(min_count=2)
            else:
                info, installed = fl.search_gp(min_count=2)[:2]
            assert min(_host(info).tolist()) >= 2 and _host(installed).tolist() == [1, 1, 1]
            fl.set_targets(seed=SEED + 1, world_radius=3.0, thresh=0.05, max_iters=100)
            fl.reset_targets()
            out = fl.rollout_targets(T, record=True)
            assert (_host(fl.tcounts)[:, 1] == 0).all()                                          # no recovery: slot t + 1 is where period t + 1 starts
            nominal, learned = _residual_rms(fl, fl._nominal, out, T), _residual_rms(fl, fl._eng, out, T)
            ratios[how] = learned / nominal
            print("%s: held-out residual RMS per axis: nominal %s, learned %s, ratio %s; targets reached in the second flight: %d"
                  % (how, nominal, learned, ratios[how], int(_host(fl.tcounts)[:, 0].sum())))
        print("first flight: %d targets reached, %d recoveries" % (tc[:, 0].sum(), tc[:, 1].sum()))
        dt = 1.0 / (N * 5)
        trajs = [circle_reference(60 + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
        fl.set_trajectories(trajs)
        fl.reset((np.arange(B) % 4).astype(np.int32), (np.arange(B) // 4).astype(np.int32))
        fl.rollout(60)
        total = float(_host(fl.tally)[:, 0].sum())
        print("the 5 m circles under the GPs learned from targets: sum of |e| over 60 steps of 64 vehicles %.6g m (532.9 m nominal, 120.6 m learned from circles)" % total)
        for how, r in ratios.items():
            assert (r < 1.0).all(), (how, r)
            assert (r < 2.0 * np.array(RATIO_MEASURED[how])).all(), (how, r)
    finally:
        fl.close()
