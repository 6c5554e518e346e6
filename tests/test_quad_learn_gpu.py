"""Learning the quadrotor's body-frame residual GPs on the device (include/admpc_quad_learn.h; ad_mpc_amd/quad_fleet.py: learn=).

The record is compared with its numpy restatement (tests/quad_learn_spec.py: one oracle RK4 step per sub-step): features, activations,
flag and latch bit for bit, y at the car's record bound carried through the chain gain of the sub-step Jacobians; the bins and the
dropped counts bit for bit; the fit bit for bit against the car's fit of the same statistics; the install by the solve of a handle
created with the same GPs; the rollout with observation by the loop it replaces; then the learning experiment and a short closed loop."""
import ctypes as C

import numpy as np
import pytest

import learn_spec as LS
import plant_spec as PS
import quad_learn_spec as QL
import quad_plant_spec as QS
import test_quad_fleet_gpu as TQ

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _lib, _stream = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._lib, TQ._stream
DT = 0.02
THREE = [dict(feat=7, out=7, lo=[-4.0], hi=[4.0], bins=[32], length_scale=2.0),
         dict(feat=[8, 12], out=8, lo=[-4.0, -1.5], hi=[4.0, 1.5], bins=[8, 4], length_scale=[2.0, 1.0], noise=1e-4),
         dict(feat=[9, 13, 16], out=9, lo=[-6.0, 0.0, 0.0], hi=[6.0, 1.0, 1.0], bins=[4, 2, 4], length_scale=[3.0, 0.5, 0.5], noise=1e-4, count_noise=0.01)]


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def quad_oracle():
    from oracle.quad_oracle import QuadOracle
    return QuadOracle()


def _obs(learn, dt=DT, substeps=1):
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, quad_learn_bins
    bins, n = quad_learn_bins(learn)
    return AdmpcQuadObserveParams(dt=dt, substeps=substeps, n_gp=n, gp=bins)


def _plant(dt=DT):
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    return quad_plant_params(SimQuad(drag=True), 5e-4, dt)


def _model_cfg(kind):
    """The three models of the record test: nominal; with the linear rotor drag; with three GPs of 8, 12 and 32 points."""
    from ad_mpc_amd.quad_config import default_quad_config, set_quad_gp
    cfg = default_quad_config(N=10)
    if kind == "rdrv":
        cfg.rdrv[0], cfg.rdrv[1], cfg.rdrv[2] = -0.3, -0.25, -0.1
    if kind == "gp":
        rng = np.random.default_rng(5)
        gps = []
        for d, n in zip(THREE, (8, 12, 32)):
            nf = len(d["lo"])
            Z = np.stack([rng.uniform(d["lo"][k], d["hi"][k], n) for k in range(nf)], axis=1)
            gps.append(dict(feat=d["feat"], out=d["out"], Z=Z, alpha=rng.normal(size=n) * 0.5, length_scale=d["length_scale"], sigma_f=0.8, ymean=0.1))
        set_quad_gp(cfg, gps)
    return cfg


_FLEET = {}


def _fleet(B):
    """(prev [B,13], now [B,13], U [B,4]): the 67 vehicles of the plant tests tiled -- vehicle 5 level with v_y = 0, vehicle 9 with a NaN
    activation -- every copy moved a little; `now` is one 20 ms period of the drag plant by the spec.  Where B > 12, vehicle 11 has a NaN
    in the state now and vehicle 12 in the state before."""
    if "base" not in _FLEET:
        X, U = QS.fleet67()
        _FLEET["base"] = (X, U, QS.step_fleet(_plant(), X, U)[0])
    X, U, now = _FLEET["base"]
    t = np.arange(B) % 67
    rng = np.random.default_rng(B)
    shift = np.where((np.arange(B) >= 67)[:, None], rng.uniform(-1e-3, 1e-3, (B, 13)), 0.0)
    prev, now, U = X[t] + shift, now[t] + shift, U[t].copy()
    if B > 12:
        now[11, 8] = np.nan
        prev[12, 10] = np.nan
    return prev, now, U


def _observe(eng, plant, obs, prev, now, U, bins=None, dropped=None, stride=4):
    """admpc_quad_observe_batch on copies: (samples [B,14], prev afterwards [B,13], bins [3,32,5], dropped [4])."""
    import torch
    B = prev.shape[0]
    x, pv = _dev(now), _dev(prev)
    u = torch.full((B, stride), float("nan"), dtype=torch.float64, device="cuda:0")
    u[:, :4] = _dev(U)
    samples = torch.full((B, 14), 7.0, dtype=torch.float64, device="cuda:0")
    bn = _dev(np.zeros((3, 32, 5)) if bins is None else bins)
    dr = _dev(np.zeros(4, dtype=np.int32) if dropped is None else dropped, torch.int32)
    rc = eng.lib.admpc_quad_observe_batch(eng._h, C.byref(plant), C.byref(obs), B, _p(u), stride, _p(x), _p(pv), _p(samples), _p(bn), _p(dr), _stream())
    assert rc == 0, eng.lib.admpc_last_error()
    torch.cuda.synchronize()
    _bits(_host(x), now, "x is read-only")
    return _host(samples), _host(pv), _host(bn), _host(dr)


# ---- 1. the record against the spec -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("kind", ["nominal", "rdrv", "gp"])
def test_the_record_matches_the_spec(quad_oracle, kind, M):
    """B = 1, 63, 64, 65 (one past a block of one wave) and 67.  Features, activations, flag and latch bit for bit;
    |dy|_2 <= M * G * 1e-12 * max(1, |v^|_2) / dt with G the chain gain of the sub-step Jacobians and 1e-12 the figure
    tests/test_learn_gpu.py uses for the car's record.  Measured on the MI355X: the largest |dy| over its bound is 8.6e-5 (G up to 4.35)."""
    from ad_mpc_amd.engine import QuadBatchSolver
    cfg = _model_cfg(kind)
    plant, obs = _plant(), _obs(THREE[:1], substeps=M)
    eng = QuadBatchSolver(cfg)
    worst = 0.0
    try:
        for B in (1, 63, 64, 65, 67):
            prev, now, U = _fleet(B)
            S, latched, _, _ = _observe(eng, plant, obs, prev, now, U, stride=4 if B != 65 else 40)
            spec = [QL.record(quad_oracle, cfg, plant, obs, prev[b], now[b], U[b]) for b in range(B)]
            want = np.stack([s[0] for s in spec])
            vh = np.stack([QL.body_velocity(s[1]) for s in spec])
            G = np.array([PS.chain_gain(s[2]) if np.isfinite(np.array(s[2])).all() else 1.0 for s in spec])
            _bits(latched, now, "the latch, B = %d" % B)
            _bits(S[:, :10], want[:, :10], "features and activations, B = %d" % B)
            _bits(S[:, 13], want[:, 13], "the flag, B = %d" % B)
            assert (want[:, 13] == 0.0).sum() == (2 if B > 12 else 0)
            ok = want[:, 13] == 1.0
            bound = M * G[ok] * 1e-12 * np.maximum(1.0, np.linalg.norm(vh[ok], axis=1)) / DT
            ratio = np.linalg.norm(S[ok, 10:13] - want[ok, 10:13], axis=1) / bound
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (B, ratio.max())
            assert np.array_equal(np.isnan(S[~ok, 10:13]), np.isnan(want[~ok, 10:13]))
            if B > 12:
                assert np.abs(want[ok, 10:13]).max() > 0.1 and S[5, 1] == 0.0 and np.isnan(U[9, 2]) and S[9, 8] == plant.u_min
                assert (S[:, 6:10] == plant.u_min).any() and (S[:, 6:10] == plant.u_max).any()
        print("%s, M = %d: largest |dy| over its bound %.3g, G up to %.3g" % (kind, M, worst, G.max()))
    finally:
        eng.close()


# ---- 2. past the grid ---------------------------------------------------------------------------------------------------------------

def test_observe_past_the_grid():
    """B = 4096 * 64 + 301: the stride loop runs and the last block is partial; the latch and the flags only."""
    from ad_mpc_amd.engine import QuadBatchSolver
    B = QS.PAST_THE_GRID
    prev, now, U = _fleet(B)
    small = slice(0, 67)
    eng = QuadBatchSolver(_model_cfg("gp"))
    try:
        S, latched, _, dropped = _observe(eng, _plant(), _obs(THREE[:1]), prev, now, U)
        s67, _, _, _ = _observe(eng, _plant(), _obs(THREE[:1]), prev[small], now[small], U[small])
    finally:
        eng.close()
    _bits(latched, now, "the latch")
    assert (S[:, 13] == 0.0).sum() == 2 and S[11, 13] == 0.0 and S[12, 13] == 0.0 and set(S[:, 13].tolist()) == {0.0, 1.0}
    _bits(S[small], s67, "the first 67 against the batch of 67")
    assert dropped[3] == 2


# ---- 3. the bins from the device's own records --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_gp", [1, 3])
def test_bins_and_dropped_counts_match_the_spec_bit_for_bit(n_gp):
    from ad_mpc_amd.engine import QuadBatchSolver
    obs, plant = _obs(THREE[:n_gp]), _plant()
    eng = QuadBatchSolver(_model_cfg("nominal"))
    try:
        for B in (1, 63, 64, 65, 200):
            prev, now, U = _fleet(B)
            S, latched, bins, dropped = _observe(eng, plant, obs, prev, now, U)
            wb, wd = np.zeros((3, 32, 5)), np.zeros(4, dtype=np.int32)
            QL.accumulate(obs, S, wb, wd)
            _bits(bins, wb, "bins, B = %d" % B); _bits(dropped, wd, "dropped, B = %d" % B)
            # a second call accumulates on top of the first: other states, from the latch of the first
            now2 = now + np.random.default_rng(B).normal(size=now.shape) * 0.05
            S2, _, bins2, dropped2 = _observe(eng, plant, obs, latched, now2, U, bins, dropped)
            QL.accumulate(obs, S2, wb, wd)
            _bits(bins2, wb, "bins after two calls, B = %d" % B); _bits(dropped2, wd, "dropped after two calls, B = %d" % B)
            assert not wb[n_gp:].any() and (wb[:n_gp, :, 0].sum(axis=1) + wd[:n_gp] + wd[3] == 2 * B).all()
            if B >= 63:
                assert wb[0, :, 0].sum() > B and wd[0] > 0 and wd[3] == 2 + 1          # the NaN state of the first call is latched: vehicle 11 again
    finally:
        eng.close()


# ---- 4. the fit against the car's fit of the same statistics ------------------------------------------------------------------------

def _fit(entry, obs, stats, min_count, rows):
    import torch
    from ad_mpc_amd.config import AdmpcGp
    n = int(obs.n_gp)
    bins = _dev(stats[:rows])
    out = torch.full((rows * C.sizeof(AdmpcGp),), 0x5A, dtype=torch.uint8, device="cuda:0")
    info = torch.full((rows,), 77, dtype=torch.int32, device="cuda:0")
    assert entry(0, C.byref(obs), min_count, _p(bins), _p(out), _p(info), None) == 0, _lib().admpc_last_error()
    raw = _host(out).tobytes()
    return [AdmpcGp.from_buffer_copy(raw, g * C.sizeof(AdmpcGp)) for g in range(n)], _host(info)[:n]


def test_the_fit_equals_the_cars_fit_of_the_same_statistics():
    """Hand-made statistics through admpc_quad_gp_fit and, with features f - 4 and out - 4, through admpc_gp_fit: everything but feat
    and out bit for bit; then a non-finite target: the empty GP and info = -(k + 1)."""
    from ad_mpc_amd.config import AdmpcObserveParams, learn_bins
    L = _lib()
    learn = [dict(THREE[0], noise=1e-4, length_scale=0.8), THREE[1],
             dict(THREE[2], feat=[9, 10, 11], lo=[-6.0, -2.0, -2.0], hi=[6.0, 2.0, 2.0], length_scale=[3.0, 1.5, 1.5])]
    qobs = _obs(learn)
    car = [dict(d, feat=[f - 4 for f in np.atleast_1d(d["feat"])], out=d["out"] - 4) for d in learn]
    cbins, n = learn_bins(car)
    cobs = AdmpcObserveParams(dt=DT, blend_min=3.0, blend_max=5.0, substeps=1, n_gp=n, gp=cbins)
    rng = np.random.default_rng(21)
    stats = np.zeros((4, 32, 5))
    for g, fill in enumerate((32, 20, 27)):
        stats[g] = LS.hand_stats(qobs.gp[g], rng, fill)
    for case in ("finite", "nan target"):
        if case == "nan target":
            k = np.flatnonzero(stats[1, :, 0] >= 4)[2]
            stats[1, k, 4] = np.inf
        q, qi = _fit(L.admpc_quad_gp_fit, qobs, stats, 4, 3)
        c, ci = _fit(L.admpc_gp_fit, cobs, stats, 4, 4)
        _bits(qi, ci, "info, %s" % case)
        for g in range(3):
            nf = int(qobs.gp[g].n_feat)
            assert [q[g].feat[d] for d in range(3)] == [int(qobs.gp[g].feat[d]) if d < nf else 0 for d in range(3)] and q[g].out == qobs.gp[g].out
            assert [c[g].feat[d] for d in range(nf)] == [q[g].feat[d] - 4 for d in range(nf)] and c[g].out == q[g].out - 4
            for k in ("n_feat", "n_points", "sigma_f", "ymean"):
                assert getattr(q[g], k) == getattr(c[g], k), (k, g)
            _bits(np.array(q[g].inv_l2[:]), np.array(c[g].inv_l2[:]), "inv_l2"); _bits(np.array(q[g].alpha[:]), np.array(c[g].alpha[:]), "alpha")
            _bits(np.array([q[g].Z[d][:] for d in range(3)]), np.array([c[g].Z[d][:] for d in range(3)]), "Z")
            assert QL.install_ok(q[g])
        if case == "finite":
            assert qi.tolist() == [int((stats[g, :, 0] >= 4).sum()) for g in range(3)] and qi.min() >= 8 and np.abs(np.array(q[0].alpha[:])).max() > 0
        else:
            assert qi[1] == -3 and q[1].n_points == 0 and q[1].ymean == 0.0 and not any(q[1].alpha[:]) and qi[0] > 0 and qi[2] > 0


# ---- 5. install -----------------------------------------------------------------------------------------------------------------------

def _solve(eng, s):
    return eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["xbar"], s["ubar"])


def _install(eng, records):
    import torch
    raw = torch.as_tensor(np.frombuffer(b"".join(bytes(r) for r in records), dtype=np.uint8).copy(), device="cuda:0")
    inst = torch.full((len(records),), 7, dtype=torch.int32, device="cuda:0")
    assert eng.lib.admpc_quad_gp_install(eng._h, len(records), _p(raw), _p(inst), _stream()) == 0, eng.lib.admpc_last_error()
    return _host(inst).tolist()


@pytest.mark.parametrize("N,B", [(10, 65), (20, 8)])
def test_an_installed_gp_solves_as_a_handle_created_with_it(N, B):
    """N = 10: the one-wave kernel; N = 20: two cooperating waves per instance."""
    from ad_mpc_amd.config import AdmpcGp
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config, set_quad_gp
    from ad_mpc_amd.quad_scenarios import random_quad_scenarios
    base_cfg = default_quad_config(N=N, t_horizon=N / 10.0)
    gps = [dict(feat=list(np.atleast_1d(d["feat"])), out=d["out"], Z=np.zeros((0, len(d["lo"]))), alpha=[], length_scale=d["length_scale"]) for d in THREE]
    place = set_quad_gp(base_cfg.copy(), gps)
    full = _model_cfg("gp")
    want_cfg = base_cfg.copy()
    want_cfg.n_gp = 3
    for g in range(3):
        C.memmove(C.byref(want_cfg.gp[g]), C.byref(full.gp[g]), C.sizeof(AdmpcGp))
    s = random_quad_scenarios(B, base_cfg, seed=N)
    learner, fresh, empty = QuadBatchSolver(place), QuadBatchSolver(want_cfg), QuadBatchSolver(place)
    try:
        base = _solve(learner, s)
        good = [AdmpcGp.from_buffer_copy(bytes(want_cfg.gp[g])) for g in range(3)]
        assert all(QL.install_ok(r) for r in good)
        assert _install(learner, good) == [1, 1, 1]
        got, want = _solve(learner, s), _solve(fresh, s)
        for a, b, what in zip(got, want, ("xbar", "ubar", "cost", "status", "iters")):
            _bits(a, b, "%s of the installed handle against the one created with the GPs" % what)
        assert np.nanmax(np.abs(got[1] - base[1])) > 1e-6                      # the GPs act
        assert learner.cfg.gp[0].n_points == 0                                 # the host copy is not changed
        # records the install refuses are installed as the empty GP: the solves are the placeholder handle's again
        nan_alpha, feat6, out10 = (AdmpcGp.from_buffer_copy(bytes(r)) for r in good)
        nan_alpha.alpha[5] = np.nan
        feat6.feat[1] = 6
        out10.out = 10
        assert not any(QL.install_ok(r) for r in (nan_alpha, feat6, out10))
        assert _install(learner, [nan_alpha, feat6, out10]) == [0, 0, 0]
        for a, b, what in zip(_solve(learner, s), _solve(empty, s), ("xbar", "ubar", "cost", "status", "iters")):
            _bits(a, b, "%s with every GP replaced by the empty one" % what)
        assert _install(learner, [good[0], feat6, good[2]]) == [1, 0, 1]
    finally:
        for e in (learner, fresh, empty):
            e.close()


# ---- 6. the rollout with observation against the loop it replaces -------------------------------------------------------------------

LEARN_STATE = ("bins", "dropped", "samples", "_prev")


def _learning_fleet(B, N, trajs, traj_of, idx0, x0, learn=None):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    fl = QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, learn=QL.EXP_LEARN if learn is None else learn)
    fl.set_trajectories(trajs)
    fl.reset(traj_of, idx0, x0)
    return fl


def test_rollout_with_observe_equals_the_loop_it_replaces():
    """N = 10, B = 67, T = 4.  `whole`: one rollout with observe; `loop`: observe_latch, then per step rollout(1) and observe();
    `plain`: the rollout without observation, whose state, records, tally and counts the observation must not change."""
    N, B, T = 10, 67, 4
    trajs = TQ._circles(N, 3.0)
    traj_of = (np.arange(B) % 2).astype(np.int32)
    idx0 = np.where(traj_of == 1, 3, (np.arange(B) * 3) % 110).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=6)
    whole, loop, plain = (_learning_fleet(B, N, trajs, traj_of, idx0, x0) for _ in range(3))
    try:
        out = whole.rollout(T, record=True, observe=True)
        ref = plain.rollout(T, record=True)
        loop.observe_latch()
        for t in range(T):
            loop.rollout(1)
            loop.observe()
        got, want, other = TQ._state(whole), TQ._state(loop), TQ._state(plain)
        for k in TQ.STATE + ("tally", "cost", "iters"):
            _bits(got[k], want[k], "%s at the end" % k); _bits(got[k], other[k], "%s against the plain rollout" % k)
        for k in LEARN_STATE:
            _bits(_host(getattr(whole, k)), _host(getattr(loop, k)), k)
        _bits(_host(out.traj), _host(ref.traj), "traj: a slot per step, as the plain rollout records it")
        _bits(_host(out.u), _host(ref.u), "u: a slot per step")
        assert np.array_equal(_host(out.traj)[0], x0) and np.array_equal(_host(out.traj)[T], got["x"])
        bins, dropped = _host(whole.bins), _host(whole.dropped)
        assert (got["counts"] == [T, 0, 0]).all() and dropped[3] == 0 and not _host(plain.bins).any()
        assert (bins[:, :, 0].sum(axis=1) + dropped[:3] == B * T).all() and bins[0, :, 0].sum() > B
        _bits(_host(whole._prev), got["x"], "the latch holds the final states")
        assert np.abs(_host(whole.samples)[:, 10:13]).max() > 0.1
    finally:
        for fl in (whole, loop, plain):
            fl.close()


# ---- 7. graph replay ----------------------------------------------------------------------------------------------------------------

def test_a_captured_rollout_reads_a_gp_installed_after_capture():
    """rollout(1) captured (one linear chain: window, solve, plant); then, outside the graph, statistics are fitted and installed; the
    next replay equals the eager step of a fleet that did the same, bit for bit, and differs from the step without the GPs."""
    import torch
    N, B = 10, 67
    trajs = TQ._circles(N, 3.0)
    traj_of = np.zeros(B, dtype=np.int32)
    idx0 = ((np.arange(B) * 3) % 100).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=9)
    eager, graphed = (_learning_fleet(B, N, trajs, traj_of, idx0, x0) for _ in range(2))
    try:
        graphed.rollout(1)                                          # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.rollout(1)
        eager.reset(traj_of, idx0, x0)
        eager.rollout(1)
        without = TQ._state(eager)
        rng = np.random.default_rng(4)
        stats = np.zeros((3, 32, 5))
        for k in range(3):
            stats[k] = LS.hand_stats(eager._obs.gp[k], rng, 20)
        for fl in (eager, graphed):
            fl.reset(traj_of, idx0, x0)
            fl.bins.copy_(_dev(stats))
            info, installed = fl.fit_gp()
            assert _host(info).tolist() == [20, 20, 20] and _host(installed).tolist() == [1, 1, 1]
        eager.rollout(1)
        g.replay()
        want, got = TQ._state(eager), TQ._state(graphed)
        for k in TQ.STATE + ("tally", "cost", "iters"):
            _bits(got[k], want[k], "%s after the replay" % k)
        assert (want["status"] == 0).all() and np.abs(want["w_opt"] - without["w_opt"]).max() > 1e-6
    finally:
        eager.close(); graphed.close()


# ---- 8. the learning experiment on the device ---------------------------------------------------------------------------------------

def test_the_learning_experiment_on_the_device(quad_oracle):
    """The experiment of test_quad_learn_cpu.py with the device's plant making the transitions and the device observing, fitting and
    installing.  The three ratios satisfy the CPU condition and agree with the spec's, recomputed from the same device transitions, to
    1e-6 relative (the margin of the car's experiment).  Measured on the MI355X: ratios 0.0194 / 0.0223 / 0.1324, relative gap to the
    spec's at most 3.9e-14."""
    import torch
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    fl = QuadFleet(QL.EXP_B, quad=SimQuad(drag=True), n_nodes=10, learn=QL.EXP_LEARN)
    try:
        nominal, plant, obs = QL.experiment_params()
        assert bytes(fl._plant) == bytes(plant) and bytes(fl._obs) == bytes(obs) and fl._nominal.cfg.n_gp == 0
        assert all(getattr(fl._nominal.cfg, k) == getattr(nominal, k) for k in ("mass", "max_thrust", "g")) and list(fl._nominal.cfg.rdrv) == [0.0] * 3
        trans, S = {}, {}
        for name in ("before", "after"):
            X, U = QL.experiment_inputs(name)
            u = _dev(U)
            fl.x.copy_(_dev(X))
            fl.set_observer(learned=False)
            fl.observe_latch()
            fl.plant_step(u)
            fl.observe(u)
            trans[name] = (X, U, _host(fl.x))
            S[name] = _host(fl.samples)
            assert (S[name][:, 13] == 1.0).all()
            if name == "before":
                assert _host(fl.dropped).tolist() == [0, 0, 0, 0]
                counts = _host(fl.bins)[:, :, 0].copy()                            # the later observations accumulate on top
                info, installed = fl.fit_gp(min_count=QL.EXP_MIN_COUNT)
                info = _host(info).tolist()
                assert min(info) >= 20 and _host(installed).tolist() == [1, 1, 1]
            else:
                fl._prev.copy_(_dev(X))
                fl.set_observer(learned=True)
                fl.observe(u)
                S["learned"] = _host(fl.samples)
        ratio = QL.rms(S["learned"]) / QL.rms(S["after"])
        exp = QL.experiment(quad_oracle, transitions=trans)
        gap = np.abs(ratio - exp["ratio"]) / exp["ratio"]
        print("points %s, ratios on the device %s, by the spec %s, relative gap %s, cond(K) %s"
              % (info, np.array2string(ratio, precision=9), np.array2string(exp["ratio"], precision=9), np.array2string(gap, precision=3),
                 ["%.3g" % c for c in exp["cond"]]))
        assert info == [g["info"] for g in exp["gps"]]
        _bits(counts, np.ascontiguousarray(exp["bins"][:, :, 0]), "the counts of the bins")
        assert (ratio <= 0.15).all(), ratio
        assert (gap <= 1e-6).all(), gap
        gps = fl.learned_gps()
        assert [len(g["alpha"]) for g in gps] == info and [g["feat"] for g in gps] == [[7], [8], [9]] and [g["out"] for g in gps] == [7, 8, 9]
    finally:
        fl.close()


# ---- 9. a short closed loop ---------------------------------------------------------------------------------------------------------

def test_a_short_closed_loop_learns_its_plant():
    """B = 64, N = 10, circles of 5 m at 2, 3, 4 and 5 m/s, drag on: 60 observed steps against the nominal model, fit and install,
    reset, 60 steps again from the same start.  The summed position-error tally of the second pass is finite and strictly smaller
    (measured on the MI355X: 532.9 m with the nominal model, 120.6 m with the learned GPs)."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, B, T = 10, 64, 60
    dt = 1.0 / (N * 5)
    trajs = [circle_reference(T + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
    traj_of = (np.arange(B) % 4).astype(np.int32)
    idx0 = (np.arange(B) // 4).astype(np.int32)
    fl = _learning_fleet(B, N, trajs, traj_of, idx0, None)
    try:
        total = []
        for r in range(2):
            fl.reset(traj_of, idx0)
            fl.rollout(T, observe=True)
            total.append(float(_host(fl.tally)[:, 0].sum()))
            assert (_host(fl.counts) == [T, 0, 0]).all()
            if r == 0:
                bins, dropped = _host(fl.bins), _host(fl.dropped)
                assert dropped[3] == 0 and (bins[:, :, 0].sum(axis=1) + dropped[:3] == B * T).all()
                info, installed = fl.fit_gp(min_count=2)
                assert min(_host(info).tolist()) >= 2 and _host(installed).tolist() == [1, 1, 1]
        print("sum of |e| over %d steps of %d vehicles: %.6g m with the nominal model, %.6g m with the learned GPs" % (T, B, total[0], total[1]))
        assert np.isfinite(total).all() and total[1] < total[0]
    finally:
        fl.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_no_ops():
    """Every refusal the header lists for the five entries, in the listed order (a call that breaks two rules is refused for the first);
    nothing on the device moves.  A model on another device needs a second GPU and is not exercised here."""
    import torch
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config
    from ad_mpc_amd.quad_fleet import QuadFleet
    N, B = 10, 5
    trajs = TQ._circles(N, 3.0)
    traj_of, idx0 = np.zeros(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    fl = _learning_fleet(B, N, trajs, traj_of, idx0, None)
    plain = TQ._fleet(B, N, trajs, traj_of, idx0, None)
    sqp_cfg = default_quad_config(); sqp_cfg.sqp_iters = 3
    sqp = QuadBatchSolver(sqp_cfg)
    L, null = fl.lib, C.c_void_p(0)
    try:
        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        bad_obs = _obs(QL.EXP_LEARN); bad_obs.substeps = 0
        bad_plant = fl._plant.copy(); bad_plant.substeps = 0
        before = {k: _host(getattr(fl, k)).copy() for k in TQ.STATE + ("tally",) + LEARN_STATE}

        latch = lambda B=B, x=_p(fl.x), prev=_p(fl._prev): L.admpc_quad_observe_latch_batch(0, B, x, prev, fl._stream())
        refused(latch(B=-1, x=null), "negative batch")
        refused(latch(x=null), "null array"); refused(latch(prev=null), "null array")
        assert latch(B=0, x=null, prev=null) == 0

        def observe(**kw):
            a = dict(model=fl._nominal._h, plant=C.byref(fl._plant), obs=C.byref(fl._obs), B=B, u=_p(fl.w_opt), stride=N * 4, x=_p(fl.x), bins=_p(fl.bins))
            a.update(kw)
            return L.admpc_quad_observe_batch(a["model"], a["plant"], a["obs"], a["B"], a["u"], a["stride"], a["x"], _p(fl._prev), _p(fl.samples),
                                              a["bins"], _p(fl.dropped), fl._stream())
        refused(observe(obs=None, plant=None), "observe parameters are not set")
        refused(observe(obs=C.byref(bad_obs), plant=None), "substeps must be in [1, 64]")
        refused(observe(plant=None, model=null), "plant parameters are not set")
        refused(observe(plant=C.byref(bad_plant), model=null), "substeps must be in [1, 1024]")
        refused(observe(model=null, B=-1), "null model")
        refused(observe(B=-1, u=null), "negative batch")
        refused(observe(u=null, stride=3), "null array"); refused(observe(bins=null), "null array")
        refused(observe(stride=3), "u_stride must be at least 4")
        assert observe(B=0, u=null, x=null) == 0

        fit = lambda obs=C.byref(fl._obs), mc=1, bins=_p(fl.bins), info=_p(fl.fit_info): L.admpc_quad_gp_fit(0, obs, mc, bins, _p(fl._gp_dev), info, fl._stream())
        refused(fit(obs=C.byref(bad_obs), mc=0), "substeps must be in [1, 64]")
        refused(fit(mc=0, bins=null), "min_count must be at least 1")
        refused(fit(bins=null), "null array"); refused(fit(info=null), "null array")

        inst = lambda s=fl._eng._h, n=3, gp=_p(fl._gp_dev), out=_p(fl.installed): L.admpc_quad_gp_install(s, n, gp, out, fl._stream())
        refused(inst(s=null, n=0), "null solver")
        refused(inst(s=fl._nominal._h, gp=null), "created with 0 GPs")
        refused(inst(n=2, gp=null), "n_gp = 2")
        refused(inst(n=0, gp=null), "n_gp = 0")
        refused(inst(gp=null), "null array"); refused(inst(out=null), "null array")

        def roll(**kw):
            a = dict(s=fl._eng._h, bank=fl._bank, plant=C.byref(fl._plant), over=5, B=B, T=2, x=_p(fl.x), tally=_p(fl.tally), model=fl._nominal._h,
                     obs=C.byref(fl._obs), prev=_p(fl._prev), dropped=_p(fl.dropped))
            a.update(kw)
            return L.admpc_quad_rollout_observe_batch(a["s"], a["bank"], a["plant"], a["over"], a["B"], a["T"], _p(fl.traj_of), _p(fl.idx), a["x"], _p(fl.x_opt),
                                                      _p(fl.w_opt), _p(fl.yref), _p(fl.yref_e), _p(fl.cost), _p(fl.status), _p(fl.iters), a["tally"],
                                                      _p(fl.counts), None, None, a["model"], a["obs"], a["prev"], _p(fl.samples), _p(fl.bins),
                                                      a["dropped"], fl._stream())
        refused(roll(obs=None, model=null), "observe parameters are not set")
        refused(roll(obs=C.byref(bad_obs), model=null), "substeps must be in [1, 64]")
        refused(roll(model=null, s=null), "null model")
        refused(roll(s=null, bank=null), "null solver")
        refused(roll(s=sqp._h, bank=null), "sqp_iters > 1")
        refused(roll(bank=null, plant=None), "null bank")
        refused(roll(plant=C.byref(bad_plant), over=0), "substeps must be in [1, 1024]")
        refused(roll(over=0, B=-1), "over must be at least 1")
        refused(roll(B=-1, T=-1), "negative batch")
        refused(roll(T=4097, x=null), "T must be in [0, 4096]")
        for k in ("x", "tally", "prev", "dropped"):
            refused(roll(**{k: null}), "admpc_quad_rollout_observe_batch: null array")
        assert roll(B=0, x=null, prev=null) == 0 and roll(T=0, x=null, prev=null) == 0
        torch.cuda.synchronize()
        for k, v in before.items():
            _bits(_host(getattr(fl, k)), v, "%s after refused calls" % k)

        # the Python layer: a fleet without learn behaves as before and refuses the learning methods
        for call in (lambda: plain.observe(), lambda: plain.observe_latch(), lambda: plain.observe_reset(), lambda: plain.fit_gp(),
                     lambda: plain.learned_gps(), lambda: plain.set_observer(True), lambda: plain.rollout(1, observe=True)):
            with pytest.raises(ValueError, match="does not learn"):
                call()
        with pytest.raises(ValueError, match="observe: u must be"):
            fl.observe(fl.w_opt[:, 0, :3])
        assert fl._eng.cfg.n_gp == 3 and fl._nominal.cfg.n_gp == 0 and fl._eng.cfg.gp[0].n_points == 0 and plain._eng.cfg.n_gp == 0
        assert [len(g["alpha"]) for g in fl.learned_gps()] == [0, 0, 0]            # nothing fitted yet: the placeholders
        # a fit whose weights overflow: the install replaces the record by the empty GP, and learned_gps returns what the handle holds
        stats = np.zeros((3, 32, 5))
        stats[0, 14], stats[0, 17] = [1.0, -0.9, 0.0, 0.0, 1e308], [1.0, 0.8, 0.0, 0.0, -1e308]
        fl.bins.copy_(_dev(stats))
        info, installed = fl.fit_gp()
        assert _host(info).tolist() == [2, 0, 0] and _host(installed).tolist() == [0, 1, 1]
        gps = fl.learned_gps()
        assert gps[0] == dict(feat=7, out=7, Z=[], alpha=[], length_scale=1.0, sigma_f=0.0, ymean=0.0) and len(gps[1]["alpha"]) == 0
        fl.observe_reset()
        assert not _host(fl.bins).any()
        # what was learned creates another fleet
        other = QuadFleet(2, gp_regressors=gps)
        other.close()
    finally:
        fl.close(); plain.close(); sqp.close()
