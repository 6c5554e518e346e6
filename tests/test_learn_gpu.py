"""Fitting the residual GP on the device (include/admpc_learn.h; ad_mpc_amd/fleet.py: observe, fit_gp, learned_gps, rollout_route(observe)).

The record is compared with its numpy restatement (tests/learn_spec.py: one oracle RK4 step per sub-step) at the plant test's bound
divided by dt; the flag, the latch, the bins and the dropped counts bit for bit; the fit by its backward error and against the spec's
mean at ten times the gap between the spec solved in float64 and in numpy.longdouble; the install by the solve of a fresh handle created
from learned_gps(); the rollout with observation by the loop it replaces."""
import ctypes as C

import numpy as np
import pytest

import learn_spec as LS
import plant_spec as PS
import test_lane_gpu as TL
import test_plant_gpu as TP

pytestmark = pytest.mark.gpu

T_HORIZON = TL.T_HORIZON
_dev, _p, _bits = TL._dev, TL._p, TL._bits
BAND = (3.0, 5.0)
RANGES = {3: (2.0, 12.0), 4: (-0.5, 0.5), 5: (-0.3, 0.3), 6: (-0.3, 0.3), 7: (-10.0, 5.0), 8: (-3.0, 3.0)}


def _learn(feat, bins, out=3, length_scale=2.0, **kw):
    feat = list(np.atleast_1d(feat))
    d = dict(feat=feat, out=out, lo=[RANGES[f][0] for f in feat], hi=[RANGES[f][1] for f in feat], bins=list(np.atleast_1d(bins)),
             length_scale=length_scale)
    d.update(kw)
    return d


FOUR = [_learn(3, 8), _learn([3, 8], [8, 4], out=4), _learn([4, 5, 7], [4, 2, 4], out=5), _learn(6, 32, out=4)]


def _obs(gps, dt=0.05, substeps=1, band=BAND):
    from ad_mpc_amd.config import AdmpcObserveParams, learn_bins
    bins, n = learn_bins(gps)
    return AdmpcObserveParams(dt=dt, blend_min=band[0], blend_max=band[1], substeps=substeps, n_gp=n, gp=bins)


def _fleet(B, seed=0):
    """(prev [B,7], now [B,7], ack, mode): the 67 vehicles of the plant test tiled, every copy moved a little; `now` a perturbation of
    `prev` of the size a period makes.  Where B > 4, vehicle 3 has a NaN in the pose now and vehicle 4 in the pose before."""
    X, ack, mode = TP._fleet67()
    rng = np.random.default_rng(100 + seed)
    t = np.arange(B) % 67
    prev = X[t] + rng.uniform(-1e-3, 1e-3, size=(B, 7))
    now = prev + rng.normal(size=(B, 7)) * np.array([0.3, 0.3, 0.02, 0.1, 0.02, 0.02, 0.02])
    if B > 4:
        now[3, 4] = np.nan
        prev[4, 5] = np.nan
    return prev, now, ack[t].copy(), mode[t].copy()


def _observe(eng, plant, obs, prev, now, ack, mode, bins=None, dropped=None):
    """admpc_observe_batch on copies: (samples [B,10], prev afterwards [B,7], bins [4,32,5], dropped [5])."""
    import torch
    B = prev.shape[0]
    st = [_dev(now[:, i]) for i in range(7)]
    pv = _dev(np.ascontiguousarray(prev.T))
    a, m = _dev(ack, torch.float32), _dev(mode, torch.int32)
    samples = torch.full((B, 10), 7.0, dtype=torch.float64, device="cuda:0")
    bn = _dev(np.zeros((4, 32, 5)) if bins is None else bins)
    dr = _dev(np.zeros(5, dtype=np.int32) if dropped is None else dropped, torch.int32)
    rc = eng.lib.admpc_observe_batch(eng._h, C.byref(plant), C.byref(obs), B, _p(a), _p(m), *[_p(t) for t in st], _p(pv), _p(samples), _p(bn), _p(dr),
                                     eng._stream())
    assert rc == 0, eng.lib.admpc_last_error()
    torch.cuda.synchronize()
    for i in range(7):
        _bits(st[i].cpu().numpy(), now[:, i], "the pose arrays are read-only")
    return samples.cpu().numpy(), pv.cpu().numpy().T.copy(), bn.cpu().numpy(), dr.cpu().numpy()


# ---- 1. the record against the spec -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_gp", [False, True])
@pytest.mark.parametrize("M", [1, 4])
def test_the_record_matches_the_spec(gpu_engine_factory, oracle, with_gp, M):
    """B = 1, 21, 22 (one past a block) and 65; |dy_j| <= M * G * 1e-12 * max(1, |x^_j|) / dt; features, inputs, flag and latch bit for bit."""
    cfg = TP._cfg(with_gp)
    dt = 0.05 if M == 1 else 0.1
    plant, obs = TP._plant(dt=dt, brake_acc=-4.0), _obs(FOUR[:1], dt=dt, substeps=M)
    eng = gpu_engine_factory(cfg)
    try:
        for B in (1, 21, 22, 65):
            prev, now, ack, mode = _fleet(B, seed=B)
            S, latched, _, _ = _observe(eng, plant, obs, prev, now, ack, mode)
            spec = [LS.record(oracle, cfg, plant, obs, prev[b], now[b], ack[b], mode[b]) for b in range(B)]
            want = np.stack([s[0] for s in spec])
            xh = np.stack([s[1] for s in spec])
            G = np.array([PS.chain_gain(s[2]) if np.isfinite(np.array(s[2])).all() else 1.0 for s in spec])
            _bits(latched, now, "the latch, B = %d" % B)
            _bits(S[:, :6], want[:, :6], "features and inputs, B = %d" % B)
            _bits(S[:, 9], want[:, 9], "the flag, B = %d" % B)
            assert (want[:, 9] == 0.0).sum() == (2 if B > 4 else 0)
            ok = want[:, 9] == 1.0
            bound = (M * G[:, None] * 1e-12 * np.maximum(1.0, np.abs(xh[:, 3:6])) / dt)[ok]
            ratio = np.abs(S[ok, 6:9] - want[ok, 6:9]) / bound
            print("B = %d, M = %d, gp = %s: largest |dy| over its bound %.3g, G up to %.3g" % (B, M, with_gp, ratio.max(), G.max()))
            assert ratio.max() <= 1.0 and np.array_equal(np.isnan(S[~ok, 6:9]), np.isnan(want[~ok, 6:9]))
            if B > 4:
                assert np.abs(want[ok, 6:9]).max() > 0.1 and {0, 1} <= set(mode.tolist())
    finally:
        eng.close()


def test_observe_past_the_grid(gpu_engine_factory):
    """B = 4096 * 21 + 301: the stride loop runs and the last block is partial; the latch and the flags only."""
    cfg = TP._cfg(True)
    B = PS.PAST_THE_GRID
    prev, now, ack, mode = _fleet(B, seed=1)
    small = slice(0, 67)
    eng = gpu_engine_factory(cfg)
    try:
        S, latched, _, dropped = _observe(eng, TP._plant(), _obs(FOUR[:1]), prev, now, ack, mode)
        s67, _, _, _ = _observe(eng, TP._plant(), _obs(FOUR[:1]), prev[small], now[small], ack[small], mode[small])
    finally:
        eng.close()
    _bits(latched, now, "the latch")
    assert (S[:, 9] == 0.0).sum() == 2 and S[3, 9] == 0.0 and S[4, 9] == 0.0 and set(S[:, 9].tolist()) == {0.0, 1.0}
    _bits(S[small], s67, "the first 67 against the batch of 67")
    assert dropped[4] == 2


# ---- 2. the bins from the device's own records --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_gp", [1, 4])
def test_bins_and_dropped_counts_match_the_spec_bit_for_bit(gpu_engine_factory, n_gp):
    cfg = TP._cfg(False)
    obs, plant = _obs(FOUR[:n_gp]), TP._plant()
    eng = gpu_engine_factory(cfg)
    try:
        for B in (1, 63, 64, 65, 200):
            prev, now, ack, mode = _fleet(B, seed=B)
            S, latched, bins, dropped = _observe(eng, plant, obs, prev, now, ack, mode)
            wb, wd = np.zeros((4, 32, 5)), np.zeros(5, dtype=np.int32)
            LS.accumulate(obs, S, wb, wd)
            _bits(bins, wb, "bins, B = %d" % B); _bits(dropped, wd, "dropped, B = %d" % B)
            # a second call accumulates on top of the first: other poses, from the latch of the first
            now2 = now + np.random.default_rng(B).normal(size=now.shape) * 0.05
            S2, _, bins2, dropped2 = _observe(eng, plant, obs, latched, now2, ack, mode, bins, dropped)
            LS.accumulate(obs, S2, wb, wd)
            _bits(bins2, wb, "bins after two calls, B = %d" % B); _bits(dropped2, wd, "dropped after two calls, B = %d" % B)
            if B >= 63:
                assert wb[0, :, 0].sum() > 0 and wd[4] == 2 + 1                    # the NaN pose of the first call is latched: vehicle 3 again
                assert not wb[n_gp:].any() and (wb[:n_gp, :, 0].sum(axis=1) + wd[:n_gp] + wd[4] == 2 * B).all()
    finally:
        eng.close()


# ---- 3. the fit from hand-made statistics -------------------------------------------------------------------------------------------

def _fit(lib, obs, stats, min_count):
    """admpc_gp_fit on uploaded statistics: (the AdmpcGp records, info)."""
    import torch
    from ad_mpc_amd.config import AdmpcGp
    n = int(obs.n_gp)
    bins = _dev(stats)
    out = torch.full((4 * C.sizeof(AdmpcGp),), 0x5A, dtype=torch.uint8, device="cuda:0")
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda:0")
    assert lib.admpc_gp_fit(0, C.byref(obs), min_count, _p(bins), _p(out), _p(info), None) == 0, lib.admpc_last_error()
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    return [AdmpcGp.from_buffer_copy(raw, g * C.sizeof(AdmpcGp)) for g in range(n)], info.cpu().numpy()[:n]


def _check_fit(G, gp, info, stats, min_count, what):
    """The mean is held to ten times a yardstick formed for THIS case's statistics (tests/learn_spec.py: yardstick), not to the figure of
    the experiment's fit in test_learn_cpu.py: the gap between float64 and longdouble of another kernel matrix says nothing about this
    one, and for the worse conditioned cases (32 points at length scale 0.6) it is larger (6.7e-13 against 2.7e-15).  No case's
    yardstick may pass 1e-11, the ceiling test_learn_cpu.py sets for the experiment's, so the bound cannot grow unnoticed."""
    want = LS.fit(G, stats, min_count)
    nf, n = int(G.n_feat), want["n_points"]
    assert info == want["info"] and gp.n_points == n and gp.n_feat == nf and gp.out == G.out, (what, info, want["info"], gp.n_points)
    assert [gp.feat[d] for d in range(3)] == [G.feat[d] if d < nf else 0 for d in range(3)] and gp.sigma_f == G.sigma_f
    _bits(np.array([gp.inv_l2[d] for d in range(3)]), np.concatenate([LS.inv_l2(G), np.zeros(3 - nf)]), what + ": inv_l2")
    Z = np.array([[gp.Z[d][i] for d in range(3)] for i in range(32)])
    alpha = np.array([gp.alpha[i] for i in range(32)])
    wantZ = np.zeros((32, 3)); wantZ[:n, :nf] = want["Z"]
    _bits(Z, wantZ, what + ": Z, zero where unused"); _bits(np.float64(gp.ymean), np.float64(want["ymean"]), what + ": ymean")
    assert not alpha[n:].any()
    if n == 0:
        return
    Zp, t, counts, ymean = LS.points(G, stats, min_count)
    K = LS.kernel_matrix(G, Z[:n, :nf], counts)                        # from the returned Z
    b = t - ymean
    res = np.abs(K @ alpha[:n] - b).max()
    bound = 64 * n * 2.2e-16 * (np.abs(K).sum(axis=1).max() * np.abs(alpha[:n]).max() + np.abs(b).max())
    rng = np.random.default_rng(n)
    probes = np.array([[rng.uniform(G.lo[d], G.hi[d]) for d in range(nf)] for _ in range(200)])
    yard = LS.yardstick(G, stats, probes, min_count)
    gap = np.abs(LS.gp_mean(G, dict(Z=Z[:n, :nf], alpha=alpha[:n], ymean=gp.ymean), probes) - LS.gp_mean(G, want, probes)).max()
    print("%s: n = %d, residual %.3g (bound %.3g), mean gap %.3g (yardstick %.3g)" % (what, n, res, bound, gap, yard))
    assert res <= bound, (what, res, bound)
    assert yard < 1e-11, (what, yard)
    assert gap <= 10.0 * yard, (what, gap, yard)


def test_the_fit_from_hand_made_statistics():
    """n = 0, 1, 8 and 32 points of one feature; then, with min_count = 4, 20 bins of three features of which some are below it, a NaN
    feature sum, all 32 bins of three features, and 8 points with a count-dependent diagonal."""
    lib = TL._lib()
    one = dict(length_scale=0.6, noise=1e-4)
    obs = _obs([_learn(3, 32, **one)] * 4)
    rng = np.random.default_rng(11)
    stats = np.zeros((4, 32, 5))
    stats[1] = LS.hand_stats(obs.gp[1], rng, 1); stats[2] = LS.hand_stats(obs.gp[2], rng, 8); stats[3] = LS.hand_stats(obs.gp[3], rng, 32)
    gps, info = _fit(lib, obs, stats, 1)
    assert info.tolist() == [0, 1, 8, 32]
    for g in range(4):
        _check_fit(obs.gp[g], gps[g], info[g], stats[g], 1, "one feature, regressor %d" % g)
    assert gps[0].ymean == 0.0 and gps[1].alpha[0] == 0.0 and gps[1].ymean == stats[1, :, 4].sum() / stats[1, :, 0].sum()

    three = dict(length_scale=[2.0, 0.4, 3.0], noise=1e-4, sigma_f=0.7)
    obs = _obs([_learn([3, 5, 7], [4, 2, 4], out=4, **three)] * 3 + [_learn(3, 8, length_scale=2.0, noise=1e-6, count_noise=0.05)])
    stats = np.zeros((4, 32, 5))
    stats[0] = LS.hand_stats(obs.gp[0], rng, 20); stats[1] = LS.hand_stats(obs.gp[1], rng, 20); stats[2] = LS.hand_stats(obs.gp[2], rng, 32)
    stats[3] = LS.hand_stats(obs.gp[3], rng, 8)
    below = int((stats[0, :, 0] >= 4).sum())
    assert 0 < below < 20                                                      # some bins are below min_count
    k = np.flatnonzero(stats[1, :, 0] >= 4)[2]
    stats[1, k, 2] = np.nan                                                    # the third point's second feature
    gps, info = _fit(lib, obs, stats, 4)
    assert info.tolist() == [below, -3, int((stats[2, :, 0] >= 4).sum()), int((stats[3, :, 0] >= 4).sum())] and info[2] > 20
    assert gps[1].n_points == 0 and gps[1].ymean == 0.0 and not any(gps[1].alpha[i] for i in range(32))        # the empty GP
    for g in range(4):
        _check_fit(obs.gp[g], gps[g], info[g], stats[g], 4, "min_count 4, regressor %d" % g)


# ---- 4. install -----------------------------------------------------------------------------------------------------------------------

def _solve(eng, s):
    return eng.solve_numpy(s["x0"], s["yref"], s["yref_e"], s["p"], s["xbar"], s["ubar"])


@pytest.mark.parametrize("N,B", [(20, 65), (40, 8)])
def test_an_installed_gp_solves_as_a_handle_created_with_it(N, B):
    import torch
    from ad_mpc_amd.config import AdmpcGp, set_gp
    from ad_mpc_amd.engine import BatchSolver
    from ad_mpc_amd.scenarios import random_scenarios
    learn = [_learn(3, 8, length_scale=2.0), _learn([3, 6], [4, 4], out=4, length_scale=[4.0, 0.5], noise=1e-4)]
    fc = TL._controller(N, B, learn=learn, blend_min=3.0, blend_max=5.0)
    fresh = empty = None
    try:
        s = random_scenarios(B, N=N, Ts=T_HORIZON / N, seed=N, blend=(3.0, 5.0))
        base = _solve(fc._eng, s)                                              # the placeholder GPs: nothing learned yet
        rng = np.random.default_rng(N)
        stats = np.zeros((4, 32, 5))
        for g in range(2):
            stats[g] = LS.hand_stats(fc._obs.gp[g], rng, 8 if g == 0 else 12)
        fc.bins.copy_(_dev(stats))
        info, installed = fc.fit_gp()
        got = _solve(fc._eng, s)
        assert info.cpu().tolist() == [8, 12] and installed.cpu().tolist() == [1, 1]
        gps = fc.learned_gps()
        assert [len(g["alpha"]) for g in gps] == [8, 12] and gps[1]["Z"].shape == (12, 2)
        fresh = BatchSolver(set_gp(fc._eng.cfg.copy(), gps), device=0)
        want = _solve(fresh, s)
        for a, b, what in zip(got, want, ("x", "u", "cost", "status", "iters")):
            _bits(a, b, "%s of the installed handle against the fresh one" % what)
        assert np.nanmax(np.abs(got[1] - base[1])) > 1e-6                      # the GP acts

        # records the install refuses are installed as the empty GP
        good = [AdmpcGp.from_buffer_copy(bytes(fresh.cfg.gp[g])) for g in range(2)]
        for field, value in (("n_points", 33), ("out", 6), ("alpha", np.nan)):
            bad = AdmpcGp.from_buffer_copy(bytes(good[0]))
            if field == "alpha":
                bad.alpha[5] = value
            else:
                setattr(bad, field, value)
            assert not LS.install_ok(bad) and LS.install_ok(good[1])
            raw = torch.as_tensor(np.frombuffer(bytes(bad) + bytes(good[1]), dtype=np.uint8).copy(), device="cuda:0")
            inst = torch.full((2,), 7, dtype=torch.int32, device="cuda:0")
            assert fc.lib.admpc_gp_install(fc._eng._h, 2, _p(raw), _p(inst), None) == 0, fc.lib.admpc_last_error()
            torch.cuda.synchronize()
            assert inst.cpu().tolist() == [0, 1], field
        half = _solve(fc._eng, s)
        gps[0] = dict(feat=3, out=3, Z=[], alpha=[], length_scale=1.0, sigma_f=0.0, ymean=0.0)
        empty = BatchSolver(set_gp(fc._eng.cfg.copy(), gps), device=0)
        for a, b, what in zip(half, _solve(empty, s), ("x", "u", "cost", "status", "iters")):
            _bits(a, b, "%s with the first GP replaced by the empty one" % what)

        # refusals: a handle created without GPs, and another n_gp than the handle's
        inst = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        assert fc.lib.admpc_gp_install(fc._nominal._h, 2, _p(raw), _p(inst), None) == -1 and b"created with 0 GPs" in fc.lib.admpc_last_error()
        assert fc.lib.admpc_gp_install(fc._eng._h, 1, _p(raw), _p(inst), None) == -1 and b"n_gp = 1" in fc.lib.admpc_last_error()
        assert fc.lib.admpc_gp_install(fc._eng._h, 2, None, _p(inst), None) == -1 and b"null array" in fc.lib.admpc_last_error()
    finally:
        fc.close()
        for e in (fresh, empty):
            if e is not None:
                e.close()


# ---- 5. the rollout with observation against the loop it replaces -------------------------------------------------------------------

def _truth(fc, gpu_engine_factory):
    """The plant of the closed-loop tests: the controller's own vehicle and bounds with the GP of the experiment on the derivative of v_x."""
    from ad_mpc_amd.config import set_gp
    return gpu_engine_factory(set_gp(fc._nominal.cfg.copy(), LS.truth_gp()))


LOOP_LEARN = [_learn(3, 8, length_scale=2.0, lo=[3.0], hi=[11.0]), _learn([3, 7], [4, 4], out=4, length_scale=[3.0, 4.0])]


def test_rollout_with_observe_equals_the_loop_it_replaces(gpu_engine_factory):
    """N = 20, B = 22, T = 5.  `whole`: one rollout with observe; `loop`: observe_latch, then per step step_route, plant_step, observe;
    `plain`: the rollout without observation, whose tally and counts the observation must not change."""
    import torch
    N, B, T = 20, 22, 5
    road = TL._road()
    pose = TL._along(road, np.linspace(3, 500, B).astype(int), seed=5)
    tk = _dev(np.zeros(B, dtype=np.int32), torch.int32)
    fcs = [TL._controller(N, B, threshold=2, learn=LOOP_LEARN) for _ in range(3)]
    whole, loop, plain = fcs
    truth = _truth(whole, gpu_engine_factory)
    try:
        for fc in fcs:
            fc.set_paths([road])
            fc.set_plant(dt=T_HORIZON / N, substeps=2, model=truth)
        pw, pl, pp = TP._poses(pose), TP._poses(pose), TP._poses(pose)
        out = whole.rollout_route(tk, *pw, steps=T, observe=True, record=True)
        ref = plain.rollout_route(tk, *pp, steps=T, record=True)
        loop.observe_latch(*pl)
        for t in range(T):
            loop.step_route(tk, *pl)
            loop.plant_step(*pl)
            loop.observe(*pl)
        want, got = TL._state(loop), TL._state(whole)
        for k in TL.STATE:
            _bits(got[k], want[k], "%s at the end" % k)
        _bits(TP._host(pw), TP._host(pl), "poses at the end"); _bits(TP._host(pw), TP._host(pp), "poses against the plain rollout")
        for k in ("bins", "dropped", "samples", "_prev"):
            _bits(getattr(whole, k).cpu().numpy(), getattr(loop, k).cpu().numpy(), k)
        _bits(out.traj.cpu().numpy(), ref.traj.cpu().numpy(), "traj: a slot per step, as the plain rollout records it")
        assert np.array_equal(out.traj.cpu().numpy()[0], pose) and np.array_equal(out.traj.cpu().numpy()[T], TP._host(pw))
        _bits(out.tally.cpu().numpy(), ref.tally.cpu().numpy(), "tally"); _bits(out.counts.cpu().numpy(), ref.counts.cpu().numpy(), "counts")
        bins, dropped = whole.bins.cpu().numpy(), whole.dropped.cpu().numpy()
        assert (out.counts.cpu().numpy()[:, 0] == T).all() and dropped[4] == 0
        assert (bins[:2, :, 0].sum(axis=1) + dropped[:2] == B * T).all() and bins[0, :, 0].sum() > B and not plain.bins.any()
        _bits(whole._prev.cpu().numpy(), TP._host(pw), "the latch holds the final poses")
    finally:
        for fc in fcs:
            fc.close()
        truth.close()


# ---- 6. graph replay ----------------------------------------------------------------------------------------------------------------

def test_a_captured_rollout_reads_the_installed_gp_without_recapture(gpu_engine_factory):
    """Capture a rollout with observe; replay, fit and install outside the graph, replay again: state, poses and bins equal the eager
    run from the same state bit for bit.  A third controller that fits without installing ends elsewhere: the GP acts."""
    import torch
    N, B, T = 20, 12, 3
    road = TL._road()
    pose = TL._along(road, np.linspace(0, 480, B).astype(int), seed=31)
    tk = _dev(np.zeros(B, dtype=np.int32), torch.int32)
    fcs = [TL._controller(N, B, threshold=1, learn=LOOP_LEARN[:1]) for _ in range(3)]
    eager, graphed, idle = fcs
    truth = _truth(eager, gpu_engine_factory)
    try:
        for fc in fcs:
            fc.set_paths([road])
            fc.set_plant(dt=T_HORIZON / N, model=truth)
        ins = TP._poses(pose)
        graphed.rollout_route(tk, *ins, steps=T, observe=True)                   # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.rollout_route(tk, *ins, steps=T, observe=True)
        ends = {}
        for fc in fcs:
            fc.reset(); fc.observe_reset()
            for r in range(2):
                if fc is graphed:
                    for i in range(7):
                        ins[i].copy_(torch.as_tensor(pose[i], device=fc.device))
                    g.replay()
                    ps = ins
                else:
                    ps = TP._poses(pose)
                    fc.rollout_route(tk, *ps, steps=T, observe=True)
                if r == 0:
                    info, installed = fc.fit_gp(install=fc is not idle)
                    torch.cuda.synchronize()
                    assert info.cpu().tolist()[0] >= 2 and (installed is None or installed.cpu().tolist() == [1])
            ends[id(fc)] = (TL._state(fc), TP._host(ps), fc.bins.cpu().numpy(), fc.dropped.cpu().numpy())
        want, got, other = ends[id(eager)], ends[id(graphed)], ends[id(idle)]
        for k in TL.STATE:
            _bits(got[0][k], want[0][k], "%s after the second replay" % k)
        _bits(got[1], want[1], "poses"); _bits(got[2], want[2], "bins"); _bits(got[3], want[3], "dropped")
        assert (want[0]["mode"] == 1).all() and np.abs(want[0]["w_opt"] - other[0]["w_opt"]).max() > 1e-9
    finally:
        for fc in fcs:
            fc.close()
        truth.close()


# ---- 7. the learning experiment on the device ---------------------------------------------------------------------------------------

def test_the_learning_experiment_on_the_device(gpu_engine_factory, oracle):
    """The experiment of test_learn_cpu.py with the device observing, fitting and installing: B = 200, one plant_step per set."""
    import torch
    from ad_mpc_amd.config import default_config
    exp = LS.experiment(oracle)
    nominal, truth_cfg, plant, obs = LS.experiment_params()
    fc = TL._controller(20, LS.EXP_B, learn=LS.EXP_LEARN)
    truth = _truth(fc, gpu_engine_factory)
    try:
        c, d = fc._nominal.cfg, default_config(N=20)
        assert all(getattr(c, k) == getattr(d, k) for k in ("mass", "L_F", "L_R", "Iz", "Cf", "Cr")) and c.n_gp == 0
        assert (fc._prm.blend_min, fc._prm.blend_max) == LS.EXP_BAND and c.lbu[0] <= -2.0 and c.ubu[0] >= 2.0
        fc.set_plant(dt=LS.EXP_DT, model=truth)
        rms = {}
        for name in ("before", "after"):
            e = exp[name]
            fc.ack.copy_(_dev(e["ack"], torch.float32)); fc.mode.copy_(_dev(e["mode"], torch.int32))
            ps = TP._poses(np.ascontiguousarray(e["X"].T))
            fc.observe_latch(*ps)
            fc.plant_step(*ps)
            fc.observe(*ps)
            S = fc.samples.cpu().numpy()
            assert (S[:, 9] == 1.0).all()
            np.testing.assert_allclose(TP._host(ps).T[:, 3:6], e["now"][:, 3:6], rtol=1e-12, atol=0)
            rms[name] = float(np.sqrt(np.mean(S[:, 6:9] ** 2)))
            if name == "before":
                _bits(fc.bins.cpu().numpy()[0, :, 0], exp["bins"][0, :, 0], "the counts of the bins")
                info, installed = fc.fit_gp()
                assert info.cpu().tolist() == [8] and installed.cpu().tolist() == [1]
                fc.set_observer(learned=True)
        ratio = rms["after"] / rms["before"]
        print("ratio on the device %.9g, by the spec %.9g" % (ratio, exp["ratio"]))
        assert abs(ratio - exp["ratio"]) <= 1e-6 * exp["ratio"] and ratio <= 0.05
    finally:
        fc.close(); truth.close()


# ---- 8. a short closed loop ---------------------------------------------------------------------------------------------------------

def test_a_short_closed_loop_learns_its_plant(gpu_engine_factory):
    """B = 64, T = 40: a kinematic controller on the plant with the GP.  The first rollout is observed against the nominal model, the
    second, from the same poses with the learned GP installed, against the learned handle: its sum of y^2 over all steps and vehicles
    is smaller.  Nothing is asserted about tracking."""
    import torch
    N, B, T = 20, 64, 40
    road = TL._road()
    pose = TL._along(road, np.linspace(3, 480, B).astype(int), seed=40)
    tk = _dev(np.zeros(B, dtype=np.int32), torch.int32)
    fc = TL._controller(N, B, threshold=3, learn=[_learn(3, 8, length_scale=2.0, lo=[2.0], hi=[12.0])])
    truth = _truth(fc, gpu_engine_factory)
    try:
        fc.set_paths([road])
        fc.set_plant(dt=T_HORIZON / N, substeps=2, model=truth)
        total = []
        for r in range(2):
            fc.reset()
            ps = TP._poses(pose)
            acc = torch.zeros((), dtype=torch.float64, device=fc.device)
            for t in range(T):
                fc.rollout_route(tk, *ps, steps=1, observe=True, accumulate=t > 0)
                S = fc.samples
                acc += torch.where(S[:, 9:10] == 1.0, S[:, 6:9] ** 2, torch.zeros_like(S[:, 6:9])).sum()
            total.append(float(acc.cpu()))
            if r == 0:
                info, installed = fc.fit_gp(min_count=5)
                fc.set_observer(learned=True)
                assert info.cpu().tolist()[0] >= 2 and installed.cpu().tolist() == [1]
                assert fc.dropped.cpu().numpy()[4] == 0 and fc.bins.cpu().numpy()[0, :, 0].sum() + fc.dropped.cpu().numpy()[0] == B * T
        print("sum of y^2 over %d steps of %d vehicles: %.6g against the nominal model, %.6g against the learned handle" % (T, B, total[0], total[1]))
        assert np.isfinite(total).all() and total[1] < total[0]
    finally:
        fc.close(); truth.close()


# ---- 9. arguments -------------------------------------------------------------------------------------------------------------------

def test_argument_errors(gpu_engine_factory):
    import torch
    N, B = 20, 6
    road = TL._road(M=200)
    pose = TL._along(road, np.linspace(5, 100, B).astype(int), seed=70)
    tk = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    plain, fc = TL._controller(N, B), TL._controller(N, B, learn=LOOP_LEARN)
    cfg = fc._nominal.cfg.copy()
    cfg.ubu[0] += 1.0
    narrow = gpu_engine_factory(cfg)
    try:
        ins = TP._poses(pose)
        plain.set_paths([road]); fc.set_paths([road])
        for call in (lambda: plain.observe(*ins), lambda: plain.observe_latch(*ins), lambda: plain.observe_reset(), lambda: plain.fit_gp(),
                     lambda: plain.learned_gps(), lambda: plain.set_observer(True), lambda: plain.rollout_route(tk, *ins, steps=1, observe=True)):
            with pytest.raises(ValueError, match="does not learn"):
                call()
        with pytest.raises(ValueError, match="bad bins"):
            TL._controller(N, B, learn=[_learn(3, 33)])
        fc.set_plant(model=narrow)
        for call in (lambda: fc.observe(*ins), lambda: fc.rollout_route(tk, *ins, steps=1, observe=True)):
            with pytest.raises(ValueError, match="lbu / ubu"):
                call()
        fc.observe_reset(); fc.learned_gps(); fc.fit_gp(install=False)             # calls that observe nothing are not refused for it
        fc.set_plant()
        with pytest.raises(ValueError, match="shape"):
            fc.observe(*ins[:6], ins[6][:5].contiguous())
        assert fc._eng.cfg.n_gp == 2 and fc._nominal.cfg.n_gp == 0 and fc._eng.cfg.gp[0].n_points == 0
        assert [len(g["alpha"]) for g in fc.learned_gps()] == [0, 0]               # nothing fitted yet: the placeholders
        # a fit whose weights overflow: the install replaces the record by the empty GP, and learned_gps returns what the handle holds
        stats = np.zeros((4, 32, 5))
        stats[0, 2], stats[0, 3] = [1.0, 5.5, 0.0, 0.0, 1e308], [1.0, 6.5, 0.0, 0.0, -1e308]
        fc.bins.copy_(_dev(stats))
        info, installed = fc.fit_gp()
        assert info.cpu().tolist() == [2, 0] and installed.cpu().tolist() == [0, 1]
        gps = fc.learned_gps()
        assert gps[0] == dict(feat=3, out=3, Z=[], alpha=[], length_scale=1.0, sigma_f=0.0, ymean=0.0) and len(gps[1]["alpha"]) == 0
        _bits(TP._host(ins), pose, "poses after refused calls")
    finally:
        plain.close(); fc.close(); narrow.close()
