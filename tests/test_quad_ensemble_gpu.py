"""A clustered GP ensemble in the quadrotor's closed loop, flown and learned on the device (include/admpc_quad_ensemble.h;
ad_mpc_amd/quad_ensemble_fleet.py).

The routing is compared with its numpy spec (tests/quad_ensemble_spec.py) and with admpc_quad_select_cluster_batch on dense copies of
the rows; the routed rollout, bit for bit, with the loop it replaces, driven from Python; a K = 1 ensemble and one of identical clusters
with QuadFleet; the cluster binning with quad_learn_spec.accumulate under the masking identity; the fit and the install with the
single-handle entries per cluster; the observed rollout with latch + (step, observe) x T and with a captured graph; then a short closed
loop that learns its plant per cluster."""
import ctypes as C

import numpy as np
import pytest

import learn_spec as LS
import quad_ensemble_spec as ES
import quad_learn_spec as QL
import quad_plant_spec as QS
import test_quad_fleet_gpu as TQ
import test_quad_learn_gpu as TL

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _stream = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._stream
SIZES = (1, 63, 64, 65, 200)
ENS_STATE = TQ.STATE + ("tally", "cost", "iters", "route")
VX = lambda lo, hi, **kw: dict(dict(feat=7, out=7, lo=[lo], hi=[hi], bins=[32], length_scale=2.0, noise=1e-4, count_noise=1e-2), **kw)


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _gps(seed):
    from test_quad_oracle import quad_gps
    return quad_gps(seed=seed)


def _fleet(B, N, trajs, traj_of, idx0, x0, quad=None, **kw):
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    fl = QuadEnsembleFleet(B, quad=SimQuad(drag=True) if quad is None else quad, n_nodes=N, **kw)
    fl.set_trajectories(trajs)
    fl.reset(traj_of, idx0, x0)
    return fl


def _state(fl):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(fl, k).cpu().numpy() for k in ENS_STATE}


def _same_state(got, want, what, keys=ENS_STATE):
    for k in keys:
        _bits(got[k], want[k], "%s: %s" % (what, k))


# ---- 1. routing from the window -------------------------------------------------------------------------------------------------------

def _windows(B, N, feats, cent, seed):
    """Random windows [B, N, 17] with unit quaternions, redrawn until the nearest and the second-nearest centroid of row 0 are 1e-6 apart;
    then the constructed rows: 0 a tie on exactly representable numbers, 1 (where B > 2) a NaN feature."""
    rng = np.random.default_rng(seed)
    Y = rng.normal(size=(B, N, 17)) * 2.0
    for b in range(B):
        while True:
            Y[b, :, 3:7] /= np.linalg.norm(Y[b, :, 3:7], axis=1, keepdims=True)
            if ES.margin(ES.z_of_row(Y[b, 0])[feats], cent) >= 1e-6:
                break
            Y[b] = rng.normal(size=(N, 17)) * 2.0
    tie = np.zeros(17); tie[3], tie[13] = 1.0, 0.5                                                # level, v = 0, first rotor at 0.5
    Y[0, 0] = tie
    if B > 2:
        Y[1, 0, 7] = np.nan
    return Y


@pytest.mark.parametrize("N", [10, 20])
def test_route_from_the_window_equals_the_spec_and_the_select_kernel(N):
    """feats (7, 13), K = 4 with centroids 1 and 2 at (+1, 0.5) and (-1, 0.5): row 0 of vehicle 0 (level, at rest, rotor 0 at 0.5) lies
    exactly between them and goes to 1, the lower index; a NaN velocity gives 0.  N = 10 at B = 1, 63, 64, 65 and 200, N = 20 at B = 65:
    the row stride is N * 17."""
    import torch
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config
    L = TQ._lib()
    feats, cent = [7, 13], np.array([[3.0, 0.9], [1.0, 0.5], [-1.0, 0.5], [-3.0, -0.6]])
    engs = [QuadBatchSolver(default_quad_config(N=N, t_horizon=N / 10.0)) for _ in range(4)]
    h = C.c_void_p(0)
    try:
        handles = (C.c_void_p * 4)(*[e._h for e in engs])
        assert L.admpc_quad_ensemble_create(handles, 4, 2, (C.c_int32 * 2)(*feats), cent.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(h)) == 0, L.admpc_last_error()
        hit = set()
        for B in (SIZES if N == 10 else (65,)):
            Y = _windows(B, N, feats, cent, seed=B + N)
            want = ES.route_window(Y, feats, cent)
            gaps = np.array([ES.margin(ES.z_of_row(Y[b, 0])[feats], cent) for b in range(B)])
            free = np.ones(B, dtype=bool); free[:2 if B > 2 else 1] = False
            assert gaps[0] == 0.0 and want[0] == 1 and (gaps[free] >= 1e-6).all()
            yref = _dev(Y)
            route = torch.full((B,), 77, dtype=torch.int32, device="cuda:0")
            assert L.admpc_quad_ensemble_route_batch(h, B, _p(yref), _p(route), _stream()) == 0, L.admpc_last_error()
            dense = torch.full((B,), 78, dtype=torch.int32, device="cuda:0")
            xs, us, cd = yref[:, 0, :13].contiguous(), yref[:, 0, 13:].contiguous(), _dev(cent)
            assert L.admpc_quad_select_cluster_batch(0, B, 2, (C.c_int32 * 2)(*feats), _p(xs), _p(us), 4, _p(cd), _p(dense), _stream()) == 0
            got = _host(route)
            _bits(got, want, "route against the spec, B = %d" % B)
            _bits(got, _host(dense), "route against admpc_quad_select_cluster_batch on dense rows, B = %d" % B)
            _bits(_host(yref), Y, "the window is read-only")
            if B > 2:
                assert got[1] == 0 and np.isnan(Y[1, 0, 7])
            hit |= set(got.tolist())
        assert hit == {0, 1, 2, 3}
    finally:
        L.admpc_quad_ensemble_destroy(h)
        for e in engs:
            e.close()


# ---- 2. the routed rollout against the loop it replaces -------------------------------------------------------------------------------

def _python_loop(fl, trajs, T):
    """The loop the routed rollout replaces, each step a call of its own: window, routing from the window, routed solve, plant step under
    w_opt[:, 0] (the noisy one on a fleet with disturbances), index update; the tally and the counts by the spec."""
    import torch
    B = fl.B
    pos = torch.empty((B, 3), dtype=torch.float64, device=fl.device)
    tally, counts = np.zeros((B, 3)), np.zeros((B, 3), dtype=np.int32)
    traj, us, routes = [_host(fl.x)], [], []
    traj_of = _host(fl.traj_of)
    for _ in range(T):
        fl.ref_chunk(pos_ref=pos)
        fl.route_window()
        fl.solve_routed()
        u0, st, pr, x = _host(fl.w_opt)[:, 0, :].copy(), _host(fl.status), _host(pos), _host(fl.x)
        for b in range(B):
            QS.tally_step(tally[b], counts[b], pr[b], x[b], st[b], not np.isfinite(u0[b]).all())
        fl.plant_step(fl.w_opt[:, 0, :])
        fl.idx.copy_(torch.as_tensor(QS.next_idx(trajs, traj_of, _host(fl.idx))))
        us.append(u0); traj.append(_host(fl.x)); routes.append(_host(fl.route).copy())
    fl.counts.copy_(torch.as_tensor(counts))
    fl.tally.copy_(torch.as_tensor(tally))
    return np.stack(traj), np.stack(us), np.stack(routes)


# Centroids on the body-frame v_x for the circles of TQ._circles(N, 3.0): the rows are 1 / (5 N) s apart, so the span the vehicles' start
# rows cover shrinks with N (0 .. -2.9 m/s at N = 10 and, wrapping, at N = 5; 0 .. -2.1 at N = 17; 0 .. -1.9 at N = 20, -1.7 at B = 33).
# N = 20: the cell boundaries -0.59 and -1.19 lie between start rows, and the vehicle at -1.174 passes -1.19 within two steps (-1.207).
VX_CENT = {5: [[-0.5], [-1.5], [-2.5]], 10: [[-0.5], [-1.5], [-2.5]], 17: [[-0.35], [-1.05], [-1.75]], 20: [[-0.29], [-0.89], [-1.49]]}


@pytest.mark.parametrize("N,B,T,noisy", [pytest.param(10, 65, 6, False, id="False"), pytest.param(10, 65, 6, True, id="True"),
                                         pytest.param(20, 33, 3, False, id="N20-False")])
def test_routed_rollout_equals_the_loop_it_replaces(N, B, T, noisy):
    """T = 6, B = 65, K = 3 clusters with distinct GPs on the body-frame v_x, which falls from 0 to -2.9 m/s along the circle the vehicles
    are spread over: every cluster solves, and vehicles cross a boundary within the run.  Once with the deterministic plant, once under
    both disturbances with drag, from the same reseed.  N = 20 (the two-wave kernel) at the sizes test_quad_fleet_gpu.py uses there,
    B = 33 and T = 3, with the deterministic plant and the centroids of VX_CENT."""
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    from ad_mpc_amd.quad_config import SimQuad
    trajs = TQ._circles(N, 3.0)
    traj_of = (np.arange(B) % 2).astype(np.int32)
    idx0 = np.where(traj_of == 1, 3, (np.arange(B) * 3) % 110).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=12)
    ens = QuadGPEnsemble([_gps(1), _gps(2), _gps(3)], VX_CENT[N], [7])
    quad = SimQuad(drag=True, noisy=True, motor_noise=True) if noisy else None
    kw = dict(ensemble=ens, quad=quad, noise_seed=5 if noisy else None)
    whole, loop = (_fleet(B, N, trajs, traj_of, idx0, x0, **kw) for _ in range(2))
    try:
        if noisy:
            whole.reseed(step=3); loop.reseed(step=3)
        out = whole.rollout(T, record=True)
        traj, us, routes = _python_loop(loop, trajs, T)
        got, want = _state(whole), _state(loop)
        _same_state(got, want, "the rollout against the loop")
        _bits(_host(out.traj), traj, "traj"); _bits(_host(out.u), us, "u"); _bits(_host(out.routes), routes, "routes")
        _bits(routes[-1], got["route"], "route holds the last period's clusters")
        assert set(routes.reshape(-1).tolist()) == {0, 1, 2} and (routes[0] != routes[-1]).any()       # every cluster solves; vehicles change cluster
        assert (got["counts"] == [T, 0, 0]).all() and (got["status"] == 0).all()
        if noisy:
            _bits(_host(whole.noise_step), _host(loop.noise_step), "noise_step"); assert (_host(whole.noise_step) == 3 + T).all()
        # the clusters act: the same fleet under one cluster's GPs alone flies elsewhere
        if not noisy:
            from ad_mpc_amd.quad_fleet import QuadFleet
            one = QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, gp_regressors=_gps(1))
            one.set_trajectories(trajs); one.reset(traj_of, idx0, x0)
            one.rollout(T)
            diff = np.abs(_host(one.w_opt) - got["w_opt"]).reshape(B, -1).max(axis=1)
            assert (diff[routes[-1] != 0] > 1e-9).all()
            one.close()
    finally:
        whole.close(); loop.close()


# ---- 3. one cluster, identical clusters, and the cluster binning ----------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(10, 4), (20, 3), (17, 3), (5, 3)])
def test_one_cluster_and_identical_clusters_fly_what_the_single_handle_flies(N, T):
    """B = 65.  N = 10 on the one-wave dense kernel, 20 on the two-wave kernel, 17 on the wide and 5 on the generic path: an ensemble of
    K = 1 and one of K = 3 identical clusters (centroids VX_CENT[N]: all three routes occur) fly the bits of the QuadFleet with those GPs."""
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    B = 65
    trajs = TQ._circles(N, 3.0)
    traj_of = (np.arange(B) % 2).astype(np.int32)
    idx0 = np.where(traj_of == 1, 3, (np.arange(B) * 3) % 110).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=2)
    gps = _gps(4)
    plain = QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, gp_regressors=gps)
    plain.set_trajectories(trajs); plain.reset(traj_of, idx0, x0)
    one = _fleet(B, N, trajs, traj_of, idx0, x0, ensemble=QuadGPEnsemble([gps], [[0.0]], [7]))
    three = _fleet(B, N, trajs, traj_of, idx0, x0, ensemble=QuadGPEnsemble([gps, gps, gps], VX_CENT[N], [7]))
    try:
        ref = plain.rollout(T, record=True)
        want = TQ._state(plain)
        for fl, what in ((one, "K = 1"), (three, "K = 3, identical clusters")):
            out = fl.rollout(T, record=True)
            _same_state(_state(fl), want, what, keys=TQ.STATE + ("tally", "cost", "iters"))
            _bits(_host(out.traj), _host(ref.traj), what + ": traj"); _bits(_host(out.u), _host(ref.u), what + ": u")
        assert not _host(one.route).any() and set(_host(three.route).tolist()) == {0, 1, 2}
    finally:
        plain.close(); one.close(); three.close()


BIN_LEARN = [[VX(-6.0, -1.0), dict(TL.THREE[1])], [VX(-2.0, 2.5, bins=[16]), dict(TL.THREE[1], lo=[-3.0, -1.0], hi=[3.0, 1.0], bins=[4, 8])],
             [VX(2.0, 4.5, bins=[8], length_scale=1.0), dict(TL.THREE[1], bins=[2, 2])]]
BIN_CENT = np.array([[-3.4], [1.1], [4.0]])          # about the 1/6, 1/2 and 5/6 quantiles of the body-frame v_x of QS.fleet67


def test_cluster_bins_and_dropped_counts_match_the_masked_spec_bit_for_bit():
    """The records of tests/test_quad_learn_gpu.py's fleet at B = 1, 63, 64, 65 and 200, two accumulating calls each, K = 3 on v_x with a
    box per cluster that is narrower than the cluster's cell.  bins[c] and dropped[c][:3] against quad_learn_spec.accumulate under block
    c of the device's own records with the flags of the other clusters' records cleared; dropped[0][3] the records that are not valid."""
    import torch
    fl = _fleet(1, 10, TQ._circles(10, 3.0), [0], [0], None, centroids=BIN_CENT, feats=[7], learn=BIN_LEARN)
    L, plant = fl.lib, TL._plant()
    assert bytes(plant) == bytes(fl._plant)
    blocks = list(fl._obs)
    try:
        for B in SIZES:
            prev, now, U = TL._fleet(B)
            wb, wd = np.zeros((3, 3, 32, 5)), np.zeros((3, 4), dtype=np.int32)
            bins, dropped = _dev(wb), _dev(wd, torch.int32)
            dropped[1:, 3] = 41                                                                  # [c > 0][3] stay as given
            wd[1:, 3] = 41
            pv, u, invalid, seen = _dev(prev), _dev(U), 0, np.zeros(3, dtype=int)
            for call in range(2):
                x = _dev(now if call == 0 else now + np.random.default_rng(B).normal(size=now.shape) * 0.05)
                samples = torch.full((B, 14), 7.0, dtype=torch.float64, device="cuda:0")
                rc = L.admpc_quad_ensemble_observe_batch(fl._ens, fl._nominal._h, C.byref(plant), B, _p(u), 4, _p(x), _p(pv), _p(samples),
                                                         _p(bins), _p(dropped), _stream())
                assert rc == 0, L.admpc_last_error()
                S = _host(samples)
                valid = S[:, 13] == 1.0
                route = ES.route_records(S, [7], BIN_CENT)
                assert min(ES.margin(r[[0]], BIN_CENT) for r in S[valid]) >= 1e-9
                invalid += int((~valid).sum())
                seen += np.bincount(route[valid], minlength=3)
                for c in range(3):
                    Sc = S.copy()
                    Sc[valid & (route != c), 13] = 0.0
                    d1 = np.zeros(4, dtype=np.int32)
                    QL.accumulate(blocks[c], Sc, wb[c], d1)
                    wd[c, :3] += d1[:3]
                wd[0, 3] += int((~valid).sum())
                _bits(_host(bins), wb, "bins after call %d, B = %d" % (call, B)); _bits(_host(dropped), wd, "dropped after call %d, B = %d" % (call, B))
                _bits(_host(pv), _host(x), "the latch")
            # the spec written from the contract agrees with the identity; every record is accounted for exactly once per regressor
            for g in range(2):
                assert wb[:, g, :, 0].sum() + wd[:, g].sum() + invalid == 2 * B
            assert not wb[:, 2].any() and not wd[:, 2].any()
            if B >= 63:
                assert (seen > 0).all() and wd[:, :2].max() > 0 and invalid >= 2
    finally:
        fl.close()


# ---- 4. fit and install ---------------------------------------------------------------------------------------------------------------

def test_fit_and_install_are_the_single_handle_entries_per_cluster():
    """Hand-made statistics: cluster 0 full, cluster 1 with no bin filled (n_points 0), cluster 2 with a target that is not finite (a
    failing pivot: the empty GP, info -(k + 1)).  gp_out[c] and info[c] bit for bit admpc_quad_gp_fit of bins[c] under block c.  After the
    install a routed solve equals the routed solve of handles created from learned_gps(); then a cluster whose weights overflow: its
    record alone becomes the empty GP."""
    import torch
    from ad_mpc_amd.config import AdmpcGp
    from ad_mpc_amd.engine import QuadEnsembleBatchSolver
    from ad_mpc_amd.quad_fleet import fleet_quad_config
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_scenarios import random_quad_scenarios
    B, N = 65, 10
    learn = [[VX(-6.0, -1.0), dict(TL.THREE[1]), dict(TL.THREE[2])], [VX(-2.0, 2.5, bins=[16]), dict(TL.THREE[1], noise=1e-3), dict(TL.THREE[2])],
             [VX(2.0, 4.5, bins=[8], length_scale=1.0), dict(TL.THREE[1]), dict(TL.THREE[2], count_noise=0.1)]]
    cent = np.array([[-3.4], [1.1], [4.0]])
    fl = _fleet(B, N, TQ._circles(N, 3.0), np.zeros(B, dtype=np.int32), np.arange(B, dtype=np.int32), None, centroids=cent, feats=[7], learn=learn)
    L, per = fl.lib, 3 * C.sizeof(AdmpcGp)
    try:
        rng = np.random.default_rng(31)
        stats = np.zeros((3, 3, 32, 5))
        for c in (0, 2):
            for g, fill in enumerate((8, 20, 27)):
                stats[c, g] = LS.hand_stats(fl._obs[c].gp[g], rng, fill)
        k = np.flatnonzero(stats[2, 1, :, 0] >= 4)[2]
        stats[2, 1, k, 4] = np.inf
        fl.bins.copy_(_dev(stats))
        fl._gp_dev.fill_(0x5A); fl.fit_info.fill_(77)
        info, _ = fl.fit_gp(min_count=4, install=False)
        got_raw, got_info = _host(fl._gp_dev).tobytes(), _host(info)
        for c in range(3):
            want, wi = TL._fit(L.admpc_quad_gp_fit, fl._obs[c], stats[c], 4, 3)
            assert got_raw[c * per:(c + 1) * per] == b"".join(bytes(r) for r in want), "gp_out of cluster %d" % c
            _bits(got_info[c], wi, "info of cluster %d" % c)
        points = [[int((stats[c, g, :, 0] >= 4).sum()) for g in range(3)] for c in range(3)]
        assert got_info[0].tolist() == points[0] and min(points[0]) >= 4 and got_info[1].tolist() == [0, 0, 0]
        assert got_info[2].tolist() == [points[2][0], -3, points[2][2]]
        points[2][1] = 0
        # install: the fleet's handles against handles created with what was learned
        info, installed = fl.fit_gp(min_count=4)
        assert (_host(installed) == 1).all()
        learned = fl.learned_gps()
        assert [[len(g["alpha"]) for g in cl] for cl in learned.clusters] == points
        assert np.array_equal(learned.centroids, cent) and learned.feats == [7]
        s = random_quad_scenarios(B, fl.cfg, seed=3)
        route = (np.arange(B) % 3).astype(np.int32)
        fresh = QuadEnsembleBatchSolver(fleet_quad_config(SimQuad(drag=True), 1.0, N), learned.clusters, cent, [7])

        rt, x0, yref, yref_e = _dev(route), _dev(s["x0"]), _dev(s["yref"]), _dev(s["yref_e"])       # alive for as long as the solves run

        def solve(handles):
            xb, ub = _dev(s["xbar"]).clone(), _dev(s["ubar"]).clone()
            cost = torch.empty(B, dtype=torch.float64, device="cuda:0"); st = torch.empty(B, dtype=torch.int32, device="cuda:0"); it = torch.empty_like(st)
            rc = L.admpc_quad_solve_batch_routed(handles, 3, B, _p(rt), _p(x0), _p(yref), _p(yref_e), None, _p(xb),
                                                 _p(ub), _p(cost), _p(st), _p(it), _stream())
            assert rc == 0, L.admpc_last_error()
            return [_host(t) for t in (xb, ub, cost, st, it)]

        got, want = solve(fl._handles), solve(fresh._handles)
        for a, b, what in zip(got, want, ("xbar", "ubar", "cost", "status", "iters")):
            _bits(a, b, "%s of the installed handles against handles created with the learned GPs" % what)
        fl.observe_reset(); fl.fit_gp()                                                          # no statistics: placeholders everywhere
        base = solve(fl._handles)
        assert np.abs(got[1] - base[1])[route != 1].max() > 1e-6 and np.array_equal(got[1][route == 1], base[1][route == 1])
        fresh.close()
        # weights that overflow in cluster 1 alone
        stats = np.zeros((3, 3, 32, 5))
        stats[1, 0, 5], stats[1, 0, 9] = [1.0, -0.9, 0.0, 0.0, 1e308], [1.0, 0.8, 0.0, 0.0, -1e308]
        stats[0, 0] = LS.hand_stats(fl._obs[0].gp[0], rng, 8)
        fl.bins.copy_(_dev(stats))
        info, installed = fl.fit_gp()
        assert _host(info).tolist() == [[8, 0, 0], [2, 0, 0], [0, 0, 0]] and _host(installed).tolist() == [[1, 1, 1], [0, 1, 1], [1, 1, 1]]
        again = fl.learned_gps().clusters
        assert again[1][0] == dict(feat=7, out=7, Z=[], alpha=[], length_scale=1.0, sigma_f=0.0, ymean=0.0) and len(again[0][0]["alpha"]) == 8
    finally:
        fl.close()


# ---- 5. the observed rollout ------------------------------------------------------------------------------------------------------------

LOOP_LEARN = [[VX(-4.0, -1.5)] + [dict(d) for d in QL.EXP_LEARN[1:]], [VX(-2.5, -0.5)] + [dict(d) for d in QL.EXP_LEARN[1:]],
              [VX(-1.5, 1.0)] + [dict(d) for d in QL.EXP_LEARN[1:]]]
LOOP_CENT = np.array([[-2.5], [-1.5], [-0.5]])
LEARN_STATE = ("bins", "dropped", "samples", "_prev")


def test_observed_rollout_equals_latch_then_step_and_observe_and_a_graph_reads_new_gps():
    """N = 10, B = 67, T = 4 on the circle at 3 m/s.  `whole`: one rollout with observe; `loop`: observe_latch, then T times rollout(1)
    and observe().  Then rollout(2) is captured on one stream, statistics are fitted and installed after the capture, and the replay
    equals the eager rollout of a fleet that did the same, and differs from the rollout before the install."""
    import torch
    N, B, T = 10, 67, 4
    trajs = TQ._circles(N, 3.0)
    traj_of = np.zeros(B, dtype=np.int32)
    idx0 = ((np.arange(B) * 3) % 100).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=6)
    whole, loop = (_fleet(B, N, trajs, traj_of, idx0, x0, centroids=LOOP_CENT, feats=[7], learn=LOOP_LEARN) for _ in range(2))
    try:
        out = whole.rollout(T, record=True, observe=True)
        loop.observe_latch()
        for t in range(T):
            loop.rollout(1)
            loop.observe()
        got, want = _state(whole), _state(loop)
        _same_state(got, want, "observed rollout against latch + (step, observe) x T")
        for k in LEARN_STATE:
            _bits(_host(getattr(whole, k)), _host(getattr(loop, k)), k)
        bins, dropped = _host(whole.bins), _host(whole.dropped)
        assert (got["counts"] == [T, 0, 0]).all() and not dropped[:, 3].any()
        for g in range(3):
            assert bins[:, g, :, 0].sum() + dropped[:, g].sum() == B * T
        assert (bins[:, 0, :, 0].sum(axis=1) > 0).all() and set(_host(out.routes).reshape(-1).tolist()) == {0, 1, 2}
        _bits(_host(whole._prev), got["x"], "the latch holds the final states")
        # a captured rollout reads the GPs installed after the capture
        eager, graphed = whole, loop
        for fl in (eager, graphed):
            fl.reset(traj_of, idx0, x0)
        graphed.rollout(2)                                                                       # every kernel has run once before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.rollout(2)
        eager.rollout(2)
        without = _state(eager)
        rng = np.random.default_rng(4)
        stats = np.zeros((3, 3, 32, 5))
        for c in range(3):
            for k in range(3):
                stats[c, k] = LS.hand_stats(eager._obs[c].gp[k], rng, 20)
        for fl in (eager, graphed):
            fl.reset(traj_of, idx0, x0)
            fl.bins.copy_(_dev(stats))
            info, installed = fl.fit_gp()
            assert (_host(info) == 20).all() and (_host(installed) == 1).all()
        eager.rollout(2)
        g.replay()
        _same_state(_state(graphed), _state(eager), "the replay against the eager rollout")
        assert (_state(eager)["status"] == 0).all() and np.abs(_state(eager)["w_opt"] - without["w_opt"]).max() > 1e-6
    finally:
        whole.close(); loop.close()


# ---- 6. a short closed loop -------------------------------------------------------------------------------------------------------------

def test_a_short_closed_loop_learns_its_plant_per_cluster():
    """The setting of tests/test_quad_learn_gpu.py's closed loop (B = 64, N = 10, circles of 5 m at 2, 3, 4 and 5 m/s, drag on, 60 observed
    steps, fit, reset, 60 steps) with K = 3 clusters on the body-frame v_x.  The centroids and the v_x boxes of the first regressor come
    from the reference trajectories alone: the terciles q1, q2 of the reference's v_x over the rows the fleet visits are the cell
    boundaries, each box is its cell widened by 0.25 m/s (0.5 m/s at the ends).  On the reference rows the three first regressors occupy
    26, 24 and 18 of their 32 bins; under the numpy plant of tests/quad_plant_spec.py flown open loop on the reference inputs 10, 24, 19.
    Measured on the MI355X: 1081 / 1370 / 1389 records per cluster on 22 / 24 / 19 occupied v_x bins, nothing dropped; summed position
    error 532.879 m with the nominal model, 120.602 m with the K = 3 clusters learned from the first pass, 120.645 m with the unclustered
    QuadFleet(learn=...) on the same run: the clusters buy 0.04 m here.  Only learned < nominal is asserted."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, B, T = 10, 64, 60
    dt = 1.0 / (N * 5)
    trajs = [circle_reference(T + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
    traj_of = (np.arange(B) % 4).astype(np.int32)
    idx0 = (np.arange(B) // 4).astype(np.int32)
    ref = np.concatenate([[QL.body_velocity(trajs[k][0][i + t])[0] for t in range(T)] for k, i in zip(traj_of, idx0)])
    q1, q2 = np.quantile(ref, [1 / 3, 2 / 3])
    mid = (q1 + q2) / 2
    cent = np.array([[2 * q1 - mid], [mid], [2 * q2 - mid]])
    boxes = [(ref.min() - 0.5, q1 + 0.25), (q1 - 0.25, q2 + 0.25), (q2 - 0.25, ref.max() + 0.5)]
    learn = [[VX(lo, hi)] + [dict(d) for d in QL.EXP_LEARN[1:]] for lo, hi in boxes]
    cell = np.array([ES.nearest([v], cent) for v in ref])
    for c, (lo, hi) in enumerate(boxes):
        k = np.floor((ref[cell == c] - lo) * (32 / (hi - lo)))
        assert len(np.unique(k[(k >= 0) & (k < 32)])) >= 8, c
    fl = _fleet(B, N, trajs, traj_of, idx0, None, centroids=cent, feats=[7], learn=learn)
    plain = TL._learning_fleet(B, N, trajs, traj_of, idx0, None)
    try:
        total = {}
        for name, f in (("clustered", fl), ("unclustered", plain)):
            total[name] = []
            for r in range(2):
                f.reset(traj_of, idx0)
                f.rollout(T, observe=True)
                total[name].append(float(_host(f.tally)[:, 0].sum()))
                assert (_host(f.counts) == [T, 0, 0]).all()
                if r == 0:
                    info, installed = f.fit_gp(min_count=2)
                    info, installed = _host(info), _host(installed)
                    if f is fl:
                        bins, dropped = _host(f.bins), _host(f.dropped)
                        occupied = (bins[:, 0, :, 0] > 0).sum(axis=1)
                        print("records per cluster %s, occupied v_x bins %s, dropped %s, points %s"
                              % (bins[:, 0, :, 0].sum(axis=1).tolist(), occupied.tolist(), dropped.tolist(), info.tolist()))
                        assert not dropped[:, 3].any() and all(bins[:, g, :, 0].sum() + dropped[:, g].sum() == B * T for g in range(3))
                        assert (occupied >= 8).all()
                    assert info.min() >= 2 and (installed == 1).all()
        print("sum of |e| over %d steps of %d vehicles: nominal %.6g m, learned with K = 3 clusters %.6g m, learned unclustered %.6g m (its nominal pass %.6g m)"
              % (T, B, total["clustered"][0], total["clustered"][1], total["unclustered"][1], total["unclustered"][0]))
        assert np.isfinite(total["clustered"]).all() and total["clustered"][1] < total["clustered"][0]
    finally:
        fl.close(); plain.close()


# ---- 7. the refusals behind a live handle -----------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_no_ops():
    """Every refusal the header lists that needs a handle, in the listed order (a call that breaks two rules is refused for the first);
    nothing on the device moves."""
    import torch
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    from ad_mpc_amd.quad_config import SimQuad, default_quad_config, quad_noise_params
    N, B = 10, 5
    trajs = TQ._circles(N, 3.0)
    traj_of, idx0 = np.zeros(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    fl = _fleet(B, N, trajs, traj_of, idx0, None, centroids=LOOP_CENT, feats=[7], learn=LOOP_LEARN)
    flies = _fleet(B, N, trajs, traj_of, idx0, None, ensemble=QuadGPEnsemble([[], []], [[0.0], [1.0]], [2]))
    sqp_cfg = default_quad_config(); sqp_cfg.sqp_iters = 3
    sqp, n20 = QuadBatchSolver(sqp_cfg), QuadBatchSolver(default_quad_config(N=20, t_horizon=2.0))
    L, null = fl.lib, C.c_void_p(0)
    try:
        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        out = C.c_void_p(0)
        H = lambda *hs: (C.c_void_p * len(hs))(*hs)
        own, nom = [s._h for s in fl._solvers], fl._nominal._h
        obs3 = (type(fl._obs[0]) * 3)(*fl._obs)

        def create(h=H(*own), K=3, nf=1, f=(7,), c=(0.0, 1.0, 2.0), obs=obs3):
            return L.admpc_quad_ensemble_create(h, K, nf, (C.c_int32 * 3)(*f), (C.c_double * 24)(*c), obs, C.byref(out))

        def blocks(**kw):
            b = (type(fl._obs[0]) * 3)(*fl._obs)
            for k, v in kw.items():
                setattr(b[2], k, v)
            return b

        other_feat = blocks(); other_feat[2].gp[1].feat[0] = 9
        other_out = blocks(); other_out[2].gp[1].out = 9
        other_box = blocks(); other_box[2].gp[0].lo[0] = -7.0; other_box[2].gp[0].nb[0] = 4; other_box[2].gp[0].length[0] = 0.3
        refused(create(h=H(own[0], n20._h, sqp._h), nf=0), "share device and horizon")              # 3 before 4
        refused(create(h=H(own[0], own[1], sqp._h), nf=0), "sqp_iters > 1")                          # 4 before 5
        refused(create(nf=0, c=(np.nan, 0.0, 0.0)), "n_feat must be in [1, 3]"); refused(create(nf=4), "n_feat must be in [1, 3]")     # 5 before 6
        refused(create(f=(17,), c=(np.nan, 0.0, 0.0)), "feature index outside"); refused(create(f=(-1,)), "feature index outside")
        refused(create(c=(0.0, np.inf, 2.0), obs=blocks(substeps=0)), "a centroid is not finite")    # 6 before 7
        refused(create(obs=blocks(substeps=0, dt=0.03), f=(2,)), "substeps must be in [1, 64]")      # 7 before 8 and 9
        bad_first = blocks(n_gp=2); bad_first[0].gp[0].nb[0] = 33
        refused(create(obs=bad_first), "regressor 0: the product of nb must not exceed 32")          # 7 in the order of the clusters
        refused(create(obs=blocks(dt=0.03), f=(2,)), "must share dt, substeps, n_gp")                # 8 before 9
        refused(create(obs=blocks(substeps=2)), "must share dt, substeps, n_gp"); refused(create(obs=blocks(n_gp=2)), "must share dt, substeps, n_gp")
        refused(create(obs=other_feat), "must share dt, substeps, n_gp"); refused(create(obs=other_out), "must share dt, substeps, n_gp")
        refused(create(f=(2,), h=H(own[0], own[1], nom)), "features in [7, 16]")                     # 9 before 10
        refused(create(h=H(own[0], own[1], nom)), "n_gp is not the observe parameters' n_gp")        # 10
        assert out.value is None
        assert create(obs=other_box) == 0, L.admpc_last_error()                                      # the box, nb and the hyperparameters may differ
        L.admpc_quad_ensemble_destroy(out)
        assert create(f=(2,), h=H(own[0], own[1], nom), obs=None) == 0                               # an ensemble that only flies: any feature, any n_gp
        L.admpc_quad_ensemble_destroy(out)

        keys = TQ.STATE + ("tally", "route") + LEARN_STATE
        before = {k: _host(getattr(fl, k)).copy() for k in keys}
        route = lambda e=fl._ens, B=B, y=_p(fl.yref), r=_p(fl.route): L.admpc_quad_ensemble_route_batch(e, B, y, r, fl._stream())
        refused(route(B=-1, y=null), "negative batch")
        refused(route(y=null), "null array"); refused(route(r=null), "null array")
        assert route(B=0, y=null, r=null) == 0

        bad_plant = fl._plant.copy(); bad_plant.substeps = 0

        def observe(**kw):
            a = dict(e=fl._ens, model=nom, plant=C.byref(fl._plant), B=B, u=_p(fl.w_opt), stride=N * 4, x=_p(fl.x), bins=_p(fl.bins))
            a.update(kw)
            return L.admpc_quad_ensemble_observe_batch(a["e"], a["model"], a["plant"], a["B"], a["u"], a["stride"], a["x"], _p(fl._prev), _p(fl.samples),
                                                       a["bins"], _p(fl.dropped), fl._stream())
        refused(observe(e=flies._ens, plant=None), "created without observe parameters")
        refused(observe(plant=None, model=null), "plant parameters are not set")
        refused(observe(plant=C.byref(bad_plant), model=null), "substeps must be in [1, 1024]")
        refused(observe(model=null, B=-1), "null model")
        refused(observe(B=-1, u=null), "negative batch")
        refused(observe(u=null, stride=3), "null array"); refused(observe(bins=null), "null array")
        refused(observe(stride=3), "u_stride must be at least 4")
        assert observe(B=0, u=null, x=null) == 0

        fit = lambda e=fl._ens, mc=1, bins=_p(fl.bins), info=_p(fl.fit_info): L.admpc_quad_ensemble_fit(e, mc, bins, _p(fl._gp_dev), info, fl._stream())
        refused(fit(e=flies._ens, mc=0), "created without observe parameters")
        refused(fit(mc=0, bins=null), "min_count must be at least 1")
        refused(fit(bins=null), "null array"); refused(fit(info=null), "null array")
        inst = lambda e=fl._ens, gp=_p(fl._gp_dev), o=_p(fl.installed): L.admpc_quad_ensemble_install(e, gp, o, fl._stream())
        refused(inst(e=flies._ens, gp=null), "created without GPs")
        refused(inst(gp=null), "null array"); refused(inst(o=null), "null array")

        noise = quad_noise_params(SimQuad(noisy=True), 5e-4, 1)
        bad_noise = quad_noise_params(SimQuad(noisy=True), 5e-4, 1); bad_noise.noisy = 2
        ns = torch.zeros(B, dtype=torch.int64, device="cuda:0")

        def roll(**kw):
            a = dict(e=fl._ens, bank=fl._bank, plant=C.byref(fl._plant), over=5, B=B, T=2, x=_p(fl.x), tally=_p(fl.tally), route=_p(fl.route), model=nom,
                     prev=_p(fl._prev), dropped=_p(fl.dropped), noise=None, ns=None)
            a.update(kw)
            return L.admpc_quad_ensemble_rollout_batch(a["e"], a["bank"], a["plant"], a["over"], a["B"], a["T"], _p(fl.traj_of), _p(fl.idx), a["x"], _p(fl.x_opt),
                                                       _p(fl.w_opt), _p(fl.yref), _p(fl.yref_e), _p(fl.cost), _p(fl.status), _p(fl.iters), a["tally"],
                                                       _p(fl.counts), None, None, a["route"], None, a["model"], a["prev"], _p(fl.samples), _p(fl.bins),
                                                       a["dropped"], a["noise"], a["ns"], fl._stream())
        refused(roll(e=flies._ens, plant=None, noise=C.byref(noise)), "created without observe parameters")
        refused(roll(plant=None, noise=C.byref(bad_noise), bank=null), "admpc_quad_rollout_noise_batch: the plant parameters are not set")
        refused(roll(noise=C.byref(bad_noise), bank=null), "must be 0 or 1")
        for model, name in ((nom, "admpc_quad_rollout_observe_batch"), (null, "admpc_quad_rollout_batch")):
            refused(roll(model=model, bank=null, plant=None), "admpc_quad_rollout_batch: null bank")
            refused(roll(model=model, plant=C.byref(bad_plant), over=0), "substeps must be in [1, 1024]")
            refused(roll(model=model, over=0, B=-1), "over must be at least 1")
            refused(roll(model=model, B=-1, T=-1), "negative batch")
            refused(roll(model=model, T=4097, x=null), "T must be in [0, 4096]")
            for k in ("x", "tally", "route"):
                refused(roll(model=model, **{k: null}), "null")
            refused(roll(model=model, noise=C.byref(noise), ns=null), "null noise_step")
            assert roll(model=model, B=0, x=null, route=null) == 0 and roll(model=model, T=0, x=null, route=null) == 0
        for k in ("prev", "dropped"):
            refused(roll(**{k: null}), "admpc_quad_rollout_observe_batch: null array")
        assert ns.sum().item() == 0
        torch.cuda.synchronize()
        for k, v in before.items():
            _bits(_host(getattr(fl, k)), v, "%s after refused calls" % k)
        # the Python layer: an ensemble that only flies refuses the learning methods
        for call in (lambda: flies.observe(), lambda: flies.observe_latch(), lambda: flies.observe_reset(), lambda: flies.fit_gp(),
                     lambda: flies.learned_gps(), lambda: flies.set_observer(True), lambda: flies.rollout(1, observe=True)):
            with pytest.raises(ValueError, match="does not learn"):
                call()
        with pytest.raises(ValueError, match="cluster must be in 0 .. 2"):
            fl.set_observer(True, cluster=3)
        assert [[len(g["alpha"]) for g in cl] for cl in fl.learned_gps().clusters] == [[0, 0, 0]] * 3       # nothing fitted yet: the placeholders
    finally:
        fl.close(); flies.close(); sqp.close(); n20.close()
