"""The trajectory generator on the device (include/admpc_quad_traj.h; QuadFleet.generate_trajectories).

Accuracy: the device against the longdouble spec (tests/quad_traj_spec.py, which tests/test_quad_traj_cpu.py pins to the reference's own
trajectories), one forward error bound per column group -- position, quaternion, velocity, rate, input -- derived in DESIGN.md from the
scan structure the kernel has (quad_traj_spec.error_bound(case, "kernel")), never from the device's output.  Every plant here has
g = 3.7: gravity in the rule is the literal 9.81.  Independence, "a generated bank is a bank", the stream and the experiment's orderings
are compared bit for bit or by the orderings of the reference's own figure."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import quad_traj_spec as TS
import test_quad_traj_cpu as TC

pytestmark = pytest.mark.gpu

DTS = [0.27, 0.25, 0.09, 0.1, 0.045, 0.05, 0.019, 0.02, 0.01, 0.005, 0.0025, 0.001]        # 2 / dt is not an integer for 0.27, 0.09, 0.045, 0.019
RATIOS = [2.01 + 0.01 * i for i in range(3200)]
# the smallest M the rule allows (n2 = 1), an odd one with n2 = 1, the edges of a wave and of a tile of the scan, two and three tiles, the
# issue's 600 and 1200, the cap
SHAPES = [34, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 600, 1200, TS.MAX_M]


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lib():
    import torch                                          # torch first, as everywhere: the library then binds to the HIP runtime torch loaded
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ad_mpc_amd import _lib as L
    return L.load()


def _plant(quad):
    from ad_mpc_amd.quad_config import SimQuad, quad_plant_params
    q = SimQuad()
    q.mass, q.max_thrust = quad["mass"], quad["max_thrust"]
    q.J, q.x_f, q.y_f, q.z_l_tau = (np.array(quad[k], dtype=np.float64) for k in ("J", "x_f", "y_f", "z_l_tau"))
    p = quad_plant_params(q, 5e-4, 0.02)
    p.g = 3.7                                             # not read: the rule's gravity is 9.81
    return p


class _Bank:
    """A generated bank of the library for cases that share dt and the vehicle."""

    def __init__(self, lib, cases, stream=None, device=0):
        from ad_mpc_amd import _lib as L
        self.lib, self.K = lib, len(cases)
        specs = [TC._spec(c) for c in cases]
        arr = (type(specs[0]) * self.K)(*specs)
        plant = _plant(cases[0]["quad"])
        self.h = C.c_void_p(0)
        L.check(lib.admpc_quad_traj_bank_generate(device, self.K, arr, C.byref(plant), cases[0]["dt"], stream, C.byref(self.h)))
        M = (C.c_int32 * self.K)()
        K, rows = C.c_int(0), C.c_int64(0)
        L.check(lib.admpc_quad_traj_bank_info(self.h, C.byref(K), C.byref(rows), M))
        self.M = list(M)
        assert K.value == self.K and rows.value == sum(self.M)

    def copy(self, k):
        from ad_mpc_amd import _lib as L
        traj, u = np.full((self.M[k], 13), 7.0), np.full((self.M[k], 4), 7.0)
        dbl = C.POINTER(C.c_double)
        L.check(self.lib.admpc_quad_traj_bank_copy(self.h, k, traj.ctypes.data_as(dbl), u.ctypes.data_as(dbl)))
        return traj, u

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.lib.admpc_quad_traj_bank_destroy(self.h)


def _bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    same = got.view(np.uint8).reshape(-1) == want.view(np.uint8).reshape(-1)
    assert same.all(), (what, int((~same).sum()), "bytes differ")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


RATIO_LOG = {}


def _within_bound(case, traj, u, what):
    """The device's rows against the longdouble spec, group by group; the ratios error / bound are printed and kept."""
    want_t, want_u = TS.generate(case, ft=np.longdouble)
    assert traj.shape == want_t.shape and u.shape == want_u.shape, (what, traj.shape, want_t.shape)
    assert np.isfinite(traj).all() and np.isfinite(u).all(), what
    err, bound = TS.group_errors(traj, u, want_t, want_u), TS.error_bound(case, "kernel")
    for k in err:
        RATIO_LOG[k] = max(RATIO_LOG.get(k, 0.0), err[k] / bound[k])
    print(what, " ".join("%s %.3g/%.3g=%.2g" % (k, err[k], bound[k], err[k] / bound[k]) for k in err))
    for k in err:
        assert err[k] <= bound[k], (what, k, err[k], bound[k])


# -- accuracy ---------------------------------------------------------------------------------------------------------------------------
def test_golden_cases_lie_within_the_error_bound(lib):
    """Every golden case, one launch per (dt, vehicle); also the reference's own stored rows at the bound plus the spec's 1e-12."""
    groups = {}
    for i, c in enumerate(TC.CASES):
        groups.setdefault((c["dt"], json.dumps(c["quad"], sort_keys=True)), []).append(i)
    for ids in groups.values():
        bank = _Bank(lib, [TC.CASES[i] for i in ids])
        try:
            for k, i in enumerate(ids):
                c = TC.CASES[i]
                assert bank.M[k] == c["M"]
                traj, u = bank.copy(k)
                _within_bound(c, traj, u, TC.IDS[i])
                bound = TS.error_bound(c, "kernel")
                ref = np.array(c["values"])
                got = np.concatenate([traj, u], axis=1)[c["rows"]]
                for name, cols in list(TS.GROUPS.items()) + [("input", slice(13, 17))]:
                    assert (np.abs(got[:, cols] - ref[:, cols]) <= bound[name] + 1e-12 * np.maximum(1.0, np.abs(ref[:, cols]))).all(), (TC.IDS[i], name)
        finally:
            bank.close()
    print("worst ratios", RATIO_LOG)


@pytest.mark.parametrize("M", SHAPES)
def test_shapes_lie_within_the_error_bound(lib, M):
    """A loop and a counter-clockwise lemniscate of exactly M rows in one launch, on the vehicle that is not the simulator's."""
    import gen_quad_traj_golden as GEN
    found = TS.find_case(M, DTS, RATIOS)
    assert found is not None, M
    dt, ratio, n = found
    lin_acc = 2.0 if M < 3000 else 0.5                    # powers of two: 2 * v_max / lin_acc is 2 * ratio exactly; fast where the rows are few
    cases = [dict(kind=kind, clockwise=cw, radius=radius, z=1.3, lin_acc=lin_acc, v_max=ratio * lin_acc, dt=dt, quad=GEN.OTHER_QUAD)
             for kind, cw, radius in (("loop", True, 4.0), ("lemniscate", False, 5.0))]
    assert all(TS.lengths(dt, c) == n for c in cases)
    if M in (33, 34):
        assert n[1] == 1
    bank = _Bank(lib, cases)
    try:
        assert bank.M == [M, M]
        for k, c in enumerate(cases):
            traj, u = bank.copy(k)
            _within_bound(c, traj, u, "M=%d dt=%g %s" % (M, dt, c["kind"]))
    finally:
        bank.close()


def test_the_row_past_the_cap_is_refused_and_no_bank_is_made(lib):
    dt, ratio, n = TS.find_case(TS.MAX_M + 1, [0.0013, 0.0007], [2.5 + 0.001 * i for i in range(40000)])
    case = dict(kind="loop", clockwise=True, radius=5.0, z=1.0, lin_acc=1.0, v_max=ratio, dt=dt, quad=TS.DEFAULT_QUAD)
    with pytest.raises(Exception, match="ADMPC_QUAD_TRAJ_MAX_M"):
        _Bank(lib, [case])


# -- independence -----------------------------------------------------------------------------------------------------------------------
def _mixed(K, seed):
    rng = np.random.RandomState(seed)
    out = []
    for k in range(K):
        v = float(np.round(rng.uniform(2.0, 12.0), 2))
        out.append(dict(kind=("loop", "lemniscate")[k % 2], clockwise=bool(rng.randint(2)), radius=float(np.round(rng.uniform(2.0, 6.0), 2)),
                        z=1.0, lin_acc=float(np.round(v / rng.uniform(2.3, 6.0), 3)), v_max=v, dt=0.02, quad=TS.DEFAULT_QUAD))
    return out


def test_a_trajectory_does_not_depend_on_its_place_or_its_neighbours(lib):
    """K = 1000 mixed specs, above the generator's 512 work-groups: one spec alone and at places 0, 500 and 999 gives the same bits; the
    neighbours of each place equal their own solo runs; two calls of the batch agree in every trajectory."""
    K = 1000
    cases = _mixed(K, 11)
    probe = dict(kind="lemniscate", clockwise=True, radius=5.0, z=1.0, lin_acc=1.75, v_max=7.0, dt=0.02, quad=TS.DEFAULT_QUAD)
    places = (0, 500, 999)
    for p in places:
        cases[p] = probe
    solo = _Bank(lib, [probe])
    first, second = _Bank(lib, cases), _Bank(lib, cases)
    try:
        want = solo.copy(0)
        assert first.M == second.M == [sum(TS.lengths(0.02, c)) for c in cases]
        for p in places:
            got = first.copy(p)
            _bits(got[0], want[0], "traj at place %d" % p); _bits(got[1], want[1], "u at place %d" % p)
        for k in (1, 499, 501, 998, 511, 512, 513):                  # the neighbours, and the first trajectories of the stride loop's second round
            alone = _Bank(lib, [cases[k]])
            try:
                got, own = first.copy(k), alone.copy(0)
                _bits(got[0], own[0], "traj %d against its solo run" % k); _bits(got[1], own[1], "u %d against its solo run" % k)
            finally:
                alone.close()
        for k in range(K):
            a, b = first.copy(k), second.copy(k)
            _bits(a[0], b[0], "traj %d of two calls" % k); _bits(a[1], b[1], "u %d of two calls" % k)
            assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and a[0][0, 0] == 0.0 and a[0][0, 1] == 0.0
    finally:
        solo.close(); first.close(); second.close()


# -- a generated bank is a bank ---------------------------------------------------------------------------------------------------------
KINDS, SPEEDS = ["loop", "lemniscate", "loop"], [2.0, 4.5, 7.0]


def _pair(B, drag=True):
    """A fleet on a generated bank and one on the uploaded copies of its trajectories."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    gen, up = QuadFleet(B, quad=SimQuad(drag=drag), n_nodes=10), QuadFleet(B, quad=SimQuad(drag=drag), n_nodes=10)
    gen.generate_trajectories(KINDS, SPEEDS)
    copies = [gen.trajectory(k) for k in range(3)]
    up.set_trajectories(copies)
    return gen, up, copies


STATE = ("x", "idx", "x_opt", "w_opt", "yref", "yref_e", "status", "tally", "counts", "cost", "iters")


def test_every_entry_that_takes_a_bank_takes_a_generated_one():
    import torch
    B = 12
    gen, up, copies = _pair(B)
    try:
        assert gen._traj is None and list(gen._M) == [c[0].shape[0] for c in copies] == list(up._M)
        for k, c in enumerate(copies):
            case = dict(kind=KINDS[k], clockwise=True, radius=5.0, z=1.0, lin_acc=0.25 * SPEEDS[k], v_max=SPEEDS[k], dt=gen.control_period,
                        quad=TS.DEFAULT_QUAD)
            _within_bound(case, c[0], c[1], "fleet trajectory %d" % k)
        M = int(gen._M[1])
        traj_of = np.array([0, 1, 2, 0, 1, 2, -1, 3, 1, 1, 0, 2], dtype=np.int32)
        idx = np.array([0, M // 2, int(gen._M[2]) - 1, int(gen._M[0]) - 3, M - 1, 17, 0, 0, M, -1, 1, 2], dtype=np.int32)
        for fl in (gen, up):
            fl.traj_of.copy_(torch.as_tensor(traj_of)); fl.idx.copy_(torch.as_tensor(idx))
            fl.ref_chunk()
        _bits(_host(gen.yref), _host(up.yref), "yref"); _bits(_host(gen.yref_e), _host(up.yref_e), "yref_e")
        assert np.isnan(_host(gen.yref)[6:10]).all() and np.isfinite(_host(gen.yref)[:6]).all()
        # reset from the device's rows against the host's, then 20 closed-loop steps from both banks
        traj_of, idx0 = np.arange(B) % 3, (np.arange(B) * 37) % 500
        gen.reset(traj_of, idx0); up.reset(traj_of, idx0)
        _bits(_host(gen.x), np.stack([copies[k][0][i] for k, i in zip(traj_of, idx0)]), "reset from the device bank")
        with pytest.raises(ValueError):
            gen.reset(np.full(B, 3), 0)
        gen.rollout(20); up.rollout(20)
        for k in STATE:
            _bits(_host(getattr(gen, k)), _host(getattr(up, k)), "after 20 steps: " + k)
        assert (_host(gen.counts)[:, 0] == 20).all() and np.isfinite(_host(gen.tally)).all()
        # a second generation replaces the bank
        gen.generate_trajectories("loop", 3.0, clockwise=False)
        assert list(gen._M) == [sum(TS.lengths(gen.control_period, {"v_max": 3.0, "lin_acc": 0.75}))]
        with pytest.raises(ValueError):
            gen.trajectory(1)
    finally:
        gen.close(); up.close()


def test_rows_entry_gives_rows_inputs_and_nan(lib):
    import torch
    cases = [TC.CASES[0], TC.CASES[6]]
    bank = _Bank(lib, cases)
    try:
        B = 700                                            # 700 * 17 doubles: more than one block
        rng = np.random.RandomState(3)
        traj_of = rng.randint(-1, 3, size=B).astype(np.int32)
        idx = rng.randint(-2, 603, size=B).astype(np.int32)
        x = torch.full((B, 13), 5.0, dtype=torch.float64, device="cuda:0"); u = torch.full((B, 4), 5.0, dtype=torch.float64, device="cuda:0")
        x_only = torch.full((B, 13), 5.0, dtype=torch.float64, device="cuda:0")
        to, ix = torch.as_tensor(traj_of).cuda(), torch.as_tensor(idx).cuda()
        p = lambda t: C.c_void_p(t.data_ptr())
        assert lib.admpc_quad_traj_rows_batch(bank.h, B, p(to), p(ix), p(x), p(u), None) == 0
        assert lib.admpc_quad_traj_rows_batch(bank.h, B, p(to), p(ix), p(x_only), None, None) == 0
        copies = [bank.copy(k) for k in range(2)]
        want_x, want_u = np.full((B, 13), np.nan), np.full((B, 4), np.nan)
        for b in range(B):
            if 0 <= traj_of[b] < 2 and 0 <= idx[b] < bank.M[traj_of[b]]:
                want_x[b], want_u[b] = copies[traj_of[b]][0][idx[b]], copies[traj_of[b]][1][idx[b]]
        ok = ~np.isnan(want_x[:, 0])
        assert 0 < ok.sum() < B
        for got, want in ((_host(x), want_x), (_host(u), want_u), (_host(x_only), want_x)):
            _bits(got[ok], want[ok], "rows in range"); assert np.isnan(got[~ok]).all()
        assert lib.admpc_quad_traj_rows_batch(bank.h, -1, p(to), p(ix), p(x), None, None) == -1
        assert lib.admpc_quad_traj_rows_batch(bank.h, 1, None, p(ix), p(x), None, None) == -1
        assert lib.admpc_quad_traj_rows_batch(bank.h, 0, None, None, None, None, None) == 0
        assert lib.admpc_quad_traj_bank_copy(bank.h, 2, None, None) == -1 and lib.admpc_quad_traj_bank_copy(bank.h, -1, None, None) == -1
    finally:
        bank.close()


def test_an_ensemble_fleet_generates_and_flies_one_step():
    import test_quad_ensemble_gpu as TE
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    fl = QuadEnsembleFleet(5, quad=SimQuad(drag=True), n_nodes=10, centroids=TE.BIN_CENT, feats=[7], learn=TE.BIN_LEARN)
    try:
        fl.generate_trajectories(["loop", "lemniscate"], 4.5)
        fl.reset([0, 1, 0, 1, 0], [0, 10, 100, 200, 300])
        want = [fl.trajectory(k)[0][i] for k, i in zip([0, 1, 0, 1, 0], [0, 10, 100, 200, 300])]
        _bits(_host(fl.x), np.stack(want), "the ensemble fleet's reset")
        fl.rollout(1)
        assert (_host(fl.counts)[:, 0] == 1).all() and np.isfinite(_host(fl.x)).all() and (_host(fl.idx) == [1, 11, 101, 201, 301]).all()
    finally:
        fl.close()


# -- the stream -------------------------------------------------------------------------------------------------------------------------
def test_generation_and_rollout_on_one_stream_need_no_synchronise_between():
    import torch
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    B, res = 8, []
    for sync in (False, True):
        fl = QuadFleet(B, quad=SimQuad(drag=True), n_nodes=10)
        s = torch.cuda.Stream()
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                fl.generate_trajectories(["lemniscate", "loop"], [7.0, 12.0])
                if sync:
                    torch.cuda.synchronize()
                fl.reset(np.arange(B) % 2, np.arange(B) * 40)
                fl.rollout(10)
            torch.cuda.synchronize()
            res.append({k: _host(getattr(fl, k)) for k in STATE})
        finally:
            fl.close()
    for k in STATE:
        _bits(res[0][k], res[1][k], "without and with a synchronise: " + k)
    assert np.isfinite(res[0]["x"]).all()


# -- the experiment ---------------------------------------------------------------------------------------------------------------------
def test_the_comparative_grid_flies_and_drag_costs_tracking_on_the_loop():
    """comparative_experiment.py's grid, loop and lemniscate x v_max {2, 4.5, 7, 9.5, 12}, radius 5, z 1, lin_acc 0.25 v: B = 10, T = 600,
    N = 10, one call, the nominal model against the perfect and against the drag simulator.  The orderings of the reference's own figure:
    on the loop the drag simulator tracks worse than the perfect one at every speed, and its error grows with v_max.  No status is looked
    at: the lemniscate's reference inputs leave [0, 1] at 9.5 and 12 m/s."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    speeds = [2.0, 4.5, 7.0, 9.5, 12.0]
    rmse = {}
    for drag in (False, True):
        fl = QuadFleet(10, quad=SimQuad(drag=drag), n_nodes=10)
        try:
            fl.generate_trajectories(["loop"] * 5 + ["lemniscate"] * 5, speeds * 2)
            assert list(fl._M) == [600] * 10
            fl.reset(np.arange(10), 0)
            fl.rollout(600)
            assert np.isfinite(_host(fl.tally)).all() and (_host(fl.counts)[:, 0] == 600).all()
            rmse[drag] = _host(fl.tracking_rmse())
        finally:
            fl.close()
    print("perfect", rmse[False], "drag", rmse[True])
    assert np.isfinite(rmse[False]).all() and np.isfinite(rmse[True]).all()
    assert (rmse[True][:5] > rmse[False][:5]).all()
    assert (np.diff(rmse[True][:5]) > 0).all()


# -- the refusals that need a device ------------------------------------------------------------------------------------------------------
def test_a_device_that_does_not_exist_and_a_bank_on_another_device(lib):
    import torch
    from ad_mpc_amd import _lib as L
    with pytest.raises(L.AdmpcError, match="-2"):
        _Bank(lib, [TC.CASES[0]], device=torch.cuda.device_count())
    with pytest.raises(L.AdmpcError, match="-2"):
        _Bank(lib, [TC.CASES[0]], device=-1)
    if torch.cuda.device_count() > 1:                      # the rollout's own refusal of a bank that lives elsewhere: needs a second GPU
        from ad_mpc_amd.quad_fleet import QuadFleet
        fl, other = QuadFleet(2, n_nodes=10), _Bank(lib, [TC.CASES[0]], device=1)
        try:
            fl.generate_trajectories("loop", 2.0)
            own, fl._bank = fl._bank, other.h
            with pytest.raises(L.AdmpcError, match="another device"):
                fl.rollout(1)
            fl._bank = own
        finally:
            fl.close(); other.close()
