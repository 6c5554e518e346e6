"""The polynomial trajectory generator on the device (include/admpc_quad_poly_traj.h; QuadFleet.generate_polynomial_trajectories and
generate_random_trajectories).

Accuracy: the device against the longdouble spec (tests/quad_poly_traj_spec.py, which tests/test_quad_poly_traj_cpu.py pins to the
reference's own trajectories), one forward error bound per column group -- position, quaternion, velocity, rate, input -- derived in
DESIGN.md (quad_poly_traj_spec.error_bound(case, "kernel")), never from the device's output; the reference's stored rows at that bound
plus the bound of the reference's own route to the coefficients plus the spec's 1e-12.  Every plant here has g = 3.7: gravity in the rule
is the literal 9.81.  Independence, "a polynomial bank is a bank", the stream and the experiment's ordering are compared bit for bit or
by the ordering of the reference's own figure.

Measured on one MI355X, the worst error / bound over the golden cases and the shapes: position 0.0091, velocity 0.0137, quaternion 1.0e-5,
rate 1.6e-6, input 2.6e-7; the reference's stored rows at 1.2e-5 of their tolerance."""
import ctypes as C
import json

import numpy as np
import pytest

import gen_quad_poly_traj_golden as GEN
import gen_quad_traj_golden as GJ
import quad_poly_traj_spec as PS
import test_quad_poly_traj_cpu as TC
from test_quad_traj_gpu import STATE, _bits, _host, _plant

pytestmark = pytest.mark.gpu

DBL = C.POINTER(C.c_double)
# (n_key, s): the smallest (every gradient one-sided), many segments of one row, a junction on the wave's edge, M = 257, a junction on the
# first row of tile 1, M = 256, M = 257 again with four segments, the reference's key count, and just under the cap (M = 15 501)
SHAPES = [(3, 1), (32, 1), (3, 32), (3, 128), (3, 256), (4, 85), (5, 64), (10, 75), (32, 500)]


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


class _Bank:
    """A polynomial bank of the library for cases that share dt, the key count and the vehicle."""

    def __init__(self, lib, cases, stream=None, device=0):
        from ad_mpc_amd import _lib as L
        self.lib, self.K = lib, len(cases)
        keys = np.ascontiguousarray(np.stack([np.asarray(c["keys"], dtype=np.float64) for c in cases]))
        speed = np.ascontiguousarray([c["speed"] for c in cases], dtype=np.float64)
        plant = _plant(cases[0]["quad"])
        self.h = C.c_void_p(0)
        L.check(lib.admpc_quad_poly_traj_bank_generate(device, self.K, keys.shape[1], keys.ctypes.data_as(DBL), speed.ctypes.data_as(DBL),
                                                       C.byref(plant), cases[0]["dt"], stream, C.byref(self.h)))
        M = (C.c_int32 * self.K)()
        K, rows = C.c_int(0), C.c_int64(0)
        L.check(lib.admpc_quad_traj_bank_info(self.h, C.byref(K), C.byref(rows), M))
        self.M = list(M)
        assert K.value == self.K and rows.value == sum(self.M)

    def copy(self, k):
        from ad_mpc_amd import _lib as L
        traj, u = np.full((self.M[k], 13), 7.0), np.full((self.M[k], 4), 7.0)
        L.check(self.lib.admpc_quad_traj_bank_copy(self.h, k, traj.ctypes.data_as(DBL), u.ctypes.data_as(DBL)))
        return traj, u

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.lib.admpc_quad_traj_bank_destroy(self.h)


RATIO_LOG = {}


def _within_bound(case, traj, u, what):
    """The device's rows against the longdouble spec, group by group; the ratios error / bound are printed and kept."""
    want_t, want_u = PS.generate(case, ft=np.longdouble, route="weights")
    assert traj.shape == want_t.shape and u.shape == want_u.shape, (what, traj.shape, want_t.shape)
    assert np.isfinite(traj).all() and np.isfinite(u).all(), what
    err, bound = PS.group_errors(traj, u, want_t, want_u), PS.error_bound(case, "kernel")
    for k in err:
        RATIO_LOG[k] = max(RATIO_LOG.get(k, 0.0), err[k] / bound[k])
    print(what, " ".join("%s %.3g/%.3g=%.2g" % (k, err[k], bound[k], err[k] / bound[k]) for k in err))
    for k in err:
        assert err[k] <= bound[k], (what, k, err[k], bound[k])
    return bound


# -- accuracy ---------------------------------------------------------------------------------------------------------------------------
def test_golden_cases_lie_within_the_error_bound(lib):
    """Every golden case, one launch per (dt, key count, vehicle); also the reference's own stored rows at the bound plus the route bound
    plus 1e-12.  Measured on one MI355X, the worst error / bound over the 23 cases: position 0.0091, velocity 0.0137, quaternion 2.1e-6,
    rate 3.5e-7, input 1.5e-8; against the reference's rows 1.2e-5 of the tolerance."""
    groups = {}
    for i, c in enumerate(TC.CASES):
        groups.setdefault((c["dt"], len(c["keys"]), json.dumps(c["quad"], sort_keys=True)), []).append(i)
    worst_ref = 0.0
    for ids in groups.values():
        bank = _Bank(lib, [TC.CASES[i] for i in ids])
        try:
            for k, i in enumerate(ids):
                c, g = TC.CASES[i], TC.GOLD["cases"][i]
                assert bank.M[k] == g["M"]
                traj, u = bank.copy(k)
                bound = _within_bound(c, traj, u, TC.IDS[i])
                route = PS.route_bound(c)
                ref = GEN.unpack(g["values"], (-1, 17))
                got = np.concatenate([traj, u], axis=1)[g["rows"]]
                for name, cols in list(PS.GROUPS.items()) + [("input", slice(13, 17))]:
                    tol = bound[name] + route[name] + 1e-12 * np.maximum(1.0, np.abs(ref[:, cols]))
                    worst_ref = max(worst_ref, float(np.max(np.abs(got[:, cols] - ref[:, cols]) / tol)))
                    assert (np.abs(got[:, cols] - ref[:, cols]) <= tol).all(), (TC.IDS[i], name)
        finally:
            bank.close()
    print("worst ratios", RATIO_LOG, "against the reference's rows", worst_ref)


@pytest.mark.parametrize("n_key,s", SHAPES)
def test_shapes_lie_within_the_error_bound(lib, n_key, s):
    """Given keyframes with n_key keys and exactly s rows per segment, on the vehicle that is not the simulator's: the speed is
    av_dist / (s dt), and the lengths entry must return s."""
    dt = 0.25 if s == 1 else 0.02                         # one row per segment: a period long enough for the vehicle to cover a segment in
    keys = GEN.given_keyframes(n_key, np.random.RandomState(1000 * n_key + s))
    speed = PS.speed_for(keys, s, dt)
    M = (n_key - 1) * s + 1
    assert TC._lib_lengths(lib, dt, keys, speed) == (0, s, M) and PS.lengths(dt, keys, speed) == (s, M)
    case = dict(keys=keys, speed=speed, dt=dt, quad=GJ.OTHER_QUAD)
    other = dict(case, keys=keys[::-1].copy())            # the same distances: the same s
    bank = _Bank(lib, [case, other])
    try:
        assert bank.M == [M, M]
        for k, c in enumerate((case, other)):
            traj, u = bank.copy(k)
            _within_bound(c, traj, u, "n_key=%d s=%d M=%d dt=%g %d" % (n_key, s, M, dt, k))
    finally:
        bank.close()
    print("worst ratios so far", RATIO_LOG)


def test_the_row_past_the_cap_is_refused_and_no_bank_is_made(lib):
    keys = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0], [3.0, 0.0, 1.0]])
    assert TC._lib_lengths(lib, 0.02, keys, PS.speed_for(keys, 5461, 0.02)) == (0, 5461, PS.MAX_M)
    with pytest.raises(Exception, match="ADMPC_QUAD_TRAJ_MAX_M"):
        _Bank(lib, [dict(keys=keys, speed=PS.speed_for(keys, 5462, 0.02), dt=0.02, quad=PS.TS.DEFAULT_QUAD)])


# -- independence -----------------------------------------------------------------------------------------------------------------------
def _mixed(K, seed):
    from ad_mpc_amd.quad_keyframes import random_keyframes
    rng = np.random.RandomState(seed)
    return [dict(keys=random_keyframes(int(rng.randint(0, 10000))), speed=float(np.round(rng.uniform(2.0, 8.0), 2)), dt=0.02, quad=PS.TS.DEFAULT_QUAD)
            for _ in range(K)]


def test_a_trajectory_does_not_depend_on_its_place_or_its_neighbours(lib):
    """K = 1000 mixed seeds and speeds, above the generator's 512 work-groups: one trajectory alone and at places 0, 500 and 999 gives the
    same bits; the neighbours of each place equal their own solo runs; two calls of the batch agree in every trajectory."""
    from ad_mpc_amd.quad_keyframes import random_keyframes
    K = 1000
    cases = _mixed(K, 11)
    probe = dict(keys=random_keyframes(303), speed=3.5, dt=0.02, quad=PS.TS.DEFAULT_QUAD)
    places = (0, 500, 999)
    for p in places:
        cases[p] = probe
    solo = _Bank(lib, [probe])
    first, second = _Bank(lib, cases), _Bank(lib, cases)
    try:
        want = solo.copy(0)
        assert first.M == second.M == [PS.lengths(0.02, c["keys"], c["speed"])[1] for c in cases]
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


# -- a polynomial bank is a bank ----------------------------------------------------------------------------------------------------------
SEEDS, SPEEDS = [1, 2, 303], [2.0, 3.5, 3.0]


def _pair(B, drag=True):
    """A fleet on a polynomial bank and one on the uploaded copies of its trajectories."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    gen, up = QuadFleet(B, quad=SimQuad(drag=drag), n_nodes=10), QuadFleet(B, quad=SimQuad(drag=drag), n_nodes=10)
    gen.generate_random_trajectories(SEEDS, SPEEDS)
    copies = [gen.trajectory(k) for k in range(3)]
    up.set_trajectories(copies)
    return gen, up, copies


def test_every_entry_that_takes_a_bank_takes_a_polynomial_one():
    import torch
    from ad_mpc_amd.quad_keyframes import random_keyframes, straight_keyframes
    B = 12
    gen, up, copies = _pair(B)
    try:
        assert gen._traj is None and list(gen._M) == [c[0].shape[0] for c in copies] == list(up._M)
        for k, c in enumerate(copies):
            case = dict(keys=random_keyframes(SEEDS[k]), speed=SPEEDS[k], dt=gen.control_period, quad=PS.TS.DEFAULT_QUAD)
            assert c[0].shape[0] == PS.lengths(gen.control_period, case["keys"], SPEEDS[k])[1]
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
        traj_of, idx0 = np.arange(B) % 3, (np.arange(B) * 29) % 400
        gen.reset(traj_of, idx0); up.reset(traj_of, idx0)
        _bits(_host(gen.x), np.stack([copies[k][0][i] for k, i in zip(traj_of, idx0)]), "reset from the device bank")
        with pytest.raises(ValueError):
            gen.reset(np.full(B, 3), 0)
        gen.rollout(20); up.rollout(20)
        for k in STATE:
            _bits(_host(getattr(gen, k)), _host(getattr(up, k)), "after 20 steps: " + k)
        assert (_host(gen.counts)[:, 0] == 20).all() and np.isfinite(_host(gen.tally)).all()
        # given keyframes, one set for two speeds: the straight line of the reference; it replaces the bank
        gen.generate_polynomial_trajectories(straight_keyframes(), [3.0, 1.5])
        assert list(gen._M) == [PS.lengths(gen.control_period, straight_keyframes(), v)[1] for v in (3.0, 1.5)]
        t, u = gen.trajectory(0)
        _within_bound(dict(keys=straight_keyframes(), speed=3.0, dt=gen.control_period, quad=PS.TS.DEFAULT_QUAD), t, u, "the straight line")
        assert (t[:, 0] == 0.0).all() and t[0, 1] == 0.0 and abs(t[-1, 1] - 6.0) < 1e-12 and (np.abs(t[:, 2] - 1.0) < 1e-12).all()
        with pytest.raises(ValueError):
            gen.trajectory(2)
    finally:
        gen.close(); up.close()


def test_an_ensemble_fleet_generates_and_flies_one_step():
    import test_quad_ensemble_gpu as TE
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    fl = QuadEnsembleFleet(5, quad=SimQuad(drag=True), n_nodes=10, centroids=TE.BIN_CENT, feats=[7], learn=TE.BIN_LEARN)
    try:
        fl.generate_random_trajectories([1, 2], 3.5)
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
                fl.generate_random_trajectories([303, 7], [3.5, 2.7])
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
def test_the_random_trajectory_of_the_comparative_experiment_flies_and_drag_costs_tracking():
    """comparative_experiment.py's first trajectory type, {"random": 1}, at its average speeds 2.0, 2.7, 3.0, 3.2, 3.5: B = 5, N = 10,
    T = M - 1 of the shortest trajectory, one call, the nominal model against the perfect and against the drag simulator.  The ordering
    of the reference's own figure: the drag simulator tracks worse than the perfect one at every speed.  No status is looked at: the
    reference inputs may leave [0, 1]."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_fleet import QuadFleet
    speeds = [2.0, 2.7, 3.0, 3.2, 3.5]
    rmse = {}
    for drag in (False, True):
        fl = QuadFleet(5, quad=SimQuad(drag=drag), n_nodes=10)
        try:
            fl.generate_random_trajectories([1] * 5, speeds)
            T = int(fl._M.min()) - 1
            assert (np.diff(fl._M) < 0).all() and T == PS.lengths(fl.control_period, TC.KEYFRAMES[1]["adjusted"], 3.5)[1] - 1
            fl.reset(np.arange(5), 0)
            fl.rollout(T)
            assert np.isfinite(_host(fl.tally)).all() and (_host(fl.counts)[:, 0] == T).all()
            rmse[drag] = _host(fl.tracking_rmse())
        finally:
            fl.close()
    print("T", T, "perfect", rmse[False], "drag", rmse[True])
    assert np.isfinite(rmse[False]).all() and np.isfinite(rmse[True]).all()
    assert (rmse[True] > rmse[False]).all()


# -- the refusal that needs a device --------------------------------------------------------------------------------------------------------
def test_a_device_that_does_not_exist(lib):
    import torch
    from ad_mpc_amd import _lib as L
    for device in (torch.cuda.device_count(), -1):
        with pytest.raises(L.AdmpcError, match="-2"):
            _Bank(lib, [TC.CASES[0]], device=device)
