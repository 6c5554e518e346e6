"""The search of the GP hyperparameters on the device (include/admpc_hyper.h; ad_mpc_amd/fleet.py: search_gp, learned_hyper).

A round is compared with its numpy restatement (tests/hyper_spec.py) candidate by candidate: the NLL at ten times the gap between the spec
solved in float64 and in numpy.longdouble plus the 64 n eps backward-error term of tests/test_learn_gpu.py, with the natural values
v = exp(theta) as the DEVICE evaluates them; the pick, the new centre, the steps and the counts bit for bit from the device's own NLLs.
The library returns the NLL of every candidate but the theta and v of the picked one only, so the device's exp is read through searches
whose slots are all fixed (one candidate, no points: it is picked and its v written): every theta a round can take, slot by slot."""
import ctypes as C

import numpy as np
import pytest

import hyper_spec as HS
import learn_spec as LS
import test_lane_gpu as TL
import test_learn_gpu as TG
import test_plant_gpu as TP

pytestmark = pytest.mark.gpu

_dev, _p, _bits, _learn, _obs = TL._dev, TL._p, TL._bits, TG._learn, TG._obs
BOX = dict(length_scale=(1e-2, 1e2), sigma_f=(1e-3, 1e2), noise=(1e-8, 1.0))         # the box of the searches (tests 4 to 6)
# The box of the rounds that are compared candidate by candidate (tests 1 and 2).  cond(K) <= 1 + n sigma_f / noise <= 1 + 100 n here,
# whatever the length scales.  The rounding of one NLL is of the order eps cond(K) times the size of its terms, with a small constant;
# inside this box that stays below the bound's second term, 64 n eps times that size (tests/hyper_spec.py evaluates both: the gap between
# float64 and longdouble is at most 0.12 of the second term for every candidate of every case below).  Past it the bound is its first
# term alone, ten times ONE draw of that rounding, the spec's; the device's is another draw of the same size, and two draws of one normal
# law differ by more than ten times the first in 6 % of the pairs, which no kernel can avoid over thousands of candidates (on the box
# above, noise down to 1e-8, the device's worst of 125 candidates on 8 points was 4.3 times over its bound, |dNLL| up to 130).
ROUND = dict(length_scale=(1e-2, 1e2), sigma_f=(0.25, 4.0), noise=(0.04, 1.0))
FIXED = dict(length_scale=(1.5, 1.5), sigma_f=(0.8, 0.8), noise=(0.05, 0.05))


def _params(gps, bounds, grid=5, rounds=1, shrink=0.5):
    from ad_mpc_amd.config import AdmpcGpSearchParams, search_boxes
    return AdmpcGpSearchParams(grid=grid, rounds=rounds, shrink=shrink, box=search_boxes(gps, bounds))


def _search(lib, obs, sp, stats, hyper, min_count=1, resume=1):
    """admpc_gp_search on uploaded statistics and state: (hyper [4,16], nll [4,4096], search_info [4,2]) afterwards."""
    import torch
    bins, hy = _dev(stats), _dev(np.asarray(hyper, dtype=np.float64))
    nll = torch.full((4, HS.SEARCH_MAX), 7.0, dtype=torch.float64, device="cuda:0")
    info = torch.full((4, 2), -9, dtype=torch.int32, device="cuda:0")
    rc = lib.admpc_gp_search(0, C.byref(obs), C.byref(sp), min_count, resume, _p(bins), _p(hy), _p(nll), _p(info), None)
    assert rc == 0, lib.admpc_last_error()
    torch.cuda.synchronize()
    _bits(bins.cpu().numpy(), np.asarray(stats, dtype=np.float64), "the statistics are read-only")
    return hy.cpu().numpy(), nll.cpu().numpy(), info.cpu().numpy()


def _device_exp(lib, values):
    """{theta: exp(theta) as the search's kernels evaluate it}, 20 values per call of a search with every slot fixed and no points."""
    vals = np.unique(np.asarray(values, dtype=np.float64))
    gps = [_learn(3, 8)] * 4
    obs, sp = _obs(gps), _params(gps, [dict(length_scale=(1.0, 1.0), sigma_f=(1.0, 1.0), noise=(1.0, 1.0))] * 4, grid=3)
    out = {}
    for i in range(0, len(vals), 20):
        chunk = np.zeros(20)
        m = len(vals[i:i + 20])
        chunk[:m] = vals[i:i + 20]
        hy = np.zeros((4, 16))
        hy[:, 0:5], hy[:, 15] = chunk.reshape(4, 5), np.inf
        got, nll, info = _search(lib, obs, sp, np.zeros((4, 32, 5)), hy)
        assert info.tolist() == [[0, 1]] * 4 and (nll[:, 0] == 0.0).all() and (got[:, 15] == 0.0).all()
        _bits(got[:, 0:10], hy[:, 0:10], "a fixed slot keeps its centre")
        out.update(zip(chunk[:m].tolist(), got[:, 10:15].reshape(-1)[:m].tolist()))
    want = np.exp(vals)
    ulp = np.abs(np.array([out[v] for v in vals.tolist()]) - want) / np.spacing(want)
    assert ulp.max() <= 4.0, "the device's exp is within 4 ulp of numpy's: %g" % ulp.max()
    return out


def _late(st, box, best):
    """A state late in a search: the centre at 0.925 of the box and steps of 0.15 of it, so that the upper candidates are clamped onto
    its upper end.  box = (free, loglo, loghi)."""
    free, loglo, loghi = box
    late = st.copy()
    late[0:5] = st[0:5] + np.where(free, 0.425 * (loghi - loglo), 0.0)
    late[5:10], late[15] = np.where(free, 0.15 * (loghi - loglo), 0.0), best
    late[10:15] = np.exp(late[0:5])
    return late


def _check_round(G, stats, box, grid, shrink, state, exps, got, what, exempt=False, min_count=1):
    """One regressor's round against the spec; got = (hyper [16], nll [4096], info [2]) of the device."""
    hy, dev_all, info = got
    nf = int(G.n_feat)
    free, loglo, loghi = HS.box_logs(list(box.lo), list(box.hi), nf)
    th = HS.thetas(state, free, loglo, loghi, grid)
    Cn = len(th)
    V = np.array([[exps[t] for t in row] for row in th.tolist()])               # the device's exp of the spec's theta
    n = len(LS.points(G, stats, min_count)[1])
    v64, size = HS.nll(G, stats, min_count, V)
    vld, _ = HS.nll(G, stats, min_count, V, np.longdouble)
    v64, size = v64.astype(np.float64), size.astype(np.float64)
    bound = HS.gaps(v64, size, vld, n)
    dev = dev_all[:Cn]
    assert (dev_all[Cn:] == 7.0).all(), what + ": nothing is written past the last candidate"
    agree = np.isfinite(v64) == np.isfinite(vld)                                # left out: float64 and longdouble disagree on the failure
    fin = agree & np.isfinite(v64)
    assert exempt or (~agree).sum() <= 0.05 * Cn, (what, int((~agree).sum()))
    assert np.isfinite(dev[fin]).all() and (dev[agree & ~fin] == np.inf).all(), what + ": finite where the spec is, +inf where it fails"
    err = np.abs(dev[fin] - v64[fin])
    worst = float((err / np.maximum(bound[fin], 1e-300)).max()) if fin.any() and n else 0.0
    print("%s: n = %d, C = %d, finite %d, left out %d, largest |dNLL| %.3g, largest over its bound %.3g"
          % (what, n, Cn, int(fin.sum()), int((~agree).sum()), err.max() if fin.any() else 0.0, worst))
    if not exempt:
        assert (err <= bound[fin]).all(), (what, worst)
    # the pick follows from the device's own values bit for bit
    new, picked, nfinite = HS.pick(state, th, V, dev, shrink)
    _bits(hy, new, what + ": centre, steps, natural values and best after the pick")
    assert info.tolist() == [picked, nfinite], (what, info, picked, nfinite)
    if picked >= 0 and not exempt and agree.all():
        at, forced = HS.forced(v64, bound)
        assert v64[picked] - v64[at] <= bound[picked] + bound[at], (what, picked, at)
        assert not forced or picked == at, (what, picked, at)
    return picked


CASES = {
    # name: (grid, [(regressor, bins filled, bounds)], exempt)
    "few": (5, [(_learn(3, 8), k, ROUND) for k in (0, 1, 2, 8)], False),
    "many": (5, [(_learn(3, 32), k, ROUND) for k in (31, 32)], False),
    "features": (5, [(_learn(3, 8), 8, FIXED), (_learn([3, 8], [8, 4], out=4), 20, ROUND), (_learn([4, 5, 7], [4, 2, 4], out=5), 20, ROUND),
                     (_learn(6, 32, out=4), 13, ROUND)], False),                                          # C = 1, 625, 3125, 125
    "grid3": (3, [(_learn(3, 8), 8, dict(ROUND, sigma_f=(0.7, 0.7))), (_learn([4, 5, 7], [4, 2, 4], out=5), 32, ROUND),
                  (_learn([3, 8], [8, 4], out=4), 11, dict(ROUND, length_scale=[(2.0, 2.0), (1.0, 1.0)]))], False),     # C = 9, 243, 9
    "grid7": (7, [(_learn(3, 8), 8, ROUND), (_learn([3, 8], [8, 4], out=4), 9, dict(ROUND, noise=(0.1, 0.1)))], False),   # C = 343, 343
    "nan": (5, [(_learn(3, 8), 8, ROUND), (_learn(3, 8), 8, ROUND)], False),
    "tiny noise": (5, [(_learn(3, 32, lo=[2.0], hi=[2.32]), 32, dict(length_scale=(0.5, 50.0), sigma_f=(0.1, 10.0), noise=(1e-16, 1e-2)))], True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_one_round_from_an_uploaded_state_matches_the_spec(name):
    """rounds = 1, resume = 1 from two uploaded states per case: the start of a search, and a state near the upper end of the box whose
    upper candidates are clamped onto each other (the lowest index of equal values is picked); `few` also from a state whose best
    cannot be improved.  C = 125 is odd: the second half of the last wave is idle."""
    lib = TL._lib()
    grid, regs, exempt = CASES[name]
    gps, bounds = [r[0] for r in regs], [r[2] for r in regs]
    obs, sp, shrink = _obs(gps), _params(gps, bounds, grid=grid, shrink=0.5), 0.5
    rng = np.random.default_rng(len(name))
    stats = np.zeros((4, 32, 5))
    for g, r in enumerate(regs):
        stats[g] = LS.hand_stats(obs.gp[g], rng, r[1])
    if name == "nan":
        stats[1, np.flatnonzero(stats[1, :, 0])[3], 4] = np.nan
    starts = [HS.init_state(list(sp.box[g].lo), list(sp.box[g].hi), int(obs.gp[g].n_feat), grid) for g in range(len(regs))]
    frees = [HS.box_logs(list(sp.box[g].lo), list(sp.box[g].hi), int(obs.gp[g].n_feat)) for g in range(len(regs))]
    runs = [("start", starts), ("late", [_late(s, f, np.inf) for s, f in zip(starts, frees)])]
    if name == "few":
        runs.append(("no better", [_late(s, f, -1e300) for s, f in zip(starts, frees)]))
    exps = _device_exp(lib, np.concatenate([HS.thetas(s, *f, grid).reshape(-1) for _, sts in runs for s, f in zip(sts, frees)]))
    for label, sts in runs:
        up = np.full((4, 16), 3.25)
        up[:len(regs)] = np.stack(sts)
        hy, nll, info = _search(lib, obs, sp, stats, up)
        _bits(hy[len(regs):], up[len(regs):], "the state past n_gp is not touched")
        assert (nll[len(regs):] == 7.0).all() and (info[len(regs):] == -9).all()
        for g in range(len(regs)):
            what = "%s, %s, regressor %d" % (name, label, g)
            picked = _check_round(obs.gp[g], stats[g], sp.box[g], grid, shrink, sts[g], exps, (hy[g], nll[g], info[g]), what, exempt)
            if name == "nan" and g == 1:
                assert picked == -1 and info[g].tolist() == [-1, 0] and (nll[g, :125] == np.inf).all()
                _bits(hy[g, 0:5], sts[g][0:5], "the centre is kept"); _bits(hy[g, 5:10], sts[g][5:10] * 0.5, "the step is shrunk")
            if label == "no better":
                assert picked == -1 and hy[g, 15] == -1e300
            if name == "features" and g == 0:
                assert info[g].tolist()[1] == 1 and (nll[g, 1:] == 7.0).all()                            # one candidate
        if name == "tiny noise" and label == "start":
            fin = np.isfinite(nll[0, :125])
            assert 0 < fin.sum() < 125 and any(fin[c] != fin[c + 1] for c in range(0, 124, 2))          # failing and finite halves share a wave


def test_rounds_one_at_a_time_equal_rounds_in_one_call():
    """R = 4, C = 125: resume = 0 with four rounds against resume = 0 with one round and three calls of resume = 1; and from an uploaded
    state, one call of four rounds against four calls of one.  The start of resume = 0 is the host's centre and step."""
    lib = TL._lib()
    gps = [_learn(3, 8), _learn(6, 32, out=4)]
    obs, rng = _obs(gps), np.random.default_rng(2)
    stats = np.zeros((4, 32, 5))
    stats[0], stats[1] = LS.hand_stats(obs.gp[0], rng, 8), LS.hand_stats(obs.gp[1], rng, 21)
    four, one = _params(gps, [ROUND, ROUND], rounds=4), _params(gps, [ROUND, ROUND], rounds=1)
    junk = np.full((4, 16), np.nan)
    whole = _search(lib, obs, four, stats, junk, resume=0)
    hy, _, info = _search(lib, obs, one, stats, junk, resume=0)
    st0 = HS.init_state(list(one.box[0].lo), list(one.box[0].hi), 1, 5)
    _bits(hy[0, 5:10], st0[5:10] * 0.5, "the step of the start, shrunk once")
    free, loglo, loghi = HS.box_logs(list(one.box[0].lo), list(one.box[0].hi), 1)
    assert info[0, 0] >= 0 and np.array_equal(hy[0, 0:5], HS.thetas(st0, free, loglo, loghi, 5)[info[0, 0]])      # the centre is a candidate of the start
    for _ in range(3):
        hy, _, info = _search(lib, obs, one, stats, hy, resume=1)
    _bits(hy, whole[0], "hyper: 1 + 3 calls against one"); _bits(info, whole[2], "search_info: 1 + 3 calls against one")
    assert np.isfinite(hy[:2, 15]).all() and np.isnan(hy[2:]).all()
    up = np.zeros((4, 16))
    up[0], up[1] = _late(st0, (free, loglo, loghi), np.inf), st0
    whole = _search(lib, obs, four, stats, up)
    hy = up
    for _ in range(4):
        hy, _, info = _search(lib, obs, one, stats, hy)
    _bits(hy, whole[0], "hyper from an uploaded state"); _bits(info, whole[2], "search_info from an uploaded state")


def _refit(lib, obs, stats, hyper, min_count):
    import torch
    from ad_mpc_amd.config import AdmpcGp
    n = int(obs.n_gp)
    bins, hy = _dev(stats), _dev(hyper)
    out = torch.full((4 * C.sizeof(AdmpcGp),), 0x5A, dtype=torch.uint8, device="cuda:0")
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda:0")
    assert lib.admpc_gp_refit(0, C.byref(obs), min_count, _p(bins), _p(hy), _p(out), _p(info), None) == 0, lib.admpc_last_error()
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    return [AdmpcGp.from_buffer_copy(raw, g * C.sizeof(AdmpcGp)) for g in range(n)], info.cpu().numpy()[:n]


def _fit_sets():
    """The two statistics sets of test_learn_gpu.test_the_fit_from_hand_made_statistics, its failing pivot included."""
    rng = np.random.default_rng(11)
    obs = _obs([_learn(3, 32, length_scale=0.6, noise=1e-4)] * 4)
    stats = np.zeros((4, 32, 5))
    stats[1] = LS.hand_stats(obs.gp[1], rng, 1); stats[2] = LS.hand_stats(obs.gp[2], rng, 8); stats[3] = LS.hand_stats(obs.gp[3], rng, 32)
    yield obs, stats, 1
    three = dict(length_scale=[2.0, 0.4, 3.0], noise=1e-4, sigma_f=0.7)
    obs = _obs([_learn([3, 5, 7], [4, 2, 4], out=4, **three)] * 3 + [_learn(3, 8, length_scale=2.0, noise=1e-6, count_noise=0.05)])
    stats = np.zeros((4, 32, 5))
    stats[0] = LS.hand_stats(obs.gp[0], rng, 20); stats[1] = LS.hand_stats(obs.gp[1], rng, 20); stats[2] = LS.hand_stats(obs.gp[2], rng, 32)
    stats[3] = LS.hand_stats(obs.gp[3], rng, 8)
    stats[1, np.flatnonzero(stats[1, :, 0] >= 4)[2], 2] = np.nan
    yield obs, stats, 4


def test_the_refit_at_the_given_values_is_the_fit_byte_for_byte():
    lib = TL._lib()
    infos = []
    for obs, stats, min_count in _fit_sets():
        hy = np.zeros((4, 16))
        for g in range(4):
            G = obs.gp[g]
            hy[g, 10:15] = [G.length[d] if d < G.n_feat else 1.0 for d in range(3)] + [G.sigma_f, G.noise]
            hy[g, 0:5], hy[g, 5:10] = np.log(hy[g, 10:15]), 0.125
        want, winfo = TG._fit(lib, obs, stats, min_count)
        got, ginfo = _refit(lib, obs, stats, hy, min_count)
        assert ginfo.tolist() == winfo.tolist()
        for g in range(4):
            assert bytes(got[g]) == bytes(want[g]), "regressor %d: the record of the re-fit is the fit's" % g
        infos.append(winfo.tolist())
        hy[1, 15], hy[3, 15] = np.inf, np.nan                                       # no optimum: the empty GP under the given head
        got, ginfo = _refit(lib, obs, stats, hy, min_count)
        assert ginfo.tolist() == [winfo[0], HS.NO_OPTIMUM, winfo[2], HS.NO_OPTIMUM] and bytes(got[0]) == bytes(want[0]) and bytes(got[2]) == bytes(want[2])
        for g in (1, 3):
            e = got[g]
            assert (e.n_points, e.ymean, e.n_feat, e.out) == (0, 0.0, want[g].n_feat, want[g].out) and LS.install_ok(e)
            assert not any(e.alpha[i] for i in range(32)) and not any(e.Z[d][i] for d in range(3) for i in range(32))
    assert infos[0] == [0, 1, 8, 32] and infos[1][1] == -3 and infos[1][2] > 20        # the cases the fit's own test has


INSTALL_LEARN = [_learn(3, 8, length_scale=2.0), _learn([3, 6], [4, 4], out=4, length_scale=[4.0, 0.5], noise=1e-4)]


def _install_stats(fc, seed):
    rng = np.random.default_rng(seed)
    stats = np.zeros((4, 32, 5))
    for g in range(2):
        stats[g] = LS.hand_stats(fc._obs.gp[g], rng, 8 if g == 0 else 12)
    return stats


def test_a_searched_gp_solves_as_a_handle_created_with_it():
    """N = 20, B = 65: search_gp on hand-made bins installs what a fresh handle created from learned_gps() solves with."""
    from ad_mpc_amd.config import AdmpcGp, set_gp
    from ad_mpc_amd.engine import BatchSolver
    from ad_mpc_amd.scenarios import random_scenarios
    N, B = 20, 65
    fc = TL._controller(N, B, learn=INSTALL_LEARN, blend_min=3.0, blend_max=5.0)
    fresh = None
    try:
        s = random_scenarios(B, N=N, Ts=TL.T_HORIZON / N, seed=N, blend=(3.0, 5.0))
        base = TG._solve(fc._eng, s)
        assert [h["nll"] for h in fc.learned_hyper()] == [np.inf] * 2 and fc.learned_hyper()[1]["length_scale"] == [4.0, 0.5]
        fc.bins.copy_(_dev(_install_stats(fc, N)))
        info, installed, hyper = fc.search_gp(rounds=4, bounds=[BOX, BOX])
        got = TG._solve(fc._eng, s)
        assert info.cpu().tolist() == [8, 12] and installed.cpu().tolist() == [1, 1] and tuple(hyper.shape) == (2, 16)
        hy = hyper.cpu().numpy()
        gps, found = fc.learned_gps(), fc.learned_hyper()
        raw = fc._gp_dev.cpu().numpy().tobytes()
        for g in range(2):
            rec = AdmpcGp.from_buffer_copy(raw, g * C.sizeof(AdmpcGp))
            nf = rec.n_feat
            assert list(gps[g]["length_scale"]) == found[g]["length_scale"] == hy[g, 10:10 + nf].tolist() and gps[g]["sigma_f"] == hy[g, 13] == rec.sigma_f
            assert (found[g]["sigma_f"], found[g]["noise"], found[g]["nll"]) == (hy[g, 13], hy[g, 14], hy[g, 15]) and np.isfinite(hy[g, 15])
            assert [1.0 / l ** 2 for l in gps[g]["length_scale"]] == [rec.inv_l2[d] for d in range(nf)]      # set_gp forms what was installed
        fresh = BatchSolver(set_gp(fc._eng.cfg.copy(), gps), device=0)
        want = TG._solve(fresh, s)
        for a, b, what in zip(got, want, ("x", "u", "cost", "status", "iters")):
            _bits(a, b, "%s of the handle after search_gp against the fresh one" % what)
        assert np.nanmax(np.abs(got[1] - base[1])) > 1e-6                          # not the placeholder
        info, installed = fc.fit_gp()                                              # a fit_gp afterwards: the given values again
        assert [g["length_scale"] for g in fc.learned_gps()] == [2.0, [4.0, 0.5]] and info.cpu().tolist() == [8, 12]
    finally:
        fc.close()
        if fresh is not None:
            fresh.close()


def test_a_captured_search_follows_the_bins_at_replay():
    """search_gp captured after one eager run; other bins, a replay: hyper, the fitted records and the install's flags equal those of
    an eager controller on the same bins bit for bit."""
    import torch
    fcs = [TL._controller(20, 4, learn=INSTALL_LEARN, blend_min=3.0, blend_max=5.0) for _ in range(2)]
    eager, graphed = fcs
    try:
        first, second = _install_stats(graphed, 1), _install_stats(graphed, 2)
        kw = dict(rounds=3, bounds=[BOX, BOX])
        graphed.bins.copy_(_dev(first))
        graphed.search_gp(**kw)                                                    # every kernel has run once before the capture
        torch.cuda.synchronize()
        before = graphed.hyper.cpu().numpy().copy()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed.search_gp(**kw)
        graphed.bins.copy_(_dev(second))
        g.replay()
        eager.bins.copy_(_dev(second))
        info, installed, _ = eager.search_gp(**kw)
        torch.cuda.synchronize()
        for k in ("hyper", "_gp_dev", "installed", "fit_info", "search_info"):
            _bits(getattr(graphed, k).cpu().numpy(), getattr(eager, k).cpu().numpy(), k + " after the replay")
        assert installed.cpu().tolist() == [1, 1] and info.cpu().tolist() == [8, 12]
        assert not np.array_equal(before[:2, 0:5], graphed.hyper.cpu().numpy()[:2, 0:5])       # the replay read the new bins
    finally:
        for fc in fcs:
            fc.close()


def test_the_search_mends_a_wrong_length_scale_on_the_device(gpu_engine_factory, oracle):
    """The experiment of test_learn_gpu.py with the length scale given as 0.3 (the truth has 2.0), B = 200: the ratio
    RMS(y_after) / RMS(y_before) after fit_gp, and after search_gp on the same bins.  searched < 0.5 * given; the device's final NLL is
    within the bound of test 1 of the spec's at the device's own values; where the gap rule forced every round's pick, the centre is
    the spec's bit for bit and the ratio the spec's to 1e-6."""
    import torch
    from ad_mpc_amd.config import search_boxes
    exp = LS.experiment(oracle)
    learn = [dict(LS.EXP_LEARN[0], length_scale=0.3)]
    fc = TL._controller(20, LS.EXP_B, learn=learn)
    truth = TG._truth(fc, gpu_engine_factory)
    try:
        fc.set_plant(dt=LS.EXP_DT, model=truth)

        def observed(name):
            e = exp[name]
            fc.ack.copy_(_dev(e["ack"], torch.float32)); fc.mode.copy_(_dev(e["mode"], torch.int32))
            ps = TP._poses(np.ascontiguousarray(e["X"].T))
            fc.observe_latch(*ps); fc.plant_step(*ps); fc.observe(*ps)
            S = fc.samples.cpu().numpy()
            assert (S[:, 9] == 1.0).all()
            return float(np.sqrt(np.mean(S[:, 6:9] ** 2)))

        rms0 = observed("before")
        bins = fc.bins.clone()
        info, installed = fc.fit_gp()
        fc.set_observer(learned=True)
        given = observed("after") / rms0
        fc.bins.copy_(bins)                                                        # the statistics of the first set alone
        info, installed, hyper = fc.search_gp(bounds=[BOX])
        searched = observed("after") / rms0
        assert info.cpu().tolist() == [8] and installed.cpu().tolist() == [1]
        hy, stats = hyper.cpu().numpy()[0], bins.cpu().numpy()[0]
        G, box = fc._obs.gp[0], search_boxes(learn, [BOX])[0]
        v64, size = HS.nll(G, stats, 1, hy[10:15])
        vld, _ = HS.nll(G, stats, 1, hy[10:15], np.longdouble)
        bound = HS.gaps(v64.astype(np.float64), size.astype(np.float64), vld, 8)[0]
        # the spec's own search on the spec's statistics, and whether the gap rule forces every pick of it
        free, loglo, loghi = HS.box_logs(list(box.lo), list(box.hi), 1)
        st, every = HS.init_state(list(box.lo), list(box.hi), 1, 5), True
        for _ in range(10):
            th = HS.thetas(st, free, loglo, loghi, 5)
            V = HS.natural(th)
            a64, asize = HS.nll(G, exp["bins"][0], 1, V)
            ald, _ = HS.nll(G, exp["bins"][0], 1, V, np.longdouble)
            every = every and HS.forced(a64.astype(np.float64), HS.gaps(a64.astype(np.float64), asize.astype(np.float64), ald, 8))[1]
            st, _, _ = HS.pick(st, th, V, a64.astype(np.float64), 0.5)
        print("ratio on the device: given %.6g, searched %.6g (length %.6g, sigma_f %.6g, noise %.6g); NLL %.12g, the spec's there %.12g (bound %.3g); "
              "every pick forced: %s" % (given, searched, hy[10], hy[13], hy[14], hy[15], v64[0], bound, every))
        assert searched < 0.5 * given
        assert abs(hy[15] - float(v64[0])) <= bound
        if every:
            _bits(hy[0:10], st[0:10], "the centre and the steps of the spec's search")
            found = HS.with_hyper(G, st[10:15])
            want = HS.experiment_ratio(oracle, exp, found, LS.fit(found, exp["bins"][0]))
            print("ratio by the spec %.9g" % want)
            assert abs(searched - want) <= 1e-6 * want
    finally:
        fc.close(); truth.close()


def test_argument_errors():
    from ad_mpc_amd._lib import AdmpcError
    plain, fc = TL._controller(20, 4), TL._controller(20, 4, learn=[_learn(3, 8, length_scale=0.7, sigma_f=1.3, noise=1e-5), _learn([4, 5, 7], [4, 2, 4], out=5)])
    try:
        for call in (lambda: plain.search_gp(), lambda: plain.learned_hyper()):
            with pytest.raises(ValueError, match="does not learn"):
                call()
        for kw, words in ((dict(grid=4), "grid must be"), (dict(grid=7), "16807 candidates"), (dict(shrink=1.0), "shrink must be"),
                          (dict(rounds=0), "rounds must be"), (dict(min_count=0), "min_count must be"), (dict(grid=6, shrink=2.0), "grid must be")):
            with pytest.raises(AdmpcError, match=words):
                fc.search_gp(**kw)
        for bounds in ([dict(sigma_f=(2.0, 1.0)), {}], [{}, dict(length_scale=(0.0, 1.0))], [{}]):
            with pytest.raises(ValueError, match="bound"):
                fc.search_gp(bounds=bounds)
        found = fc.learned_hyper()                                                 # no search yet: the given values
        assert found[0] == dict(length_scale=[0.7], sigma_f=1.3, noise=1e-5, nll=np.inf) and found[1]["length_scale"] == [2.0] * 3
        assert not fc.hyper.cpu().numpy().any() and [len(g["alpha"]) for g in fc.learned_gps()] == [0, 0]
        fc.search_gp(grid=7, rounds=1, bounds=[{}, dict(noise=(1e-4, 1e-4))])      # 7^3 and 7^4 candidates pass
        assert np.isfinite(fc.learned_hyper()[0]["nll"])
    finally:
        plain.close(); fc.close()
