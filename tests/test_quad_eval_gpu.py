"""The evaluation of the learned GPs on a flight log on the device (include/admpc_quad_eval.h; csrc/admpc_quad_eval.hip;
QuadEnsembleFleet.fit_gp / search_gp (factor=True), factor_gp, evaluate_log, evaluation) against the numpy spec,
tests/quad_eval_spec.py, which tests/test_quad_eval_cpu.py pins to the reference's predict and select_gp.

The factor: n, Z, alpha, ymean and info are the fit's and the re-fit's BITS; W is held to |W L - I| <= 64 u cond_2(K) against the spec's L.
The evaluation: routes, counts and info are exact; a record's mean and std^2 are held to the bounds of tests/test_quad_eval_cpu.py's
docstring against the spec evaluated in numpy.longdouble FROM THE DEVICE'S OWN FACTOR (both sides read the same alpha and W, so the
mean's bound is the dot product's alone); a sum is held within (M + 1) u sum |terms| -- its order is free, and a term is rounded once
when it is formed -- plus the summed bounds of its records; the 3-std count lies between the spec's counts without and with the records
whose margin ||r| - 3 std| is below their own bound."""
import ctypes as C

import numpy as np
import pytest

import learn_spec as LS
import quad_clusters_spec as CS
import quad_eval_spec as EV
import test_quad_fleet_gpu as TQ

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _stream = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._stream
SIZES = (1, 63, 64, 65, 256, 257, CS.BLOCKS_MAX * 256 + 1)         # the last is past the grid, into the stride loop
SHAPES = ((1, 1, 1), (3, 3, 2), (8, 3, 3), (3, 1, 3), (8, 3, 1), (3, 3, 1), (3, 3, 2))          # (K, n_gp, n_feat) of the size at the same place
FILLS = (32, 31, 1, 0)                                             # the points of regressor (c, g): FILLS[(c + g) % 4]
PAD = 8
U, LD = EV.U, np.longdouble
EINVAL = -1


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ensemble(K, n_gp, n_feat, far=True, **kw):
    """A fleet that learns K clusters of n_gp regressors on n_feat features, boxes and given values differing per cluster; with `far` the
    last of three or more centroids lies where no record is."""
    from ad_mpc_amd.quad_config import SimQuad
    from ad_mpc_amd.quad_ensemble_fleet import QuadEnsembleFleet
    feats = [7, 8, 9][:n_feat]
    learn = [[dict(feat=feats, out=7 + g, lo=[-9.0 + 0.5 * c] * n_feat, hi=[9.0 + 0.5 * c] * n_feat, bins=[32] + [1] * (n_feat - 1),
                   length_scale=[1.0 + 0.25 * c + 0.1 * g] * n_feat, sigma_f=0.5 + 0.1 * g, noise=1e-4 * (c + 1), count_noise=1e-2 if g < 2 else 0.0) for g in range(n_gp)]
             for c in range(K)]
    cent = (np.linspace(-5.0, 5.0, K).reshape(K, 1) * np.ones((1, n_feat)) + 0.1 * np.arange(n_feat)) if K > 1 else np.zeros((1, n_feat))
    if far and K >= 3:
        cent[-1] = 100.0
    return QuadEnsembleFleet(4, quad=SimQuad(drag=True), n_nodes=10, centroids=cent, feats=feats, learn=learn, **kw), feats, cent


def _stats(fl, seed, fills=FILLS):
    rng = np.random.default_rng(seed)
    stats = np.zeros((fl.K, 3, 32, 5))
    for c in range(fl.K):
        for g in range(fl.n_learn):
            stats[c, g] = LS.hand_stats(fl._obs[c].gp[g], rng, fills[(c + g) % len(fills)])
    return stats


class Dev:
    """The two entries over device scratch of the test's own, for an ensemble fleet and up to M records."""

    def __init__(self, fl, M):
        import torch
        self.fl, self.L, self.K = fl, fl.lib, fl.K
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda:0")
        self.rec, self.per = z(M + PAD, EV.REC), z(M + PAD, 3, 2)
        self.factor, self.finfo = torch.full((fl.K, 3, EV.FACTOR), -3.0, dtype=torch.float64, device="cuda:0"), z(fl.K, 3, dtype=torch.int32)
        self.partial, self.stats, self.info = z(CS.BLOCKS_MAX, fl.K * 24), z(fl.K, 3, 8), z(4, dtype=torch.int32)
        self.bins, self.drag = z(fl.K, 3, 32, 5), z(3)

    def make_factor(self, stats, hyper=None, min_count=1):
        self.bins.copy_(_dev(stats))
        rc = self.L.admpc_quad_ensemble_factor(self.fl._ens, min_count, _p(self.bins), _p(hyper), _p(self.factor), _p(self.finfo), _stream())
        assert rc == 0, self.L.admpc_last_error()
        return _host(self.factor).copy(), _host(self.finfo).copy()

    def load(self, S):
        full = np.full((self.rec.shape[0], EV.REC), -7.5)
        full[:S.shape[0]] = S
        full[S.shape[0]:, 13] = 1.0                                  # a pad row would take part if a kernel ran past M
        self.rec.copy_(_dev(full))
        self.per.fill_(-7.5)
        return full

    def evaluate(self, M, take_pruned=0, drag=None, per=True):
        if drag is not None:
            self.drag.copy_(_dev(np.asarray(drag, dtype=np.float64)))
        rc = self.L.admpc_quad_ensemble_evaluate(self.fl._ens, M, _p(self.rec), take_pruned, _p(self.factor), _p(self.drag) if drag is not None else None,
                                                 _p(self.per) if per else None, _p(self.partial), _p(self.stats), _p(self.info), _stream())
        assert rc == 0, self.L.admpc_last_error()
        return _host(self.per).copy(), _host(self.stats).copy(), _host(self.info).copy()


def _fit_records(fl, dev, stats, hyper=None):
    """What admpc_quad_ensemble_fit (hyper None) or _refit writes for the statistics: ([K][3] AdmpcGp, info [K, 3])."""
    import torch
    from ad_mpc_amd.config import AdmpcGp
    gp = torch.zeros(fl.K * 3 * C.sizeof(AdmpcGp), dtype=torch.uint8, device="cuda:0")
    info = torch.zeros((fl.K, 3), dtype=torch.int32, device="cuda:0")
    dev.bins.copy_(_dev(stats))
    if hyper is None:
        rc = fl.lib.admpc_quad_ensemble_fit(fl._ens, 1, _p(dev.bins), _p(gp), _p(info), _stream())
    else:
        rc = fl.lib.admpc_quad_ensemble_refit(fl._ens, 1, _p(dev.bins), _p(hyper), _p(gp), _p(info), _stream())
    assert rc == 0, fl.lib.admpc_last_error()
    raw = _host(gp).tobytes()
    size = C.sizeof(AdmpcGp)
    return [[AdmpcGp.from_buffer_copy(raw[(c * 3 + g) * size:(c * 3 + g + 1) * size]) for g in range(3)] for c in range(fl.K)], _host(info)


def _same_as_the_fit(fl, blocks, finfo, gps, info, what):
    """The factor blocks against the fit's records: n, the head, Z, alpha, ymean and info, bit for bit; rows past n and the pad are 0."""
    _bits(finfo[:, :fl.n_learn], info[:, :fl.n_learn], what + ": info")
    for c in range(fl.K):
        for g in range(3):
            b = blocks[c, g]
            if g >= fl.n_learn:
                assert (b == -3.0).all(), (what, c, g)                # entries past n_gp are not written
                continue
            G = gps[c][g]
            head = [G.n_points, G.n_feat, G.feat[0], G.feat[1], G.feat[2], G.out, G.sigma_f, G.inv_l2[0], G.inv_l2[1], G.inv_l2[2], G.ymean, 0, 0, 0, 0, 0]
            _bits(b[:16], np.array(head, dtype=np.float64), "%s: (%d, %d) the head" % (what, c, g))
            _bits(b[EV.F_Z:EV.F_ALPHA].reshape(3, 32), np.array(G.Z, dtype=np.float64), "%s: (%d, %d) Z" % (what, c, g))
            _bits(b[EV.F_ALPHA:EV.F_W], np.array(G.alpha, dtype=np.float64), "%s: (%d, %d) alpha" % (what, c, g))
            n = G.n_points
            assert not b[EV.F_W + n * (n + 1) // 2:].any(), (what, c, g)


def _w_is_the_inverse(fl, blocks, stats, hyper=None):
    worst = 0.0
    for c in range(fl.K):
        for g in range(fl.n_learn):
            f = EV.factor_from_bins(fl._obs[c].gp[g], stats[c, g], 1, None if hyper is None else hyper[c, g], LD)
            d = EV.unpack(blocks[c, g], LD)
            assert d["n"] == f["n"], (c, g)
            if f["n"]:
                err = float(np.abs(d["W"] @ f["L"] - np.eye(f["n"], dtype=LD)).max())
                assert err <= 64.0 * U * f["cond"], (c, g, err, f["cond"])
                worst = max(worst, err / (64.0 * U * f["cond"]))
    return worst


# ---- 1. the factor ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,n_gp,n_feat", [(1, 1, 1), (3, 3, 2), (8, 3, 3), (3, 1, 3), (1, 3, 2)])
def test_factor_is_the_fit_bit_for_bit_and_w_inverts_l(K, n_gp, n_feat):
    fl, feats, cent = _ensemble(K, n_gp, n_feat)
    try:
        dev = Dev(fl, 1)
        stats = _stats(fl, 3 + K)
        if K == 3 and n_gp == 3:
            stats[2, 2, np.flatnonzero(stats[2, 2, :, 0])[4], 4] = np.nan        # a failure at step 5 of (2, 2)
        blocks, finfo = dev.make_factor(stats)
        gps, info = _fit_records(fl, dev, stats)
        _same_as_the_fit(fl, blocks, finfo, gps, info, "given")
        seen = sorted({int(v) for v in finfo[:, :n_gp].reshape(-1)})
        assert set(seen) >= ({32} if K * n_gp == 1 else {0, 1, 31, 32} if K * n_gp >= 4 else {32, 31, 1}), seen
        if K == 3 and n_gp == 3:
            assert finfo[2, 2] == -5 and blocks[2, 2, 0] == 0.0 and blocks[2, 2, 10] == 0.0
        stats[np.isnan(stats)] = 0.5
        if K == 3 and n_gp == 3:
            blocks, finfo = dev.make_factor(stats)
        print("K = %d n_gp = %d n_feat = %d: |W L - I| at most %.3g of its bound" % (K, n_gp, n_feat, _w_is_the_inverse(fl, blocks, stats)))
    finally:
        fl.close()


def test_factor_after_a_search_is_the_refit_and_a_failed_pivot_and_no_optimum_are_empty():
    fl, feats, cent = _ensemble(3, 3, 1)
    try:
        dev = Dev(fl, 1)
        stats = _stats(fl, 9, fills=(32, 31, 20, 27))
        stats[2, 0] = 0.0
        twin = np.flatnonzero(stats[1, 2, :, 0])[:2]                   # the first two points with the same mean: with sigma_f = 1, no count
        stats[1, 2, twin[1]] = stats[1, 2, twin[0]]                    # noise and a noise that 1 swallows, the second pivot of (1, 2) is exactly 0
        fl.bins.copy_(_dev(stats))
        info, installed, hyper = fl.search_gp(rounds=2, install=False)
        hy = _host(hyper).copy()
        hy[1, 2, 10:15], hy[1, 2, 15] = [1.5, 1.0, 1.0, 1.0, 1e-300], 7.0
        hy[0, 1, 15] = np.inf                                          # a search that found no finite NLL
        fl.hyper.copy_(_dev(hy))
        blocks, finfo = dev.make_factor(stats, fl.hyper)
        gps, info = _fit_records(fl, dev, stats, fl.hyper)
        _same_as_the_fit(fl, blocks, finfo, gps, info, "searched")
        assert finfo[1, 2] == -2 and finfo[0, 1] == EV.NO_OPTIMUM and finfo[2, 0] == 0 and finfo[0, 0] == 32
        for c, g in ((1, 2), (0, 1), (2, 0)):
            assert blocks[c, g, 0] == 0.0 and blocks[c, g, 10] == 0.0 and not blocks[c, g, 16:].any() and blocks[c, g, 6] == hy[c, g, 13]
        _bits(blocks[0, 0, 6:10], np.array([hy[0, 0, 13], 1.0 / (hy[0, 0, 10] * hy[0, 0, 10]), 0.0, 0.0]), "the searched hyperparameters of (0, 0)")
        hy[1, 2, 14] = 1e-3
        hy[0, 1, 15] = 1.0
        stats[1, 2, twin[1], 1] += 0.05 * stats[1, 2, twin[1], 0]
        fl.hyper.copy_(_dev(hy))
        blocks, finfo = dev.make_factor(stats, fl.hyper)
        print("searched: |W L - I| at most %.3g of its bound" % _w_is_the_inverse(fl, blocks, stats, hy))
        # the fleet's own chain: factor=True follows the re-fit from the same bins and the same hyper
        fl.close()
        fl, feats, cent = _ensemble(3, 3, 1, log_steps=2)
        fl.bins.copy_(_dev(stats))
        fl.fit_gp(install=False, factor=True)
        given, _ = Dev(fl, 1).make_factor(stats)
        _bits(_host(fl.factor), given, "fit_gp(factor=True)")
        fl.search_gp(rounds=2, install=False, factor=True)
        searched, sinfo = Dev(fl, 1).make_factor(stats, fl.hyper)
        _bits(_host(fl.factor), searched, "search_gp(factor=True)"); _bits(_host(fl.factor_info), sinfo, "factor_info")
        assert not np.array_equal(searched, given)
        _bits(_host(fl.factor_gp()), sinfo, "factor_gp() after a search reads hyper")
    finally:
        fl.close()


# ---- 2. the evaluation ----------------------------------------------------------------------------------------------------------------------

def _records(M, seed, feats, cent, dirty=True):
    """Records with v_b in the boxes of _ensemble and y a smooth function of it; with `dirty` all three flag values, a fourth, entries that
    are not finite; a record within 1e-6 of a tie between two centroids is taken out (flag 0)."""
    rng = np.random.default_rng(seed)
    S = rng.uniform(-8.5, 8.5, (M, EV.REC))
    S[:, 10:13] = np.sin(S[:, 0:3]) - 0.3 * S[:, 0:3] + 0.3 * rng.standard_normal((M, 3))
    S[:, 13] = 1.0
    if dirty and M >= 8:
        S[::7, 13], S[3::11, 13], S[5::13, 13] = 0.0, EV.PRUNED, 3.0
        S[2::17, int(rng.integers(0, 13))] = np.nan
        S[4::19, 11] = np.inf
    fin = np.isfinite(S[:, :13]).all(axis=1)
    with np.errstate(all="ignore"):
        S[fin & (EV.route(S, feats, cent)[1] < 1e-6), 13] = 0.0
    return S


def _hold(dev, fl, feats, stats, full, M, take_pruned, drag, got, what, min_count=1):
    """The device's outputs of an evaluation against the spec from the device's own factor: see the module's docstring."""
    per, dstats, dinfo = got
    blocks = _host(dev.factor)
    cent = fl._device_centroids()
    n_gp = fl.n_learn
    fd = [[EV.unpack(blocks[c, g], LD) for g in range(n_gp)] for c in range(fl.K)]
    cond = [[EV.factor_from_bins(fl._obs[c].gp[g], stats[c, g], min_count)["cond"] for g in range(n_gp)] for c in range(fl.K)]
    S = full[:M]
    want = EV.evaluate(S, feats, cent, fd, take_pruned, drag, LD)
    part, route = want["part"], want["route"]
    _bits(dinfo, want["info"], what + ": info")
    # per record: the pad rows and the regressors past n_gp untouched, NaN where a record does not take part
    assert (per[M:] == -7.5).all() and (per[:M, n_gp:] == -7.5).all() and np.isnan(per[:M, :n_gp][~part]).all(), what
    mu, sd = per[:M, :n_gp, 0].astype(LD), per[:M, :n_gp, 1].astype(LD)
    assert np.isfinite(per[:M, :n_gp][part]).all() and (sd[part] >= 0).all(), what
    _bits(_host(dev.rec), full, what + ": the records are read only")
    bm, bv = np.zeros((M, n_gp), dtype=LD), np.zeros((M, n_gp), dtype=LD)
    worst = [0.0, 0.0]
    for c in range(fl.K):
        at = part & (route == c)
        for g in range(n_gp):
            f = fd[c][g]
            bm[at, g] = 4.0 * (f["n"] + 8) * U * (abs(LD(f["ymean"])) + want["absdot"][at, g])
            if drag is not None:
                bm[at, g] += 4.0 * U * np.abs(drag[f["out"] - 7] * S[at, f["out"] - 7])      # the product and the sum of the drag term
            bv[at, g] = 64.0 * U * cond[c][g] * (float(f["sigma_f"]) + EV.JITTER)
    em, evar = np.abs(mu - want["mu"])[part], np.abs(sd * sd - np.maximum(want["var"], 0))[part]
    assert (em <= bm[part]).all() and (evar <= bv[part] + 4.0 * U * np.maximum(want["var"], 0)[part]).all(), \
        (what, float((em / np.maximum(bm[part], 1e-300)).max()), float((evar / bv[part]).max()))
    if part.any():
        worst = [float((em / np.maximum(bm[part], 1e-300)).max()), float((evar / bv[part]).max())]
    assert not (want["var"][part] < -bv[part]).any()
    # the statistics: the counts exact, the 3-std count between the spec's two, the sums within their bounds
    bs = np.minimum(np.sqrt(bv), bv / np.maximum(want["std"], 1e-300)) + 2.0 * U * want["std"]
    edge = want["margin"] < bm + 3.0 * bs + 8.0 * U * np.abs(want["res"])
    res, y, std = np.abs(want["res"]), np.abs(want["y"]), want["std"]
    for c in range(fl.K):
        at = part & (route == c)
        m = int(at.sum())
        for g in range(3):
            d = dstats[c, g]
            if g >= n_gp or m == 0:
                assert not d.any(), (what, c, g)
                continue
            assert d[0] == m, (what, c, g)
            inside = (res[at, g] <= 3.0 * std[at, g])
            lo, hi = int((inside & ~edge[at, g]).sum()), int((inside | edge[at, g]).sum())
            assert lo <= d[6] <= hi, (what, c, g, lo, d[6], hi)
            near0 = int((np.abs(want["var"][at, g]) <= bv[at, g]).sum())
            assert (want["var"][at, g] < -bv[at, g]).sum() <= d[7] <= (want["var"][at, g] < 0).sum() + near0, (what, c, g)
            for k, terms, each in ((1, y[at, g], 0 * bm[at, g]), (2, y[at, g] ** 2, 0 * bm[at, g]), (3, res[at, g], bm[at, g]),
                                   (4, res[at, g] ** 2, 2.0 * res[at, g] * bm[at, g] + bm[at, g] ** 2), (5, std[at, g], bs[at, g])):
                bound = (m + 1) * U * terms.sum() + each.sum()
                assert abs(LD(d[k]) - terms.sum()) <= bound, (what, c, g, k, float(d[k]), float(terms.sum()), float(bound))
    return want, worst, bm


@pytest.mark.parametrize("M,shape", list(zip(SIZES, SHAPES)))
def test_evaluation_equals_the_spec_within_the_bounds(M, shape):
    K, n_gp, n_feat = shape
    fl, feats, cent = _ensemble(K, n_gp, n_feat)
    try:
        dev = Dev(fl, M)
        stats = _stats(fl, 20 + K + n_feat)
        dev.make_factor(stats)
        S = _records(M, 30 + M % 97, feats, cent)
        for take_pruned, drag in ((0, None), (1, np.array([-0.3, 0.2, -0.1]))):
            full = dev.load(S)
            dev.stats.fill_(-3.0); dev.info.fill_(-3); dev.partial.fill_(float("nan"))
            got = dev.evaluate(M, take_pruned, drag)
            want, worst, _ = _hold(dev, fl, feats, stats, full, M, take_pruned, drag, got, "M = %d K = %d take_pruned = %d" % (M, K, take_pruned))
            nblk = min(-(-M // 256), CS.BLOCKS_MAX)
            rows = _host(dev.partial)
            assert not np.isnan(rows[:nblk]).any() and np.isnan(rows[nblk:]).all()
            print("M = %d (K, n_gp, n_feat) = %s take_pruned = %d: info %s, worst ratio to the bound, mean %.3g, std^2 %.3g"
                  % (M, shape, take_pruned, got[2].tolist(), worst[0], worst[1]))
            # two runs, the same bits; without per_record the statistics are the same
            again = dev.evaluate(M, take_pruned, drag)
            _bits(again[0], got[0], "two runs: per_record"); _bits(again[1], got[1], "two runs: stats"); _bits(again[2], got[2], "two runs: info")
            dev.per.fill_(-7.5)
            bare = dev.evaluate(M, take_pruned, drag, per=False)
            assert (bare[0] == -7.5).all()
            _bits(bare[1], got[1], "without per_record: stats")
        if M >= 256:
            info = got[2]
            route = want["route"][want["part"]]
            assert info[2] > 0 and info[3] > 0 and len(set(route[:64].tolist())) >= min(K, 2)       # clusters alternate inside a wave
            if K >= 3:
                assert not got[1][K - 1].any() and got[1][0, 0, 0] > 0                                     # the far cluster has no record
    finally:
        fl.close()


def test_nobody_takes_part_and_empty_factors():
    fl, feats, cent = _ensemble(3, 3, 1)
    try:
        M = 300
        dev = Dev(fl, M)
        stats = _stats(fl, 4)
        dev.make_factor(np.zeros_like(stats))                          # every factor empty: mean 0, the prior's variance
        S = _records(M, 5, feats, cent)
        full = dev.load(S)
        per, dstats, info = dev.evaluate(M)
        want, _, _ = _hold(dev, fl, feats, np.zeros_like(stats), full, M, 0, None, (per, dstats, info), "empty factors")
        p = want["part"]
        assert (per[:M][p][:, :, 0] == 0.0).all() and not dstats[..., 7].any()
        for g in range(3):
            assert (per[:M][p][:, g, 1] == np.sqrt(0.5 + 0.1 * g + 1e-8)).all()
        _bits(dstats[..., 1], dstats[..., 3], "empty factors: the augmented error is the nominal one")
        S[:, 13] = np.where(np.arange(M) % 2 == 0, 0.0, 3.0)
        S[1, 13], S[1, 4] = 1.0, np.nan
        dev.load(S)
        dev.stats.fill_(5.0); dev.info.fill_(5)
        per, dstats, info = dev.evaluate(M)
        assert info.tolist() == [EV.ENOVALID, 0, M - 1, 1] and not dstats.any() and np.isnan(per[:M]).all() and (per[M:] == -7.5).all()
    finally:
        fl.close()


def test_a_captured_evaluation_picks_up_a_new_factor_at_replay():
    import torch
    fl, feats, cent = _ensemble(3, 3, 1)
    try:
        M = 700
        dev = Dev(fl, M)
        first, second = _stats(fl, 1), _stats(fl, 2, fills=(27, 32, 20, 31))
        dev.make_factor(first)
        dev.load(_records(M, 8, feats, cent))
        eager_first = dev.evaluate(M)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rc = dev.L.admpc_quad_ensemble_evaluate(fl._ens, M, _p(dev.rec), 0, _p(dev.factor), None, _p(dev.per), _p(dev.partial), _p(dev.stats),
                                                    _p(dev.info), _stream())
            assert rc == 0
        dev.make_factor(second)
        dev.stats.fill_(9.0); dev.info.fill_(9); dev.per.fill_(-7.5)
        g.replay()
        replay = (_host(dev.per).copy(), _host(dev.stats).copy(), _host(dev.info).copy())
        eager_second = dev.evaluate(M)
        for a, b, what in zip(replay, eager_second, ("per_record", "stats", "info")):
            _bits(a, b, "the replay against the eager run under the new factor: " + what)
        assert not np.array_equal(replay[1], eager_first[1]) and np.array_equal(replay[2], eager_first[2])
    finally:
        fl.close()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_no_ops():
    fl, feats, cent = _ensemble(3, 3, 1, log_steps=2)
    other = C.c_void_p(0)
    try:
        L = fl.lib
        M = 50
        dev = Dev(fl, M)
        stats = _stats(fl, 1)
        dev.make_factor(stats)
        full = dev.load(_records(M, 2, feats, cent))
        good = dev.evaluate(M)
        # an ensemble of the same handles without observe parameters, clustering on a feature the record does not hold
        c3 = np.zeros((3, 1))
        assert L.admpc_quad_ensemble_create(fl._handles, 3, 1, (C.c_int32 * 1)(3), c3.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(other)) == 0
        e, P = fl._ens, _p
        arrays = lambda: [P(dev.bins), None, P(dev.factor), P(dev.finfo)]
        fac = lambda ens, mc, a: L.admpc_quad_ensemble_factor(ens, mc, *a, _stream())
        ev = lambda ens, M_, tp, a: L.admpc_quad_ensemble_evaluate(ens, M_, a[0], tp, a[1], None, None, a[2], a[3], a[4], _stream())
        evarr = lambda: [P(dev.rec), P(dev.factor), P(dev.partial), P(dev.stats), P(dev.info)]
        nul4, nul5 = [None] * 4, [None] * 5
        table = [
            # (call, the whole message): every later refusal's cause is present too, so the pair pins the order
            (lambda: fac(None, 0, nul4), "admpc_quad_ensemble_factor: null ensemble"),
            (lambda: fac(other, 0, nul4), "admpc_quad_ensemble_factor: the ensemble was created without observe parameters"),
            (lambda: fac(e, 0, nul4), "admpc_quad_ensemble_factor: min_count must be at least 1"),
            (lambda: fac(e, 1, nul4), "admpc_quad_ensemble_factor: null array argument"),
            (lambda: ev(None, -1, 2, nul5), "admpc_quad_ensemble_evaluate: null ensemble"),
            (lambda: ev(other, -1, 2, nul5), "admpc_quad_ensemble_evaluate: the clustering features must lie in [7, 16]: the sample record holds no others"),
            (lambda: ev(e, -1, 2, nul5), "admpc_quad_ensemble_evaluate: the number of records must be in [0, INT32_MAX]"),
            (lambda: ev(e, 2 ** 31, 2, nul5), "admpc_quad_ensemble_evaluate: the number of records must be in [0, INT32_MAX]"),
            (lambda: ev(e, M, 2, nul5), "admpc_quad_ensemble_evaluate: take_pruned must be 0 or 1"),
            (lambda: ev(e, 0, -1, nul5), "admpc_quad_ensemble_evaluate: take_pruned must be 0 or 1"),
            (lambda: ev(e, M, 1, nul5), "admpc_quad_ensemble_evaluate: null array argument"),
        ]
        for call, message in table:
            assert call() == EINVAL and L.admpc_last_error().decode() == message, message
        for k in (0, 2, 3):
            a = arrays(); a[k] = None
            assert fac(e, 1, a) == EINVAL and b"null array" in L.admpc_last_error(), k
        for k in range(5):
            a = evarr(); a[k] = None
            assert ev(e, M, 0, a) == EINVAL and b"null array" in L.admpc_last_error(), k
        assert ev(e, 0, 0, nul5) == 0 and ev(e, 0, 1, evarr()) == 0          # M == 0 is a no-op behind the refusals of the scalars
        _bits(_host(dev.stats), good[1], "the statistics after the refusals and the no-ops"); _bits(_host(dev.info), good[2], "info")
        _bits(_host(dev.rec), full, "the records")
        # the fleet refuses before a launch, in its order
        with pytest.raises(ValueError, match="nothing evaluated yet"):
            fl.evaluation()
        with pytest.raises(ValueError, match="the log is empty"):
            fl.evaluate_log()
        fl.log_count = 2
        with pytest.raises(ValueError, match="no factor yet"):
            fl.evaluate_log(drag=True)
        fl.factor_gp()
        with pytest.raises(ValueError, match="fit_rdrv"):
            fl.evaluate_log(drag=True)
        with pytest.raises(ValueError, match="include_pruned"):
            fl.evaluate_log(include_pruned=3)
        s, info, per = fl.evaluate_log()
        assert per is None and _host(info).tolist() == [EV.ENOVALID, 0, 8, 0]                      # the zeroed log holds no valid record
        with pytest.raises(ValueError, match="units"):
            fl.evaluation(units="metres")
        assert fl.evaluation().count.tolist() == [[0] * 3] * 3
        nolog, _, _ = _ensemble(1, 1, 1)
        try:
            for call in (nolog.evaluate_log, nolog.factor_gp, lambda: nolog.fit_gp(factor=True), lambda: nolog.search_gp(factor=True)):
                with pytest.raises(ValueError, match="keeps no log"):
                    call()
        finally:
            nolog.close()
    finally:
        if other:
            fl.lib.admpc_quad_ensemble_destroy(other)
        fl.close()


# ---- 4. the experiment ------------------------------------------------------------------------------------------------------------------------

def _flight():
    """The setting of tests/test_quad_prune_gpu.py's flights -- B = 64, N = 10, circles of 5 m at 2, 3, 4 and 5 m/s, drag on, 60 steps, a
    K = 1 fleet with log_steps = 60 -- with every length scale GIVEN as 0.3, as in the experiment whose ordering of fit_gp and search_gp
    the README reports (tests/test_quad_hyper_gpu.py's closing test)."""
    import quad_learn_spec as QL
    import test_quad_ensemble_gpu as TE
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, B, T = 10, 64, 60
    dt = 1.0 / (N * 5)
    trajs = [circle_reference(T + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
    traj_of = (np.arange(B) % 4).astype(np.int32)
    idx0 = (np.arange(B) // 4).astype(np.int32)
    ref = np.concatenate([[QL.body_velocity(trajs[k][0][i + t])[0] for t in range(T)] for k, i in zip(traj_of, idx0)])
    learn = [[TE.VX(ref.min() - 0.5, ref.max() + 0.5, length_scale=0.3)] + [dict(d, length_scale=0.3) for d in QL.EXP_LEARN[1:]]]
    fl = TE._fleet(B, N, trajs, traj_of, idx0, None, centroids=[[float(np.median(ref))]], feats=[7], learn=learn, log_steps=T)
    return fl, traj_of, idx0, T, B


def test_a_second_flight_scores_the_gps_of_the_first_on_the_device():
    """The flight of _flight: fit_gp(factor=True)
    on the first flight, log_reset(), a second flight from other places on the trajectories, evaluate_log().  The device's
    augmented_rms / nominal_rms per axis is the host's recomputation from the same log through the spec (from the device's factor, in
    longdouble) within the bounds of the sums; it is below 1 on every axis; and after search_gp(factor=True) on the bins of the first
    flight it is not above the fit_gp one.  The ratios, mean_std and the 3-std coverage are printed; no coverage is pinned.
    Measured on the MI355X: fit_gp 0.01284 / 0.06947 / 0.13721 (mean std 0.0139 / 0.319 / 0.179, every record inside 3 std), search_gp
    0.00377 / 0.00608 / 0.09681 (mean std 0.0032 / 0.0033 / 0.0035; 93.4 % / 78.2 % / 83.6 % inside 3 std); no variance clipped.  With the
    length scales given as 2.0 the fit_gp ratios are 0.00428 / 0.00717 / 0.09636: the search is then better on two axes and 0.5 % worse on
    the third -- it maximises the likelihood of the first flight's bins, not the held-out error."""
    fl, traj_of, idx0, T, B = _flight()
    try:
        fl.rollout(T, observe=True, log=True)
        bins = fl.bins.clone()
        info, installed = fl.fit_gp(min_count=2, install=False, factor=True)
        assert (_host(info) >= 1).all(), _host(info)
        fl.log_reset()
        fl.reset(traj_of, (idx0 + 7).astype(np.int32))
        fl.rollout(T, observe=True, log=True)
        log = _host(fl.log).reshape(-1, EV.REC).copy()
        factor_before = _host(fl.factor).copy()
        stats, einfo, per = fl.evaluate_log(per_record=True)
        _bits(_host(fl.factor), factor_before, "the factor does not depend on what the second flight added to the bins")
        given = fl.evaluation()
        M = T * B
        assert _host(einfo).tolist()[0] == 0 and given.count.sum(axis=0).tolist() == [int(_host(einfo)[1])] * 3 and per.shape == (M, 3, 2)
        dev = types_dev(fl, log, per, stats, einfo)
        want, worst, bm = _hold(dev, fl, fl.feats, _host(bins), log, M, 0, None, (_host(per), _host(stats), _host(einfo)), "the flight", min_count=2)
        ratio = given.total.augmented_rms / given.total.nominal_rms
        p = want["part"]
        spec = np.sqrt((want["res"][p] ** 2).sum(axis=0) / (want["y"][p] ** 2).sum(axis=0))
        r, y, m = np.abs(want["res"][p]), want["y"][p], int(p.sum())
        b2, b4 = (m + 1) * U * (y * y).sum(axis=0), (m + 1) * U * (r * r).sum(axis=0) + (2.0 * r * bm[p] + bm[p] ** 2).sum(axis=0)
        rel = 0.5 * (b4 / (r * r).sum(axis=0) + b2 / (y * y).sum(axis=0)) + 4.0 * U          # the root of a quotient of two sums held to b4, b2
        assert (np.abs(ratio.astype(LD) - spec) <= rel * spec).all(), (ratio, spec, rel)
        print("fit_gp:    augmented / nominal rms per axis %s, mean_std %s, within 3 std %s, clipped %s"
              % (ratio.tolist(), given.total.mean_std.tolist(), given.total.within_3std.tolist(), given.total.clipped.tolist()))
        assert (ratio < 1.0).all(), ratio
        v = fl.evaluation(units="velocity")
        assert np.allclose(v.total.augmented_mae, given.total.augmented_mae * fl.control_period, rtol=1e-15)
        fl.bins.copy_(bins)                                            # the statistics of the first flight alone
        fl.search_gp(min_count=2, install=False, factor=True)
        fl.evaluate_log()
        searched = fl.evaluation()
        sratio = searched.total.augmented_rms / searched.total.nominal_rms
        print("search_gp: augmented / nominal rms per axis %s, mean_std %s, within 3 std %s, clipped %s"
              % (sratio.tolist(), searched.total.mean_std.tolist(), searched.total.within_3std.tolist(), searched.total.clipped.tolist()))
        assert (sratio <= ratio).all(), (sratio, ratio)
    finally:
        fl.close()


def types_dev(fl, log, per, stats, info):
    """What _hold reads of a Dev, over the fleet's own tensors."""
    import types
    return types.SimpleNamespace(factor=fl.factor, rec=fl.log.view(-1, EV.REC))
