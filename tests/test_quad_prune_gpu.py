"""The prune of the flight log and the RDRv drag fit on the device (include/admpc_quad_prune.h; csrc/admpc_quad_prune.hip;
QuadEnsembleFleet.prune_log / fit_rdrv / learned_rdrv) against the numpy spec, tests/quad_prune_spec.py, which
tests/test_quad_prune_cpu.py pins to the reference's prune_dataset and linear_rdrv_fitting.

The prune is a rule of decisions: flags, info, counts and the lo / hi of every column are held to the spec EXACTLY, on every record
count at which the grid changes shape and past it, every bin count at the ends of its range, and on data made to sit on edges.  The drag
fit is a sum, whose order is not part of the contract: it is held within ten times the gap between the spec in float64 and in
numpy.longdouble at the same size (measured on the MI355X: 0.05 to 2.1 gaps)."""
import numpy as np
import pytest

import quad_clusters_spec as CS
import quad_learn_spec as QL
import quad_prune_spec as PS
import test_quad_ensemble_gpu as TE
import test_quad_fleet_gpu as TQ

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _stream = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._stream
VX = TE.VX
SIZES = (1, 63, 64, 65, 256, 257, CS.BLOCKS_MAX * 256 + 1)         # the last is past the grid, into the stride loops
BINS = (1, 2, 3, 40, 255, 256)
PAD = 8                                                             # rows behind the records, which no kernel may touch
LD = np.longdouble
X_CAP = 9.0                                                         # v_b ~ 6 N(0, 1): about one record in seven is capped


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Dev:
    """The library's entries over device scratch of the test's own, for up to M records."""

    def __init__(self, M):
        import torch
        from ad_mpc_amd import _lib
        self.L = _lib.load()
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda:0")
        self.rec = z(M + PAD, PS.REC)
        self.partial, self.edges = z(CS.BLOCKS_MAX, 9), z(4, PS.BINS_MAX + 1)
        self.counts, self.info = z(4, PS.BINS_MAX, dtype=torch.int32), z(8, dtype=torch.int32)
        self.rpartial, self.d, self.sums, self.rinfo = z(CS.BLOCKS_MAX, 7), z(3), z(3, 2), z(2, dtype=torch.int32)
        self.installed = z(1, dtype=torch.int32)

    def load(self, S):
        """S [M, 14] and PAD rows of a pattern behind it; returns the host copy of all of it."""
        full = np.full((self.rec.shape[0], PS.REC), -7.5)
        full[:S.shape[0]] = S
        full[S.shape[0]:, 13] = 1.0                                  # a pad row would take part if a kernel ran past M
        self.rec.copy_(_dev(full))
        return full

    def prune(self, M, x_cap, n_bins, thresh):
        rc = self.L.admpc_quad_records_prune(0, M, _p(self.rec), float("inf") if x_cap is None else x_cap, n_bins, thresh, _p(self.partial),
                                             _p(self.edges), _p(self.counts), _p(self.info), _stream())
        assert rc == 0, self.L.admpc_last_error()

    def fit(self, M, axes=7):
        rc = self.L.admpc_quad_rdrv_fit(0, M, axes, _p(self.rec), _p(self.rpartial), _p(self.d), _p(self.sums), _p(self.rinfo), _stream())
        assert rc == 0, self.L.admpc_last_error()
        return _host(self.d).copy(), _host(self.sums).copy(), _host(self.rinfo).tolist()


def _drag_close(d, records, what):
    """d [3] against the longdouble spec within the forward bound of a float64 sum of n terms in ANY order, n u sum |terms| for S_xy and
    for S_xx, carried through the quotient: |d - D| <= 4 n 2^-53 (sum |v y| / S_xx + |D|)."""
    D = PS.rdrv(records, 7, LD)[0]
    use = records[:, 13] == 1.0
    v, y = records[use, 0:3].astype(LD), records[use, 10:13].astype(LD)
    bound = 4.0 * use.sum() * 2.0 ** -53 * (np.abs(v * y).sum(axis=0) / (v * v).sum(axis=0) + np.abs(D))
    assert (np.abs(d.astype(LD) - D) <= bound).all(), (what, d.tolist(), D.tolist(), bound.tolist())


def _thresh(M):
    return 0.0137 if M < 1000 else 0.00137


def _check(dev, full, M, x_cap, n_bins, thresh, what):
    """The device's state after a prune of the M records of `full` against the spec's: exactly."""
    want = PS.prune(full[:M], x_cap, n_bins, thresh)
    assert want["margin"] > 1e-6, (what, want["margin"])              # the precondition: no bin ratio at thresh
    exp = full.copy()
    exp[:M] = want["records"]
    got = _host(dev.rec)
    _bits(got, exp, what + ": the records (entries 0 .. 12, the flags, the pad rows)")
    _bits((got[:M, 13] == 1.0) & want["part"], want["kept"], what + ": the kept mask")
    _bits(_host(dev.info), want["info"], what + ": info")
    _bits(_host(dev.counts), want["counts"], what + ": counts")
    if want["edges"] is not None:
        e = _host(dev.edges)
        _bits(e[:, 0].copy(), want["lo"], what + ": lo"); _bits(e[:, n_bins].copy(), want["hi"], what + ": hi")
        _bits(e[:, :n_bins + 1].copy(), np.array(want["edges"]), what + ": edges")
    return want


# ---- 1. the kept mask, the flags, info, counts and the ranges -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", PS.KINDS)
def test_prune_equals_the_spec_exactly(kind):
    dev = Dev(SIZES[-1])
    seen = np.zeros(8, dtype=np.int64)
    for M in SIZES:
        S = PS.records(kind, M, seed=11)
        for n_bins in BINS:
            full = dev.load(S)
            dev.edges.fill_(-3.0); dev.counts.fill_(-3); dev.info.fill_(-3); dev.partial.fill_(float("nan"))
            dev.prune(M, X_CAP, n_bins, _thresh(M))
            want = _check(dev, full, M, X_CAP, n_bins, _thresh(M), "%s M = %d n_bins = %d" % (kind, M, n_bins))
            seen += want["info"] > 0
            nblk = min(-(-M // 256), CS.BLOCKS_MAX)
            part = _host(dev.partial)
            assert not np.isnan(part[:nblk]).any() and np.isnan(part[nblk:]).all() and part[:nblk, 8].sum() == want["info"][1]      # a block without a record: +-inf
            e = _host(dev.edges)
            assert (e[:, n_bins + 1:] == -3.0).all()                  # the rest of a row of edges is not written
    # the fixture reaches what it is there for
    assert seen[1] == len(SIZES) * len(BINS) and (seen[3] > 0 or kind == "one")
    if kind in ("heavy", "quarter", "pythagorean"):
        assert (seen[4:] > 0).all() and seen[2] > 0, seen
    if kind == "constant":
        assert seen[5] > 0                                           # the constant column on the middle edge of an even n_bins


def test_records_on_edges_take_the_closed_upper_side():
    """Whole and quarter numbers with a range that makes the edges whole too: a record ON e[idx] below which the bin is sparse is pruned,
    though its own bin is not (the reference's closed comparison), and the device agrees with the spec on every one."""
    M, n_bins = 4000, 8
    rng = np.random.default_rng(5)
    S = PS.records("quarter", M, seed=2, dirty=False)
    y = rng.choice([0.0, 1.0, 2.0, 4.0, 5.0, 6.0, 7.0, 8.0], (M, 3))
    y[:2] = [[3.0, 3.0, 3.0], [3.5, 3.5, 3.5]]                      # the edges of every axis are 0, 1, ..., 8; bin 3 = [3, 4) holds two records
    S[:, 10:13] = y
    dev = Dev(M)
    full = dev.load(S)
    dev.prune(M, None, n_bins, 0.00137)
    want = _check(dev, full, M, None, n_bins, 0.00137, "on the edges")
    flags = want["records"][:, 13]
    # bin 3 is sparse.  4.0 lies in bin 4, which is not, and is pruned for lying on the sparse bin's upper edge; 5.0 and the rest stay
    for j in range(3):
        assert np.array_equal(want["edges"][j], np.arange(9.0)) and want["counts"][j, 3] == 2 and want["counts"][j, :8].min() == 2
        assert want["info"][4 + j] == 2 + (y[:, j] == 4.0).sum() > 300
    assert (flags[(y == 4.0).any(axis=1)] == 2.0).all() and flags[0] == flags[1] == 2.0 and want["info"][3] == 0


# ---- 2. idempotence, restore, nobody takes part ---------------------------------------------------------------------------------------------

def test_pruning_twice_is_once_restore_and_enovalid():
    M = 3000
    S = PS.records("heavy", M, seed=4)
    dev = Dev(M)
    full = dev.load(S)
    dev.prune(M, X_CAP, 40, 0.00137)
    once = (_host(dev.rec).copy(), _host(dev.info).copy(), _host(dev.counts).copy(), _host(dev.edges).copy())
    want = _check(dev, full, M, X_CAP, 40, 0.00137, "once")
    assert 0 < want["info"][2] < want["info"][1] < M and (want["records"][:, 13] != S[:, 13]).any()
    dev.prune(M, X_CAP, 40, 0.00137)
    for got, first, what in zip((_host(dev.rec), _host(dev.info), _host(dev.counts), _host(dev.edges)), once, ("records", "info", "counts", "edges")):
        _bits(got, first, "twice against once: " + what)
    # another rule on the pruned log gives what it gives on the fresh one
    dev.prune(M, None, 7, 0.0137)
    _check(dev, full, M, None, 7, 0.0137, "a second rule on a pruned log")
    # restore
    dev.prune(M, None, 40, 0.0)
    got, info = _host(dev.rec), _host(dev.info)
    assert (got[:M][want["part"], 13] == 1.0).all() and info.tolist() == [0, want["info"][1], want["info"][1], 0, 0, 0, 0, 0]
    _bits(got[:M][~want["part"]], S[~want["part"]], "restore: who does not take part")
    # nobody takes part: status, zeros, and nothing else written
    Z = S.copy()
    Z[:, 13] = np.where(np.arange(M) % 2 == 0, 0.0, 3.0)
    Z[1, 13], Z[1, 11] = 1.0, np.inf
    full = dev.load(Z)
    dev.counts.fill_(5); dev.info.fill_(5); dev.edges.fill_(-3.0)
    dev.prune(M, X_CAP, 40, 0.00137)
    _bits(_host(dev.rec), full, "ENOVALID: the records")
    assert _host(dev.info).tolist() == [PS.ENOVALID, 0, 0, 0, 0, 0, 0, 0] and not _host(dev.counts).any() and (_host(dev.edges) == -3.0).all()


# ---- 3. the drag fit and its install ------------------------------------------------------------------------------------------------------------

def _gap(M):
    """The largest relative distance between the spec in float64 and in longdouble over eight draws of M records: what float64 sums of this
    length lose, whatever their order."""
    g = 0.0
    for seed in range(8):
        S = PS.records("heavy", M, seed=100 + seed, dirty=False)
        a, b = PS.rdrv(S, 7)[0], PS.rdrv(S, 7, LD)[0]
        g = max(g, float(np.abs((a.astype(LD) - b) / b).max()))
    return g


@pytest.mark.parametrize("M", SIZES)
def test_rdrv_fit_within_ten_gaps_of_the_longdouble_spec(M):
    dev = Dev(M)
    S = PS.records("heavy", M, seed=21)
    if M > 1:
        S = PS.prune(S, X_CAP, 40, _thresh(M))["records"]              # flags 0, 1, 2 and 3: only 1.0 counts
        S[np.isnan(S[:, 10:13]).any(axis=1), 13] = 0.0                # the NaN records of the fixture are another test's
    full = dev.load(S)
    d, sums, info = dev.fit(M)
    want, wsums, n_used, status = PS.rdrv(S, 7, LD)
    gap = _gap(M)
    err = float(np.abs((d.astype(LD) - want) / want).max())
    print("M = %d: n_used %d, D %s, relative error %.3e, gap %.3e" % (M, n_used, d.tolist(), err, gap))
    assert info == [n_used, 0] and status == 0 and n_used == (S[:, 13] == 1.0).sum()
    assert err <= 10.0 * gap
    assert float(np.abs((sums.astype(LD) - wsums) / wsums).max()) <= 10.0 * gap
    _bits(_host(dev.rec), full, "the fit writes no record")
    d2, sums2, info2 = dev.fit(M)
    _bits(d2, d, "two runs: D"); _bits(sums2, sums, "two runs: sums"); assert info2 == info
    # the mask: an axis that is not asked is 0, the others keep their bits
    d5, sums5, info5 = dev.fit(M, 5)
    assert d5[1] == 0.0 and not sums5[1].any() and info5 == info
    _bits(d5[[0, 2]], d[[0, 2]], "axes 0 and 2 alone")


def test_rdrv_failures_and_the_install():
    import torch
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config
    from ad_mpc_amd.quad_scenarios import random_quad_scenarios
    M = 500
    dev = Dev(M)
    S = PS.records("heavy", M, seed=8, dirty=False)
    S[:, 13] = 2.0
    dev.load(S)
    assert dev.fit(M)[2] == [0, -1]                                  # nothing with flag 1.0: S_xx = 0
    S[:, 13], S[:, 2] = 1.0, 0.0
    dev.load(S)
    assert dev.fit(M)[2] == [M, -3] and dev.fit(M, 3)[2] == [M, 0] and dev.fit(M, 4)[2] == [M, -3]
    S[7, 11] = np.nan                                                # flag 1.0 and not finite: it shows, it is not skipped
    dev.load(S)
    assert dev.fit(M)[2] == [M, -2] and dev.fit(M, 1)[2] == [M, 0]
    qc = default_quad_config()
    qs = random_quad_scenarios(16, qc, seed=2)
    solve = lambda s: s.solve_numpy(qs["x0"], qs["yref"], qs["yref_e"], qs["xbar"], qs["ubar"])
    h = QuadBatchSolver(qc)
    try:
        L = h.lib
        plain = solve(h)
        # declined: a failed status over good values; then a value that is not finite under a good status
        dev.installed.fill_(7)
        good, failed = _dev(np.array([-0.1, -0.2, -0.3])), _dev(np.array([M, -1], dtype=np.int32))
        assert L.admpc_quad_rdrv_install(h._h, _p(good), _p(failed), _p(dev.installed), _stream()) == 0
        bad, ok = _dev(np.array([0.1, np.nan, 0.2])), torch.zeros(2, dtype=torch.int32, device="cuda:0")
        flag = torch.full((1,), 7, dtype=torch.int32, device="cuda:0")
        assert L.admpc_quad_rdrv_install(h._h, _p(bad), _p(ok), _p(flag), _stream()) == 0
        assert _host(dev.installed).tolist() == [0] and _host(flag).tolist() == [0]
        for a, b in zip(solve(h), plain):
            _bits(a, b, "a declined install moves nothing")
        # taken
        S = PS.records("heavy", M, seed=9, dirty=False)
        S[:, 10:13] = -0.3 * S[:, 0:3] * [1.0, 1.2, 0.1] + 0.05 * S[:, 10:13]
        dev.load(S)
        d, sums, info = dev.fit(M)
        assert info == [M, 0] and (d < 0).all()
        assert L.admpc_quad_rdrv_install(h._h, _p(dev.d), _p(dev.rinfo), _p(dev.installed), _stream()) == 0
        assert _host(dev.installed).tolist() == [1]
        assert tuple(h.cfg.rdrv) == (0.0, 0.0, 0.0)                  # the host copy is not changed
        learned = solve(h)
        cfg = default_quad_config()
        for i in range(3):
            cfg.rdrv[i] = float(d[i])
        fresh = QuadBatchSolver(cfg)
        try:
            for a, b in zip(learned, solve(fresh)):
                _bits(a, b, "the solve after the install against a handle created with that drag")
        finally:
            fresh.close()
        assert not np.array_equal(learned[1], plain[1])
        # refusals behind a live handle, in their order
        assert L.admpc_quad_rdrv_install(None, None, None, None, _stream()) == -1 and b"null solver" in L.admpc_last_error()
        for k in range(3):
            arrs = [_p(dev.d), _p(dev.rinfo), _p(dev.installed)]
            arrs[k] = None
            assert L.admpc_quad_rdrv_install(h._h, *arrs, _stream()) == -1 and b"null array" in L.admpc_last_error()
        for a, b in zip(solve(h), learned):
            _bits(a, b, "a refused install moves nothing")
    finally:
        h.close()


# ---- 4. the chain on a fleet, captured ----------------------------------------------------------------------------------------------------------

def _log_fleet(B, steps, K=1, **kw):
    N = 10
    trajs = TQ._circles(N, 3.0)
    traj_of, idx0 = np.zeros(B, dtype=np.int32), ((np.arange(B) * 3) % 100).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=6)
    cent, learn = (TE.LOOP_CENT, TE.LOOP_LEARN) if K == 3 else ([[0.0]], [TE.LOOP_LEARN[0]])
    return TE._fleet(B, N, trajs, traj_of, idx0, x0, centroids=cent, feats=[7], learn=learn, log_steps=steps, **kw)


def _drag_log(steps, B, seed):
    """Records whose y is a drag in the body velocity, heavy-tailed noise on top, v_x inside the boxes of TE.LOOP_LEARN."""
    S = PS.records("heavy", steps * B, seed=seed, dirty=False)
    S[:, 0] = np.random.default_rng(seed).uniform(-4.5, 1.5, steps * B)
    S[:, 10:13] = -0.25 * S[:, 0:3] + 0.05 * S[:, 10:13]
    S[::9, 13], S[::11, 13] = 0.0, 2.0                              # records that are not valid, and records an earlier prune took out
    return S.reshape(steps, B, PS.REC)


def test_the_chain_is_captured_and_replayed_on_new_data():
    import torch
    B, steps = 67, 4
    fl = _log_fleet(B, steps, K=3)
    try:
        first, second = _drag_log(steps, B, 1), _drag_log(steps, B, 2)
        fl.log.copy_(_dev(first)); fl.log_count = steps

        def chain():
            fl.prune_log(X_CAP, 40, 0.0137)
            return fl.fit_rdrv()

        def state():
            return {k: _host(getattr(fl, k)).copy() for k in ("log", "prune_info", "prune_counts", "bins", "dropped", "rdrv", "rdrv_sums",
                                                               "rdrv_info", "rdrv_installed")}

        chain()                                                       # eager, once: also the warm-up of the capture
        eager_first = state()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            chain()
        fl.log.copy_(_dev(second))
        for k in ("prune_info", "rdrv_info", "rdrv_installed"):
            getattr(fl, k).fill_(9)
        g.replay()
        got = state()
        want = PS.prune(second.reshape(-1, PS.REC), X_CAP, 40, 0.0137)
        assert want["margin"] > 1e-6
        _bits(got["log"].reshape(-1, PS.REC), want["records"], "the replay: the flags of the new log")
        _bits(got["prune_info"], want["info"], "the replay: info"); _bits(got["prune_counts"], want["counts"], "the replay: counts")
        assert 0 < want["info"][2] < want["info"][1]
        wb, wd = np.zeros((3, 3, 32, 5)), np.zeros((3, 4), dtype=np.int32)
        CS.rebin(list(fl._obs), [7], np.asarray(TE.LOOP_CENT, dtype=np.float64), want["records"].reshape(steps, B, PS.REC), wb, wd)
        _bits(got["bins"], wb, "the replay: the bins hold the pruned log"); _bits(got["dropped"], wd, "the replay: dropped")
        ub, ud = np.zeros_like(wb), np.zeros_like(wd)
        CS.rebin(list(fl._obs), [7], np.asarray(TE.LOOP_CENT, dtype=np.float64), second, ub, ud)
        assert ub[..., 0].sum() > wb[..., 0].sum()                    # the pruned records are in no bin
        D, _, n_used, status = PS.rdrv(want["records"], 7, LD)
        assert got["rdrv_info"].tolist() == [n_used, 0] == [int(want["info"][2]), 0] and got["rdrv_installed"].tolist() == [1, 1, 1]
        _drag_close(got["rdrv"], want["records"], "the replay: the drag")
        assert np.abs(got["rdrv"] + 0.25).max() < 0.05 and status == 0
        _bits(np.diag(fl.learned_rdrv()), got["rdrv"], "learned_rdrv")
        assert not np.array_equal(got["rdrv"], eager_first["rdrv"])
        # the same chain, eager, on the same data: the same bits
        fl.log.copy_(_dev(second))
        chain()
        for k, v in state().items():
            _bits(v, got[k], "eager against the replay: " + k)
    finally:
        fl.close()


# ---- 5. refusals and no-ops ---------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_no_ops():
    import torch
    M = 100
    dev = Dev(M)
    L = dev.L
    full = dev.load(PS.records("heavy", M, seed=1))
    dev.info.fill_(4); dev.counts.fill_(4); dev.edges.fill_(4.0); dev.partial.fill_(4.0); dev.rinfo.fill_(4); dev.d.fill_(4.0)
    arrays = lambda: [_p(dev.partial), _p(dev.edges), _p(dev.counts), _p(dev.info)]
    call = lambda M_, cap, n, t, rec=True, arrs=None: L.admpc_quad_records_prune(0, M_, _p(dev.rec) if rec else None, cap, n, t, *(arrs or arrays()), _stream())
    bad = [(-1, "number of records"), (0, "n_bins"), (float("nan"), "thresh"), (-1.0, "x_cap")]
    for i in range(4):                                               # everything from refusal i on is wrong: i is reported
        a = [M, 40, 0.001, 16.0]
        for j in range(i, 4):
            a[j] = bad[j][0]
        assert call(a[0], a[3], a[1], a[2], rec=False) == -1 and bad[i][1].encode() in L.admpc_last_error(), i
    assert call(2 ** 31, 16.0, 40, 0.001) == -1 and call(M, 16.0, 257, 0.001) == -1 and call(M, 16.0, 40, 1.5) == -1 and call(M, 0.0, 40, 0.001) == -1
    assert call(M, 16.0, 40, 0.001, rec=False) == -1 and b"null array" in L.admpc_last_error()
    for k in range(4):
        arrs = arrays(); arrs[k] = None
        assert call(M, 16.0, 40, 0.001, arrs=arrs) == -1 and b"null array" in L.admpc_last_error()
    fit = lambda M_, axes, arrs: L.admpc_quad_rdrv_fit(0, M_, axes, *arrs, _stream())
    farr = lambda: [_p(dev.rec), _p(dev.rpartial), _p(dev.d), _p(dev.sums), _p(dev.rinfo)]
    assert fit(-1, 0, [None] * 5) == -1 and b"number of records" in L.admpc_last_error()
    assert fit(M, 0, [None] * 5) == -1 and b"axes" in L.admpc_last_error() and fit(M, 8, farr()) == -1
    for k in range(5):
        arrs = farr(); arrs[k] = None
        assert fit(M, 7, arrs) == -1 and b"null array" in L.admpc_last_error()
    # the no-ops: M == 0 with every array null, and with arrays that must stay as they are
    assert call(0, float("inf"), 1, 0.0, rec=False, arrs=[None] * 4) == 0 and call(0, 16.0, 256, 1.0) == 0 and fit(0, 7, [None] * 5) == 0 and fit(0, 1, farr()) == 0
    _bits(_host(dev.rec), full, "the records after the refusals and the no-ops")
    assert (_host(dev.info) == 4).all() and (_host(dev.counts) == 4).all() and (_host(dev.edges) == 4.0).all() and (_host(dev.partial) == 4.0).all()
    assert (_host(dev.rinfo) == 4).all() and (_host(dev.d) == 4.0).all()
    # the fleet refuses before a launch
    fl = _log_fleet(5, 2)
    try:
        for call_ in (fl.prune_log, fl.fit_rdrv):
            with pytest.raises(ValueError, match="the log is empty"):
                call_()
        fl.log_count = 2
        for kw in (dict(bins=0), dict(bins=257), dict(thresh=1.5), dict(x_cap=0.0)):
            with pytest.raises(ValueError):
                fl.prune_log(**kw)
        with pytest.raises(ValueError):
            fl.fit_rdrv(axes=(6,))
        assert _host(fl.prune_info).tolist() == [0] * 8 and _host(fl.rdrv_info).tolist() == [0, 0]
    finally:
        fl.close()
    nolog, drag = _log_fleet(5, 0), _log_fleet(5, 2, rdrv_d_mat=np.diag([0.1, 0.1, 0.0]))
    try:
        with pytest.raises(ValueError, match="keeps no log"):
            nolog.prune_log()
        with pytest.raises(ValueError, match="keeps no log"):
            nolog.fit_rdrv()
        drag.log_count = 2
        with pytest.raises(ValueError, match="non-zero rdrv_d_mat"):
            drag.fit_rdrv()
        assert torch.cuda.is_available()
    finally:
        nolog.close(); drag.close()


# ---- 6. flights ---------------------------------------------------------------------------------------------------------------------------------

def _flight(**kw):
    """The setting of tests/test_quad_clusters_gpu.py's closing test -- B = 64, N = 10, circles of 5 m at 2, 3, 4 and 5 m/s, drag on, 60
    steps -- as a K = 1 fleet with log_steps = 60."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, B, T = 10, 64, 60
    dt = 1.0 / (N * 5)
    trajs = [circle_reference(T + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
    traj_of = (np.arange(B) % 4).astype(np.int32)
    idx0 = (np.arange(B) // 4).astype(np.int32)
    ref = np.concatenate([[QL.body_velocity(trajs[k][0][i + t])[0] for t in range(T)] for k, i in zip(traj_of, idx0)])
    learn = [[VX(ref.min() - 0.5, ref.max() + 0.5)] + [dict(d) for d in QL.EXP_LEARN[1:]]]
    fl = TE._fleet(B, N, trajs, traj_of, idx0, None, centroids=[[float(np.median(ref))]], feats=[7], learn=learn, log_steps=T, **kw)
    return fl, traj_of, idx0, T, B


def test_a_noisy_flight_is_pruned_before_it_is_clustered_and_fitted():
    """The reference's default data collection, noisy and motor_noise both on: rollout(observe, log) -> prune_log() -> fit_clusters() ->
    fit_gp().  The device's flags equal the spec's on the downloaded log, something is pruned, and the bins the GPs are fitted to are the
    re-bin of the PRUNED log, bit for bit.
    Measured on the MI355X: 3827 of the 3840 records kept (3 pruned by axis 1, 10 by axis 2, none by the cap or the norm); the smallest
    relative distance of a bin ratio to thresh is 0.0417 (4 / 3840 against 0.001)."""
    from ad_mpc_amd.quad_config import SimQuad
    fl, traj_of, idx0, T, B = _flight(quad=SimQuad(drag=True, noisy=True, motor_noise=True), noise_seed=5)
    try:
        fl.rollout(T, observe=True, log=True)
        flown = _host(fl.log).reshape(-1, PS.REC).copy()
        info = fl.prune_log()
        want = PS.prune(flown, 16.0, 40, 0.001)
        assert want["margin"] > 1e-6
        got = _host(fl.log).reshape(-1, PS.REC)
        print("noisy flight: info %s, kept share %.4f, margin %.3g" % (_host(info).tolist(), want["info"][2] / max(1, want["info"][1]), want["margin"]))
        _bits(got, want["records"], "the flags of the pruned flight"); _bits(_host(info), want["info"], "info")
        _bits(_host(fl.prune_counts), want["counts"], "counts")
        assert want["info"][0] == 0 and 0 < want["info"][2] < want["info"][1] <= T * B
        ginfo, perm, installed = fl.fit_clusters()
        fit_info, gp_installed = fl.fit_gp(min_count=2)
        assert _host(ginfo).tolist()[2:] == [0, int(want["info"][2])]       # the EM saw the kept records and no others
        cent = fl.learned_clusters().means
        wb, wd = np.zeros((1, 3, 32, 5)), np.zeros((1, 4), dtype=np.int32)
        CS.rebin(list(fl._obs), [7], fl.centroids, want["records"].reshape(T, B, PS.REC), wb, wd)
        _bits(_host(fl.bins), wb, "the bins the GPs were fitted to: the pruned log"); _bits(_host(fl.dropped), wd, "dropped")
        ub, ud = np.zeros_like(wb), np.zeros_like(wd)
        CS.rebin(list(fl._obs), [7], fl.centroids, flown.reshape(T, B, PS.REC), ub, ud)
        assert ub[..., 0].sum() > wb[..., 0].sum() and wd[0, 3] == ud[0, 3] + (want["info"][1] - want["info"][2])
        assert np.isfinite(cent).all() and (_host(gp_installed) == 1).all()
    finally:
        fl.close()


def test_a_flight_learns_its_linear_drag_and_flies_better():
    """Without noise: rollout(observe, log) -> fit_rdrv() -> reset -> rollout.  Only learned < nominal is asserted; the metres and the
    coefficients are printed.
    Measured on the MI355X: nominal 532.879 m (the figure of tests/test_quad_clusters_gpu.py's flight), 145.861 m with the drag
    -0.5444 / -0.5400 / -0.1047 learned from the first pass."""
    fl, traj_of, idx0, T, B = _flight()
    try:
        fl.rollout(T, observe=True, log=True)
        nominal = float(_host(fl.tally)[:, 0].sum())
        d, info, installed = fl.fit_rdrv()
        log = _host(fl.log).reshape(-1, PS.REC)
        want = PS.rdrv(log, 7, LD)
        assert _host(info).tolist() == [want[2], 0] and _host(installed).tolist() == [1]
        _drag_close(_host(d), log, "the drag of the flight")
        D = fl.learned_rdrv()
        assert D.shape == (3, 3) and np.array_equal(np.diag(np.diag(D)), D) and np.array_equal(np.diag(D), _host(d))
        fl.reset(traj_of, idx0)
        fl.rollout(T)
        learned = float(_host(fl.tally)[:, 0].sum())
        print("sum of |e| over %d steps of %d vehicles: nominal %.6g m, with the RDRv drag %s learned from the first pass %.6g m"
              % (T, B, nominal, np.diag(D).tolist(), learned))
        assert (_host(fl.counts) == [T, 0, 0]).all() and np.isfinite([nominal, learned]).all() and learned < nominal
    finally:
        fl.close()
