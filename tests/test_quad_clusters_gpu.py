"""The centroids of a clustered GP ensemble found on the device (include/admpc_quad_clusters.h; ad_mpc_amd/quad_ensemble_fleet.py) on the
GPU, against the numpy spec of tests/quad_clusters_spec.py, which tests/test_quad_clusters_cpu.py pins to sklearn's GaussianMixture: one EM
iteration and whole fits, determinism, the failures, the install, the log and the re-bin, the refusals, and a short closed loop that
learns its clusters and their GPs from its own flight.

One iteration runs on every instantiation of the E kernel (K = 1 .. 8) and on every shape of the M kernel's row reduction; the fixtures
that are not easy (quad_clusters_spec.hard) are held to the spec in numpy.longdouble, within ten times the gap between that and the spec
in float64; and after every such fit the device's own state is asked what needs no spec (_statements)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import quad_clusters_spec as CS
import quad_ensemble_spec as ES
import quad_learn_spec as QL
import test_quad_ensemble_gpu as TE
import test_quad_fleet_gpu as TQ

pytestmark = pytest.mark.gpu

_dev, _p, _host, _bits, _stream = TQ._dev, TQ._p, TQ._host, TQ._bits, TQ._stream
VX = TE.VX
SIZES = (1, 63, 64, 65, 256, 257, CS.BLOCKS_MAX * 256 + 1)         # the last is past the grid, into the stride loop
LD = np.longdouble
E_KERNEL_K = (1, 2, 3, 4, 5, 6, 7, 8)                               # the instantiations of admpc_quad_gmm_e_kernel<K, START>, each run at d = 3
ONE_ITERATION = [(d, K) for d in (1, 2) for K in (1, 2, 3, 8)] + [(3, K) for K in E_KERNEL_K]
# the M kernel adds the rows of partial sixteen at a time, then a tail: no full group; one and no tail; one and a tail of 1; a tail of 15;
# two and a tail of 1; fifteen and a tail of 15.  M = 256 nblk - 3: the last block is not full
ROW_COUNTS = (15, 16, 17, 31, 33, 255)
PAD = 8                                                             # rows of packed behind the records, which no kernel may touch


@pytest.fixture(autouse=True)
def _needs_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def handle():
    """One quadrotor handle: an ensemble that only clusters may name the same handle K times."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config
    s = QuadBatchSolver(default_quad_config())
    yield s
    s.close()


class Ens:
    """admpc_quad_ensemble_create over K copies of one handle, with the scratch of a fit of up to M records."""

    def __init__(self, handle, K, feats, cent, M):
        import torch
        self.L, self.K, self.d, self.feats = handle.lib, K, len(feats), list(feats)
        self.h = C.c_void_p(0)
        cent = np.ascontiguousarray(cent, dtype=np.float64)
        rc = self.L.admpc_quad_ensemble_create((C.c_void_p * K)(*[handle._h] * K), K, self.d, (C.c_int32 * self.d)(*feats),
                                               cent.ctypes.data_as(C.POINTER(C.c_double)), None, C.byref(self.h))
        assert rc == 0, self.L.admpc_last_error()
        z = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda:0")
        self.packed, self.partial = z(max(M, 1) + PAD, 4), z(CS.BLOCKS_MAX, CS.PARTIAL)
        self.gmm, self.info = z(1 + K, CS.ROW), z(4, dtype=torch.int32)
        self.perm, self.installed, self.cent = z(K, dtype=torch.int32), z(1, dtype=torch.int32), z(K, self.d)

    def fit(self, rec, init=None, max_iter=100, tol=1e-3, reg=1e-6, resume=0, M=None):
        M = rec.shape[0] if M is None else M
        rc = self.L.admpc_quad_clusters_fit(self.h, max_iter, tol, reg, resume, M, _p(rec), _p(init), _p(self.packed), _p(self.partial), _p(self.gmm),
                                            _p(self.info), _stream())
        assert rc == 0, self.L.admpc_last_error()

    def install(self):
        rc = self.L.admpc_quad_clusters_install(self.h, _p(self.gmm), _p(self.info), _p(self.perm), _p(self.installed), _stream())
        assert rc == 0, self.L.admpc_last_error()
        return _host(self.perm).tolist(), int(_host(self.installed)[0]), self.centroids()

    def centroids(self):
        assert self.L.admpc_quad_ensemble_centroids_get(self.h, _p(self.cent), _stream()) == 0
        return _host(self.cent).copy()

    def state(self):
        return _host(self.gmm).copy(), _host(self.info).copy()

    def poison(self, M):
        """NaN wherever a fit of M records has nothing to read: all of partial, which the E kernel writes before the M kernel reads, and
        packed behind row M."""
        self.partial.fill_(float("nan")); self.packed[M:].fill_(float("nan"))

    def untouched(self, M, what):
        """After a fit that ran its E kernel: the first nblk rows of partial hold 10 K + 1 sums each and nothing else was written."""
        nblk, ne = min(-(-M // 256), CS.BLOCKS_MAX), 10 * self.K + 1
        partial, packed = _host(self.partial), _host(self.packed)
        assert np.isfinite(partial[:nblk, :ne]).all() and np.isnan(partial[:nblk, ne:]).all() and np.isnan(partial[nblk:]).all(), what
        assert np.isnan(packed[M:]).all() and packed[M:].shape[0] >= PAD and np.isfinite(packed[:M]).all(), what

    def close(self):
        self.L.admpc_quad_ensemble_destroy(self.h)


@functools.lru_cache(maxsize=None)
def _blobs(d, nb, n, seed):
    return CS.blobs(d, nb, n=n, seed=seed)                          # drawn once; _records copies what it changes


def _records(d, K, M, seed=0):
    """The first M records of a fixture of max(K, 2) blobs, with a cleared flag, a NaN and an infinite feature sprinkled in (M >= 63);
    poor initial means; the range of every feature over the WHOLE fixture, which the tolerances scale with."""
    nb = max(K, 2)
    rec, init = _blobs(d, nb, -(-SIZES[-1] // nb), seed)
    span = np.ptp(rec[:, :d], axis=0)
    rec = rec[:M].copy()
    if M >= 63:
        rec[5::17, 13] = 0.0
        rec[7::29, 0] = np.nan
        rec[11::31, d - 1] = np.inf
        rec[13::37, d if d < 3 else 5] = np.nan                    # an entry the clustering does not read: the record counts
    return rec, init[:K].copy(), span


def _close(got, want, d, span, scale, what, bound=True):
    """Means within scale x the feature's range, covariances within scale x range^2, weights within scale, the bound within
    scale x (1 + |bound|); n_valid and the flags exact."""
    (gg, gi), (wg, wi) = got, want
    assert gi.tolist() == wi.tolist(), (what, gi, wi)
    gw, gm, gc, _ = CS.unpack(gg, d)
    ww, wm, wc, _ = CS.unpack(wg, d)
    em, ec = np.abs(gm - wm) / span, np.abs(gc - wc) / np.outer(span, span)
    ew, eb = np.abs(gw - ww).max(), (abs(gg[0, 0] - wg[0, 0]) / (1.0 + abs(wg[0, 0])) if np.isfinite(wg[0, 0]) else float(gg[0, 0] != wg[0, 0]))
    print("%s: means %.2e covariances %.2e weights %.2e bound %.2e (of ranges; bound %.3f)" % (what, em.max(), ec.max(), ew, eb, wg[0, 0]))
    assert em.max() <= scale and ec.max() <= scale and ew <= scale and (eb <= scale or not bound), what
    assert gg[0, 2] == wg[0, 2] == wi[3], what


# ---- 1. one iteration from a given state -------------------------------------------------------------------------------------------------

def _held(got, lo, hi, d, span, present, what):
    """The device's state against the spec in longdouble (hi), each of means, covariances, weights and the bound within
    max(present, 10 x the gap between the spec in float64 (lo) and hi) in the scaling of _close; info and n_valid the float64 spec's,
    exactly.  The factor 10 is hyper_spec's and tests/test_learn_gpu.py's: two correct orders of evaluation differ by a small multiple of
    that gap.  Prints, and returns, (gap, distance, ratio) per quantity."""
    (gg, gi), (wg, wi) = got, lo
    assert gi.tolist() == wi.tolist() == hi[1].tolist(), (what, gi, wi, hi[1])
    gap, dist = CS.scaled_gap(wg, hi[0], d, span), CS.scaled_gap(gg, hi[0], d, span)
    allowed = np.maximum(present, 10.0 * gap)
    for q, g, e, a in zip(("means", "covariances", "weights", "bound"), gap, dist, allowed):
        print("%s: %-11s gap %.2e device %.2e ratio %s allowed %.2e" % (what, q, g, e, "%.2f" % (e / g) if g > 0.0 else "-", a))
    assert (dist <= allowed).all(), (what, dist, allowed)
    assert gg[0, 2] == wg[0, 2] == wi[3], what
    return gap, dist


def _product(gmm):
    """max |P' Sigma P - I| over the components of a float64 state, the product formed in longdouble: what is left is the rounding of the
    stored state and whatever the factor does not owe to its covariance."""
    worst = 0.0
    for g in np.asarray(gmm, dtype=np.float64)[1:].astype(LD):
        P, S = g[10:16][CS.TRI] * np.triu(np.ones((3, 3))), g[4:10][CS.TRI]
        worst = max(worst, float(np.abs(P.T @ S @ P - np.eye(3)).max()))
    return worst


def _statements(got, hi, d, what):
    """What a state the device left says about itself, whatever the spec: the N_k add up to the records that count (plus the K guards of
    10 eps) within K units in the last place of n_valid, the weights to that sum over n_valid to the same figure; g[16] is the sum of the
    logs of the stored factor's diagonal, bit for bit in numpy's order or within 3 units in the last place of its largest term (each
    log is good to one); P' Sigma P is the identity within 10 x what the state of the longdouble spec, rounded to float64, leaves of it
    -- that reference taken as no less than 2^-52, below which a state stored in float64 falls by chance alone (one component in one
    feature has a single entry); the rows of a feature that is not there are the identity's."""
    gg, gi = got
    K, n_valid = gg.shape[0] - 1, gg[0, 2]
    assert gi[2] == 0 and n_valid == gi[3] > 0, what
    N = gg[1:, 17].astype(LD).sum()
    assert abs(float(N - (LD(n_valid) + K * LD(CS.TINY)))) <= K * np.spacing(n_valid), (what, N, n_valid)
    assert abs(float(gg[1:, 0].astype(LD).sum() - N / LD(n_valid))) <= K * np.spacing(1.0), (what, gg[1:, 0])
    logs = np.log(gg[1:, [10, 13, 15]])
    ulp = np.spacing(np.maximum(np.abs(logs).max(axis=1), np.abs(gg[1:, 16])))
    assert (np.abs(gg[1:, 16] - ((logs[:, 0] + logs[:, 1]) + logs[:, 2])) <= 3.0 * ulp).all(), (what, gg[1:, 16], logs)
    dev, ref = _product(gg), max(_product(hi[0]), 2.0 ** -52)
    print("%s: |P' Sigma P - I| device %.2e, the longdouble spec's state in float64 %.2e" % (what, dev, ref))
    assert dev <= 10.0 * ref, (what, dev, ref)
    g = gg[1:]
    if d < 3:
        assert (g[:, 3] == 0.0).all() and (g[:, [6, 8, 12, 14]] == 0.0).all() and (g[:, [9, 15]] == 1.0).all(), what
    if d < 2:
        assert (g[:, 2] == 0.0).all() and (g[:, [5, 11]] == 0.0).all() and (g[:, [7, 13]] == 1.0).all(), what


def _one_iteration(e, d, K, M):
    """The body of the two tests below at M records: the device's own start plus one iteration, and one iteration from the spec's state
    with resume = 1, both from scratch filled with NaN, both against the float64 spec at the tolerances of the first test's docstring
    and asked _statements against the longdouble spec's iteration of the same state."""
    feats = CS.FIXTURE_FEATS[d]
    rec, init, span = _records(d, K, M)
    packed = CS.pack(rec, feats)
    if K > 1:
        assert CS.nearest_rows(packed[packed[:, 3] == 1.0, :d], init)[1].min() >= 1e-9
    gmm, info = np.zeros((1 + K, CS.ROW)), np.zeros(4, dtype=np.int32)
    assert CS.start(packed, init, d, 1e-6, gmm, info) and info[3] == packed[:, 3].sum() and (M < 63 or info[3] < M)
    drec = _dev(rec)
    # the device's own start, max_iter = 1: start + one iteration
    e.gmm.fill_(3.0); e.info.fill_(5); e.poison(M)
    e.fit(drec, _dev(init), max_iter=1, tol=0.0)
    _bits(_host(e.packed)[:M], packed, "packed, M = %d" % M)
    e.untouched(M, "M %d: the start and one iteration" % M)
    own = e.state()
    # one iteration from the spec's state
    given = gmm.copy()
    e.gmm.copy_(_dev(gmm)); e.info.copy_(_dev(info)); e.poison(M)
    e.fit(drec, None, max_iter=1, tol=0.0, resume=1)
    e.untouched(M, "M %d: one iteration" % M)
    hi = (gmm.astype(LD), info.copy())
    assert CS.iterate(packed.astype(LD), d, 0.0, 1e-6, *hi)
    want = (gmm, info)
    assert CS.iterate(packed, d, 0.0, 1e-6, gmm, info) and info.tolist() == [1, 0, 0, int(packed[:, 3].sum())]
    _close(e.state(), want, d, span, 1e-12, "d %d K %d M %d: one iteration" % (d, K, M))
    _close(own, want, d, span, 1e-12, "d %d K %d M %d: the start and one iteration" % (d, K, M), bound=M > 1)
    _statements(e.state(), hi, d, "d %d K %d M %d: one iteration" % (d, K, M))
    _statements(own, hi, d, "d %d K %d M %d: the start and one iteration" % (d, K, M))
    assert M < 63 or not np.array_equal(given[1:], gmm[1:])                                    # the iteration moved the state


@pytest.mark.parametrize("d,K", ONE_ITERATION)
def test_one_iteration_from_a_given_state_equals_the_spec(handle, d, K):
    """The state the spec's start step leaves is given to the device, which runs one iteration of it with resume = 1; and the start step
    itself.  Tolerance, derived: a responsibility that matters has a log-ratio above -40, so exp gives it to a few tens of units in the
    last place, and the sums of a few 1e4 positive terms keep that; means, weights and the bound therefore lie within about 1e-14 of
    their scale.  Asserted: 1e-12 x the feature's range (range^2 for covariances, 1 + |bound| for the bound), the range being that of
    the fixture whose first M records are used.  n_valid exact.  The device's own start followed by one iteration is held to the same
    figures, but for the bound at M = 1: the covariance of a single point is the regulariser alone, 1e-6, to which the start adds the
    rounding of D D' - s s', about 1e-16 x range^2, and the log-determinant in the bound divides that by the regulariser: an error of
    1e-10 x range^2 there says nothing about the kernel (the means, covariances and weights are held at M = 1 too).
    Every K of e_launch's switch runs at d = 3, in both START flavours (test_every_instantiation_of_the_e_kernel_is_run holds the list
    to the switch); d = 1 and 2 at K = 1, 2, 3 and 8.  The derivation does not depend on K <= 8."""
    e = Ens(handle, K, CS.FIXTURE_FEATS[d], np.zeros((K, d)), SIZES[-1])
    try:
        for M in SIZES:
            _one_iteration(e, d, K, M)
    finally:
        e.close()


@pytest.mark.parametrize("nblk", ROW_COUNTS)
@pytest.mark.parametrize("K", [1, 5, 8])
def test_one_iteration_at_every_shape_of_the_row_reduction(handle, K, nblk):
    """The M kernel's sum over the rows of partial in its general shape -- full groups of sixteen and a tail -- and at the edges of it
    (ROW_COUNTS), at the narrowest, a middle and the widest row (10 K + 1 columns: 11, 51, 81; the last takes a second pass of the
    wave).  SIZES reaches 1, 2 and 256 rows only.  The same checks and tolerances as the test above: its derivation covers M <= 65 537."""
    M = 256 * nblk - 3
    assert min(-(-M // 256), CS.BLOCKS_MAX) == nblk and M <= SIZES[-1]
    e = Ens(handle, K, CS.FIXTURE_FEATS[3], np.zeros((K, 3)), M)
    try:
        _one_iteration(e, 3, K, M)
    finally:
        e.close()


def test_every_instantiation_of_the_e_kernel_is_run():
    """The K the one-iteration test runs at d = 3 are exactly the cases of e_launch's switch; the row counts hold a full group with a tail."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ad_mpc_amd", "csrc", "admpc_quad_clusters.hip")).read()
    switch = re.search(r"switch \(K\) \{([^}]*)\}", src).group(1)
    cases = [int(k) for k in re.findall(r"E_CASE\((\d+)\)", switch)]
    assert cases == list(E_KERNEL_K) == list(range(1, CS.PARTIAL // 10 + 1)) and re.sub(r"E_CASE\(\d+\)|\s", "", switch) == ""
    assert sorted(K for d, K in ONE_ITERATION if d == 3) == cases and len(set(ONE_ITERATION)) == len(ONE_ITERATION)
    assert re.search(r"for \(; r \+ 15 < nblk; r \+= 16\)", src)
    assert any(n > 16 and n % 16 for n in ROW_COUNTS) and all(256 * n - 3 <= SIZES[-1] for n in ROW_COUNTS)


# ---- 2. whole fits ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,K", CS.FIXTURES)
def test_full_fits_equal_the_spec(handle, d, K):
    """The fixtures of the CPU test, sklearn's defaults.  Within 1e-10 x range: four orders over what an independent implementation,
    sklearn, achieves against the spec on the CPU (tests/test_quad_clusters_cpu.py: 7e-15).  Iteration count and converged equal the
    spec's: no change of the bound lies near tol on these fixtures (the CPU test asserts it)."""
    rec, init = CS.blobs(d, K)
    feats, span = CS.FIXTURE_FEATS[d], np.ptp(rec[:, :d], axis=0)
    e = Ens(handle, K, feats, init, rec.shape[0])
    try:
        e.fit(_dev(rec), None)                                                                     # init NULL: the ensemble's present centroids
        want = CS.fit(rec, feats, init)
        assert want[1][1] == 1 and 2 <= want[1][0] < 30
        _close(e.state(), want, d, span, 1e-10, "d %d K %d: whole fit" % (d, K))
        perm, installed, cent = e.install()
        wc, wp, wi = CS.install(want[0], want[1], init)
        assert installed == wi == 1 and perm == wp.tolist() and np.abs(cent - wc).max() <= 1e-10 * span.max()
        assert np.abs(cent[:, 0] - 2.5 * np.arange(K)).max() < 0.15
    finally:
        e.close()


# ---- 2b. the fixtures that are not easy ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hard(name, reg, tol=1e-3, max_iter=CS.HARD_MAX_ITER):
    """The fixture through the spec in float64 and in longdouble, once per module."""
    return CS.hard_run(name, reg, np.float64, tol, max_iter), CS.hard_run(name, reg, LD, tol, max_iter)


@pytest.mark.parametrize("name,reg", CS.HARD_CASES)
def test_hard_fixtures_equal_the_longdouble_spec_within_ten_gaps(handle, name, reg):
    """What a closed loop logs (quad_clusters_spec.hard: overlapping clusters, a spread of the size of reg_covar, an offset 1e6 spreads
    away, nearly dependent features, scales 1e3 apart, outliers, a component without a record): one iteration from the float64 spec's
    start (resume = 1) and the whole fit from the device's own start (tol = 1e-3).  The tolerances of the easy fixtures (1e-12 and
    1e-10 of the scale) are argued for well-conditioned data and do not carry here; each quantity is held to
    max(that, 10 x the gap between the spec in float64 and in longdouble), the distance taken to the longdouble spec (_held).  The gap is
    computed here, from the spec alone.  info equals the float64 spec's: tests/test_quad_clusters_cpu.py holds every change of the
    bound away from tol by 100 gaps.
    Measured on the MI355X: see the table of DESIGN.md's section on the centroids."""
    lo, hi = _hard(name, reg)
    d, K, M, span = lo["d"], lo["K"], lo["rec"].shape[0], lo["span"]
    e = Ens(handle, K, lo["feats"], np.zeros((K, d)), M)
    try:
        drec, what = _dev(lo["rec"]), "%s reg %g" % (name, reg)
        e.gmm.copy_(_dev(lo["given"][0])); e.info.copy_(_dev(lo["given"][1])); e.poison(M)
        e.fit(drec, None, max_iter=1, tol=0.0, reg=reg, resume=1)
        e.untouched(M, what)
        _held(e.state(), lo["one"], hi["one"], d, span, 1e-12, what + ", one iteration")
        _statements(e.state(), hi["one"], d, what + ", one iteration")
        e.gmm.fill_(3.0); e.info.fill_(5); e.poison(M)
        e.fit(drec, _dev(lo["init"]), max_iter=CS.HARD_MAX_ITER, tol=1e-3, reg=reg)
        e.untouched(M, what)
        assert lo["whole"][1][1] == 1 and lo["whole"][1][0] >= 2
        _held(e.state(), lo["whole"], hi["whole"], d, span, 1e-10, what + ", whole fit of %d iterations" % lo["whole"][1][0])
        _statements(e.state(), hi["whole"], d, what + ", whole fit")
        if name == "starved":
            assert e.state()[0][3, 17] == CS.TINY and e.state()[0][3, 1] == 40.0                  # no record, the mean where it was put
    finally:
        e.close()


def test_a_component_without_a_record_and_without_a_regulariser_fails_the_start(handle):
    """`starved` at reg_covar = 0: the third initial mean takes no record, its covariance is zero and its first pivot fails."""
    name, reg = CS.HARD_FAILS
    rec, init = CS.hard(name)
    M = rec.shape[0]
    e = Ens(handle, 3, [7], init, M)
    try:
        e.gmm.fill_(7.0); e.info.fill_(9); e.poison(M)
        e.fit(_dev(rec), None, max_iter=3, reg=reg)
        gmm, info = e.state()
        assert info.tolist() == [0, 0, -3, M] and (gmm == 7.0).all()
        e.untouched(M, "the failed start")
        perm, installed, cent = e.install()
        assert installed == 0 and perm == [0, 1, 2] and np.array_equal(cent, init)
        want = CS.fit(rec, [7], init, max_iter=3, reg_covar=reg, gmm=np.full((4, CS.ROW), 7.0), info=np.full(4, 9, dtype=np.int32))
        assert want[1].tolist() == info.tolist() and np.array_equal(want[0], gmm)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["anisotropic", "overlap"])
def test_without_a_regulariser_the_bound_does_not_decrease(handle, name):
    """EM's bound is monotone, and at reg_covar = 0 the M step maximises exactly: a decrease is rounding.  40 iterations at tol = 0,
    one per resumed call: no change of the bound lies below -10 x the largest gap in `change` between the spec in float64 and in
    longdouble on this fixture (the CPU test: that spec's own never decreases by more than 1e-15 (1 + |bound|)).  One call of 40
    leaves the same bits; the state is held as a whole fit's."""
    lo, hi = _hard(name, 0.0, 0.0, 40)
    d, K, M = lo["d"], lo["K"], lo["rec"].shape[0]
    gap = max(abs(float(a - b)) for a, b in zip(lo["changes"], hi["changes"]))
    assert len(lo["changes"]) == 39 and gap > 0.0
    e = Ens(handle, K, lo["feats"], lo["init"], M)
    try:
        drec, changes = _dev(lo["rec"]), []
        e.gmm.fill_(3.0); e.info.fill_(5); e.poison(M)
        e.fit(drec, None, max_iter=1, tol=0.0, reg=0.0)
        for _ in range(39):
            changes.append(e.state()[0][0, 1])
            e.fit(drec, None, max_iter=1, tol=0.0, reg=0.0, resume=1)
        changes.append(e.state()[0][0, 1])
        stepped = e.state()
        print("%s: smallest change of the bound %.3e on the device, %.3e in float64, %.3e in longdouble; largest gap in change %.3e"
              % (name, min(changes), min(lo["changes"]), float(min(hi["changes"])), gap))
        assert changes[0] == np.inf and stepped[1].tolist() == [40, 0, 0, M]
        assert min(changes[1:]) >= -10.0 * gap, (changes, gap)
        e.gmm.fill_(3.0); e.info.fill_(5); e.poison(M)
        e.fit(drec, None, max_iter=40, tol=0.0, reg=0.0)
        _bits(e.state()[0], stepped[0], "one call of 40 against 40 calls of one"); _bits(e.state()[1], stepped[1], "info")
        e.untouched(M, name)
        _held(stepped, lo["whole"], hi["whole"], d, lo["span"], 1e-10, "%s reg 0, 40 iterations" % name)
        _statements(stepped, hi["whole"], d, "%s reg 0, 40 iterations" % name)
    finally:
        e.close()


# ---- 3. determinism ------------------------------------------------------------------------------------------------------------------------

def test_fits_are_deterministic_resumable_and_capturable(handle):
    import torch
    d, K = 2, 3
    rec, init = CS.blobs(d, K, n=30000)                                                            # 90 000 records: past the grid
    e = Ens(handle, K, CS.FIXTURE_FEATS[d], init, rec.shape[0])
    try:
        drec, dinit = _dev(rec), _dev(init)

        def run(**kw):
            e.gmm.fill_(0.0); e.info.fill_(0); e.partial.fill_(9.0)
            e.fit(drec, dinit, **kw)
            return e.state()

        first, again = run(max_iter=6, tol=0.0), run(max_iter=6, tol=0.0)
        _bits(again[0], first[0], "two runs: gmm"); _bits(again[1], first[1], "two runs: info")
        assert first[1].tolist() == [6, 0, 0, 90000]
        run(max_iter=1, tol=0.0)
        for _ in range(5):
            e.fit(drec, None, max_iter=1, tol=0.0, resume=1)
        _bits(e.state()[0], first[0], "6 x one iteration against one call of 6")
        assert e.state()[1].tolist() == first[1].tolist()
        # iterations behind the convergence change nothing
        short, long_ = run(max_iter=40, tol=1e-3), run(max_iter=80, tol=1e-3)
        assert short[1][1] == 1 and short[1][0] < 40
        _bits(long_[0], short[0], "iterations after convergence: gmm"); _bits(long_[1], short[1], "iterations after convergence: info")
        e.fit(drec, None, max_iter=3, tol=1e-3, resume=1)
        _bits(e.state()[0], short[0], "a resumed call after convergence")
        # captured into a graph
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.fit(drec, dinit, max_iter=6, tol=0.0)
        e.gmm.fill_(0.0); e.info.fill_(0)
        g.replay()
        got = e.state()
        _bits(got[0], first[0], "the replay: gmm"); _bits(got[1], first[1], "the replay: info")
    finally:
        e.close()


# ---- 4. failures -----------------------------------------------------------------------------------------------------------------------------

def test_failures_freeze_the_state_and_the_install_declines(handle):
    same = np.zeros((50, 14)); same[:, 0], same[:, 13] = 1.25, 1.0
    e = Ens(handle, 2, [7], [[4.0], [2.0]], 50)
    try:
        e.gmm.fill_(7.0); e.info.fill_(9)
        e.fit(_dev(same), _dev(np.array([[1.0], [1.0]])), max_iter=3, reg=0.0)
        gmm, info = e.state()
        assert info.tolist() == [0, 0, -1, 50] and (gmm == 7.0).all()                             # component 0 took every point: a zero pivot
        perm, installed, cent = e.install()
        assert installed == 0 and perm == [0, 1] and cent.tolist() == [[4.0], [2.0]]
        # a failure in a later iteration: the state of the iteration before it stays
        rec, init = CS.blobs(1, 2)
        big = Ens(handle, 2, [7], init, rec.shape[0])
        try:
            big.fit(_dev(rec), None, max_iter=2, tol=0.0)
            good = big.state()
            broken = good[0].copy(); broken[2, 0] = np.nan                                        # a weight that is not a number: every sum follows
            big.gmm.copy_(_dev(broken))
            big.fit(_dev(rec), None, max_iter=3, tol=0.0, resume=1)
            gmm, info = big.state()
            assert info.tolist() == [2, 0, -1, 800]
            _bits(gmm, broken, "the state after a failed iteration")
        finally:
            big.close()
        same[:, 13] = 0.0
        e.gmm.fill_(7.0); e.info.fill_(9)
        e.fit(_dev(same), None, max_iter=3)
        gmm, info = e.state()
        assert info.tolist() == [0, 0, CS.ENOVALID, 0] and (gmm == 7.0).all()
        assert e.install()[1] == 0
    finally:
        e.close()


# ---- 5. install ----------------------------------------------------------------------------------------------------------------------------

def test_installed_centroids_route_bin_and_reach_a_captured_rollout():
    import torch
    N, B, steps = 10, 67, 2
    trajs = TQ._circles(N, 3.0)
    traj_of, idx0 = np.zeros(B, dtype=np.int32), ((np.arange(B) * 3) % 100).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=6)
    mk = lambda: TE._fleet(B, N, trajs, traj_of, idx0, x0, centroids=TE.LOOP_CENT, feats=[7], learn=TE.LOOP_LEARN, log_steps=steps)
    fl, eager = mk(), mk()
    try:
        L = fl.lib
        # a mixture by hand: the means arrive sorted along the first feature, ties to the lower component
        state = np.zeros((4, CS.ROW)); state[1:, 1] = [-0.75, -3.0, -0.75]; state[1:, 0] = 1 / 3
        fl.gmm.copy_(_dev(state)); fl.gmm_info.zero_()
        assert L.admpc_quad_clusters_install(fl._ens, _p(fl.gmm), _p(fl.gmm_info), _p(fl.perm), _p(fl.centroids_installed), fl._stream()) == 0
        fl._moved = True
        new = np.array([[-3.0], [-0.75], [-0.75]])
        assert _host(fl.perm).tolist() == [1, 0, 2] and _host(fl.centroids_installed).tolist() == [1]
        assert np.array_equal(fl._device_centroids(), new)
        # set and get round-trip; a value that is not finite is refused on the device
        new = np.array([[-2.9], [-1.1], [0.2]])
        assert _host(fl.set_centroids(new)).tolist() == [1] and np.array_equal(fl._device_centroids(), new)
        bad = _dev(np.array([[0.0], [np.nan], [1.0]])); flag = torch.ones(1, dtype=torch.int32, device="cuda:0")
        assert L.admpc_quad_ensemble_centroids_set(fl._ens, _p(bad), _p(flag), fl._stream()) == 0
        assert _host(flag).tolist() == [0] and np.array_equal(fl._device_centroids(), new)
        # routing from the window
        Y = TE._windows(B, N, [7], new, seed=3)
        fl.yref.copy_(_dev(Y))
        want = ES.route_window(Y, [7], new)
        _bits(_host(fl.route_window()), want, "route_window under the new centroids")
        assert not np.array_equal(want, ES.route_window(Y, [7], TE.LOOP_CENT)) and set(want.tolist()) == {0, 1, 2}
        # the bin kernel: hand-made records re-binned
        rng = np.random.default_rng(5)
        log = rng.normal(size=(steps, B, 14)); log[:, :, 0] = rng.uniform(-4.5, 1.5, (steps, B)); log[:, :, 13] = 1.0; log[1, 3, 13] = 0.0
        assert min(ES.margin(r[[0]], new) for r in log.reshape(-1, 14)) >= 1e-9
        fl.log.copy_(_dev(log)); fl.log_count = steps
        fl.bins.fill_(3.0); fl.dropped.fill_(3)
        fl.rebin()
        wb, wd = np.zeros((3, 3, 32, 5)), np.zeros((3, 4), dtype=np.int32)
        CS.rebin(list(fl._obs), [7], new, log, wb, wd)
        _bits(_host(fl.bins), wb, "bins re-binned under the new centroids"); _bits(_host(fl.dropped), wd, "dropped re-binned")
        ob = np.zeros_like(wb); od = np.zeros_like(wd)
        CS.rebin(list(fl._obs), [7], TE.LOOP_CENT, log, ob, od)
        assert not np.array_equal(ob, wb) and wd[0, 3] == 1
        # a captured rollout flies the centroids installed after the capture
        for f in (fl, eager):
            f.set_centroids(TE.LOOP_CENT); f.reset(traj_of, idx0, x0)
        fl.rollout(2)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fl.rollout(2)
        eager.rollout(2)
        old = TE._state(eager)
        moved = np.array([[-3.2], [-2.0], [-1.2]])
        for f in (fl, eager):
            f.reset(traj_of, idx0, x0); f.set_centroids(moved)
        eager.rollout(2)
        g.replay()
        TE._same_state(TE._state(fl), TE._state(eager), "the replay against the eager rollout under the moved centroids")
        assert not np.array_equal(TE._state(eager)["route"], old["route"])
    finally:
        fl.close(); eager.close()


# ---- 6. the log and the re-bin -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [5, 70])
def test_logged_rollout_equals_the_observed_loop_and_rebin_restores_the_bins(B):
    N, T = 10, 3
    trajs = TQ._circles(N, 3.0)
    traj_of, idx0 = np.zeros(B, dtype=np.int32), ((np.arange(B) * 3) % 100).astype(np.int32)
    x0 = TQ._start(trajs, traj_of, idx0, seed=6)
    whole, loop = (TE._fleet(B, N, trajs, traj_of, idx0, x0, centroids=TE.LOOP_CENT, feats=[7], learn=TE.LOOP_LEARN, log_steps=T + 1) for _ in range(2))
    try:
        whole.samples.fill_(41.0)
        whole.rollout(1, observe=True, log=True)                                                   # the cursor: T more steps behind this one
        whole.log_reset(); whole.observe_reset(); whole.reset(traj_of, idx0, x0)
        whole.log.fill_(0.0)
        whole.rollout(T, observe=True, log=True)
        assert whole.log_count == T and (_host(whole.samples) == 41.0).all()                      # samples: neither read nor written
        loop.observe_latch()
        for t in range(T):
            loop.rollout(1)
            loop.observe()
            _bits(_host(whole.log)[t], _host(loop.samples), "log[%d] against the samples of step %d" % (t, t))
        TE._same_state(TE._state(whole), TE._state(loop), "logged rollout against latch + (step, observe) x T")
        for k in ("bins", "dropped", "_prev"):
            _bits(_host(getattr(whole, k)), _host(getattr(loop, k)), k)
        assert not _host(whole.log)[T].any()
        flown_b, flown_d = _host(whole.bins).copy(), _host(whole.dropped).copy()
        assert flown_b[:, 0, :, 0].sum() + flown_d[:, 0].sum() + flown_d[0, 3] == B * T
        whole.bins.fill_(5.0); whole.dropped.fill_(5)
        whole.rebin()
        _bits(_host(whole.bins), flown_b, "bins after zero and rebin"); _bits(_host(whole.dropped), flown_d, "dropped after zero and rebin")
        with pytest.raises(ValueError, match="do not fit into the log"):
            whole.rollout(2, observe=True, log=True)
        with pytest.raises(ValueError, match="needs observe=True"):
            whole.rollout(1, log=True)
        whole.rollout(1, observe=True, log=True)
        assert whole.log_count == T + 1 and _host(whole.log)[T].any()
    finally:
        whole.close(); loop.close()


# ---- 7. the refusals behind a live handle --------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_and_the_no_ops():
    import torch
    from ad_mpc_amd.quad_3d_optimizer import QuadGPEnsemble
    N, B, T = 10, 5, 2
    trajs = TQ._circles(N, 3.0)
    traj_of, idx0 = np.zeros(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    fl = TE._fleet(B, N, trajs, traj_of, idx0, None, centroids=TE.LOOP_CENT, feats=[7], learn=TE.LOOP_LEARN, log_steps=T)
    flies = TE._fleet(B, N, trajs, traj_of, idx0, None, ensemble=QuadGPEnsemble([[], []], [[0.0], [1.0]], [2]))
    L, null = fl.lib, C.c_void_p(0)
    try:
        def refused(rc, words):
            assert rc == -1 and words in L.admpc_last_error().decode(), (rc, L.admpc_last_error())

        keys = TQ.STATE + ("tally", "route", "bins", "dropped", "samples", "_prev", "log", "gmm", "gmm_info", "perm")
        before = {k: _host(getattr(fl, k)).copy() for k in keys}
        cent0 = fl._device_centroids().copy()
        bad_plant = fl._plant.copy(); bad_plant.substeps = 0

        def logged(**kw):
            a = dict(e=fl._ens, plant=C.byref(fl._plant), B=B, T=T, x=_p(fl.x), model=fl._nominal._h, prev=_p(fl._prev), samples=null, bins=_p(fl.bins),
                     log=_p(fl.log), over=fl.over)
            a.update(kw)
            return L.admpc_quad_ensemble_rollout_log_batch(a["e"], fl._bank, a["plant"], a["over"], a["B"], a["T"], _p(fl.traj_of), _p(fl.idx), a["x"],
                                                           _p(fl.x_opt), _p(fl.w_opt), _p(fl.yref), _p(fl.yref_e), _p(fl.cost), _p(fl.status), _p(fl.iters),
                                                           _p(fl.tally), _p(fl.counts), None, None, _p(fl.route), None, a["model"], a["prev"], a["samples"],
                                                           a["bins"], _p(fl.dropped), None, None, a["log"], fl._stream())
        refused(logged(e=flies._ens, over=0), "created without observe parameters")
        refused(logged(plant=C.byref(bad_plant), model=null), "substeps must be in [1, 1024]")      # the rollout's own, then the null model
        refused(logged(over=0, model=null), "over must be at least 1")
        refused(logged(B=-1, model=null, log=null), "negative batch")
        refused(logged(model=null, log=null), "admpc_quad_ensemble_rollout_log_batch: null model")
        refused(logged(model=null, B=0), "null model")
        refused(logged(over=0, log=null), "over must be at least 1")                                 # with a model: the observed rollout's, then the log
        refused(logged(T=4097, log=null), "T must be in [0, 4096]")
        refused(logged(x=null, log=null), "admpc_quad_rollout_observe_batch: null array")
        refused(logged(prev=null, log=null), "admpc_quad_rollout_observe_batch: null array")
        refused(logged(bins=null, log=null), "admpc_quad_rollout_observe_batch: null array")
        refused(logged(log=null), "admpc_quad_ensemble_rollout_log_batch: null log")
        assert logged(B=0, log=null, x=null) == 0 and logged(T=0, log=null, x=null) == 0

        rec, packed, partial = _p(fl.log), _p(fl._packed), _p(fl._partial)

        def fit(**kw):
            a = dict(e=fl._ens, it=5, tol=1e-3, reg=1e-6, resume=0, M=B * T, rec=rec, init=null, packed=packed, partial=partial, gmm=_p(fl.gmm), info=_p(fl.gmm_info))
            a.update(kw)
            return L.admpc_quad_clusters_fit(a["e"], a["it"], a["tol"], a["reg"], a["resume"], a["M"], a["rec"], a["init"], a["packed"], a["partial"],
                                             a["gmm"], a["info"], fl._stream())
        refused(fit(e=flies._ens, it=0), "clustering features must lie in [7, 16]")
        refused(fit(it=0, tol=-1.0), "max_iter must be in [1, 1000]"); refused(fit(it=1001, tol=np.nan), "max_iter must be in [1, 1000]")
        refused(fit(tol=-1e-9, reg=-1.0), "tol must not be negative"); refused(fit(tol=np.nan, reg=-1.0), "tol must not be negative")
        refused(fit(reg=-1e-9, resume=2), "reg_covar must be finite"); refused(fit(reg=np.inf, resume=2), "reg_covar must be finite")
        refused(fit(reg=np.nan, resume=2), "reg_covar must be finite")
        refused(fit(resume=2, M=-1), "resume must be 0 or 1"); refused(fit(resume=-1, M=-1), "resume must be 0 or 1")
        refused(fit(M=-1, rec=null), "negative number of records")
        for name in ("rec", "packed", "partial", "gmm", "info"):
            refused(fit(**{name: null}), "admpc_quad_clusters_fit: null array")
        assert fit(M=0, rec=null, packed=null, partial=null, gmm=null, info=null) == 0

        inst = lambda g=_p(fl.gmm), i=_p(fl.gmm_info), p=_p(fl.perm), o=_p(fl.centroids_installed): L.admpc_quad_clusters_install(fl._ens, g, i, p, o, fl._stream())
        for kw in (dict(g=null), dict(i=null), dict(p=null), dict(o=null)):
            refused(inst(**kw), "admpc_quad_clusters_install: null array")
        refused(L.admpc_quad_ensemble_centroids_set(fl._ens, null, _p(fl.centroids_installed), fl._stream()), "centroids_set: null array")
        refused(L.admpc_quad_ensemble_centroids_set(fl._ens, _p(fl._cent_dev), null, fl._stream()), "centroids_set: null array")
        refused(L.admpc_quad_ensemble_centroids_get(fl._ens, null, fl._stream()), "centroids_get: null array")

        rebin = lambda e=fl._ens, s=T, b=B, lg=_p(fl.log), bn=_p(fl.bins), dr=_p(fl.dropped): L.admpc_quad_clusters_rebin(e, s, b, lg, bn, dr, fl._stream())
        refused(rebin(e=flies._ens, s=-1), "created without observe parameters")
        refused(rebin(s=-1, lg=null), "negative steps or batch"); refused(rebin(b=-1, lg=null), "negative steps or batch")
        for kw in (dict(lg=null), dict(bn=null), dict(dr=null)):
            refused(rebin(**kw), "admpc_quad_clusters_rebin: null array")
        assert rebin(s=0, lg=null, bn=null, dr=null) == 0 and rebin(b=0, lg=null, bn=null, dr=null) == 0

        # the Python layer, behind a handle
        with pytest.raises(ValueError, match="the log is empty"):
            fl.fit_clusters()
        with pytest.raises(ValueError, match="does not learn"):
            flies.fit_clusters()
        with pytest.raises(ValueError, match="set_centroids: c must be K x len"):
            fl.set_centroids([[0.0], [1.0]])
        with pytest.raises(ValueError, match="not finite"):
            fl.set_centroids([[0.0], [np.nan], [1.0]])
        torch.cuda.synchronize()
        for k in keys:
            _bits(_host(getattr(fl, k)), before[k], "%s after the refusals" % k)
        fl._moved = True
        assert np.array_equal(fl._device_centroids(), cent0)
    finally:
        fl.close(); flies.close()


# ---- 8. a short closed loop -----------------------------------------------------------------------------------------------------------------

def test_a_short_closed_loop_learns_its_clusters_and_their_gps():
    """The setting of tests/test_quad_ensemble_gpu.py's closing test (B = 64, N = 10, circles of 5 m at 2, 3, 4 and 5 m/s, drag on, 60
    observed steps, fit, reset, 60 steps) with K = 3 clusters on the body-frame v_x, but the centroids are NOT taken from the terciles of
    the reference: the fleet starts from poor ones (the 5 %, 15 % and 90 % quantiles), logs its flight, finds its centroids
    (fit_clusters: sklearn's defaults), re-bins, fits its GPs and flies again.  Every cluster bins over the whole range of v_x, since
    cluster c keeps block c wherever its centroid goes.  The device's centroids equal the spec's on the downloaded log within
    1e-10 x range; every cluster holds between 10 % and 80 % of the valid records, by the spec alone too; the summed position error
    lies below the nominal model's.
    Measured on the MI355X: centroids -4.109 / -2.235 / -0.707 from -4.554 / -3.435 / -0.399 after 26 iterations; 12.5 % / 34.8 % / 52.7 %
    of the 3840 records per cluster; summed position error 532.879 m with the nominal model, 120.158 m with the clusters found and
    learned from the first pass (tests/test_quad_ensemble_gpu.py: 120.602 m with centroids given at the terciles of the reference,
    120.645 m unclustered).  Only learned < nominal is asserted."""
    from ad_mpc_amd.quad_scenarios import circle_reference
    N, B, T = 10, 64, 60
    dt = 1.0 / (N * 5)
    trajs = [circle_reference(T + 80, dt, 5.0, v) for v in (2.0, 3.0, 4.0, 5.0)]
    traj_of = (np.arange(B) % 4).astype(np.int32)
    idx0 = (np.arange(B) // 4).astype(np.int32)
    ref = np.concatenate([[QL.body_velocity(trajs[k][0][i + t])[0] for t in range(T)] for k, i in zip(traj_of, idx0)])
    poor = np.quantile(ref, [0.05, 0.15, 0.9]).reshape(3, 1)
    learn = [[VX(ref.min() - 0.5, ref.max() + 0.5)] + [dict(d) for d in QL.EXP_LEARN[1:]] for _ in range(3)]
    fl = TE._fleet(B, N, trajs, traj_of, idx0, None, centroids=poor, feats=[7], learn=learn, log_steps=T)
    try:
        fl.rollout(T, observe=True, log=True)
        nominal = float(_host(fl.tally)[:, 0].sum())
        info, perm, installed = fl.fit_clusters()
        fit_info, gp_installed = fl.fit_gp(min_count=2)
        got = fl.learned_clusters()
        log = _host(fl.log).reshape(-1, 14)
        span = np.ptp(log[log[:, 13] == 1.0, 0])
        gmm, winfo, packed, changes = np.zeros((4, CS.ROW)), np.zeros(4, dtype=np.int32), CS.pack(log, [7]), []
        assert CS.start(packed, poor, 1, 1e-6, gmm, winfo)
        for _ in range(100):
            if CS.iterate(packed, 1, 1e-3, 1e-6, gmm, winfo):
                changes.append(abs(gmm[0, 1]))
        # the stop does not hang on the last places: the bounds of the device and of the spec agree within 1e-10 (1 + |bound|), a change
        # within twice that; no change of this flight comes nearer to tol than 1e-8 (on the way down the changes pass tol slowly, so the
        # band of the CPU fixtures, 0.8 tol .. 1.25 tol, is not to be had here)
        print("changes of the bound: %s" % ["%.6e" % ch for ch in changes])
        assert min(abs(ch - 1e-3) for ch in changes) > 1e-8, changes
        cent, wperm, ok = CS.install(gmm, winfo, poor)
        share = np.bincount(ES.route_records(log[log[:, 13] == 1.0], [7], cent), minlength=3) / float((log[:, 13] == 1.0).sum())
        print("centroids %s from %s after %d iterations (converged %d), shares %s, weights %s" % (fl.centroids.ravel().tolist(), poor.ravel().tolist(),
                                                                                              got.n_iter, got.converged, share.tolist(), got.weights.tolist()))
        assert ok == 1 and _host(installed).tolist() == [1] and got.status == 0 and _host(info).tolist() == winfo.tolist()
        assert got.perm.tolist() == wperm.tolist() and (got.n_iter, int(got.converged)) == (int(winfo[0]), int(winfo[1]))
        assert np.abs(fl.centroids - cent).max() <= 1e-10 * span and np.abs(got.means - gmm[1:, 1:2]).max() <= 1e-10 * span
        assert (share >= 0.1).all() and (share <= 0.8).all(), share
        assert np.array_equal(fl.learned_gps().centroids, fl.centroids) and (np.diff(fl.centroids[:, 0]) > 0).all()
        bins, dropped = _host(fl.bins), _host(fl.dropped)
        wb, wd = np.zeros((3, 3, 32, 5)), np.zeros((3, 4), dtype=np.int32)
        CS.rebin(list(fl._obs), [7], fl.centroids, log.reshape(T, B, 14), wb, wd)
        _bits(bins, wb, "the bins the GPs were fitted to: the log under the learned centroids"); _bits(dropped, wd, "dropped")
        assert _host(fit_info).min() >= 2 and (_host(gp_installed) == 1).all()
        fl.reset(traj_of, idx0)
        fl.rollout(T)
        learned = float(_host(fl.tally)[:, 0].sum())
        print("sum of |e| over %d steps of %d vehicles: nominal %.6g m, with K = 3 clusters found and learned from the first pass %.6g m" % (T, B, nominal, learned))
        assert (_host(fl.counts) == [T, 0, 0]).all() and np.isfinite([nominal, learned]).all() and learned < nominal
    finally:
        fl.close()
