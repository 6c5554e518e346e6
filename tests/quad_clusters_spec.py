"""The Gaussian-mixture EM, the install and the re-bin of include/admpc_quad_clusters.h restated in numpy (TEST INFRASTRUCTURE), built on
tests/quad_ensemble_spec.py.

The state is the header's: gmm float64 [1 + K, 18] and info int32 [4].  The formulas are the device's -- hard responsibilities from the
nearest initial mean at the start, sklearn's full-covariance log-density through the precision's Cholesky factor, the moments taken about
the CURRENT mean and shifted in the M step, the 3 x 3 Cholesky written out -- but the sums over the records are numpy's, whose order is
its own: the order inside the sums is not part of the contract.  tests/test_quad_clusters_cpu.py pins this file to
sklearn.mixture.GaussianMixture, the class the reference calls.

pack, start, iterate, fit and their helpers take the arithmetic as `dtype` (float64 by default), as learn_spec.fit does, so that the same
lines run in float64 and in numpy.longdouble; the gap between the two is the yardstick of the GPU tests on data where a tolerance argued
by hand would not hold (the fixtures of hard() below).  What the device holds as doubles stays those doubles in both: the records, the
initial means, tol, reg_covar, LOG_2PI and TINY.  So does the start's nearest-mean rule, which is a decision, not an approximation."""
import numpy as np

import quad_ensemble_spec as ES
import quad_learn_spec as QL

ROW, PARTIAL, BLOCKS_MAX, ENOVALID, REC = 18, 81, 256, -100, ES.REC
TINY = 10.0 * 2.0 ** -52
LOG_2PI = float(np.log(2.0 * np.pi))
TRI = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])          # where entry (i, j) of a symmetric 3 x 3 sits among its six stored values


def pack(records, feats, dtype=np.float64):
    """packed float64 [M, 4]: (z_0, z_1, z_2, flag), the features past d at 0; a record counts (flag 1) if its own flag is 1.0 and its d
    features are finite, and its row is zero otherwise."""
    S = np.asarray(records, dtype=np.float64).reshape(-1, REC)
    out = np.zeros((S.shape[0], 4), dtype=dtype)
    z = S[:, [f - QL.FEAT0 for f in feats]]
    ok = (S[:, REC - 1] == 1.0) & np.isfinite(z).all(axis=1)
    out[ok, :len(feats)] = z[ok]
    out[ok, 3] = 1.0
    return out


def nearest_rows(x, init):
    """quad_ensemble_spec.nearest for every row of x [n, d] at once: the distance arithmetic in its order, each operation rounded on its
    own, the first smallest distance winning; and the gap to the second nearest [n] (inf for one mean), which the tests hold above 1e-9."""
    dist = np.zeros((x.shape[0], init.shape[0]))
    for c in range(init.shape[0]):
        acc = np.zeros(x.shape[0])
        for j in range(init.shape[1]):
            e = x[:, j] - init[c, j]
            acc = acc + e * e
        dist[:, c] = np.sqrt(acc)
    two = np.sort(dist, axis=1)
    return np.argmin(dist, axis=1), (two[:, 1] - two[:, 0] if init.shape[0] > 1 else np.full(x.shape[0], np.inf))


def _moments(x, r, means):
    """The sums the E kernel's blocks write: S [K, 10] = sum r_k, sum r_k D [3], sum r_k D D' [6], D = x - means[k]."""
    K = means.shape[0]
    S = np.zeros((K, 10), dtype=x.dtype)
    for k in range(K):
        D = x - means[k]
        rD = r[:, k, None] * D
        S[k, 0], S[k, 1:4] = r[:, k].sum(), rD.sum(axis=0)
        S[k, 4:10] = [(rD[:, i] * D[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return S


def _m_step(gmm, info, S, lse_sum, means, d, n_valid, tol, reg, start):
    """The M kernel, in place, in the arithmetic of S; returns False where it failed (the state then stays)."""
    K, dt = S.shape[0], S.dtype.type
    rows, bad, reg = np.zeros((K, ROW), dtype=dt), [], dt(reg)
    with np.errstate(all="ignore"):
        for k in range(K):
            N = S[k, 0] + TINY
            s = S[k, 1:4] / N
            m = means[k] + s
            c = S[k, 4:10] / N - np.array([s[0] * s[0], s[0] * s[1], s[0] * s[2], s[1] * s[1], s[1] * s[2], s[2] * s[2]])
            c[[0, 3, 5]] += reg
            if d < 2:
                m[1], c[1], c[3], c[4] = 0.0, 0.0, 1.0, 0.0
            if d < 3:
                m[2], c[2], c[4], c[5] = 0.0, 0.0, 0.0, 1.0
            p0 = c[0]; l00 = np.sqrt(p0); l10 = c[1] / l00; l20 = c[2] / l00
            p1 = c[3] - l10 * l10; l11 = np.sqrt(p1); l21 = (c[4] - l20 * l10) / l11
            p2 = c[5] - l20 * l20 - l21 * l21; l22 = np.sqrt(p2)
            if not all(p > 0.0 and np.isfinite(p) for p in (p0, p1, p2)):
                bad.append(k)
                continue
            P00, P11, P22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
            P01 = -(l10 * P00) / l11; P12 = -(l21 * P11) / l22; P02 = -(l20 * P00 + l21 * P01) / l22
            rows[k, 0], rows[k, 1:4], rows[k, 4:10] = N / n_valid, m, c
            rows[k, 10:16] = [P00, P01, P02, P11, P12, P22]
            rows[k, 16], rows[k, 17] = np.log(P00) + np.log(P11) + np.log(P22), N
    if bad:
        info[2] = -(bad[0] + 1)
        if start:
            info[0], info[1], info[3] = 0, 0, int(n_valid)
        return False
    lb, change = -np.inf, np.inf
    if not start:
        lb = lse_sum / n_valid
        change = lb - gmm[0, 0]
    gmm[1:] = rows
    gmm[0] = 0.0
    gmm[0, :3] = lb, change, n_valid
    info[0] = 0 if start else info[0] + 1
    info[1] = int((not start) and abs(change) < tol)
    info[2], info[3] = 0, int(n_valid)
    return True


def start(packed, init, d, reg_covar, gmm, info):
    """The start step, in place, in the arithmetic of packed: hard responsibilities from the nearest initial mean
    (quad_ensemble_spec.nearest's rule: ties to the lower index; in float64 whatever the arithmetic), one M step."""
    init = np.asarray(init, dtype=np.float64).reshape(-1, d)
    K = init.shape[0]
    x = packed[packed[:, 3] == 1.0, :3]
    if x.shape[0] == 0:
        info[:] = 0, 0, ENOVALID, 0
        return False
    means = np.zeros((K, 3), dtype=packed.dtype); means[:, :d] = init
    r = np.zeros((x.shape[0], K), dtype=packed.dtype)
    r[np.arange(x.shape[0]), nearest_rows(x[:, :d].astype(np.float64), init)[0]] = 1.0
    return _m_step(gmm, info, _moments(x, r, means), 0.0, means, d, float(x.shape[0]), 0.0, reg_covar, True)


def iterate(packed, d, tol, reg_covar, gmm, info):
    """One EM iteration, in place, in the arithmetic of packed (gmm is of that type); nothing once converged or a status is set."""
    if info[1] or info[2]:
        return False
    x = packed[packed[:, 3] == 1.0, :3]
    K = gmm.shape[0] - 1
    means = gmm[1:, 1:4].copy()
    dt = packed.dtype.type
    lp = np.zeros((x.shape[0], K), dtype=dt)
    with np.errstate(all="ignore"):
        for k in range(K):
            P = gmm[1 + k, 10:16][TRI] * np.triu(np.ones((3, 3)))
            y = (x - means[k]) @ P
            lp[:, k] = (np.log(gmm[1 + k, 0]) + gmm[1 + k, 16] - dt(0.5 * d) * dt(LOG_2PI)) - 0.5 * (y * y).sum(axis=1)
        mx = lp.max(axis=1)
        lse = mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1))
        r = np.exp(lp - lse[:, None])
    return _m_step(gmm, info, _moments(x, r, means), lse.sum(), means, d, gmm[0, 2], tol, reg_covar, False)


def fit(records, feats, init, max_iter=100, tol=1e-3, reg_covar=1e-6, gmm=None, info=None, resume=False, dtype=np.float64):
    """admpc_quad_clusters_fit: (gmm [1 + K, 18] of `dtype`, info int32 [4]).  A gmm that is given is of `dtype`."""
    d = len(feats)
    packed = pack(records, feats, dtype)
    if not resume:
        K = np.asarray(init).reshape(-1, d).shape[0]
        gmm = np.zeros((1 + K, ROW), dtype=dtype) if gmm is None else gmm
        info = np.zeros(4, dtype=np.int32) if info is None else info
        start(packed, init, d, reg_covar, gmm, info)
    for _ in range(int(max_iter)):
        iterate(packed, d, tol, reg_covar, gmm, info)
    return gmm, info


def unpack(gmm, d):
    """(weights [K], means [K, d], covariances [K, d, d], precision factors [K, d, d]) of a state."""
    g = gmm[1:]
    return g[:, 0].copy(), g[:, 1:1 + d].copy(), g[:, 4:10][:, TRI][:, :d, :d].copy(), (g[:, 10:16][:, TRI] * np.triu(np.ones((3, 3))))[:, :d, :d].copy()


def install(gmm, info, cent):
    """admpc_quad_clusters_install: (centroids [K, d], perm int32 [K], installed)."""
    cent = np.asarray(cent, dtype=np.float64)
    K, d = cent.shape
    means = gmm[1:, 1:1 + d]
    if info[2] != 0 or not np.isfinite(means).all():
        return cent.copy(), np.arange(K, dtype=np.int32), 0
    perm = np.array(sorted(range(K), key=lambda k: (means[k, 0], k)), dtype=np.int32)
    return means[perm].copy(), perm, 1


def rebin(blocks, feats, cent, log, bins, dropped):
    """admpc_quad_clusters_rebin, in place: the ensemble's bin kernel once per logged step log[t] ([steps, B, 14]), in order."""
    for step in np.asarray(log, dtype=np.float64):
        ES.accumulate(blocks, feats, cent, step, bins, dropped)


def blobs(d, K, n=400, sigma=0.4, gap=2.5, seed=0):
    """A fixture: K blobs of n points in d features, centres `gap` apart along the first feature, as records [K n, 14] (valid), and
    poor initial means [K, d]."""
    rng = np.random.default_rng(seed + 10 * d + K)
    centres = np.zeros((K, d)); centres[:, 0] = gap * np.arange(K)
    if d > 1:
        centres[:, 1:] = rng.normal(size=(K, d - 1))
    pts = np.concatenate([c + sigma * rng.normal(size=(n, d)) for c in centres])
    pts = pts[rng.permutation(pts.shape[0])]
    rec = rng.normal(size=(pts.shape[0], REC))
    rec[:, :d] = pts
    rec[:, REC - 1] = 1.0
    init = centres + 0.6 * rng.normal(size=centres.shape)
    return rec, init


def _records_of(pts, rng):
    """pts [M, d] shuffled into valid records [M, 14], the entries the clustering does not read random."""
    pts = pts[rng.permutation(pts.shape[0])]
    rec = rng.normal(size=(pts.shape[0], REC))
    rec[:, :pts.shape[1]] = pts
    rec[:, REC - 1] = 1.0
    return rec


# name: (d, K, the reg_covar values the fixture is fitted at)
HARD = {"overlap": (2, 3, (1e-6,)), "hover": (3, 3, (1e-6, 1e-9)), "hover_offset": (3, 3, (1e-9,)), "anisotropic": (3, 2, (1e-9, 0.0)),
        "mixed_scales": (2, 4, (1e-6,)), "outliers": (1, 2, (1e-6,)), "starved": (1, 3, (1e-6,))}
HARD_CASES = tuple((name, reg) for name, (_, _, regs) in HARD.items() for reg in regs)
HARD_FAILS = ("starved", 0.0)                             # the start fails with info[2] = -3: the third component has no record and no regulariser
HARD_MAX_ITER = 200
ANISO = np.array([[1.0, 0.0, 0.0], [0.999, 0.03, 0.0], [0.5, 0.5, 1e-3]])


def hard(name, n=400, seed=0):
    """The fixtures that are not easy, as (records [M, 14], initial means [K, d]): what a closed loop logs and blobs() does not look like.
    overlap       unit-variance blobs 1.5 apart, poor initial means
    hover         rotor activations near the hover value: centres 0.245 + 0.004 k on the diagonal, sigma 1e-3 (variance 1e-6 = reg_covar)
    hover_offset  the same 1e3 away from the origin: the shifted moments against the one-pass ones
    anisotropic   points A n about centres 4 apart, n standard normal: strongly correlated features, the smallest pivot 1e-6
    mixed_scales  sigma 1 with centres 5 apart in the first feature, sigma 1e-3 about 0.25 + 0.01 k in the second
    outliers      two blobs, one record at 500 and one at -800
    starved       two blobs and a third initial mean at 40, which takes no record at the start"""
    d, K, _ = HARD[name]
    rng = np.random.default_rng(seed + 1000 * sorted(HARD).index(name))
    if name == "overlap":
        centres = np.stack([1.5 * np.arange(K), np.array([0.0, 0.6, -0.3])], axis=1)
        pts = np.concatenate([c + rng.normal(size=(n, d)) for c in centres])
        init = centres + 0.8 * rng.normal(size=centres.shape)
    elif name in ("hover", "hover_offset"):
        centres = np.repeat((0.245 + 0.004 * np.arange(K))[:, None], d, axis=1)
        pts = np.concatenate([c + 1e-3 * rng.normal(size=(n, d)) for c in centres])
        init = centres + 1.5e-3 * rng.normal(size=centres.shape)
        if name == "hover_offset":
            pts, init = pts + 1e3, init + 1e3
    elif name == "anisotropic":
        centres = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0]])
        pts = np.concatenate([c + rng.normal(size=(n, d)) @ ANISO.T for c in centres])
        init = centres + 0.5 * rng.normal(size=centres.shape)
    elif name == "mixed_scales":
        centres = np.stack([5.0 * np.arange(K), 0.25 + 0.01 * np.arange(K)], axis=1)
        pts = np.concatenate([c + rng.normal(size=(n, d)) * [1.0, 1e-3] for c in centres])
        init = centres + rng.normal(size=centres.shape) * [1.0, 2e-3]
    elif name == "outliers":
        pts = np.concatenate([rng.normal(size=(n, 1)), 6.0 + rng.normal(size=(n, 1)), [[500.0], [-800.0]]])
        init = np.array([[-1.0], [7.5]])
    else:
        pts = np.concatenate([0.5 * rng.normal(size=(n, 1)), 3.0 + 0.5 * rng.normal(size=(n, 1))])
        init = np.array([[0.4], [2.2], [40.0]])
    return _records_of(pts, rng), init


def hard_run(name, reg_covar, dtype=np.float64, tol=1e-3, max_iter=HARD_MAX_ITER):
    """A hard fixture through the spec in `dtype`, as a dict: rec, init, d, K, feats, span (the range of every feature), margin (the
    smallest nearest-mean margin at the start), given (the state the FLOAT64 start leaves, which the device can be handed), one (that
    state after one iteration in `dtype`), whole (the fit from `dtype`'s own start) and changes (the change of the bound of every
    iteration of the fit that ran, the first, which is infinite, left out).  A state is (gmm, info); one is None where the start fails."""
    d, K, _ = HARD[name]
    rec, init = hard(name)
    feats = FIXTURE_FEATS[d]
    packed = pack(rec, feats, dtype)
    out = dict(rec=rec, init=init, d=d, K=K, feats=feats, span=np.ptp(rec[:, :d], axis=0), one=None, changes=[],
               margin=nearest_rows(pack(rec, feats)[:, :d], init)[1].min())
    given = np.zeros((1 + K, ROW)), np.zeros(4, dtype=np.int32)
    if start(pack(rec, feats), init, d, reg_covar, *given):
        out["one"] = given[0].astype(dtype), given[1].copy()
        assert iterate(packed, d, 0.0, reg_covar, *out["one"])
    gmm, info = np.zeros((1 + K, ROW), dtype=dtype), np.zeros(4, dtype=np.int32)
    start(packed, init, d, reg_covar, gmm, info)
    for _ in range(max_iter):
        if iterate(packed, d, tol, reg_covar, gmm, info) and info[0] > 1:
            out["changes"].append(gmm[0, 1])
    out["given"], out["whole"] = given, (gmm, info)
    return out


def scaled_gap(got, want, d, span):
    """The distance of two states in the scaling of the GPU tests, formed in want's arithmetic: (means / the feature's range,
    covariances / range^2, weights, the bound / (1 + |bound|)), each the largest over its entries."""
    dt = want.dtype.type
    gw, gm, gc, _ = unpack(got.astype(dt), d)
    ww, wm, wc, _ = unpack(want, d)
    span = np.asarray(span, dtype=dt)
    bound = abs(dt(got[0, 0]) - want[0, 0]) / (1.0 + abs(want[0, 0])) if np.isfinite(want[0, 0]) else dt(got[0, 0] != want[0, 0])
    return np.array([(np.abs(gm - wm) / span).max(), (np.abs(gc - wc) / np.outer(span, span)).max(), np.abs(gw - ww).max(), bound], dtype=np.float64)


FIXTURES = ((1, 2), (2, 3), (3, 4))                       # (d, K) of the fits the CPU test pins to sklearn and the GPU tests reuse
FIXTURE_FEATS = {1: [7], 2: [7, 8], 3: [7, 8, 9]}
