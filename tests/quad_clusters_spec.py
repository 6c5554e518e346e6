"""The Gaussian-mixture EM, the install and the re-bin of include/admpc_quad_clusters.h restated in numpy (TEST INFRASTRUCTURE), built on
tests/quad_ensemble_spec.py.

The state is the header's: gmm float64 [1 + K, 18] and info int32 [4].  The formulas are the device's -- hard responsibilities from the
nearest initial mean at the start, sklearn's full-covariance log-density through the precision's Cholesky factor, the moments taken about
the CURRENT mean and shifted in the M step, the 3 x 3 Cholesky written out -- but the sums over the records are numpy's, whose order is
its own: the order inside the sums is not part of the contract.  tests/test_quad_clusters_cpu.py pins this file to
sklearn.mixture.GaussianMixture, the class the reference calls."""
import numpy as np

import quad_ensemble_spec as ES
import quad_learn_spec as QL

ROW, PARTIAL, BLOCKS_MAX, ENOVALID, REC = 18, 81, 256, -100, ES.REC
TINY = 10.0 * 2.0 ** -52
LOG_2PI = float(np.log(2.0 * np.pi))
TRI = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])          # where entry (i, j) of a symmetric 3 x 3 sits among its six stored values


def pack(records, feats):
    """packed float64 [M, 4]: (z_0, z_1, z_2, flag), the features past d at 0; a record counts (flag 1) if its own flag is 1.0 and its d
    features are finite, and its row is zero otherwise."""
    S = np.asarray(records, dtype=np.float64).reshape(-1, REC)
    out = np.zeros((S.shape[0], 4))
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
    S = np.zeros((K, 10))
    for k in range(K):
        D = x - means[k]
        rD = r[:, k, None] * D
        S[k, 0], S[k, 1:4] = r[:, k].sum(), rD.sum(axis=0)
        S[k, 4:10] = [(rD[:, i] * D[:, j]).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return S


def _m_step(gmm, info, S, lse_sum, means, d, n_valid, tol, reg, start):
    """The M kernel, in place; returns False where it failed (the state then stays)."""
    K = S.shape[0]
    rows, bad = np.zeros((K, ROW)), []
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
    """The start step, in place: hard responsibilities from the nearest initial mean (quad_ensemble_spec.nearest's rule: ties to the
    lower index), one M step."""
    init = np.asarray(init, dtype=np.float64).reshape(-1, d)
    K = init.shape[0]
    x = packed[packed[:, 3] == 1.0, :3]
    if x.shape[0] == 0:
        info[:] = 0, 0, ENOVALID, 0
        return False
    means = np.zeros((K, 3)); means[:, :d] = init
    r = np.zeros((x.shape[0], K))
    r[np.arange(x.shape[0]), nearest_rows(x[:, :d], init)[0]] = 1.0
    return _m_step(gmm, info, _moments(x, r, means), 0.0, means, d, float(x.shape[0]), 0.0, reg_covar, True)


def iterate(packed, d, tol, reg_covar, gmm, info):
    """One EM iteration, in place; nothing once converged or a status is set."""
    if info[1] or info[2]:
        return False
    x = packed[packed[:, 3] == 1.0, :3]
    K = gmm.shape[0] - 1
    means = gmm[1:, 1:4].copy()
    lp = np.zeros((x.shape[0], K))
    with np.errstate(all="ignore"):
        for k in range(K):
            P = gmm[1 + k, 10:16][TRI] * np.triu(np.ones((3, 3)))
            y = (x - means[k]) @ P
            lp[:, k] = (np.log(gmm[1 + k, 0]) + gmm[1 + k, 16] - 0.5 * d * LOG_2PI) - 0.5 * (y * y).sum(axis=1)
        mx = lp.max(axis=1)
        lse = mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1))
        r = np.exp(lp - lse[:, None])
    return _m_step(gmm, info, _moments(x, r, means), lse.sum(), means, d, gmm[0, 2], tol, reg_covar, False)


def fit(records, feats, init, max_iter=100, tol=1e-3, reg_covar=1e-6, gmm=None, info=None, resume=False):
    """admpc_quad_clusters_fit: (gmm [1 + K, 18], info int32 [4])."""
    d = len(feats)
    packed = pack(records, feats)
    if not resume:
        K = np.asarray(init).reshape(-1, d).shape[0]
        gmm = np.zeros((1 + K, ROW)) if gmm is None else gmm
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


FIXTURES = ((1, 2), (2, 3), (3, 4))                       # (d, K) of the fits the CPU test pins to sklearn and the GPU tests reuse
FIXTURE_FEATS = {1: [7], 2: [7, 8], 3: [7, 8, 9]}
