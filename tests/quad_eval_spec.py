"""The evaluation of the learned GPs on a log of include/admpc_quad_eval.h restated in numpy (TEST INFRASTRUCTURE), built on
tests/learn_spec.py (the points and K of a fit), tests/hyper_spec.py (a regressor at searched hyperparameters) and
tests/quad_ensemble_spec.py (the routing).

A FACTOR is a dict: n, n_feat, feat [3], out, sigma_f, inv_l2 [3], ymean, Z [n, n_feat], alpha [n], W [n, n] = L^-1 (lower triangular),
info (n, or the fit's failure code), cond = cond_2(K) (1 without points).  It is made by a Cholesky factorisation and forward
substitution on the identity, never by `inv`, in float64 or -- by the dtype argument -- in numpy.longdouble.  `pack` / `unpack` move it
to and from the device's block of 672 doubles, so that the per-record arithmetic can be restated from the DEVICE's factor.

`evaluate` gives, for every record, what the bounds of the tests need next to the outputs: sum_i |k_i alpha_i|, |k|_2 |alpha|_2,
cond_2(K) of the record's regressor, and the margin ||r| - 3 std|."""
import numpy as np

import hyper_spec as HS
import learn_spec as LS
import quad_ensemble_spec as ES

FACTOR, STATS, ENOVALID, NPT, REC, GP_MAX = 672, 8, -100, 32, 14, 3
F_Z, F_ALPHA, F_W = 16, 112, 144
JITTER = 1e-8                                                     # gp.py:427
U = 2.0 ** -53
NO_OPTIMUM = -33
PRUNED = 2.0
LD = np.longdouble


def cholesky(K):
    """(L, 0), or (None, k + 1) where pivot k is not positive and finite; the arithmetic of K's dtype, a column per step."""
    n, dt = K.shape[0], K.dtype.type
    L = np.zeros_like(K)
    for k in range(n):
        with np.errstate(invalid="ignore", over="ignore"):
            d = K[k, k] - (L[k, :k] * L[k, :k]).sum(dtype=dt)
        if not (d > 0 and np.isfinite(d)):
            return None, k + 1
        L[k, k] = np.sqrt(d)
        for r in range(k + 1, n):
            L[r, k] = (K[r, k] - (L[r, :k] * L[k, :k]).sum(dtype=dt)) / L[k, k]
    return L, 0


def solve(L, b):
    """alpha of L L' alpha = b."""
    n, dt = L.shape[0], L.dtype.type
    w, a = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    for k in range(n):
        w[k] = (b[k] - (L[k, :k] * w[:k]).sum(dtype=dt)) / L[k, k]
    for k in range(n - 1, -1, -1):
        a[k] = (w[k] - (L[k + 1:, k] * a[k + 1:]).sum(dtype=dt)) / L[k, k]
    return a


def inverse_lower(L):
    """W = L^-1 by forward substitution on the identity, a row per step: W[r, j] = (delta_rj - sum_{k = j}^{r - 1} L[r, k] W[k, j]) / L[r, r]."""
    n, dt = L.shape[0], L.dtype.type
    W = np.zeros_like(L)
    for r in range(n):
        for j in range(r + 1):
            W[r, j] = ((dt(1.0) if j == r else dt(0.0)) - (L[r, j:r] * W[j:r, j]).sum(dtype=dt)) / L[r, r]
    return W


def empty_factor(feat, out, sigma_f, inv_l2, info=0, dtype=np.float64):
    nf = len(feat)
    return dict(n=0, n_feat=nf, feat=list(feat) + [0] * (3 - nf), out=int(out), sigma_f=np.float64(sigma_f),
                inv_l2=np.array(list(inv_l2)[:nf] + [0.0] * (3 - nf)), ymean=np.float64(0.0), Z=np.zeros((0, nf)), alpha=np.zeros(0, dtype=dtype),
                W=np.zeros((0, 0), dtype=dtype), info=int(info), cond=1.0, L=np.zeros((0, 0), dtype=dtype))


def make_factor(Z, t, ymean, diag, feat, out, sigma_f, inv_l2, dtype=np.float64, finite_targets=True):
    """The factor of the n points Z [n, nf] with targets t, the diagonal `diag` [n] on K = sigma_f exp(-1/2 d^2): Z, t, ymean and the
    hyperparameters are float64 data, the solve runs in `dtype`."""
    Z, t = np.asarray(Z, dtype=np.float64), np.asarray(t, dtype=np.float64)
    n, nf = Z.shape
    f = empty_factor(feat, out, sigma_f, inv_l2, 0, dtype)
    if n == 0:
        return f
    il = np.asarray(inv_l2, dtype=np.float64)[:nf].astype(dtype)
    Zd = Z.astype(dtype)
    with np.errstate(all="ignore"):
        K = dtype(sigma_f) * np.exp(dtype(-0.5) * ((Zd[:, None, :] - Zd[None, :, :]) ** 2 * il).sum(axis=2)) + np.diag(np.asarray(diag).astype(dtype))
    L, failed = cholesky(K)
    bad = [k + 1 for k in range(n) if not np.isfinite(t[k])]
    first = min([failed or n + 1] + bad)                           # the device tests pivot k and point k's target at step k
    if first <= n:
        f["info"] = -first
        return f
    f.update(n=n, ymean=np.float64(ymean), Z=Z, alpha=solve(L, t.astype(dtype) - dtype(ymean)), W=inverse_lower(L), info=n, L=L,
             cond=float(np.linalg.cond(K.astype(np.float64))))
    return f


def factor_from_bins(G, stats, min_count=1, hyper=None, dtype=np.float64):
    """admpc_quad_ensemble_factor for one regressor: G an AdmpcGpBins, stats float64 [32, 5]; hyper None (G's own hyperparameters) or
    the [16] a search left (natural values at 10 .. 14, the best NLL at 15: not finite -> the empty factor, info NO_OPTIMUM)."""
    nf = int(G.n_feat)
    feat = [int(G.feat[d]) for d in range(nf)]
    H = G if hyper is None else HS.with_hyper(G, np.asarray(hyper, dtype=np.float64)[10:15])
    il = LS.inv_l2(H)
    if hyper is not None and not np.isfinite(hyper[15]):
        return empty_factor(feat, int(G.out), H.sigma_f, il, NO_OPTIMUM, dtype)
    Z, t, counts, ymean = LS.points(G, np.asarray(stats, dtype=np.float64), min_count)
    with np.errstate(divide="ignore", invalid="ignore"):
        diag = np.float64(H.noise) + np.float64(G.count_noise) / counts
    return make_factor(Z, t, ymean, diag, feat, int(G.out), H.sigma_f, il, dtype)


def pack(f):
    """The device's block [672] of a factor."""
    b = np.zeros(FACTOR)
    n, nf = f["n"], f["n_feat"]
    b[0], b[1], b[2:5], b[5], b[6], b[7:10], b[10] = n, nf, f["feat"], f["out"], f["sigma_f"], f["inv_l2"], f["ymean"]
    for d in range(nf):
        b[F_Z + d * NPT:F_Z + d * NPT + n] = f["Z"][:, d]
    b[F_ALPHA:F_ALPHA + n] = f["alpha"]
    for i in range(n):
        b[F_W + i * (i + 1) // 2:F_W + i * (i + 1) // 2 + i + 1] = f["W"][i, :i + 1]
    return b


def unpack(b, dtype=np.float64):
    """A factor from a device block: its arrays in `dtype`, their values the block's bits."""
    b = np.asarray(b, dtype=np.float64)
    n, nf = int(b[0]), int(b[1])
    W = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        W[i, :i + 1] = b[F_W + i * (i + 1) // 2:F_W + i * (i + 1) // 2 + i + 1]
    Z = np.stack([b[F_Z + d * NPT:F_Z + d * NPT + n] for d in range(nf)], axis=1) if nf else np.zeros((n, 0))
    return dict(n=n, n_feat=nf, feat=[int(v) for v in b[2:5]], out=int(b[5]), sigma_f=b[6], inv_l2=b[7:10].copy(), ymean=b[10], Z=Z,
                alpha=b[F_ALPHA:F_ALPHA + n].astype(dtype), W=W, info=n, cond=None, L=None)


def predict(f, z, dtype=np.float64):
    """(mu [m], var [m], sum_i |k_i alpha_i| [m], |k|_2 |alpha|_2 [m]) of factor f at z [m, n_feat], var not clipped."""
    z = np.asarray(z, dtype=np.float64).reshape(-1, max(1, f["n_feat"]))[:, :f["n_feat"]].astype(dtype)
    m, n = z.shape[0], f["n"]
    kss = dtype(f["sigma_f"]) + dtype(JITTER)
    if n == 0:
        return np.full(m, dtype(f["ymean"])), np.full(m, kss), np.zeros(m, dtype=dtype), np.zeros(m, dtype=dtype)
    il = np.asarray(f["inv_l2"], dtype=np.float64)[:f["n_feat"]].astype(dtype)
    k = dtype(f["sigma_f"]) * np.exp(dtype(-0.5) * ((z[:, None, :] - f["Z"].astype(dtype)[None, :, :]) ** 2 * il).sum(axis=2))      # [m, n]
    a = f["alpha"].astype(dtype)
    mu = dtype(f["ymean"]) + (k * a).sum(axis=1, dtype=dtype)
    v = k @ f["W"].astype(dtype).T
    var = kss - (v * v).sum(axis=1, dtype=dtype)
    return mu, var, np.abs(k * a).sum(axis=1), np.sqrt((k * k).sum(axis=1)) * np.sqrt((a * a).sum())


def take_part(S, take_pruned=0):
    """(takes part, skipped by flag, skipped as not finite), boolean [M] each."""
    S = np.asarray(S, dtype=np.float64).reshape(-1, REC)
    flag = (S[:, 13] == 1.0) | ((S[:, 13] == PRUNED) & bool(take_pruned))
    fin = np.isfinite(S[:, :13]).all(axis=1)
    return flag & fin, ~flag, flag & ~fin


def distances(z, cent):
    """[m, K]: quad_ensemble_spec.distances for every row of z [m, d], the sum serial from 0, every operation rounded on its own."""
    z, cent = np.asarray(z, dtype=np.float64), np.asarray(cent, dtype=np.float64)
    acc = np.zeros((z.shape[0], cent.shape[0]))
    for j in range(z.shape[1]):
        e = z[:, j:j + 1] - cent[None, :, j]
        acc = acc + e * e
    return np.sqrt(acc)


def route(S, feats, cent):
    """(cluster int32 [M], gap [M] between the two nearest distances: inf for one cluster) of the records' own features, as
    quad_ensemble_spec.route_records (ties to the lower index); for records whose features are finite."""
    S = np.asarray(S, dtype=np.float64).reshape(-1, REC)
    d = distances(S[:, [f - 7 for f in feats]], cent)
    s = np.sort(d, axis=1)
    return np.argmin(d, axis=1).astype(np.int32), (s[:, 1] - s[:, 0] if d.shape[1] > 1 else np.full(d.shape[0], np.inf))


def evaluate(S, feats, cent, factors, take_pruned=0, drag=None, dtype=np.float64):
    """admpc_quad_ensemble_evaluate: S [M, 14], factors [K][n_gp].  A dict: part, route, gap, mu / std / var / res / y / absdot / knorm /
    cond / margin / clipped [M, n_gp] (NaN, False where a record does not take part; mu with the drag term), stats [K, 3, 8], info [4]."""
    S = np.asarray(S, dtype=np.float64).reshape(-1, REC)
    M, K, n_gp = S.shape[0], len(factors), len(factors[0])
    part, by_flag, not_fin = take_part(S, take_pruned)
    r = np.zeros(M, dtype=np.int32)
    gap = np.full(M, np.inf)
    with np.errstate(all="ignore"):
        r[part], gap[part] = route(S[part], feats, cent)
    out = {k: np.full((M, n_gp), np.nan, dtype=dtype) for k in ("mu", "std", "var", "res", "y", "absdot", "knorm", "margin")}
    out["cond"], out["clipped"] = np.full((M, n_gp), np.nan), np.zeros((M, n_gp), dtype=bool)
    stats = np.zeros((K, GP_MAX, STATS), dtype=dtype)
    for c in range(K):
        at = np.nonzero(part & (r == c))[0]
        for g in range(n_gp):
            f = factors[c][g]
            if at.size == 0:
                continue
            z = S[at][:, [f["feat"][d] - 7 for d in range(f["n_feat"])]]
            mu, var, absdot, knorm = predict(f, z, dtype)
            a = f["out"] - 7
            y = S[at, 10 + a].astype(dtype)
            if drag is not None:
                mu = mu + dtype(drag[a]) * S[at, a].astype(dtype)
            std = np.sqrt(np.maximum(var, dtype(0.0)))
            res = y - mu
            out["mu"][at, g], out["std"][at, g], out["var"][at, g], out["res"][at, g], out["y"][at, g] = mu, std, var, res, y
            out["absdot"][at, g], out["knorm"][at, g], out["clipped"][at, g] = absdot, knorm, var < 0
            out["margin"][at, g] = np.abs(np.abs(res) - dtype(3.0) * std)
            if f["cond"] is not None:
                out["cond"][at, g] = f["cond"]
            stats[c, g] = [at.size, np.abs(y).sum(), (y * y).sum(), np.abs(res).sum(), (res * res).sum(), std.sum(),
                           (np.abs(res) <= dtype(3.0) * std).sum(), (var < 0).sum()]
    took = int(part.sum())
    out.update(part=part, route=r, gap=gap, stats=stats, info=np.array([0 if took else ENOVALID, took, by_flag.sum(), not_fin.sum()], dtype=np.int32))
    return out


def stats_of(ev, K):
    """stats [K, 3, 8] recomputed from the per-record outputs of `evaluate` (or of the device: mu, std, y, clipped, route, part)."""
    n_gp = ev["mu"].shape[1]
    stats = np.zeros((K, GP_MAX, STATS), dtype=ev["mu"].dtype)
    for c in range(K):
        at = ev["part"] & (ev["route"] == c)
        for g in range(n_gp):
            y, mu, std = ev["y"][at, g], ev["mu"][at, g], ev["std"][at, g]
            res = y - mu
            stats[c, g] = [at.sum(), np.abs(y).sum(), (y * y).sum(), np.abs(res).sum(), (res * res).sum(), std.sum(),
                           (np.abs(res) <= 3.0 * std).sum(), ev["clipped"][at, g].sum()]
    return stats


# ---- the fixtures of the golden file (tests/gen_quad_eval_golden.py, tests/golden/quad_eval_vectors.json) -----------------------------------
# (seed, n_feat, n, K): the reference's K is homoscedastic, so count_noise = 0 and noise = sigma_n^2
SIGMA_F, SIGMA_N, QUERIES = 0.5, 0.01, 200
GOLDEN_CASES = tuple((100 + i, nf, n, K) for i, (nf, n, K) in enumerate(
    [(1, 1, 1), (1, 2, 1), (1, 31, 1), (1, 32, 1), (2, 1, 3), (2, 2, 1), (2, 31, 3), (2, 32, 1), (3, 1, 1), (3, 2, 3), (3, 31, 1), (3, 32, 3),
     (1, 32, 3), (2, 32, 3), (3, 31, 3), (1, 31, 3)]))


def golden_fixture(seed, nf, n, K):
    """The seeded fixture of a golden case: feats, centroids [K, nf], per cluster (x_train [n, nf], y_train [n], ymean, lengths [nf]),
    and the queries z [200, nf].  Training points lie around their cluster's centroid, spread enough to keep K well conditioned."""
    rng = np.random.default_rng(seed)
    feats = [7, 8, 9][:nf]
    cent = np.sort(rng.uniform(-6.0, 6.0, (K, nf)), axis=0)
    clusters = []
    for c in range(K):
        x = cent[c] + rng.uniform(-3.0, 3.0, (n, nf))
        y = np.sin(x.sum(axis=1)) + 0.3 * x[:, 0] + 0.05 * rng.standard_normal(n)
        total = np.float64(0.0)
        for v in y:
            total = total + v
        clusters.append((x, y, total / np.float64(n), rng.uniform(0.8, 2.5, nf)))
    z = rng.uniform(-9.0, 9.0, (QUERIES, nf))
    return feats, cent, clusters, z


def golden_factors(clusters, feats, dtype=np.float64):
    """One factor per cluster of a golden fixture (regressor 0, out = feats[0])."""
    return [[make_factor(x, y, ym, np.full(len(y), SIGMA_N ** 2), feats, feats[0], SIGMA_F, 1.0 / (l * l), dtype)] for x, y, ym, l in clusters]
