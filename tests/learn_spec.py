"""The record, the binning, the fit and the install check of include/admpc_learn.h restated in numpy (TEST INFRASTRUCTURE), one vehicle or
one regressor at a time.

One `Oracle.rk4_sens(cfg, x, u, p, h)` per sub-step gives the model's prediction (the oracle carries the GP residual of cfg), as in
tests/plant_spec.py, whose blend and inputs are used as they stand.  Every other operation is a single numpy operation in the order the
header states; the sums of a bin run in the lane order of the device.  The fit takes the arithmetic it solves in as an argument, so
that the same lines run in float64 and in numpy.longdouble."""
import ctypes as C

import numpy as np

import plant_spec as PS

WAVE, NPT, REC, ACC, GP_MAX = 64, 32, 10, 5, 4


def record(oracle, cfg, plant, obs, prev, now, ack, mode):
    """One vehicle: (the sample [10], the prediction x^ [7], the state Jacobians of the sub-steps).  cfg: the MODEL's configuration."""
    prev, now = np.array(prev, dtype=np.float64), np.array(now, dtype=np.float64)
    p = PS.blend(prev[3], obs.blend_min, obs.blend_max)
    u = PS.inputs(cfg, plant, ack, mode)
    M = int(obs.substeps)
    h = np.float64(obs.dt) / M
    x, jac = prev.copy(), []
    for _ in range(M):
        x, A, _ = oracle.rk4_sens(cfg, x, u, p, h)
        jac.append(A)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (now[3:6] - x[3:6]) / np.float64(obs.dt)
    rec = np.concatenate([prev[3:7], u, y, [0.0]])
    rec[9] = 1.0 if np.isfinite(rec[:9]).all() else 0.0
    return rec, x, jac


def bin_index(G, z):
    """The bin of the feature values z (one per used feature) under the AdmpcGpBins G, or None outside its box."""
    k = 0
    for d in range(int(G.n_feat)):
        s = np.float64(G.nb[d]) / (np.float64(G.hi[d]) - np.float64(G.lo[d]))
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.float64(z[d]) - np.float64(G.lo[d])) * s
        kd = np.floor(t)
        if not (t >= 0.0 and kd < G.nb[d]):
            return None
        k = k * int(G.nb[d]) + int(kd)
    return k


def accumulate(obs, samples, bins, dropped):
    """admpc_bin_kernel, in place: bins float64 [n_gp.., 32, 5], dropped int32 [5]."""
    samples = np.asarray(samples, dtype=np.float64).reshape(-1, REC)
    for g in range(int(obs.n_gp)):
        G = obs.gp[g]
        nf = int(G.n_feat)
        part = np.zeros((WAVE, NPT, ACC))
        for b, r in enumerate(samples):
            if not r[9] == 1.0:
                dropped[GP_MAX] += 1 if g == 0 else 0
                continue
            z = [r[int(G.feat[d]) - 3] for d in range(nf)]
            k = bin_index(G, z)
            if k is None:
                dropped[g] += 1
                continue
            add = np.zeros(ACC)
            add[0], add[1:1 + nf], add[4] = 1.0, z, r[6 + int(G.out) - 3]
            part[b % WAVE, k] = part[b % WAVE, k] + add
        for lane in range(WAVE):                                        # lane 0 first, onto the stored value
            bins[g] = bins[g] + part[lane]
        n_bins = int(G.nb[0]) * int(G.nb[1]) * int(G.nb[2])
        assert not part[:, n_bins:].any()


def inv_l2(G):
    return np.array([1.0 / (np.float64(G.length[d]) * np.float64(G.length[d])) for d in range(int(G.n_feat))])


def points(G, stats, min_count):
    """(Z [n, nf], t [n], counts [n], ymean) of the bins with count >= min_count, in float64 as the device forms them."""
    nf = int(G.n_feat)
    n_bins = int(G.nb[0]) * int(G.nb[1]) * int(G.nb[2])
    keep = [k for k in range(n_bins) if stats[k, 0] >= min_count]
    with np.errstate(invalid="ignore", divide="ignore"):
        Z = np.array([stats[k, 1:1 + nf] / stats[k, 0] for k in keep], dtype=np.float64).reshape(len(keep), nf)
        t = np.array([stats[k, 4] / stats[k, 0] for k in keep], dtype=np.float64)
    total = np.float64(0.0)
    for v in t:
        total = total + v
    ymean = total / np.float64(len(keep)) if keep else np.float64(0.0)
    return Z, t, stats[keep, 0].astype(np.float64), ymean


def kernel_matrix(G, Z, counts, dtype=np.float64):
    Z = Z.astype(dtype)
    il = inv_l2(G).astype(dtype)
    d2 = ((Z[:, None, :] - Z[None, :, :]) ** 2 * il).sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        diag = dtype(G.noise) + dtype(G.count_noise) / counts.astype(dtype)
    return dtype(G.sigma_f) * np.exp(dtype(-0.5) * d2) + np.diag(diag)


def cholesky_solve(K, b):
    """(alpha, 0) or (None, k + 1) where pivot k is not positive and finite; the arithmetic of K's dtype, a column per step."""
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
    w = np.zeros(n, dtype=dt)
    for k in range(n):
        w[k] = (b[k] - (L[k, :k] * w[:k]).sum(dtype=dt)) / L[k, k]
    a = np.zeros(n, dtype=dt)
    for k in range(n - 1, -1, -1):
        a[k] = (w[k] - (L[k + 1:, k] * a[k + 1:]).sum(dtype=dt)) / L[k, k]
    return a, 0


def fit(G, stats, min_count=1, dtype=np.float64):
    """admpc_gp_fit for one regressor: stats float64 [32, 5].  A dict with n_points, Z, alpha, ymean, info -- the empty GP on failure.
    Z, t and ymean are float64 whatever `dtype`: they are the data of the solve, which runs in `dtype`."""
    Z, t, counts, ymean = points(G, np.asarray(stats, dtype=np.float64), min_count)
    n, nf = len(t), int(G.n_feat)
    empty = dict(n_points=0, Z=np.zeros((0, nf)), alpha=np.zeros(0, dtype=dtype), ymean=np.float64(0.0), info=0)
    if n == 0:
        return empty
    K = kernel_matrix(G, Z, counts, dtype)
    bad = [k for k in range(n) if not np.isfinite(t[k])]
    alpha, failed = cholesky_solve(K, t.astype(dtype) - dtype(ymean))
    first = min([failed or n + 1] + [k + 1 for k in bad])              # the device tests pivot k and point k's target at step k
    if first <= n:
        empty["info"] = -first
        return empty
    return dict(n_points=n, Z=Z, alpha=alpha, ymean=ymean, info=n)


def gp_mean(G, gp, z, dtype=np.float64):
    """The mean of a fitted GP (a dict of fit, or of FleetController.learned_gps) at the points z [m, nf]."""
    z = np.asarray(z, dtype=dtype).reshape(-1, int(G.n_feat))
    Z = np.asarray(gp["Z"], dtype=dtype).reshape(-1, int(G.n_feat))
    if Z.shape[0] == 0:
        return np.full(z.shape[0], dtype(gp["ymean"]))
    d2 = ((z[:, None, :] - Z[None, :, :]) ** 2 * inv_l2(G).astype(dtype)).sum(axis=2)
    return (dtype(G.sigma_f) * np.exp(dtype(-0.5) * d2)) @ np.asarray(gp["alpha"], dtype=dtype) + dtype(gp["ymean"])


def yardstick(G, stats, probes, min_count=1):
    """The largest gap, over the probe points, between the mean of the fit solved in numpy.longdouble and of the fit solved in float64."""
    lo, hi = fit(G, stats, min_count, np.float64), fit(G, stats, min_count, np.longdouble)
    return float(np.abs(gp_mean(G, hi, probes, np.longdouble) - gp_mean(G, lo, probes, np.float64).astype(np.longdouble)).max())


def as_set_gp(G, gp):
    """A dict of fit as config.set_gp takes it."""
    nf = int(G.n_feat)
    return dict(feat=[int(G.feat[d]) for d in range(nf)], out=int(G.out), Z=np.asarray(gp["Z"], dtype=np.float64),
                alpha=np.asarray(gp["alpha"], dtype=np.float64), length_scale=[float(G.length[d]) for d in range(nf)],
                sigma_f=float(G.sigma_f), ymean=float(gp["ymean"]))


def install_ok(gp):
    """The check of admpc_gp_install on an AdmpcGp."""
    nf, n = int(gp.n_feat), int(gp.n_points)
    if not (1 <= nf <= 3 and 3 <= int(gp.out) <= 5 and 0 <= n <= NPT and all(3 <= int(gp.feat[d]) <= 8 for d in range(nf))):
        return False
    nums = [gp.sigma_f, gp.ymean] + [gp.inv_l2[d] for d in range(nf)] + [gp.alpha[i] for i in range(n)] + \
        [gp.Z[d][i] for d in range(nf) for i in range(n)]
    return bool(np.isfinite(np.array(nums, dtype=np.float64)).all())


def hand_stats(G, rng, fill):
    """Statistics of a regressor with `fill` of its bins filled: bin centres jittered, 3 to 9 samples each."""
    nb = [int(G.nb[d]) for d in range(3)]
    stats = np.zeros((32, 5))
    ks = rng.permutation(nb[0] * nb[1] * nb[2])[:fill]
    for k in ks:
        idx = np.unravel_index(k, nb)
        c = float(rng.integers(3, 10))
        z = [G.lo[d] + (idx[d] + rng.uniform(0.3, 0.7)) * (G.hi[d] - G.lo[d]) / nb[d] for d in range(int(G.n_feat))]
        stats[k, 0], stats[k, 1:1 + int(G.n_feat)], stats[k, 4] = c, np.array(z) * c, c * np.sin(3.0 * z[0]) + c * rng.normal() * 0.1
    return stats


# ---- the learning experiment ---------------------------------------------------------------------------------------------------------

EXP_B, EXP_DT, EXP_BAND = 200, 0.05, (100.0, 110.0)
EXP_LEARN = [dict(feat=3, out=3, lo=[2.0], hi=[12.0], bins=[8], length_scale=2.0, sigma_f=1.0, noise=1e-6, count_noise=0.0)]


def truth_gp():
    """The residual of the plant: a GP of 8 points on v_x in [2, 12] acting on the derivative of v_x, of the family that is fitted."""
    Z = np.linspace(2.0, 12.0, 8)
    alpha = np.array([0.8, -0.5, 0.3, 0.6, -0.7, 0.4, 0.2, -0.6])
    return [dict(feat=3, out=3, Z=Z, alpha=alpha, length_scale=2.0, sigma_f=1.0, ymean=0.3)]


def experiment_fleet(seed):
    """(X [200, 7], ack float32 [200, 4], mode [200]): poses and MPC records clear of every clip of the plant step -- speeds inside
    (2.2, 11.8) however the period changes them, steering small and slow, inputs inside their bounds, yaw away from +-pi."""
    rng = np.random.default_rng(seed)
    B = EXP_B
    X = np.stack([rng.uniform(-50, 50, B), rng.uniform(-50, 50, B), rng.uniform(-2.5, 2.5, B), rng.uniform(2.4, 11.6, B),
                  rng.uniform(-0.1, 0.1, B), rng.uniform(-0.05, 0.05, B), rng.uniform(-0.1, 0.1, B)], axis=1)
    ack = np.zeros((B, 4), dtype=np.float32)
    ack[:, 3], ack[:, 1] = rng.uniform(-2.0, 2.0, B), rng.uniform(-0.5, 0.5, B)
    ack[:, 0], ack[:, 2] = X[:, 6], X[:, 3]
    return X, ack, np.ones(B, dtype=np.int32)


def experiment_params():
    from ad_mpc_amd.config import AdmpcObserveParams, AdmpcPlantParams, default_config, learn_bins, set_gp
    bins, n_gp = learn_bins(EXP_LEARN)
    obs = AdmpcObserveParams(dt=EXP_DT, blend_min=EXP_BAND[0], blend_max=EXP_BAND[1], substeps=1, n_gp=n_gp, gp=bins)
    plant = AdmpcPlantParams(dt=EXP_DT, blend_min=EXP_BAND[0], blend_max=EXP_BAND[1], brake_acc=-10.0, v_min=0.0, substeps=1, reserved=0)
    nominal = default_config(N=20)
    truth = set_gp(default_config(N=20), truth_gp())
    return nominal, truth, plant, obs


def experiment(oracle):
    """The spec's run of the experiment: observe 200 steps of the truth against the nominal model, fit, observe 200 fresh steps against
    the learned model.  A dict with the samples before and after, the statistics, the fit and RMS(y_after) / RMS(y_before)."""
    from ad_mpc_amd.config import default_config, set_gp
    nominal, truth, plant, obs = experiment_params()
    G = obs.gp[0]
    out = {}
    model = nominal
    for name, seed in (("before", 101), ("after", 102)):
        X, ack, mode = experiment_fleet(seed)
        now = np.stack([PS.step(oracle, truth, plant, X[b], ack[b], mode[b], clear=True)[0] for b in range(EXP_B)])
        S = np.stack([record(oracle, model, plant, obs, X[b], now[b], ack[b], mode[b])[0] for b in range(EXP_B)])
        assert (S[:, 9] == 1.0).all()
        out[name] = dict(X=X, ack=ack, mode=mode, now=now, samples=S)
        if name == "before":
            bins, dropped = np.zeros((GP_MAX, NPT, ACC)), np.zeros(GP_MAX + 1, dtype=np.int32)
            accumulate(obs, S, bins, dropped)
            gp = fit(G, bins[0])
            model = set_gp(default_config(N=20), [as_set_gp(G, gp)])
            out.update(bins=bins, dropped=dropped, gp=gp, learned=model)
    rms = lambda S: float(np.sqrt(np.mean(S[:, 6:9] ** 2)))
    out["ratio"] = rms(out["after"]["samples"]) / rms(out["before"]["samples"])
    return out
