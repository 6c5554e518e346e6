"""The search of include/admpc_hyper.h restated in numpy (TEST INFRASTRUCTURE), one regressor at a time: the decoding of a round's
candidates, the negative log marginal likelihood (NLL) of each, the pick, and the rounds.

The points are learn_spec.points; the Cholesky and the forward solve are learn_spec.cholesky_solve's arithmetic, a column per step,
for all candidates of a round at once and in the arithmetic given as an argument (float64 or numpy.longdouble), as learn_spec.fit takes
it.  The natural values v = exp(theta) of the candidates come from the caller, so that a GPU test can pass the device's own; `natural`
is numpy's.  Logarithms of the box are math.log: the C library's, as the library's host side takes them."""
import math

import numpy as np

import learn_spec as LS

NSLOT, HYP, SEARCH_MAX, NO_OPTIMUM = 5, 16, 4096, -33
LOG_2PI = 1.8378770664093454836


def used_slots(nf):
    return [d for d in range(NSLOT) if d >= 3 or d < nf]


def box_logs(lo, hi, nf):
    """(free [5] bool, loglo [5], loghi [5]); the slot of an unused feature is not free and has both logarithms 0."""
    free, loglo, loghi = np.zeros(NSLOT, dtype=bool), np.zeros(NSLOT), np.zeros(NSLOT)
    for d in used_slots(nf):
        free[d], loglo[d], loghi[d] = lo[d] != hi[d], math.log(lo[d]), math.log(hi[d])
    return free, loglo, loghi


def init_state(lo, hi, nf, grid):
    """hyper [16] as resume == 0 leaves it, with numpy's exp for the natural values."""
    free, loglo, loghi = box_logs(lo, hi, nf)
    st = np.zeros(HYP)
    st[0:5] = 0.5 * (loglo + loghi)
    st[5:10] = np.where(free, (loghi - loglo) / np.float64(grid - 1), 0.0)
    st[10:15] = np.exp(st[0:5])
    st[15] = np.inf
    return st


def n_candidates(free, grid):
    return int(grid) ** int(np.sum(free))


def thetas(state, free, loglo, loghi, grid):
    """theta [C, 5] of a round's candidates: one digit per free slot, the last free slot the fastest; every operation rounded on its own."""
    C = n_candidates(free, grid)
    th = np.tile(np.asarray(state[0:5], dtype=np.float64), (C, 1))
    rem = np.arange(C)
    for d in range(NSLOT - 1, -1, -1):
        if free[d]:
            digit, rem = rem % grid, rem // grid
            off = (digit - (grid - 1) // 2).astype(np.float64) * np.float64(state[5 + d])
            th[:, d] = np.minimum(np.maximum(th[:, d] + off, loglo[d]), loghi[d])
    return th


def natural(th):
    return np.exp(np.asarray(th, dtype=np.float64))


def nll(G, stats, min_count, V, dtype=np.float64):
    """(NLL [C], size [C]) of the candidates with the natural values V [C, 5], solved in `dtype`.  +inf where a pivot is not positive and
    finite or a point's target is not finite; 0 for no points.  size = sum |log L_kk| + w'w / 2 + n log(2 pi) / 2, the magnitude of what
    is summed (for a bound on the rounding of the sum)."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, NSLOT)
    Z, t, counts, ymean = LS.points(G, np.asarray(stats, dtype=np.float64), min_count)
    C, n, nf = V.shape[0], len(t), int(G.n_feat)
    if n == 0:
        return np.zeros(C, dtype=dtype), np.zeros(C, dtype=dtype)
    il = (1.0 / (V[:, :nf] * V[:, :nf])).astype(dtype)                         # float64 as the device forms it, then widened
    Zd = Z.astype(dtype)
    e2 = (Zd[:, None, :] - Zd[None, :, :]) ** 2                                # [n, n, nf]
    with np.errstate(all="ignore"):
        d2 = (e2[None] * il[:, None, None, :]).sum(axis=3)
        diag = V[:, 4].astype(dtype)[:, None] + dtype(G.count_noise) / counts.astype(dtype)[None, :]
        K = V[:, 3].astype(dtype)[:, None, None] * np.exp(dtype(-0.5) * d2)
        K[:, np.arange(n), np.arange(n)] += diag
        b = t.astype(dtype) - dtype(ymean)
        L = np.zeros_like(K)
        w = np.zeros((C, n), dtype=dtype)
        failed = np.zeros(C, dtype=bool)
        for k in range(n):
            d = K[:, k, k] - (L[:, k, :k] * L[:, k, :k]).sum(axis=1, dtype=dtype)
            failed |= ~((d > 0) & np.isfinite(d)) | (not np.isfinite(t[k]))
            L[:, k, k] = np.sqrt(d)
            if k + 1 < n:
                L[:, k + 1:, k] = (K[:, k + 1:, k] - (L[:, k + 1:, :k] * L[:, k:k + 1, :k]).sum(axis=2, dtype=dtype)) / L[:, k, k][:, None]
        for k in range(n):
            w[:, k] = (b[k] - (L[:, k, :k] * w[:, :k]).sum(axis=1, dtype=dtype)) / L[:, k, k]
        logs = np.log(L[:, np.arange(n), np.arange(n)])
        half = dtype(0.5) * (w * w).sum(axis=1, dtype=dtype)
        const = dtype(0.5) * dtype(n) * dtype(LOG_2PI)
        val = logs.sum(axis=1, dtype=dtype) + half + const
        size = np.abs(logs).sum(axis=1, dtype=dtype) + half + const
    val[failed], size[failed] = np.inf, np.inf
    return val, size


def pick(state, th, V, values, shrink):
    """The pick of a round: (the new state [16], picked, the number of finite values).  values [C] as the NLL kernel left them."""
    x = np.asarray(values, dtype=np.float64)
    finite = np.isfinite(x)
    x = np.where(finite, x, np.inf)
    at = int(np.argmin(x))                                                     # the lowest index of the minimum
    new = np.array(state, dtype=np.float64)
    picked = -1
    if x[at] < state[15]:
        new[0:5], new[10:15], new[15], picked = th[at], V[at], x[at], at
    new[5:10] = new[5:10] * np.float64(shrink)
    return new, picked, int(finite.sum())


def search(G, stats, lo, hi, grid=5, rounds=10, shrink=0.5, min_count=1, dtype=np.float64, state=None):
    """`rounds` rounds from `state` (None: the start of resume == 0) with numpy's exp: (state, [picked of every round])."""
    free, loglo, loghi = box_logs(lo, hi, int(G.n_feat))
    st = init_state(lo, hi, int(G.n_feat), grid) if state is None else np.array(state, dtype=np.float64)
    picks = []
    for _ in range(rounds):
        th = thetas(st, free, loglo, loghi, grid)
        V = natural(th)
        val, _ = nll(G, stats, min_count, V, dtype)
        st, picked, _ = pick(st, th, V, val.astype(np.float64), shrink)
        picks.append(picked)
    return st, picks


def with_hyper(G, v):
    """A copy of the AdmpcGpBins G with length, sigma_f and noise set from the natural values v [5]."""
    H = type(G).from_buffer_copy(bytes(G))
    for d in range(int(G.n_feat)):
        H.length[d] = float(v[d])
    H.sigma_f, H.noise = float(v[3]), float(v[4])
    return H


def gaps(values, size64, valuesld, n):
    """The bound on |NLL_device - NLL_spec64| per candidate: ten times the gap between the spec solved in float64 and in longdouble, and
    the backward-error term 64 n eps of the sums (test_learn_gpu._check_fit) on the size of what is summed."""
    with np.errstate(invalid="ignore"):
        return 10.0 * np.abs(values.astype(np.longdouble) - valuesld).astype(np.float64) + 64 * n * 2.2e-16 * size64


def forced(values, bound):
    """Whether the minimum of `values` is so far below the best value distinct from it that a device within `bound` of every value
    must pick it: the gap exceeds both candidates' bounds.  (the lowest index of the minimum, forced or not)"""
    x = np.where(np.isfinite(values), values, np.inf)
    at = int(np.argmin(x))
    rest = x > x[at]
    if not np.isfinite(x[at]):
        return at, bool(np.isinf(x).all())
    if not rest.any():
        return at, True
    other = int(np.flatnonzero(rest)[np.argmin(x[rest])])
    gap = x[other] - x[at]
    return at, bool(gap > max(bound[at], bound[other] if np.isfinite(bound[other]) else 0.0))


def experiment_ratio(oracle, exp, G, gp):
    """RMS(y_after) / RMS(y_before) of learn_spec.experiment with the GP `gp` (a dict of learn_spec.fit under the AdmpcGpBins G) as the
    learned model of the second set."""
    from ad_mpc_amd.config import default_config, set_gp
    nominal, truth, plant, obs = LS.experiment_params()
    model = set_gp(default_config(N=20), [LS.as_set_gp(G, gp)])
    a = exp["after"]
    S = np.stack([LS.record(oracle, model, plant, obs, a["X"][b], a["now"][b], a["ack"][b], a["mode"][b])[0] for b in range(LS.EXP_B)])
    rms = lambda s: float(np.sqrt(np.mean(s[:, 6:9] ** 2)))
    return rms(S) / rms(exp["before"]["samples"])
