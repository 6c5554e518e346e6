"""The numpy restatement of the rule of include/admpc_quad_select.h: the training points the reference's
``distance_maximizing_points_1d`` (utils/utils.py:536-581) picks for a one-feature regressor -- a histogram of ``n`` bins over the
feature values, the median record of every bin -- written from the rule's text, every step an explicit comparison; and the same over
a log of sample records for all regressors of all clusters.  tests/test_quad_select_cpu.py pins ``select_1d`` to the reference's own
function through tests/golden/quad_select_vectors.json; tests/test_quad_select_gpu.py holds the device to ``select_log``.

The one deliberate difference: a bin without a member gives no point (-1), where the reference draws a random record."""
import numpy as np

import quad_ensemble_spec as ES

REC, NPT, GMAX, ENOVALID = 14, 32, 3, -100


def edges(lo, hi, n):
    """np.linspace(lo, hi, n + 1) as the rule states it: e_j = lo + j * ((hi - lo) / n) for j < n, e_n = hi; lo - 0.5 and hi + 0.5 for
    a range that is a point."""
    lo, hi = np.float64(lo), np.float64(hi)
    if lo == hi:
        lo, hi = lo - np.float64(0.5), hi + np.float64(0.5)
    step = (hi - lo) / np.float64(n)
    return np.array([lo + np.float64(j) * step for j in range(n)] + [hi], dtype=np.float64)


def select_1d(z, n, variant=None):
    """The index into ``z`` (finite float64 [N]) of the record picked for each of the ``n`` bins, -1 for a bin without a member.
    ``variant`` names one of the wrong rules that the tests must tell from the right one: "keep_last" (no member set aside),
    "highest" (the highest equal index), "hi_in_last" (z == hi into the last bin), "formula" (the bin by the histogram's arithmetic),
    "low_byte" (the median compared without the lowest 8 bits of the value)."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    out = np.full(n, -1, dtype=np.int64)
    if z.size == 0:
        return out
    e = edges(z.min(), z.max(), n)
    b = (z[:, None] >= e[None, :]).sum(axis=1) - 1                 # np.digitize(z, e) - 1: the edges that are <= z, less one
    if variant == "hi_in_last":
        b = np.minimum(b, n - 1)
    if variant == "formula":
        with np.errstate(all="ignore"):
            b = np.minimum(np.floor((z - e[0]) / (e[n] - e[0]) * n).astype(np.int64), n)
    for j in range(n):
        mem = np.flatnonzero(b == j)                               # ascending record index
        if mem.size == 0:
            continue
        rest = mem[:-1] if (mem.size % 2 == 0 and variant != "keep_last") else mem
        vals = np.sort(z[rest])
        med = vals[(vals.size - 1) // 2]
        if variant == "low_byte":
            key = lambda v: np.asarray(v, dtype=np.float64).view(np.uint64) >> np.uint64(8)
            same = mem[key(z[mem] + 0.0) == key(np.array([med]) + 0.0)[0]]
        else:
            same = mem[z[mem] == med]
        out[j] = same[-1] if variant == "highest" else same[0]
    return out


def select_log(log, cent, feats, regs, n_points):
    """``select_1d`` for every regressor of every cluster over a log [M, 14]: ``cent`` [K, d] the centroids, ``feats`` the clustering
    features, ``regs`` a list of (feature, output) per regressor, ``n_points`` one bin count per regressor.  Returns
    (bins [K, 3, 32, 5], sel int32 [K, 3, 32], info int32 [K, 3, 4]) as include/admpc_quad_select.h lays them out."""
    log = np.asarray(log, dtype=np.float64).reshape(-1, REC)
    cent = np.asarray(cent, dtype=np.float64)
    K = cent.shape[0]
    bins, sel, info = np.zeros((K, GMAX, NPT, 5)), np.full((K, GMAX, NPT), -1, dtype=np.int32), np.zeros((K, GMAX, 4), dtype=np.int32)
    valid = np.flatnonzero(log[:, REC - 1] == 1.0)
    route = ES.route_records(log[valid], feats, cent) if valid.size else np.zeros(0, dtype=np.int32)
    for c in range(K):
        mine = valid[route == c]
        for g, (f, o) in enumerate(regs):
            n = int(n_points[g])
            z, y = log[mine, f - 7], log[mine, 10 + o - 7]
            part = mine[np.isfinite(z) & np.isfinite(y)]
            picked = select_1d(log[part, f - 7], n)
            rows = [int(part[i]) for i in picked if i >= 0]
            for j, i in enumerate(picked):
                sel[c, g, j] = part[i] if i >= 0 else -1
            for r, i in enumerate(rows):
                bins[c, g, r] = [1.0, log[i, f - 7], 0.0, 0.0, log[i, 10 + o - 7]]
            info[c, g] = [len(rows), part.size, n - len(rows), 0 if part.size else ENOVALID]
    return bins, sel, info


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------------
def values(kind, N, seed):
    """The seeded feature values float64 [N] of a fixture."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.normal(size=N)
    if kind == "uniform":
        return rng.uniform(-3.0, 2.0, size=N)
    if kind == "eighths":                                          # many ties, the member set aside among them
        return np.round(rng.normal(size=N) * 8.0) / 8.0
    if kind == "signs":                                            # both signs, and zeros of both signs
        v = np.round(rng.normal(size=N) * 4.0) / 4.0
        return np.where(rng.integers(0, 2, size=N) == 1, -v, v) * np.where(rng.integers(0, 2, size=N) == 1, -1.0, 1.0)
    if kind == "lowbits":                                          # eight groups whose members differ only in the lowest 8 bits
        base = (1.0 + 0.25 * rng.integers(0, 8, size=N)).astype(np.float64).view(np.uint64)
        return (base + rng.integers(0, 256, size=N).astype(np.uint64)).view(np.float64)
    if kind == "constant":
        return np.full(N, 0.625)
    if kind == "few":                                              # the smallest sets: N = 2, 3
        return np.array([0.5, -1.25, 0.75])[:N]
    raise ValueError(kind)


# (kind, N, n_points, seed): what the reference is run on for tests/golden/quad_select_vectors.json
GOLDEN_CASES = [
    ("normal", 200, 20, 1), ("normal", 1000, 32, 2), ("normal", 5000, 32, 3), ("normal", 5000, 20, 4), ("normal", 777, 7, 5),
    ("uniform", 3000, 7, 6), ("uniform", 2000, 32, 7), ("uniform", 500, 1, 8), ("uniform", 500, 2, 9), ("uniform", 901, 20, 10),
    ("eighths", 4000, 32, 11), ("eighths", 1500, 20, 12), ("signs", 1500, 20, 13), ("signs", 640, 7, 14),
    ("lowbits", 800, 8, 15), ("lowbits", 2500, 7, 16), ("constant", 300, 3, 17), ("constant", 64, 1, 18), ("few", 2, 1, 19), ("few", 3, 2, 20),
]
