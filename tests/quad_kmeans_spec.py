"""The k-means++ seeding and the Lloyd k-means of include/admpc_quad_kmeans.h restated in numpy (TEST INFRASTRUCTURE), built on
tests/quad_noise_spec.py (the generator) and tests/quad_clusters_spec.py (the pack and the nearest-centre rule).

The decisions are the header's: the uniforms of Philox4x32-10 under the counter (round, draw, call, WORD), centre 0 the r-th counting
record, the candidates by the first inclusive cumulative sum of D2 that reaches the threshold, the smallest candidate potential with
ties to the lower trial, the labels by the routing's nearest-centre arithmetic, scikit-learn's two stops in its order.  The sums are
numpy's, whose order is its own: the order inside the sums is not part of the contract.  `dtype` is the arithmetic of the sums, the
potentials, the centres and the tolerance (float64 by default; numpy.longdouble is the yardstick of the GPU tests); what the device
holds as doubles stays those doubles: the records, the uniforms, D2 (the header's formula bit for bit) and the nearest-centre rule,
which reads the centres rounded to double.

Every run reports its MARGIN: the smallest distance, relative to the potential, of any threshold from the two cumulative sums that
bracket it and of the two smallest candidate potentials of a round from each other; and the smallest gap of any record's two nearest
centre distances, relative to the larger, over every labelling pass.  tests/test_quad_kmeans_cpu.py pins this file to scikit-learn's
_kmeans_plusplus and KMeans."""
import math

import numpy as np

import quad_clusters_spec as CS
import quad_noise_spec as NS

WORD, PARTIAL, STATE, EFEW, ENOVALID = 0x4B4D2B2B, 33, 48, -101, CS.ENOVALID


def work_doubles(M):
    return 2 * ((M + 255) // 256) + CS.BLOCKS_MAX * PARTIAL + STATE


def trials(K):
    return 2 + int(math.log(K))


def uniforms(seed, draw, c, n):
    """The first n uniforms of round c under (seed, draw): word t % 2 of call t // 2."""
    key = (int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff)
    out = []
    for j in range((n + 1) // 2):
        o = NS.philox4x32_10((c, draw, j, WORD), key)
        out += [int(o[0]) | int(o[1]) << 32, int(o[2]) | int(o[3]) << 32]
    return [(float(w >> 11) + 0.5) * 2.0 ** -53 for w in out[:n]]


def dsq(x, c):
    """((x0 - c0)^2 + (x1 - c1)^2) + (x2 - c2)^2 in float64, every operation rounded on its own; x [n, 3], c [3]."""
    e = x - c
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def seeding(x, K, seed, draw, dtype=np.float64):
    """x float64 [n, 3] (the counting records, the features past d at 0) -> (positions [K] among the counting records or None, status,
    potential, margin)."""
    n = x.shape[0]
    if n == 0:
        return None, ENOVALID, dtype(0.0), np.inf
    if n < K:
        return None, EFEW, dtype(0.0), np.inf
    u0 = uniforms(seed, draw, 0, 1)[0]
    pos = [min(int(math.floor(u0 * float(n))), n - 1)]
    D = dsq(x, x[pos[0]])
    pot = D.astype(dtype).sum()
    margin = np.inf
    T = trials(K)
    for c in range(1, K):
        if not pot > 0.0:
            return None, EFEW, pot, margin
        cum = np.cumsum(D.astype(dtype))
        cands, pots = [], []
        for u in uniforms(seed, draw, c, T):
            tau = dtype(u) * pot
            at = int(np.searchsorted(cum, tau, side="left"))
            below = cum[at - 1] if at > 0 else dtype(0.0)
            above = cum[at] if at < n else dtype(np.inf)
            margin = min(margin, float(min(tau - below, above - tau) / pot))
            at = min(at, n - 1)
            cands.append(at)
            pots.append(np.minimum(D, dsq(x, x[at])).astype(dtype).sum())
        best = int(np.argmin(np.array(pots, dtype=dtype)))                                       # the first smallest
        two = sorted(p for t, p in enumerate(pots) if cands[t] != cands[best])
        if two:
            margin = min(margin, float((two[0] - pots[best]) / pot))
        D = np.minimum(D, dsq(x, x[cands[best]]))
        pot = pots[best]
        pos.append(cands[best])
    return np.array(pos, dtype=np.int64), 0, pot, margin


def _label(x, d, cen):
    lab, gap = CS.nearest_rows(x[:, :d], np.asarray(cen[:, :d], dtype=np.float64))
    if cen.shape[0] > 1:
        dist = np.sqrt(np.stack([((x[:, :d] - np.asarray(cen[k, :d], dtype=np.float64)) ** 2).sum(axis=1) for k in range(cen.shape[0])], axis=1))
        two = np.sort(dist, axis=1)
        with np.errstate(all="ignore"):
            rel = np.where(two[:, 1] > 0.0, gap / two[:, 1], np.inf)
        return lab, float(rel.min())
    return lab, np.inf


def lloyd(x, d, start, max_iter=300, tol=1e-4, dtype=np.float64):
    """scikit-learn's _kmeans_single_lloyd from the centres start [K, d] over x [n, 3]: a dict with centers [K, d] (dtype), labels,
    iterations, converged (0, 1, 2), status (0 or -(k + 1)), inertia, tol_abs, shift, margin (the labelling passes')."""
    K, n = start.shape[0], x.shape[0]
    xd = x.astype(dtype)
    mean = xd[:, :d].sum(axis=0) / n
    tol_abs = dtype(tol) * (((xd[:, :d] - mean) ** 2).sum(axis=0) / n).sum() / d
    cen = np.zeros((K, 3), dtype=dtype)
    cen[:, :d] = start
    old, margin, shift, conv, its = np.full(n, -1), np.inf, dtype(0.0), 0, 0
    out = dict(tol_abs=tol_abs, status=0)
    for _ in range(int(max_iter)):
        lab, gap = _label(x, d, cen)
        margin = min(margin, gap)
        counts = np.bincount(lab, minlength=K)
        if (counts == 0).any():
            out.update(status=-(int(np.flatnonzero(counts == 0)[0]) + 1), iterations=its, converged=0, margin=margin, labels=lab)
            return out
        new = cen.copy()
        for k in range(K):
            new[k] = cen[k] + (xd[lab == k] - cen[k]).sum(axis=0) / counts[k]
        new64, cen64 = new.astype(np.float64), cen.astype(np.float64)                            # the device holds the centres as doubles
        shift = (((new64 - cen64).astype(dtype)) ** 2).sum()
        cen = new64.astype(dtype) if dtype is np.float64 else new
        its += 1
        if np.array_equal(lab, old):
            conv = 2
            break
        old = lab
        if shift <= tol_abs:
            conv = 1
            break
    if conv != 2:
        lab, gap = _label(x, d, cen)
        margin = min(margin, gap)
        counts = np.bincount(lab, minlength=K)
        if (counts == 0).any():
            out.update(status=-(int(np.flatnonzero(counts == 0)[0]) + 1), iterations=its, converged=conv, margin=margin, labels=lab)
            return out
    inertia = ((xd - cen[lab]) ** 2).sum()
    out.update(centers=cen[:, :d].copy(), labels=lab, iterations=its, converged=conv, inertia=inertia, shift=shift, margin=margin)
    return out


def fit(records, feats, K, seed, draw=0, max_iter=300, tol=1e-4, dtype=np.float64):
    """admpc_quad_kmeans_fit over records [M, 14]: a dict with idx int64 [K] (record indices), labels int32 [M] (-1 where a record does
    not count), centers [K, d] or None after a failure, info int32 [4], stats [4] (inertia, tol_abs, shift, potential), margin, and
    bound: what the accuracy bounds of the header need (n_k, the largest |x - c| per cluster, the moments behind tol_abs)."""
    d = len(feats)
    packed = CS.pack(records, feats)
    ok = packed[:, 3] == 1.0
    where = np.flatnonzero(ok)
    x = np.ascontiguousarray(packed[ok, :3])
    labels = np.full(packed.shape[0], -1, dtype=np.int32)
    out = dict(idx=None, labels=labels, centers=None, stats=np.zeros(4, dtype=dtype), margin=np.inf)
    pos, status, pot, margin = seeding(x, K, seed, draw, dtype)
    if status:
        out.update(info=np.array([0, 0, status, x.shape[0]], dtype=np.int32), margin=margin)
        return out
    run = lloyd(x, d, x[pos, :d], max_iter, tol, dtype)
    out.update(idx=where[pos], margin=min(margin, run["margin"]))
    out["info"] = np.array([run["iterations"], run["converged"], run["status"], x.shape[0]], dtype=np.int32)
    if run["status"]:
        return out
    labels[where] = run["labels"]
    out.update(centers=run["centers"], stats=np.array([run["inertia"], run["tol_abs"], run["shift"], pot], dtype=dtype))
    LD = np.longdouble
    cen = np.zeros((K, 3), dtype=LD); cen[:, :d] = run["centers"]
    reach = np.array([float(np.abs(x[run["labels"] == k].astype(LD) - cen[k]).max()) for k in range(K)])
    e = x.astype(LD) - x[0].astype(LD) if ok[0] else x.astype(LD)
    n = x.shape[0]
    out["bound"] = dict(n=n, n_k=np.bincount(run["labels"], minlength=K), reach=reach, size=np.abs(run["centers"]).max(axis=1).astype(np.float64),
                        moments=float(((e[:, :d] ** 2).sum(axis=0) / n + (e[:, :d].sum(axis=0) / n) ** 2).sum()))
    return out


def bounds(spec, K, d, tol):
    """The header's forward error bounds for a fit: (centres [K], inertia, tol_abs), absolute.  A centre is c + S / N in doubles: the
    last addition rounds by u |c|; S is n_k differences, each rounded, added in n_k - 1 additions, and divided once."""
    u, b = 2.0 ** -53, spec["bound"]
    return u * b["size"] + (b["n_k"] + 3) * u * b["reach"], (b["n"] + 4) * u * float(spec["stats"][0]), (b["n"] + 6) * u * tol * b["moments"] / d


# ---- the data of the tests ----------------------------------------------------------------------------------------------------------------

def cloud(M, K, d, seed, spread=0.6):
    """records [M, 14] whose d features 7 .. 7 + d - 1 are K blobs 3 apart along a diagonal, shuffled in log order; all count."""
    rng = np.random.default_rng(1000 * seed + 10 * K + d)
    rec = np.zeros((M, 14))
    which = rng.integers(0, K, size=M)
    rec[:, :d] = 3.0 * which[:, None] * (np.arange(d) + 1.0) / d + spread * rng.standard_normal((M, d))
    rec[:, 3:13] = rng.standard_normal((M, 10))
    rec[:, 13] = 1.0
    return rec


def spoil(rec, d):
    """Records that do not count at index 0, at M - 1, across a tile boundary and filling a whole tile where the log has one to spare:
    a cleared flag, a pruned 2.0, a feature that is not finite."""
    rec = rec.copy()
    M = rec.shape[0]
    rec[0, 13] = 0.0
    rec[M - 1, 13] = 2.0
    if M > 260:
        rec[254:256, 13] = 2.0
        rec[256, 0] = np.nan
        rec[257, d - 1] = np.inf
    if M > 1100:
        rec[512:768, 13] = 0.0
    return rec


# (M, K, d, seed): every M, K and d of the issue; tests/test_quad_kmeans_cpu.py holds the margin of each at 1e-9 or more
GPU_CASES = ((63, 1, 1, 0), (63, 2, 2, 1), (63, 3, 3, 2), (256, 2, 1, 0), (256, 3, 2, 1), (256, 8, 3, 2), (257, 1, 3, 0), (257, 3, 1, 1),
             (257, 8, 2, 2), (4097, 2, 3, 0), (4097, 3, 2, 1), (4097, 8, 1, 2), (65793, 3, 3, 0), (65793, 8, 2, 1))
FEATS = {1: [7], 2: [7, 8], 3: [7, 8, 9]}


def gpu_case(M, K, d, seed):
    return spoil(cloud(M, K, d, seed), d)


EDGE_SEED = 0


def edges():
    """records [1000, 14], K = 3 on feature 7: one blob lives in the records 0 .. 199 alone and one in 800 .. 999 alone, so the seeding
    takes a candidate from the first tile and one from the last."""
    rng = np.random.default_rng(77)
    rec = np.zeros((1000, 14))
    rec[:, 0] = 0.5 * rng.standard_normal(1000)
    rec[:200, 0] -= 6.0
    rec[800:, 0] += 6.0
    rec[:, 3:13] = rng.standard_normal((1000, 10))
    rec[:, 13] = 1.0
    rec[0, 13] = 0.0
    return rec


# (seed, status): under these seeds the seeding of empties() places centres at 6, 10 and 31; the middle cluster takes the 10s and the 20s,
# its mean moves to 15, and the second labelling pass hands the 10s to the left cluster and the 20s to the right: cluster k, the one that
# was seeded at 10, is empty, after one iteration
EMPTY_SEEDS = ((171985, -1), (139145, -2), (44844, -3))


def empties():
    """records [23, 14], K = 3 on feature 7: 6 points at 6, 6 at 10, 6 at 20, 4 at 21 (each within 0.01) and one at 31, shuffled."""
    rng = np.random.default_rng(23)
    v = np.concatenate([6 + rng.uniform(-.01, .01, 6), 10 + rng.uniform(-.01, .01, 6), 20 + rng.uniform(-.01, .01, 6), 21 + rng.uniform(-.01, .01, 4), [31.0]])
    rec = np.zeros((23, 14))
    rec[:, 0] = np.round(v, 4)[rng.permutation(23)]
    rec[:, 13] = 1.0
    return rec
