"""The prune of a log of sample records and the RDRv drag fit of include/admpc_quad_prune.h restated in numpy (TEST INFRASTRUCTURE).

prune() is the header's rule, vectorised, with O(1) work per record: who takes part, the four columns, np.linspace's edges and
np.histogram's uniform-bin index written out operation by operation (numpy rounds every one on its own, and so does the device), the
sparse bins from count / n_valid, and the closed upper edge of the reference's `bins[j + 1] >= y >= bins[j]`.  It also returns the smallest
relative distance of any bin ratio to thresh: the reference normalises the NORM's ratios twice (utils.py:507, 513), the header does not,
and the two agree unless a ratio is within rounding of thresh -- the tests assert that none is.  tests/test_quad_prune_cpu.py pins this
file to the reference's own prune_dataset and linear_rdrv_fitting through tests/golden/quad_prune_vectors.json, and the counts to
np.histogram.

rdrv() takes the arithmetic as `dtype`, as quad_clusters_spec does: the gap between float64 and numpy.longdouble is the yardstick of the
GPU test of the drag fit.  The order inside its sums is numpy's own and not part of the contract.

records() builds the seeded fixtures both the golden file and the GPU tests use."""
import numpy as np

REC, BINS_MAX, ENOVALID, PRUNED = 14, 256, -100, 2.0
KINDS = ("heavy", "quarter", "constant", "pythagorean", "one")


def take_part(S):
    """bool [M]: flag 1.0 or 2.0, and the body velocity (0 .. 2) and y (10 .. 12) finite."""
    S = np.asarray(S, dtype=np.float64).reshape(-1, REC)
    return ((S[:, 13] == 1.0) | (S[:, 13] == PRUNED)) & np.isfinite(S[:, 0:3]).all(axis=1) & np.isfinite(S[:, 10:13]).all(axis=1)


def columns(y):
    """[n, 4]: y_0, y_1, y_2 and sqrt((y_0^2 + y_1^2) + y_2^2), every operation rounded on its own."""
    y = np.asarray(y, dtype=np.float64).reshape(-1, 3)
    c = np.empty((y.shape[0], 4))
    c[:, :3] = y
    c[:, 3] = np.sqrt((y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2])
    return c


def edges_of(col, n_bins):
    """np.histogram's edges of one column [n] (n > 0): np.linspace(lo, hi, n_bins + 1) written out."""
    lo, hi = float(col.min()), float(col.max())
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    step = (hi - lo) / n_bins
    e = np.arange(0, n_bins + 1).astype(np.float64) * step + lo
    e[n_bins] = hi
    return e


def bin_index(v, e, n_bins):
    """np.histogram's uniform-bin index of every v [n] among the edges e [n_bins + 1], held into 0 .. n_bins - 1."""
    lo, hi = e[0], e[n_bins]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = ((v - lo) / (hi - lo)) * n_bins
    f = np.nan_to_num(f, nan=0.0, posinf=float(n_bins), neginf=0.0)                       # the device: not >= 0 -> 0, >= n_bins -> n_bins
    idx = np.clip(f, 0.0, float(n_bins)).astype(np.intp)                                   # truncation, as astype(np.intp) in numpy
    idx[idx == n_bins] -= 1
    idx[v < e[idx]] -= 1
    idx = np.maximum(idx, 0)
    idx[(v >= e[idx + 1]) & (idx != n_bins - 1)] += 1
    return idx


def prune(records, x_cap=16.0, n_bins=40, thresh=0.001):
    """admpc_quad_records_prune on records [M, 14] (not changed).  Returns a dict: records (the copy with the new flags), part and kept
    (bool [M]), info int32 [8], counts int32 [4, 256], edges (a list of four arrays [n_bins + 1], None with ENOVALID), lo and hi [4], and
    margin, the smallest relative distance of a bin ratio to thresh (inf for thresh == 0)."""
    S = np.array(records, dtype=np.float64).reshape(-1, REC)
    x_cap = np.inf if x_cap is None else float(x_cap)
    part = take_part(S)
    n = int(part.sum())
    info, counts = np.zeros(8, dtype=np.int32), np.zeros((4, BINS_MAX), dtype=np.int32)
    out = dict(records=S, part=part, kept=np.zeros(S.shape[0], dtype=bool), info=info, counts=counts, edges=None, lo=None, hi=None, margin=np.inf)
    if n == 0:
        info[0] = ENOVALID
        return out
    c = columns(S[part, 10:13])
    capped = (np.abs(S[part, 0:3]) > x_cap).any(axis=1)
    gone, edges, margin = capped.copy(), [], np.inf
    info[1], info[3] = n, int(capped.sum())
    for j in range(4):
        e = edges_of(c[:, j], n_bins)
        idx = bin_index(c[:, j], e, n_bins)
        h = np.bincount(idx, minlength=n_bins)
        ratio = h.astype(np.float64) / float(n)
        sparse = ratio < thresh
        if thresh > 0.0:
            margin = min(margin, float(np.abs(ratio - thresh).min() / thresh))
        below = np.maximum(idx - 1, 0)
        hit = sparse[idx] | ((idx > 0) & (c[:, j] == e[idx]) & sparse[below])
        info[4 + j] = int(hit.sum())
        gone |= hit
        counts[j, :n_bins] = h
        edges.append(e)
    info[2] = int((~gone).sum())
    S[part, 13] = np.where(gone, PRUNED, 1.0)
    out["kept"][part] = ~gone
    out.update(edges=edges, lo=np.array([e[0] for e in edges]), hi=np.array([e[-1] for e in edges]), margin=margin)
    return out


def rdrv(records, axes=7, dtype=np.float64):
    """admpc_quad_rdrv_fit: (D [3], sums [3, 2], n_used, status) in `dtype` over the records whose flag is exactly 1.0."""
    S = np.asarray(records, dtype=np.float64).reshape(-1, REC)
    use = S[:, 13] == 1.0
    v, y = S[use, 0:3].astype(dtype), S[use, 10:13].astype(dtype)
    D, sums, status = np.zeros(3, dtype=dtype), np.zeros((3, 2), dtype=dtype), 0
    with np.errstate(all="ignore"):
        for i in (2, 1, 0):
            if not (axes >> i) & 1:
                continue
            xy, xx = (v[:, i] * y[:, i]).sum(dtype=dtype), (v[:, i] * v[:, i]).sum(dtype=dtype)
            d = xy / xx
            if not (xx > 0 and np.isfinite(xx) and np.isfinite(d)):
                status = -(i + 1)
            D[i], sums[i] = d, (xy, xx)
    return D, sums, int(use.sum()), status


def pythagorean_triples():
    """Integer (a, b, c, d) with a^2 + b^2 + c^2 = d^2, d <= 45: norms that are whole numbers, so that they fall ON edges."""
    out = []
    for a in range(1, 30):
        for b in range(a, 30):
            for c in range(b, 30):
                d = int(round(np.sqrt(a * a + b * b + c * c)))
                if d * d == a * a + b * b + c * c and d <= 45:
                    out.append((a, b, c, d))
    return np.array(out, dtype=np.float64)


def clean(kind, M, seed):
    """(v_b [M, 3], y [M, 3]) of fixture `kind`, all finite."""
    rng = np.random.default_rng([seed, KINDS.index(kind), M])
    v = rng.standard_normal((M, 3)) * 6.0
    if kind == "heavy":
        y = rng.standard_t(2.0, (M, 3)) * np.array([1.0, 0.5, 2.0]) + 0.3 * v / 6.0
    elif kind == "quarter":
        y = np.round(rng.standard_normal((M, 3)) * 2.0 * 4.0) / 4.0
    elif kind == "constant":
        y = rng.standard_normal((M, 3))
        y[:, 1] = 0.75
    elif kind == "pythagorean":
        T = pythagorean_triples()
        t = T[rng.integers(0, len(T), M), :3]
        y = t[np.arange(M)[:, None], np.argsort(rng.random((M, 3)), axis=1)] * rng.choice([-1.0, 1.0], (M, 3))
    else:
        y = rng.standard_normal((M, 3))
    return v, y


def records(kind, M, seed=0, dirty=True):
    """Fixture `kind` as records float64 [M, 14].  With `dirty`, interleaved: about one record in eight with flag 0 (and values that must
    not count), one in sixteen with NaN in y under flag 1.0, one in eight that enters with flag 2.0; record 0 always takes part.  Kind
    "one": only record M // 2 takes part."""
    v, y = clean(kind, M, seed)
    rng = np.random.default_rng([seed, 99, KINDS.index(kind), M])
    S = rng.standard_normal((M, REC))
    S[:, 0:3], S[:, 10:13], S[:, 13] = v, y, 1.0
    if kind == "one":
        S[:, 13] = rng.choice([0.0, 3.0, -1.0, np.nan], M)
        S[: M // 2, 10] = 1e6
        S[M // 2, 13] = 1.0
        return S
    if dirty and M > 1:
        u = rng.random(M)
        off, nan, two = u < 0.125, (u >= 0.125) & (u < 0.1875), (u >= 0.1875) & (u < 0.3125)
        off[0] = nan[0] = False
        S[off, 13] = rng.choice([0.0, 3.0, 0.5], int(off.sum()))
        S[off, 10:13] = 1e9
        S[nan, 10 + (np.arange(M)[nan] % 3)] = np.nan
        S[two, 13] = PRUNED
    return S


# the fixtures of tests/golden/quad_prune_vectors.json: (kind, M, n_bins, thresh, x_cap or None, seed); no thresh of the form k / M
GOLDEN_CASES = (
    ("heavy", 1, 8, 0.0137, 16.0, 1), ("heavy", 2, 3, 0.0137, 16.0, 2), ("heavy", 17, 1, 0.0137, 16.0, 3), ("heavy", 500, 40, 0.00137, 16.0, 4),
    ("heavy", 2000, 40, 0.00137, 16.0, 5), ("heavy", 2000, 128, 0.00137, None, 6), ("heavy", 1999, 3, 0.0137, 9.0, 7),
    ("quarter", 300, 8, 0.0213, 16.0, 8), ("quarter", 2000, 40, 0.00713, 16.0, 9), ("quarter", 1000, 128, 0.00213, None, 10),
    ("constant", 200, 8, 0.0137, 16.0, 11), ("constant", 200, 3, 0.0137, 16.0, 12), ("constant", 64, 1, 0.0137, 16.0, 13),
    ("pythagorean", 1500, 40, 0.00713, 16.0, 14), ("pythagorean", 777, 8, 0.0213, None, 15), ("pythagorean", 2000, 128, 0.00137, 12.0, 16),
)
