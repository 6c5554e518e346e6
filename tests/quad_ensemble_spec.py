"""The routing and the cluster binning of include/admpc_quad_ensemble.h restated in numpy (TEST INFRASTRUCTURE), built on
tests/quad_learn_spec.py and tests/learn_spec.py.

The routing is written as the device's loop -- best = inf, index 0, a strictly smaller distance wins -- so that ties go to the lower
index and a feature that is not finite gives cluster 0; every operation is rounded on its own (the body-frame map is
quad_learn_spec.body_velocity's), which the device's route reproduces wherever the two nearest distances are not within a few units in
the last place of each other: `margin` gives that gap, and the tests hold their inputs to 1e-6.  The binning is written from the
contract itself, lane by lane, not through the masking identity that the tests hold it against."""
import numpy as np

import learn_spec as LS
import quad_learn_spec as QL

WAVE, NPT, REC, ACC, GP_MAX, CLUSTERS_MAX = QL.WAVE, QL.NPT, QL.REC, QL.ACC, QL.GP_MAX, 8


def distances(z, cent):
    """[K]: sqrt(((z_0 - c_0)^2 + (z_1 - c_1)^2) + (z_2 - c_2)^2) for every centroid, the sum serial from 0."""
    z, cent = np.asarray(z, dtype=np.float64).reshape(-1), np.asarray(cent, dtype=np.float64)
    out = np.zeros(cent.shape[0])
    with np.errstate(all="ignore"):
        for c in range(cent.shape[0]):
            acc = np.float64(0.0)
            for j in range(z.size):
                e = z[j] - cent[c, j]
                acc = acc + e * e
            out[c] = np.sqrt(acc)
    return out


def nearest(z, cent):
    """The index of the nearest centroid: ties to the lower index, distances that are not finite lose to cluster 0."""
    best, bi = np.inf, 0
    for c, d in enumerate(distances(z, cent)):
        if d < best:
            best, bi = d, c
    return bi


def margin(z, cent):
    """The gap between the nearest and the second-nearest distance (inf for one cluster; NaN where a feature is not finite)."""
    d = np.sort(distances(z, cent))
    return np.inf if d.size < 2 else d[1] - d[0]


def z_of_row(row):
    """z [17] of one row [17] of a reference window: the state with its velocity rotated into the body frame by the row's own
    quaternion, then the input."""
    row = np.asarray(row, dtype=np.float64)
    z = row.copy()
    z[7:10] = QL.body_velocity(row[:13])
    return z


def route_window(yref, feats, cent):
    """route int32 [B] from row 0 of the windows yref [B, N, 17]."""
    return np.array([nearest(z_of_row(w[0])[list(feats)], cent) for w in np.asarray(yref, dtype=np.float64)], dtype=np.int32)


def route_records(samples, feats, cent):
    """The cluster int32 [B] of every sample record [B, 14] from its own features: feature f reads entry f - 7."""
    S = np.asarray(samples, dtype=np.float64).reshape(-1, REC)
    return np.array([nearest(r[[f - QL.FEAT0 for f in feats]], cent) for r in S], dtype=np.int32)


def accumulate(blocks, feats, cent, samples, bins, dropped):
    """admpc_quad_ensemble_bin_kernel, in place: bins float64 [K, 3, 32, 5], dropped int32 [K, 4]; blocks: the K AdmpcQuadObserveParams.
    A valid record of another cluster is absent to the waves of cluster c but keeps its lane (b % 64)."""
    S = np.asarray(samples, dtype=np.float64).reshape(-1, REC)
    valid = S[:, REC - 1] == 1.0
    route = route_records(S, feats, cent)
    dropped[0][GP_MAX] += int((~valid).sum())
    for c, obs in enumerate(blocks):
        for g in range(int(obs.n_gp)):
            G = obs.gp[g]
            nf = int(G.n_feat)
            part = np.zeros((WAVE, NPT, ACC))
            for b, r in enumerate(S):
                if not valid[b] or route[b] != c:
                    continue
                z = [r[int(G.feat[d]) - QL.FEAT0] for d in range(nf)]
                k = LS.bin_index(G, z)
                if k is None:
                    dropped[c][g] += 1
                    continue
                add = np.zeros(ACC)
                add[0], add[1:1 + nf], add[4] = 1.0, z, r[QL.Y0 + int(G.out) - QL.FEAT0]
                part[b % WAVE, k] = part[b % WAVE, k] + add
            for lane in range(WAVE):                                    # lane 0 first, onto the stored value
                bins[c][g] = bins[c][g] + part[lane]


def accumulate_masked(blocks, feats, cent, samples, bins, dropped):
    """The same by the masking identity: cluster c is quad_learn_spec.accumulate under block c of the records with the flag of every
    other cluster's record cleared; the records that were not valid to begin with are counted once, in dropped[0][3]."""
    S = np.asarray(samples, dtype=np.float64).reshape(-1, REC)
    valid = S[:, REC - 1] == 1.0
    route = route_records(S, feats, cent)
    for c, obs in enumerate(blocks):
        Sc = S.copy()
        Sc[valid & (route != c), REC - 1] = 0.0
        d1 = np.zeros(GP_MAX + 1, dtype=np.int32)
        QL.accumulate(obs, Sc, bins[c], d1)
        dropped[c][:GP_MAX] += d1[:GP_MAX]
    dropped[0][GP_MAX] += int((~valid).sum())
