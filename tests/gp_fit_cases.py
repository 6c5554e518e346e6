"""Named statistics for the GP fit and the NLL of the search (TEST INFRASTRUCTURE, numpy only): every point count, the patterns at the
edges of the compaction, every failure site, and hard kernel matrices.  tests/test_gp_fit_cases_cpu.py holds the conditions these inputs
must meet on the numpy spec alone; tests/test_gp_fit_cases.py runs them on the device.

A case is a regressor as a plain dict (`learn` turns it into what config.learn_bins or quad_config.quad_learn_bins take), statistics
[32, 5] (count, three feature sums, target sum), the min_count it is fitted under, and what the table SAYS the fit must find: the rows
that are points, n and info.  These are written down by construction, never taken from the spec or the device.

Every point has a count of 4 to 9 and every other row a count of 0, 1 to 3 or NaN, so a case has the same points under min_count 1 and
min_count 4 unless it is the one about min_count."""
import numpy as np

SEED = 1
# one feature on [2, 12]; three on the boxes of v_x, r and a_x of tests/test_learn_gpu.py
LO3, HI3 = [2.0, -0.3, -10.0], [12.0, 0.3, 5.0]
EASY = dict(bins=[32], lo=[2.0], hi=[12.0], length_scale=[0.6], sigma_f=1.0, noise=1e-4, count_noise=0.0)
EASY3 = dict(bins=[4, 2, 4], lo=LO3, hi=HI3, length_scale=[2.0, 0.4, 3.0], sigma_f=0.7, noise=1e-4, count_noise=0.0)
GRID8 = dict(EASY, bins=[8])
GRID421 = dict(EASY3, bins=[4, 2, 1])
# length 1e-4 on bins 0.3125 wide: every off-diagonal entry of K is exp(-0.5 * d^2 * 1e8) with d > 0.1, which is 0 in float64 and in
# longdouble; 1 + 1e-300 is 1 in both.  K is the identity but for what a case puts into it, and every pivot is exact.
EXACT = dict(EASY, length_scale=[1e-4], noise=1e-300)

# the boxes of the NLL rounds: 25 candidates each (grid 5)
ROUND1 = dict(length_scale=(1e-2, 1e2), sigma_f=(0.7, 0.7), noise=(0.04, 1.0))
ROUND3 = dict(length_scale=[(1e-2, 1e2), (0.4, 0.4), (3.0, 3.0)], sigma_f=(0.7, 0.7), noise=(0.04, 1.0))
DEAD = dict(length_scale=(1e-4, 1e-3), sigma_f=(1.0, 1.0), noise=(1e-300, 1e-200))        # K stays exact: every candidate fails
OVERFLOW = dict(length_scale=(1e-4, 1e-3), sigma_f=(1.7e308, 1.7e308), noise=(1e308, 1e308))
TWIN_FREE = dict(length_scale=(1e-4, 1e-3), sigma_f=(1.0, 1.0), noise=(1e-300, 1e-2))     # noise 1e-2 alone makes the twin's pivot positive

CAR_FEAT, QUAD_FEAT = {1: [3], 2: [3, 5], 3: [3, 5, 7]}, {1: [7], 2: [8, 12], 3: [9, 13, 16]}


class Case:
    def __init__(self, name, kind, reg, stats, rows, info=None, min_count=1, zeroed=None, box=None):
        self.name, self.kind, self.reg, self.stats, self.min_count = name, kind, reg, stats, min_count
        self.rows = [int(k) for k in rows]              # the rows the fit must take as its points, ascending
        self.n = len(self.rows)
        self.info = self.n if info is None else info    # a failure: -(site + 1), and the record is the empty GP
        self.zeroed = zeroed                            # the same statistics with every row past the product of bins zeroed, or None
        self.box = box or (ROUND1 if len(reg["bins"]) == 1 else ROUND3)

    def __repr__(self):
        return "Case(%s)" % self.name


def learn(reg, out, feats=CAR_FEAT):
    """The regressor as a dict of the `learn` lists of the fleets; feats: CAR_FEAT or QUAD_FEAT."""
    return dict(reg, feat=feats[len(reg["bins"])], out=out)


def n_bins(reg):
    return int(np.prod(reg["bins"]))


def fill(reg, rows, rng, scale=1.0, offset=0.0):
    """Statistics with the given rows filled: inside the grid a jittered bin centre, past it a point anywhere in the box (what a larger
    grid left behind); 4 to 9 samples each, the target sin(3 z_0) + 0.1 N(0, 1), times `scale`, plus `offset`."""
    nb, nf = list(reg["bins"]), len(reg["bins"])
    stats = np.zeros((32, 5))
    for k in rows:
        c = float(rng.integers(4, 10))
        if k < n_bins(reg):
            idx = np.unravel_index(k, nb)
            u = [(idx[d] + rng.uniform(0.3, 0.7)) / nb[d] for d in range(nf)]
        else:
            u = [rng.uniform(0.0, 1.0) for d in range(nf)]
        z = np.array([reg["lo"][d] + u[d] * (reg["hi"][d] - reg["lo"][d]) for d in range(nf)])
        y = offset + scale * (np.sin(3.0 * z[0]) + 0.1 * rng.normal())
        stats[k, 0], stats[k, 1:1 + nf], stats[k, 4] = c, c * z, c * y
    return stats


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def _subset(rng, total, n):
    return sorted(rng.permutation(total)[:n].tolist())


def _table():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))

    # ---- the sweep: every n of one feature, the edges and the middle of three
    for n in range(33):
        rng = _rng(1, n)
        rows = _subset(rng, 32, n)
        add("sweep1-n%02d" % n, "sweep", EASY, fill(EASY, rows, rng), rows)
    for n in (0, 1, 2, 3, 16, 17, 31, 32):
        rng = _rng(3, n)
        rows = _subset(rng, 32, n)
        add("sweep3-n%02d" % n, "sweep", EASY3, fill(EASY3, rows, rng), rows)

    # ---- which bins are points
    for name, rows in (("last-bin", [31]), ("bin0", [0]), ("first-and-last", [0, 31]), ("even-bins", range(0, 32, 2)), ("odd-bins", range(1, 32, 2)),
                       ("all-but-bin0", range(1, 32)), ("all-but-last", range(0, 31))):
        rows = list(rows)
        add(name, "pattern", EASY, fill(EASY, rows, _rng(5, len(name), rows[0])), rows)
    # a smaller grid in front of what a larger one left behind: rows 8 .. 31 hold statistics with counts of 4 to 9
    for name, reg, inside in (("grid8-full", GRID8, range(8)), ("grid8-two", GRID8, [1, 7]), ("grid8-last", GRID8, [7]), ("grid8-none", GRID8, []),
                              ("grid421-full", GRID421, range(8)), ("grid421-two", GRID421, [0, 6])):
        inside = list(inside)
        stats = fill(reg, inside + list(range(8, 32)), _rng(7, len(name), len(inside)))
        zeroed = stats.copy()
        zeroed[8:] = 0.0
        add(name + "-stale", "pattern", reg, stats, inside, zeroed=zeroed)
    # a row that is no point between rows that are: a NaN count; a count below min_count
    rng = _rng(9)
    rows = _subset(rng, 32, 17)
    stats = fill(EASY, rows, rng)
    hole = rows[8]
    stats[hole, 0] = np.nan
    add("nan-count", "pattern", EASY, stats, [k for k in rows if k != hole])
    rng = _rng(10)
    rows = _subset(rng, 32, 17)
    stats = fill(EASY, rows, rng)
    low = [rows[0], rows[7], rows[16]]
    for i, k in enumerate(low):
        stats[k] = stats[k] / stats[k, 0] * (1.0 + i)                     # counts 1, 2, 3
    add("below-min-count", "pattern", EASY, stats, [k for k in rows if k not in low], min_count=4)

    # ---- failure sites on the exact K
    for site in (1, 16, 31):                                              # the twin: the zero pivot at step `site` of 32
        stats = fill(EXACT, range(32), _rng(11, site))
        stats[site, 0:4] = stats[site - 1, 0:4]                           # the same count and sums: the same Z bit for bit, another target
        add("twin-at-%02d" % site, "failure", EXACT, stats, range(32), info=-(site + 1), box=DEAD)
    for label, value in (("inf", np.inf), ("nan", np.nan)):               # a target that is not finite, at point 0, 8 and 16 of 17
        for site in (0, 8, 16):
            rng = _rng(12, site, len(label))
            rows = _subset(rng, 32, 17)
            stats = fill(EXACT, rows, rng)
            stats[rows[site], 4] = value
            add("%s-target-at-%02d" % (label, site), "failure", EXACT, stats, rows, info=-(site + 1), box=DEAD)
    for site in (0, 16):                                                  # a NaN feature sum at the first and at the last point
        rng = _rng(13, site)
        rows = _subset(rng, 32, 17)
        stats = fill(EXACT, rows, rng)
        stats[rows[site], 1] = np.nan
        add("nan-feature-at-%02d" % site, "failure", EXACT, stats, rows, info=-(site + 1), box=DEAD)
    # sigma_f + noise overflows float64: the first pivot is +inf.  (It is 2.7e308 in longdouble, whose range is wider: the one failure
    # that belongs to the number format and not to the data.)
    rng = _rng(14)
    rows = _subset(rng, 32, 5)
    huge = dict(EXACT, sigma_f=1.7e308, noise=1e308)
    add("overflowing-pivot", "failure", huge, fill(huge, rows, rng), rows, info=-1, box=OVERFLOW)

    # ---- hard kernel matrices, 32 points each
    all32 = list(range(32))
    hard = [("long-length-noise1e-8", dict(EASY, length_scale=[50.0], noise=1e-8), {}),
            ("long-length-noise1e-6", dict(EASY, length_scale=[50.0], noise=1e-6), {}),
            ("small-sigma_f", dict(EASY, sigma_f=1e-6, noise=1e-10), {}),
            ("large-sigma_f", dict(EASY, sigma_f=1e6, noise=1e-2), {}),
            ("count-noise", dict(EASY, count_noise=1.0, noise=1e-8), {}),
            ("short-length", dict(EASY, length_scale=[0.01]), {}),
            ("three-long-lengths", dict(EASY3, length_scale=[20.0, 5.0, 30.0], sigma_f=1.0, noise=1e-7), {}),
            ("large-targets", EASY, dict(scale=1e-3, offset=1e6))]
    for i, (name, reg, kw) in enumerate(hard):
        rng = _rng(15, i)
        stats = fill(reg, all32, rng, **kw)
        if name == "count-noise":                                         # counts 10^0 .. 10^6, the sums scaled with them
            for k in all32:
                stats[k] = stats[k] / stats[k, 0] * 10.0 ** rng.integers(0, 7)
        add(name, "hard", reg, stats, all32)
    return cases


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def of_kind(*kinds):
    return [c for c in CASES if c.kind in kinds]


def chunks(cases, size=4):
    """The cases in launches of `size` regressors that share a min_count."""
    out = []
    for m in sorted({c.min_count for c in cases}):
        same = [c for c in cases if c.min_count == m]
        out += [same[i:i + size] for i in range(0, len(same), size)]
    return out


# The 24 regressors of the ensemble test, K = 8 clusters of 3.  The clusters of an ensemble agree in every regressor's features, so
# regressors 0 and 1 of a cluster have one feature and regressor 2 has three.  None of these cases depends on min_count.
ENSEMBLE = [("sweep1-n00", "sweep1-n01", "sweep3-n01"), ("sweep1-n02", "sweep1-n03", "sweep3-n03"), ("sweep1-n15", "sweep1-n16", "sweep3-n16"),
            ("sweep1-n17", "twin-at-16", "sweep3-n17"), ("sweep1-n31", "sweep1-n32", "sweep3-n31"), ("grid8-full-stale", "inf-target-at-16", "grid421-full-stale"),
            ("nan-feature-at-00", "grid8-two-stale", "grid421-two-stale"), ("all-but-bin0", "even-bins", "sweep3-n32")]
ENSEMBLE_FEAT = ([7], [8], [9, 13, 16])
assert len(ENSEMBLE) == 8 and all(BY_NAME[k].min_count == 1 and len(BY_NAME[k].reg["bins"]) == len(ENSEMBLE_FEAT[g])
                                  for names in ENSEMBLE for g, k in enumerate(names))
