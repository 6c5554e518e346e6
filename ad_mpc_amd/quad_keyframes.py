"""The position keyframes of the reference's polynomial trajectories, on the host with numpy alone: ``random_keyframes(seed)`` is
``random_periodical_trajectory(random_state=seed, map_limits=None)`` (utils/keyframe_3d_gen.py:61-157) with the two adjustments of
``random_trajectory`` (utils/trajectories.py:330-338), ``straight_keyframes()`` the three points of ``straight_trajectory`` (:307-311).
``QuadFleet.generate_polynomial_trajectories`` turns keyframes into trajectories on the device (include/admpc_quad_poly_traj.h).

The reference samples three Gaussian-process priors with scikit-learn.  ``GaussianProcessRegressor.sample_y`` of an unfitted regressor
is ``RandomState(seed).multivariate_normal(0, kernel(X))``, and legacy numpy's multivariate_normal is
``standard_normal(n) @ (sqrt(s)[:, None] * v)`` with ``u, s, v = svd(cov)``: the covariance does not depend on the seed, so its
decomposition is done once per axis and kept.  The kernel matrices are formed by the operations scikit-learn's ``ExpSineSquared`` uses, in
their order: singular values of a periodic kernel on a uniform grid come in pairs, and the basis of such a pair follows the last bits.
Map limits are not offered."""
import numpy as np

N_HR, N_KEY = 100, 10                  # the high-resolution samples per axis and the keyframes taken from them
# per axis: the linspace's end, and the (length_scale, periodicity) of the ExpSineSquared kernels that are summed (keyframe_3d_gen.py:66-77)
_AXES = ((60.0, ((4.5, 30.0), (4.5, 60.0))),       # x
         (30.0, ((4.5, 30.0), (4.0, 15.0))),       # y
         (60.0, ((5.5, 60.0),)))                   # z
_FACTORS = []                          # sqrt(s)[:, None] * v of every axis, filled at the first call


def _exp_sine_squared(x, length_scale, periodicity):
    dists = np.abs(x[:, None] - x[None, :])        # squareform(pdist(X, "euclidean")) of one column
    arg = np.pi * dists / periodicity
    sin_of_arg = np.sin(arg)
    return np.exp(-2 * (sin_of_arg / length_scale) ** 2)


def _factors():
    if not _FACTORS:
        for end, kernels in _AXES:
            x = np.linspace(0, end, N_HR)
            cov = _exp_sine_squared(x, *kernels[0])
            for k in kernels[1:]:
                cov = cov + _exp_sine_squared(x, *k)
            _, s, v = np.linalg.svd(cov)
            _FACTORS.append(np.sqrt(s)[:, None] * v)
    return _FACTORS


def raw_keyframes(seed):
    """[10,3]: the ``curve`` that ``random_periodical_trajectory(random_state=seed)`` returns."""
    hr = []
    for f in _factors():
        draw = np.random.RandomState(int(seed)).standard_normal((1, N_HR)).reshape(-1, N_HR)
        hr.append(np.dot(draw, f).T)               # [100,1], as sample_y returns it
    lo, hi = [np.min(a, 0) for a in hr], [np.max(a, 0) for a in hr]
    scaling = np.mean([hi[c] - lo[c] for c in range(3)])
    hr = [(a - (lo[c] + (hi[c] - lo[c]) / 2)) * 6 / scaling for c, a in enumerate(hr)]        # center_and_scale
    ind = np.linspace(0, N_HR - 1, N_KEY, dtype=int)
    ind[-1] = 0
    return np.concatenate([a[ind, :] for a in hr], 1)


def random_keyframes(seed):
    """[10,3]: the keyframes ``random_trajectory(quad, dt, seed, speed, map_name=None)`` fits its polynomial through: the curve above
    shifted to start at x = y = 0, and lifted by twice its lowest z where that is negative."""
    pos = raw_keyframes(seed)
    pos[:, 0] -= pos[0, 0]
    pos[:, 1] -= pos[0, 1]
    min_z = np.min(pos[:, -1])
    if min_z < 0:
        pos[:, -1] = pos[:, -1] + 2 * min_z * np.sign(min_z)
    return pos


def straight_keyframes():
    """[3,3]: ``straight_trajectory``'s keyframes, y from -3 to 3 at z = 1."""
    pos = np.zeros((3, 3))
    pos[:, 1] = np.linspace(-3, 3, 3)
    pos[:, 2] = 1
    return pos
