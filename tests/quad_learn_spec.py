"""The record of include/admpc_quad_learn.h restated in numpy (TEST INFRASTRUCTURE), one vehicle or one regressor at a time, and the
learning experiment of the quadrotor in the spec alone.

One `QuadOracle.rk4_sens(cfg, x, u, h)` per sub-step gives the model's prediction and its Jacobian (the oracle carries rdrv and the GP
residual of cfg, the features from the integrated state); the body-frame map is written element by element in the order the header
states, not as a `dot`; the activations are tests/quad_plant_spec.py's.  Binning, fit and install check are tests/learn_spec.py's: they
are imported, and the quadrotor's record layout is passed in by presenting every regressor's features, target and flag at the places
of the car's record (feature d at entry d, the target at entry 6, the flag at entry 9), which leaves the order of every sum as it is."""
import ctypes as C
import types

import numpy as np

import learn_spec as LS
import quad_plant_spec as QS

WAVE, NPT, REC, ACC, GP_MAX = 64, 32, 14, 5, 3
FEAT0, Y0 = 7, 10                        # feature index f reads entry f - 7; output `out` reads entry 10 + out - 7


def body_velocity(s):
    """v_b,i = (R[0][i] * v_0 + R[1][i] * v_1) + R[2][i] * v_2 with R of s's own quaternion, every operation rounded on its own."""
    with np.errstate(all="ignore"):
        R = QS.rot(np.asarray(s, dtype=np.float64)[3:7])
        v = np.asarray(s, dtype=np.float64)[7:10]
        return np.array([(R[0][i] * v[0] + R[1][i] * v[1]) + R[2][i] * v[2] for i in range(3)], dtype=np.float64)


def activations(plant, u):
    """a [4]: rule 1 of admpc_quad_plant_step_batch (quad_plant_spec.activations with a thrust of 1 per unit activation)."""
    unit = types.SimpleNamespace(u_min=np.float64(plant.u_min), u_max=np.float64(plant.u_max), max_thrust=np.float64(1.0))
    return QS.activations(unit, u)[0]


def record(oracle, cfg, plant, obs, prev, now, u):
    """One vehicle: (the sample [14], the prediction x^ [13], the state Jacobians of the sub-steps).  cfg: the MODEL's configuration."""
    prev, now = np.array(prev, dtype=np.float64), np.array(now, dtype=np.float64)
    a = activations(plant, u)
    M = int(obs.substeps)
    h = np.float64(obs.dt) / M
    x, jac = prev.copy(), []
    for _ in range(M):
        x, A, _ = oracle.rk4_sens(cfg, x, a, h)
        jac.append(A)
    with np.errstate(all="ignore"):
        y = (body_velocity(now) - body_velocity(x)) / np.float64(obs.dt)
    rec = np.concatenate([body_velocity(prev), prev[10:13], a, y, [0.0]])
    rec[13] = 1.0 if np.isfinite(rec[:13]).all() else 0.0
    return rec, x, jac


def _as_car(G):
    """One regressor of the quadrotor as learn_spec reads one of the car: feature d at index 3 + d, the output at 3."""
    from ad_mpc_amd.config import AdmpcGpBins, AdmpcObserveParams
    g = AdmpcGpBins.from_buffer_copy(bytes(G))
    for d in range(int(G.n_feat)):
        g.feat[d] = 3 + d
    g.out = 3
    gps = (AdmpcGpBins * LS.GP_MAX)()
    gps[0] = g
    return AdmpcObserveParams(dt=1.0, blend_min=0.0, blend_max=1.0, substeps=1, n_gp=1, gp=gps)


def accumulate(obs, samples, bins, dropped):
    """admpc_quad_bin_kernel, in place: bins float64 [3, 32, 5], dropped int32 [4] -- learn_spec.accumulate per regressor."""
    samples = np.asarray(samples, dtype=np.float64).reshape(-1, REC)
    for g in range(int(obs.n_gp)):
        G = obs.gp[g]
        S = np.zeros((samples.shape[0], LS.REC))
        for d in range(int(G.n_feat)):
            S[:, d] = samples[:, int(G.feat[d]) - FEAT0]
        S[:, 6], S[:, 9] = samples[:, Y0 + int(G.out) - FEAT0], samples[:, REC - 1]
        b1, d1 = np.zeros((LS.GP_MAX, NPT, ACC)), np.zeros(LS.GP_MAX + 1, dtype=np.int32)
        b1[0] = bins[g]
        LS.accumulate(_as_car(G), S, b1, d1)
        bins[g] = b1[0]
        dropped[g] += d1[0]
        if g == 0:
            dropped[GP_MAX] += d1[LS.GP_MAX]


def install_ok(gp):
    """The check of admpc_quad_gp_install on an AdmpcGp: the quadrotor's ranges here, the rest by learn_spec.install_ok."""
    from ad_mpc_amd.config import AdmpcGp
    nf = int(gp.n_feat)
    if not (1 <= nf <= 3 and 7 <= int(gp.out) <= 9 and all(7 <= int(gp.feat[d]) <= 16 for d in range(nf))):
        return False
    car = AdmpcGp.from_buffer_copy(bytes(gp))
    car.out = 3
    for d in range(nf):
        car.feat[d] = 3
    return LS.install_ok(car)


def as_set_gp(G, gp):
    return LS.as_set_gp(G, gp)


# ---- the learning experiment ---------------------------------------------------------------------------------------------------------

EXP_B, EXP_DT, EXP_MIN_COUNT = 512, 0.02, 2
EXP_LEARN = [dict(feat=7 + i, out=7 + i, lo=[-9.0], hi=[9.0], bins=[32], length_scale=2.0, sigma_f=1.0, noise=1e-4, count_noise=1e-2) for i in range(3)]
EXP_SEEDS = (("before", 1, 11), ("after", 7, 17))          # the set learned from and the held-out set: (states, activations)


def experiment_inputs(name):
    """(X [512,13], U [512,4]): quad_plant_spec.random_states and activations uniform in [0.1, 0.9]."""
    _, sx, su = [e for e in EXP_SEEDS if e[0] == name][0]
    return QS.random_states(EXP_B, sx), np.random.default_rng(su).uniform(0.1, 0.9, (EXP_B, 4))


def experiment_params():
    """(the nominal configuration, the drag plant of one 20 ms period in 40 sub-steps, the observe parameters)."""
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, SimQuad, default_quad_config, quad_learn_bins, quad_plant_params
    bins, n_gp = quad_learn_bins(EXP_LEARN)
    obs = AdmpcQuadObserveParams(dt=EXP_DT, substeps=1, n_gp=n_gp, gp=bins)
    plant = quad_plant_params(SimQuad(drag=True), 5e-4, EXP_DT)
    return default_quad_config(N=10), plant, obs


def rms(S):
    return np.sqrt(np.mean(np.asarray(S)[:, Y0:Y0 + 3] ** 2, axis=0))


def learn(obs, S, min_count=EXP_MIN_COUNT):
    """(bins, dropped, the fits, cond(K) per regressor) of the samples S."""
    bins, dropped = np.zeros((GP_MAX, NPT, ACC)), np.zeros(GP_MAX + 1, dtype=np.int32)
    accumulate(obs, S, bins, dropped)
    gps = [LS.fit(obs.gp[g], bins[g], min_count) for g in range(int(obs.n_gp))]
    cond = []
    for g in range(int(obs.n_gp)):
        Z, t, counts, _ = LS.points(obs.gp[g], bins[g], min_count)
        cond.append(float(np.linalg.cond(LS.kernel_matrix(obs.gp[g], Z, counts))) if len(t) else 0.0)
    return bins, dropped, gps, cond


def experiment(oracle, transitions=None):
    """The spec's run of the experiment: observe 512 periods of the drag plant against the nominal model, fit, observe the held-out 512
    against the learned model.  `transitions`: {name: (X, U, now)} to use instead of the spec's own plant (the device's, for instance).
    A dict with the samples of both sets, the statistics, the fits, cond(K) and the ratios RMS(y_after) / RMS(y_before) per axis, where
    y_before is the held-out set's residual against the NOMINAL model."""
    from ad_mpc_amd.quad_config import set_quad_gp
    nominal, plant, obs = experiment_params()
    out = {}
    for name, _, _ in EXP_SEEDS:
        if transitions is None:
            X, U = experiment_inputs(name)
            now = QS.step_fleet(plant, X, U)[0]
        else:
            X, U, now = transitions[name]
        out[name] = dict(X=X, U=U, now=now)
        out[name]["samples"] = np.stack([record(oracle, nominal, plant, obs, X[b], now[b], U[b])[0] for b in range(X.shape[0])])
    bins, dropped, gps, cond = learn(obs, out["before"]["samples"])
    learned = set_quad_gp(nominal.copy(), [as_set_gp(obs.gp[g], gps[g]) for g in range(3)])
    a = out["after"]
    a["learned_samples"] = np.stack([record(oracle, learned, plant, obs, a["X"][b], a["now"][b], a["U"][b])[0] for b in range(a["X"].shape[0])])
    out.update(bins=bins, dropped=dropped, gps=gps, cond=cond, learned=learned, before_rms=rms(a["samples"]), after_rms=rms(a["learned_samples"]))
    out["ratio"] = out["after_rms"] / out["before_rms"]
    return out
