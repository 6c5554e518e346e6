"""The plant step, the tally and the counts of include/admpc_plant.h restated in numpy (TEST INFRASTRUCTURE), one vehicle at a time.

One `Oracle.rk4_sens(cfg, x, u, p, h)` per sub-step gives phi (the oracle carries the GP residual of cfg) and the state Jacobian A of
the sub-step; the command arrives as float32 and is widened, as on the device.  Every other operation is a single numpy float64
operation, in the order the header states."""
import numpy as np

GRID, TASKS = 4096, 63                                                # admpc_plant.hip: the launch line and LIN_TASKS
VEHICLES_PER_BLOCK = TASKS // 3
PAST_THE_GRID = GRID * VEHICLES_PER_BLOCK + 301                       # 86 317 vehicles: the stride loop runs


def blend(vx, blend_min, blend_max):
    """host.vel_switch on the plant's band; numpy's clip keeps NaN."""
    return np.clip((np.float64(vx) - blend_min) / (blend_max - blend_min), 0.0, 1.0)


def inputs(cfg, plant, ack, mode):
    """(u0, u1) of the record: ack float32 [4], mode int."""
    acc, rate = np.float64(np.float32(ack[3])), np.float64(np.float32(ack[1]))
    if int(mode) == 1 and np.isfinite(acc) and np.isfinite(rate):
        return np.array([min(max(acc, cfg.lbu[0]), cfg.ubu[0]), min(max(rate, cfg.lbu[1]), cfg.ubu[1])])
    return np.array([max(plant.brake_acc, cfg.lbu[0]), 0.0])


def wrap(a):
    """bound_angle_within_pi (ref_traj.py:28); numpy's % on float64 is the floor modulo."""
    return (np.float64(a) + np.pi) % (2.0 * np.pi) - np.pi


def step(oracle, cfg, plant, x, ack, mode, clear=False):
    """One period for one vehicle: (the new state [7], the state Jacobians of the M sub-steps).  clear: assert that no branch hinges
    on rounding -- no steering or speed within 1e-9 of its clamp before it is applied, no yaw ending within 1e-6 of +-pi."""
    x = np.array(x, dtype=np.float64)
    p = blend(x[3], plant.blend_min, plant.blend_max)
    u = inputs(cfg, plant, ack, mode)
    M = int(plant.substeps)
    h = np.float64(plant.dt) / M
    jac = []
    for _ in range(M):
        phi, A, _ = oracle.rk4_sens(cfg, x, u, p, h)
        x = phi.copy()
        if clear:
            assert min(abs(x[6] - cfg.lbx_delta), abs(x[6] - cfg.ubx_delta)) > 1e-9 and abs(x[3] - plant.v_min) > 1e-9, x
        if x[6] < cfg.lbx_delta:
            x[6] = cfg.lbx_delta
        if x[6] > cfg.ubx_delta:
            x[6] = cfg.ubx_delta
        if x[3] < plant.v_min:
            x[3] = plant.v_min
        jac.append(A)
    x[2] = wrap(x[2])
    if clear:
        assert np.pi - abs(x[2]) > 1e-6, x
    return x, jac


def chain_gain(jac):
    """G: the largest infinity norm of the products A_M ... A_{j+1}, j = 0 .. M (the empty product is the identity), floored at 1 --
    how far an error made in sub-step j can have grown at the end of the period."""
    P, G = np.eye(jac[0].shape[0]), 1.0
    for A in reversed(jac):
        P = P @ A
        G = max(G, float(np.abs(P).sum(axis=1).max()))
    return G


def tally_step(tally, counts, err, mode, status, valid):
    """One step of the rollout's sums for one vehicle, in place: tally float64 [3], counts int32 [3], err the step's out_err [3]."""
    ey, epsi = np.float64(err[1]), np.float64(err[2])
    if np.isfinite(ey) and np.isfinite(epsi):
        tally[0] = tally[0] + ey * ey
        tally[1] = tally[1] + epsi * epsi
        tally[2] = max(tally[2], abs(ey))
    counts[0] += 1
    counts[1] += 1 if int(mode) == 1 else 0
    counts[2] += 1 if (int(status) != 0 or int(valid) == 0) else 0
