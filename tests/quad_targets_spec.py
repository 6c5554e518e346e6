"""The rules of include/admpc_quad_targets.h restated in numpy (TEST INFRASTRUCTURE), one vehicle at a time: the uniforms of a target
and the two samplers (experiments/point_tracking_and_record.py:82-107), the reach test (utils/utils.py:276), `fast`, the recovery, the
point reference, the plant period with the reach test behind every sub-step and the bookkeeping of a reach, and the record over the
time a vehicle really flew.  Built on tests/quad_plant_spec.py (the simulator's update), tests/quad_noise_spec.py (Philox4x32-10, the
disturbances) and tests/quad_learn_spec.py (the record).  tests/test_quad_targets_cpu.py holds the sampler and the reach test against
the reference's own functions at 1e-15."""
import numpy as np

import quad_learn_spec as QL
import quad_noise_spec as NS
import quad_plant_spec as QS

TWO_PI = 6.283185307179586
LAST = 0xffffffff                                                    # call j of a target takes the fourth counter word LAST - j
MODES = {"preset": 0, "aggressive": 1, "uniform": 2}


def words(seed, b, t):
    """raw [..., 4] uint64: w0, w1 of call 0 and w0, w1 of call 1 of vehicle(s) b's target number(s) t (broadcast)."""
    b, t = np.broadcast_arrays(np.asarray(b, dtype=np.uint64), np.asarray(t, dtype=np.uint64))
    key = (int(seed) & 0xffffffff, int(seed) >> 32)
    out = np.zeros(b.shape + (4,), dtype=np.uint64)
    for j in range(2):
        o = NS.philox4x32_10((b, t & NS.MASK, t >> np.uint64(32), np.uint64(LAST - j)), key)
        out[..., 2 * j] = o[0] | o[1] << np.uint64(32)
        out[..., 2 * j + 1] = o[2] | o[3] << np.uint64(32)
    return out


def uniforms(raw):
    """u [..., 3] of the words raw [..., 4]: u0, u1 of call 0 and u0 of call 1."""
    return ((np.asarray(raw, dtype=np.uint64)[..., :3] >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def sample(mode, R, p, u):
    """The next target [..., 3] from the position(s) p [..., 3] under the uniforms u [..., 3]: every operation rounded on its own."""
    p, u, R = np.asarray(p, dtype=np.float64), np.asarray(u, dtype=np.float64), np.float64(R)
    if mode == 1:
        th, ps = TWO_PI * u[..., 0], TWO_PI * u[..., 1]
        r = R + (u[..., 2] - 0.5) * R
        rs = r * np.sin(th)
        return np.stack([p[..., 0] + rs * np.cos(ps), p[..., 1] + rs * np.sin(ps), p[..., 2] + r * np.cos(th)], axis=-1)
    assert mode == 2
    return -R + (2.0 * R) * u


def draw(tp, b, t, p):
    """The target number t gives vehicle b at position p (modes 1 and 2)."""
    return sample(int(tp.mode), tp.world_radius, p, uniforms(words(tp.seed, b, t)))


def dist(t, p):
    """d = sqrt(((t0 - p0)^2 + (t1 - p1)^2) + (t2 - p2)^2)."""
    with np.errstate(all="ignore"):
        e = np.asarray(t, dtype=np.float64) - np.asarray(p, dtype=np.float64)
        return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def too_fast(x, v_max):
    """1 iff one of x[7], x[8], x[9] is greater than v_max: signed, and a NaN compares false."""
    with np.errstate(invalid="ignore"):
        return np.int32(1 if (x[7] > v_max or x[8] > v_max or x[9] > v_max) else 0)


def is_done(tp, st, b):
    return int(tp.mode) == 0 and int(st["target_no"][b]) >= int(tp.n_preset)


def reset(tp, X, presets=None):
    """The state admpc_quad_targets_reset_batch leaves: a dict of target [B,3], target_no [B] uint64, n_iter, fast [B] int32, tcounts [B,5]."""
    B = X.shape[0]
    st = dict(target=np.zeros((B, 3)), target_no=np.zeros(B, dtype=np.uint64), n_iter=np.zeros(B, dtype=np.int32),
              fast=np.array([too_fast(X[b], tp.v_max) for b in range(B)], dtype=np.int32), tcounts=np.zeros((B, 5), dtype=np.int32))
    for b in range(B):
        st["target"][b] = presets[b, 0] if int(tp.mode) == 0 else draw(tp, b, 0, X[b, 0:3])
    return st


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def row_of(target):
    return np.concatenate([np.asarray(target, dtype=np.float64), [1.0, 0.0, 0.0, 0.0], np.zeros(6)])


def window(tp, st, X, N, prev=None):
    """admpc_quad_target_window_batch, in place on X, st and prev: (yref [B,N,17], yref_e [B,13], recovered [B] bool)."""
    B = X.shape[0]
    yref, yref_e, rec = np.zeros((B, N, 17)), np.zeros((B, 13)), np.zeros(B, dtype=bool)
    for b in range(B):
        row = row_of(st["target"][b])
        if not is_done(tp, st, b) and (st["fast"][b] != 0 or st["n_iter"][b] > tp.max_iters):
            X[b] = row
            if prev is not None:
                prev[b] = row
            st["n_iter"][b] = 0
            st["tcounts"][b, 1] += 1
            rec[b] = True
        yref[b, :, :13] = row
        yref_e[b] = row
    return yref, yref_e, rec


def plant_step(plant, tp, noise, st, X, U, status=None, noise_step=None, presets=None, ids=None):
    """admpc_quad_plant_target_step_batch, in place on X, st and noise_step: (nsub [B] int32, margins: per vehicle the list of
    d - thresh behind every sub-step it flew, positions: per vehicle the positions behind those sub-steps).  ids: the vehicles' numbers
    in their fleet where the rows are a sample of one (default: row b is vehicle b): what the draws and the targets are keyed by."""
    B, S = X.shape[0], int(plant.substeps)
    nsub, margins, positions = np.zeros(B, dtype=np.int32), [], []
    for b in range(B):
        x = np.array(X[b], dtype=np.float64)
        vid = b if ids is None else int(ids[b])
        st["fast"][b] = too_fast(x, tp.v_max)
        f, replaced = QS.activations(plant, U[b])
        a = np.array([plant.u_min if not np.isfinite(np.float64(U[b][i])) else max(min(np.float64(U[b][i]), plant.u_max), plant.u_min) for i in range(4)])
        done = is_done(tp, st, b)
        s = [x[0:3].copy(), x[3:7].copy(), x[7:10].copy(), x[10:13].copy()]
        z = NS.draws(noise.seed, vid, noise_step[b], np.arange(S)) if noise is not None else None
        n, reached, marg, pos = S, False, [], []
        for m in range(S):
            with np.errstate(all="ignore"):
                s = NS.update(plant, noise, s, a, z[m]) if noise is not None else QS.update(plant, s, f)
            d = dist(st["target"][b], s[0])
            marg.append(d - tp.thresh)
            pos.append(np.array(s[0], dtype=np.float64))
            if not done and d < tp.thresh:
                n, reached = m + 1, True
                break
        X[b] = np.concatenate(s)
        nsub[b] = n
        margins.append(marg); positions.append(pos)
        if noise is not None:
            noise_step[b] += np.uint64(1)
        if done:
            continue
        tc = st["tcounts"][b]
        tc[2] += 1
        if status is not None and int(status[b]) != 0:
            tc[3] += 1
        if replaced:
            tc[4] += 1
        st["n_iter"][b] = (0 if reached else st["n_iter"][b]) + 1
        if reached:
            tc[0] += 1
            st["target_no"][b] += np.uint64(1)
            no = int(st["target_no"][b])
            if int(tp.mode) == 0:
                if no < int(tp.n_preset):
                    st["target"][b] = presets[b, no]
            else:
                st["target"][b] = draw(tp, vid, no, X[b, 0:3])
    return nsub, margins, positions


def period_of(plant, obs, nsub):
    """dt_b = obs->dt where nsub == plant->substeps, else (double)nsub * plant->dt."""
    return np.float64(obs.dt) if int(nsub) == int(plant.substeps) else np.float64(int(nsub)) * np.float64(plant.dt)


def record(oracle, cfg, plant, obs, prev, now, u, nsub):
    """quad_learn_spec.record run at the period the vehicle flew; a record with nsub < 1 is invalid."""
    own = type(obs).from_buffer_copy(bytes(obs))
    own.dt = float(period_of(plant, obs, nsub))
    with np.errstate(all="ignore"):
        rec, xh, jac = QL.record(oracle, cfg, plant, own, prev, now, u)
    if int(nsub) < 1:
        rec[13] = 0.0
    return rec, xh, jac
