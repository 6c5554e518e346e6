"""Every refusal of the six fleet entry points that share their checks (admpc_control_step_batch, _bank_batch, _lane_batch,
admpc_rollout_lane_batch, admpc_rollout_observe_lane_batch, admpc_plant_step_batch): return code and WHOLE message, as a table.

The messages carry the name of the entry point whose check refuses, which is not always the one called (a rollout reports the lane
step's refusals under the lane step's name), and where two arguments are at fault the first check in the order of the library wins;
the pairs at the end of each block pin that order.  No row reaches the device: controller state and poses are compared bit for bit
afterwards.  Refusals that need a second GPU (a bank, plant or model on another device) or a failing HIP call are not reachable here."""
import ctypes as C

import numpy as np
import pytest

import test_lane_gpu as TL
import test_plant_gpu as TP

pytestmark = pytest.mark.gpu

N, B = 20, 6
EINVAL = -1
STEP, BANK, LANE = "admpc_control_step_batch: ", "admpc_control_step_bank_batch: ", "admpc_control_step_lane_batch: "
ROLL, OBS, PLANT = "admpc_rollout_lane_batch: ", "admpc_rollout_observe_lane_batch: ", "admpc_plant_step_batch: "
NULL = C.c_void_p(0)

# (argument overrides, message behind the prefix): the parameter blocks, refused by one function each under the caller's name
LANE_PARAMS = [
    (dict(lane=None), "the lane parameters are not set"),
    (dict(lane=dict(L=33)), "L must be in [34, 256]"),
    (dict(lane=dict(L=257)), "L must be in [34, 256]"),
    (dict(lane=dict(back=-1)), "back and ahead must not be negative"),
    (dict(lane=dict(ahead=-1)), "back and ahead must not be negative"),
    (dict(idx=NULL), "null lane_idx"),
]
PLANT_PARAMS = [
    (dict(plant=None), "the plant parameters are not set"),
    (dict(plant=dict(dt=0.0)), "dt must be positive and finite"),
    (dict(plant=dict(dt=float("inf"))), "dt must be positive and finite"),
    (dict(plant=dict(blend_max=3.0, blend_min=3.0)), "blend_max must exceed blend_min"),
    (dict(plant=dict(brake_acc=0.5)), "brake_acc must not be positive"),
    (dict(plant=dict(v_min=-0.5)), "v_min must not be negative"),
    (dict(plant=dict(substeps=0)), "substeps must be in [1, 64]"),
    (dict(plant=dict(substeps=65)), "substeps must be in [1, 64]"),
]
OBSERVE_PARAMS = [
    (dict(obs=None), "the observe parameters are not set"),
    (dict(obs=dict(dt=0.0)), "dt must be positive and finite"),
    (dict(obs=dict(blend_max=3.0, blend_min=3.0)), "blend_max must exceed blend_min"),
    (dict(obs=dict(substeps=65)), "substeps must be in [1, 64]"),
    (dict(obs=dict(n_gp=0)), "n_gp must be in [1, 4]"),
    (dict(obs=dict(n_gp=5)), "n_gp must be in [1, 4]"),
    (dict(gp=dict(n_feat=0)), "regressor 0: n_feat must be in [1, 3]"),
    (dict(gp=dict(feat=(2, 0, 0))), "regressor 0: feat must be in [3, 8]"),
    (dict(gp=dict(out=6)), "regressor 0: out must be in [3, 5]"),
    (dict(gp=dict(nb=(0, 1, 1))), "regressor 0: nb must be >= 1, and 1 for an unused feature"),
    (dict(gp=dict(nb=(8, 2, 1))), "regressor 0: nb must be >= 1, and 1 for an unused feature"),
    (dict(gp=dict(nb=(33, 1, 1))), "regressor 0: the product of nb must not exceed 32"),
    (dict(gp=dict(hi=(2.0, 0.0, 0.0))), "regressor 0: lo and hi must be finite, hi > lo"),
    (dict(gp=dict(sigma_f=0.0)), "regressor 0: sigma_f must be positive and finite"),
    (dict(gp=dict(length=(0.0, 0.0, 0.0))), "regressor 0: length must be positive and finite"),
    (dict(gp=dict(noise=0.0)), "regressor 0: noise must be positive and finite"),
    (dict(gp=dict(count_noise=-1.0)), "regressor 0: count_noise must not be negative"),
]
# what the three steps share, in the order of their checks; `far` is a handle of N = 80, `other` one of N = 40
HEAD = [
    (dict(s=None), "null solver / params or negative batch"),
    (dict(prm=None), "null solver / params or negative batch"),
    (dict(B=-1), "null solver / params or negative batch"),
    (dict(s="far"), "the solver's N must be in [3, 64] (the waypoint kernel's horizon)"),
]
BANK_OF = [
    (dict(bank=None), "the bank is not set"),
    (dict(s="other"), "the bank's horizon H must equal the solver's N"),
    (dict(bank="other"), "the bank's horizon H must equal the solver's N"),
]
STEP_PARAMS = [
    (dict(prm=dict(threshold=-1)), "bad step parameters"),
    (dict(prm=dict(blend_max=3.0, blend_min=3.0)), "bad step parameters"),
    (dict(prm=dict(blend_max=float("nan"))), "bad step parameters"),
]
HEAD_PAIRS = [
    (dict(B=-1, s="other"), "null solver / params or negative batch"),             # the batch before the horizon
    (dict(B=-1, s="far"), "null solver / params or negative batch"),
    (dict(s="far", prm=dict(threshold=-1)), "the solver's N must be in [3, 64] (the waypoint kernel's horizon)"),
    (dict(B=0, prm=dict(threshold=-1)), "bad step parameters"),                    # an empty batch passes only the checks of its arrays
]
BANK_PAIRS = [
    (dict(s="far", bank=None), "the solver's N must be in [3, 64] (the waypoint kernel's horizon)"),
    (dict(bank=None, prm=dict(threshold=-1)), "the bank is not set"),
    (dict(s="other", prm=dict(threshold=-1)), "the bank's horizon H must equal the solver's N"),
]
NULL_POSE = [dict(px=NULL), dict(yaw_rate=NULL), dict(steer=NULL)]
NULL_OUT = [dict(x_opt=NULL), dict(has_valid=NULL), dict(work=NULL), dict(ack=NULL), dict(status=NULL)]


def _rows(prefix, pairs):
    return [(over, EINVAL, prefix + what) for over, what in pairs]


def _nulls(prefix, overs, what="null array argument", **also):
    return [(dict(o, **also), EINVAL, prefix + what) for o in overs]


TABLE = {
    "step": _rows(STEP, HEAD) + _rows(STEP, [
        (dict(path=None), "the path is not set"),
        (dict(path=dict(M=1)), "the path is not set"),
        (dict(path=dict(curv=None)), "the path is not set"),
        (dict(s="other"), "the path horizon H must equal the solver's N"),
        (dict(path=dict(H=21)), "the path horizon H must equal the solver's N"),
        (dict(path=dict(dt=0.0)), "the path needs dt > 0"),
    ]) + _rows(STEP, STEP_PARAMS) + _nulls(STEP, NULL_POSE + NULL_OUT) + _rows(STEP, HEAD_PAIRS) + _rows(STEP, [
        (dict(s="far", path=None), "the solver's N must be in [3, 64] (the waypoint kernel's horizon)"),
        (dict(path=None, prm=dict(threshold=-1)), "the path is not set"),
        (dict(path=dict(H=21, dt=0.0)), "the path horizon H must equal the solver's N"),
        (dict(path=dict(dt=0.0), prm=dict(threshold=-1)), "the path needs dt > 0"),
        (dict(prm=dict(threshold=-1), px=NULL), "bad step parameters"),
    ]),
    "bank": _rows(BANK, HEAD + BANK_OF + STEP_PARAMS) + _nulls(BANK, [dict(tk=NULL)] + NULL_POSE + NULL_OUT) +
            _rows(BANK, HEAD_PAIRS + BANK_PAIRS + [(dict(prm=dict(threshold=-1), tk=NULL), "bad step parameters")]),
    "lane": _rows(LANE, LANE_PARAMS + HEAD + BANK_OF + STEP_PARAMS) + _nulls(LANE, [dict(tk=NULL)] + NULL_POSE + NULL_OUT) +
            _rows(LANE, HEAD_PAIRS + BANK_PAIRS + [
                (dict(lane=None, B=-1), "the lane parameters are not set"),      # the lane before the batch
                (dict(idx=NULL, s=None), "null lane_idx"),
                (dict(lane=dict(L=33), idx=NULL), "L must be in [34, 256]"),
            ]),
    # a rollout: its own lane and plant refusals, then the lane step's under the lane step's name, then its arrays, T, tally and counts
    "rollout": _rows(ROLL, LANE_PARAMS + PLANT_PARAMS) + _rows(LANE, HEAD + BANK_OF + STEP_PARAMS) +
               _nulls(ROLL, [dict(tk=NULL)] + NULL_POSE + NULL_OUT) + _rows(ROLL, [
                   (dict(T=-1), "T must be in [0, 4096]"),
                   (dict(T=4097), "T must be in [0, 4096]"),
                   (dict(tally=NULL), "null tally or counts"),
                   (dict(counts=NULL), "null tally or counts"),
                   (dict(lane=None, plant=None), "the lane parameters are not set"),
                   (dict(T=-1, tally=NULL), "T must be in [0, 4096]"),                 # T before the tally
                   (dict(T=-1, px=NULL), "null array argument"),                       # the arrays before T
                   (dict(T=-1, B=0), "T must be in [0, 4096]"),
               ]) + _rows(LANE, HEAD_PAIRS + BANK_PAIRS + [
                   (dict(B=-1, T=-1), "null solver / params or negative batch"),
                   (dict(prm=dict(threshold=-1), px=NULL), "bad step parameters"),
               ]) + _rows(ROLL, [
                   (dict(lane=None, B=-1), "the lane parameters are not set"),
                   (dict(plant=None, B=-1), "the plant parameters are not set"),
                   (dict(plant=dict(dt=0.0), s=None), "dt must be positive and finite"),
               ]),
    # the same with observation: its own parameters and model first; its arrays, tally and counts among them, last and under its name
    "observe": _rows(OBS, OBSERVE_PARAMS + [(dict(model=None), "null model")]) + _rows(ROLL, LANE_PARAMS + PLANT_PARAMS) +
               _rows(LANE, HEAD + BANK_OF + STEP_PARAMS) + _rows(ROLL, [
                   (dict(T=-1), "T must be in [0, 4096]"),
                   (dict(T=4097), "T must be in [0, 4096]"),
                   (dict(T=-1, tally=NULL), "T must be in [0, 4096]"),
                   (dict(T=-1, px=NULL), "T must be in [0, 4096]"),                    # unlike the plain rollout: its arrays come last
               ]) + _nulls(OBS, [dict(tk=NULL)] + NULL_POSE + NULL_OUT + [dict(tally=NULL), dict(counts=NULL), dict(prev=NULL),
                                                                             dict(samples=NULL), dict(bins=NULL), dict(dropped=NULL)]) +
               _rows(OBS, [
                   (dict(obs=None, model=None), "the observe parameters are not set"),
                   (dict(obs=dict(dt=0.0), lane=None), "dt must be positive and finite"),
                   (dict(model=None, lane=None), "null model"),
                   (dict(model=None, B=-1), "null model"),
               ]) + _rows(LANE, HEAD_PAIRS + BANK_PAIRS + [(dict(B=-1, T=-1), "null solver / params or negative batch")]),
    "plant": _rows(PLANT, PLANT_PARAMS + [
        (dict(model=None), "null model or negative batch"),
        (dict(B=-1), "null model or negative batch"),
        (dict(plant=None, model=None), "the plant parameters are not set"),
    ]) + _nulls(PLANT, [dict(ack=NULL), dict(mode=NULL)] + NULL_POSE),
}
# an empty batch and a rollout of no step return 0 behind the parameter checks and before those of the arrays
EMPTY = {
    "step": [dict(B=0), dict(B=0, px=NULL, work=NULL)],
    "bank": [dict(B=0), dict(B=0, tk=NULL, px=NULL, work=NULL)],
    "lane": [dict(B=0), dict(B=0, tk=NULL, px=NULL, work=NULL)],
    "rollout": [dict(B=0), dict(T=0), dict(B=0, px=NULL, tally=NULL), dict(T=0, tally=NULL, counts=NULL)],
    "observe": [dict(B=0), dict(T=0), dict(B=0, px=NULL, prev=NULL), dict(T=0, tally=NULL, samples=NULL)],
    "plant": [dict(B=0), dict(B=0, ack=NULL, px=NULL)],
}
POSE = ("px", "py", "yaw", "vx", "vy", "yaw_rate", "steer")
OUT = ("x_opt", "w_opt", "safe_count", "prev_u", "has_valid", "work", "ack", "mode", "valid", "status")


def _changed(struct, fields):
    """A copy of a ctypes structure with some fields set (a tuple sets an array field; None a pointer field to null)."""
    s = type(struct).from_buffer_copy(bytes(struct))
    for k, v in fields.items():
        setattr(s, k, type(getattr(s, k))(*v) if isinstance(v, tuple) else v)
    return s


def test_every_refusal_by_code_and_whole_message():
    import torch
    from ad_mpc_amd.config import AdmpcLaneParams, default_config
    from ad_mpc_amd.engine import BatchSolver
    road = TL._road(M=200)
    pose = TL._along(road, np.linspace(5, 100, B).astype(int), seed=70)
    ins = TP._poses(pose)
    tk = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    fc = TL._controller(N, B, learn=[dict(feat=[3], out=3, lo=[2.0], hi=[12.0], bins=[8], length_scale=2.0)])
    other = TL._controller(40, B)
    far = BatchSolver(default_config(N=80, Ts=TL.T_HORIZON / 80), device=0)
    L = fc.lib
    try:
        fc.set_traj(*road)
        fc.set_paths([road])
        other.set_paths([road])
        handles = dict(s=dict(other=other._eng._h, far=far._h), bank=dict(other=other._bank))
        blocks = dict(path=fc._path, prm=fc._prm, lane=AdmpcLaneParams(L=64, back=8, ahead=64), plant=fc._plant,
                      obs=fc._observe_params("rollout_route"))
        base = dict(s=fc._eng._h, bank=fc._bank, pm=None, model=fc._observer._h, B=B, T=2, tk=TL._p(tk), idx=TL._p(fc.lane_idx),
                    work=TL._p(fc._work), prev=TL._p(fc._prev))
        base.update({k: TL._p(t) for k, t in zip(POSE, ins)})
        base.update({k: TL._p(getattr(fc, k)) for k in OUT + ("cost", "tally", "counts", "samples", "bins", "dropped") if k != "work"})
        keep = []                                                       # the changed parameter blocks, alive while the library reads them

        def args(over):
            a, over = dict(base), dict(over)
            gp = over.pop("gp", None)
            if gp is not None:                                          # regressor 0 of the observe parameters
                over["obs"] = dict(gp=(_changed(blocks["obs"].gp[0], gp),) + tuple(blocks["obs"].gp)[1:])
            for k, blk in blocks.items():
                v = over.pop(k, {})
                keep.append(None if v is None else _changed(blk, v))
                a[k] = None if v is None else C.byref(keep[-1])
            for k, v in over.items():
                a[k] = handles[k][v] if isinstance(v, str) else v
            return a

        def call(entry, over):
            a = args(over)
            p, o, st = [a[k] for k in POSE], [a[k] for k in OUT], fc._eng._stream()
            roll = (a["s"], a["bank"], a["lane"], a["prm"], a["pm"], a["plant"], a["B"], a["T"], a["tk"], a["idx"], *p, *o, a["cost"],
                    a["tally"], a["counts"], None)
            if entry == "step":
                return L.admpc_control_step_batch(a["s"], a["path"], a["prm"], a["B"], *p, *o, st)
            if entry == "bank":
                return L.admpc_control_step_bank_batch(a["s"], a["bank"], a["prm"], a["B"], a["tk"], *p, *o, a["cost"], st)
            if entry == "lane":
                return L.admpc_control_step_lane_batch(a["s"], a["bank"], a["lane"], a["prm"], a["B"], a["tk"], a["idx"], *p, *o, a["cost"], st)
            if entry == "rollout":
                return L.admpc_rollout_lane_batch(*roll, st)
            if entry == "observe":
                return L.admpc_rollout_observe_lane_batch(*roll, a["model"], a["obs"], a["prev"], a["samples"], a["bins"], a["dropped"], st)
            return L.admpc_plant_step_batch(a["model"], a["plant"], a["B"], a["ack"], a["mode"], *p, st)

        def observed():
            return [getattr(fc, k).cpu().numpy().copy() for k in ("tally", "counts", "samples", "bins", "dropped", "_prev")]

        before, learnt = TL._state(fc), observed()
        wrong = []
        for entry, rows in TABLE.items():
            for over, code, msg in rows:
                rc = call(entry, over)
                got = L.admpc_last_error().decode()
                if (rc, got) != (code, msg):
                    wrong.append((entry, over, rc, got, msg))
            for over in EMPTY[entry]:
                rc = call(entry, over)
                if rc != 0:
                    wrong.append((entry, over, rc, L.admpc_last_error().decode(), "0"))
        assert not wrong, "\n".join("%s %r: %d %r, expected %r" % w for w in wrong)
        after = TL._state(fc)
        for k in TL.STATE:
            TL._bits(after[k], before[k], "%s after refused calls" % k)
        TL._bits(TP._host(ins), pose, "poses after refused calls")
        for a, b in zip(observed(), learnt):
            TL._bits(a, b, "tally, counts and the observation after refused calls")
    finally:
        fc.close(); other.close(); far.close()
