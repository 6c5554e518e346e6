"""Times solver_type "SQP" inside the one-wave solve kernel (include/admpc_quad_sqp.h; QuadBatchSolver.set_sqp) against what it replaces
and against the RTI loop, N = 10.

  A. one solve at B = 4096 and at B = 1, (qp_max, tol) = (100, 1e-6), on random_quad_scenarios(B, cfg, seed=7, pos_err=0.8, tilt=0.2,
     aggressive=0.0) -- the family of the tests: `host`, a handle built with cfg.sqp_iters = 100, sqp_tol = 1e-6 (four launches per QP,
     the linearisation through global memory), against `kernel`, a handle with set_sqp(100, 1e-6) (one launch).  A call is: the iterate
     put back to its start (two device copies, in both forms), the solve, a stream synchronisation; wall time by the host clock, the
     median of `--calls` calls per window.  The two forms ALTERNATE, three windows each: median, smallest, largest of the three.  With it
     the mean and the largest qps, and whether the two forms returned the same bits.
  B. rollout_targets at B = 4096, drag on: a period of a fleet in "SQP" (terminal_cost on, as the reference's point tracking sets it)
     against a period of the same fleet in "SQP_RTI", as captured graphs of `--steps` periods replayed, alternating, three times each.
     After T = 60 periods from the reference's start state (a run of its own, eager): the mean qps per period, the targets reached and
     the mean periods per reached target, for both.

The kernels' own times come from running `rocprofv3 --kernel-trace --stats -- python scripts/quad_sqp_time.py --brief` in a run of its
own (--brief: part A alone, two calls of each form and batch size behind one warm-up call).

    python scripts/quad_sqp_time.py [--calls 5] [--steps 5] [--replays 4] [--windows 5] [--brief] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from quad_rollout_time import B, OVER, emit, graph_capture, graph_measure  # noqa: E402  (puts the repository root on sys.path)
from quad_clusters_time import three  # noqa: E402
from ad_mpc_amd.engine import QuadBatchSolver  # noqa: E402
from ad_mpc_amd.quad_config import SimQuad, default_quad_config  # noqa: E402
from ad_mpc_amd.quad_fleet import QuadFleet  # noqa: E402
from ad_mpc_amd.quad_scenarios import random_quad_scenarios  # noqa: E402

N, MODE, T_FLIGHT = 10, (100, 1e-6), 60


def solve_forms(nb, a):
    cfg = default_quad_config(N=N)
    s = random_quad_scenarios(nb, cfg, seed=7, pos_err=0.8, tilt=0.2, aggressive=0.0)
    hc = cfg.copy(); hc.sqp_iters, hc.sqp_tol = MODE
    host, kern = QuadBatchSolver(hc), QuadBatchSolver(cfg)
    kern.set_sqp(*MODE)
    d = lambda k: torch.as_tensor(np.ascontiguousarray(s[k]), device=host.device)
    x0, yr, ye, xs, us = d("x0"), d("yref"), d("yref_e"), d("xbar"), d("ubar")
    out = {}
    for name in ("host", "kernel"):
        out[name] = dict(x=xs.clone(), u=us.clone(), cost=torch.zeros(nb, dtype=torch.float64, device=host.device),
                         st=torch.zeros(nb, dtype=torch.int32, device=host.device), it=torch.zeros(nb, dtype=torch.int32, device=host.device))
    qps = torch.zeros(nb, dtype=torch.int32, device=host.device)

    def call(name):
        o = out[name]
        o["x"].copy_(xs); o["u"].copy_(us)
        if name == "host":
            host.solve(x0, yr, ye, o["x"], o["u"], o["cost"], o["st"], o["it"])
        else:
            kern.solve_sqp(x0, yr, ye, o["x"], o["u"], o["cost"], o["st"], o["it"], qps=qps)
        torch.cuda.current_stream().synchronize()

    def window(name, calls):
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call(name)
            t.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(t))

    for name in ("host", "kernel"):                                # warm-up: code objects, the host loop's workspace
        call(name)
    meds = {"host": [], "kernel": []}
    for _ in range(1 if a.brief else 3):
        for name in ("host", "kernel"):
            meds[name].append(window(name, 2 if a.brief else a.calls))
    r = {name: three(v) for name, v in meds.items()}
    r["host_over_kernel"] = r["host"][0] / r["kernel"][0]
    q, st = qps.cpu().numpy(), out["kernel"]["st"].cpu().numpy()
    r["qps_mean"], r["qps_max"] = float(q.mean()), int(q.max())
    r["statuses_0_2_4"] = [int((st == v).sum()) for v in (0, 2, 4)]
    r["same_bits"] = all(bool(torch.equal(out["host"][k], out["kernel"][k])) for k in ("x", "u", "cost", "st", "it"))
    host.close(); kern.close()
    return r


def flight(a):
    make = lambda kind: QuadFleet(B, quad=SimQuad(drag=True), n_nodes=N, reference_over_sampling=OVER, solver_type=kind, terminal_cost=True, sqp=MODE)
    r = {}
    # the flight itself: T_FLIGHT periods, one at a time, so that the QPs of every period can be read
    for kind in ("SQP", "SQP_RTI"):
        fl = make(kind)
        fl.set_targets(seed=7)
        fl.reset_targets()
        qps = torch.zeros(B, dtype=torch.int32, device=fl.device)
        per = []
        for _ in range(T_FLIGHT):
            xo, wo = fl.x_opt.clone(), fl.w_opt.clone()
            out = fl.rollout_targets(1, record=True)
            if kind == "SQP":                                      # the period's solve once more, on copies of what it started from, for its qps
                fl._eng.solve_sqp(out.traj[0].contiguous(), fl.yref, fl.yref_e, xo, wo, qps=qps)
                per.append(float(qps.double().mean()))
        tc = fl.tcounts.cpu().numpy()
        reached = int(tc[:, 0].sum())
        r[kind] = {"targets_reached": reached, "recoveries": int(tc[:, 1].sum()), "status_nonzero_periods": int(tc[:, 3].sum()),
                   "periods_per_target": B * T_FLIGHT / max(reached, 1)}
        if per:
            r[kind]["qps_mean_per_period"] = float(np.mean(per))
            r[kind]["qps_mean_first_and_last_period"] = [per[0], per[-1]]
        fl.close()
    # the period's time: graphs of a.steps periods from the start state, alternating
    fleets = {kind: make(kind) for kind in ("SQP", "SQP_RTI")}
    graphs = {}
    for kind, fl in fleets.items():
        fl.set_targets(seed=7)
        fl.reset_targets()
        graphs[kind] = graph_capture(lambda fl=fl: fl.rollout_targets(a.steps), a.replays)
    meds = {kind: [] for kind in fleets}
    for _ in range(3):
        for kind in fleets:
            meds[kind].append(graph_measure(graphs[kind], a.steps, a.replays, a.windows)[0])
    for kind in fleets:
        r[kind]["period_us"] = three(meds[kind])
        fleets[kind].close()
    r["sqp_over_rti"] = r["SQP"]["period_us"][0] / r["SQP_RTI"]["period_us"][0]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--replays", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "quad_sqp_time.py measures on the GPU"
    res = {"case": "N = %d, (qp_max, tol) = (%d, %g); A: one solve, host loop against in-kernel loop; B: rollout_targets at B = %d, drag on, "
                   "aggressive targets (R = 3 m, 5 cm), terminal cost on" % ((N,) + MODE + (B,)),
           "calls_per_window": a.calls, "steps_per_graph": a.steps, "replays_per_window": a.replays, "windows": a.windows, "alternations": 3,
           "microseconds": "median, smallest, largest of three", "device": torch.cuda.get_device_name(0)}
    for nb in (4096, 1):
        res["solve_B%d" % nb] = solve_forms(nb, a)
    if not a.brief:
        res["rollout_targets"] = flight(a)
    emit(res, a.out)


if __name__ == "__main__":
    main()
