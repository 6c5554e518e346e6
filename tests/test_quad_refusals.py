"""Every refusal of the quadrotor's fleet and learning entry points (include/admpc_quad_fleet.h, include/admpc_quad_learn.h): return code
and WHOLE message, as a table, in the manner of tests/test_fleet_refusals.py.

The messages carry the name of the entry point whose check refuses, which is not always the one called (the observed rollout reports the
plain rollout's refusals under the plain rollout's name), and where two arguments are at fault the first check in the order of the
library wins; the pairs in each block pin that order.  The rows of HOST need neither a handle nor a device and run without a GPU, over
host buffers; with a GPU they run again among the rest, over the fleet's own arrays.  No row reaches the device: the fleet's state, tally
and learning buffers are compared bit for bit afterwards.  Refusals that need a second GPU (a bank or a model on another device) or a
failing HIP call are not reachable here."""
import ctypes as C
import os

import numpy as np
import pytest

import quad_learn_spec as QL

N, B, T = 10, 5, 2
EINVAL, ENODEV = -1, -2
PLANT, BANK, CHUNK, ROLL = ("admpc_quad_plant_step_batch: ", "admpc_quad_traj_bank_create: ", "admpc_quad_ref_chunk_batch: ",
                            "admpc_quad_rollout_batch: ")
LATCH, OBSERVE, FIT, INSTALL, OBSERVED = ("admpc_quad_observe_latch_batch: ", "admpc_quad_observe_batch: ", "admpc_quad_gp_fit: ",
                                          "admpc_quad_gp_install: ", "admpc_quad_rollout_observe_batch: ")
INF = float("inf")

# (argument overrides, message behind the prefix): the parameter blocks, refused by one function each under the caller's name.
# plant=None, obs=None: a null pointer; plant=dict(..), obs=dict(..): the block with these fields changed; gp, gp1: regressor 0, 1 of obs
PLANT_PARAMS = [
    (dict(plant=None), "the plant parameters are not set"),
    (dict(plant=dict(dt=0.0)), "dt must be positive and finite"),
    (dict(plant=dict(dt=INF)), "dt must be positive and finite"),
    (dict(plant=dict(substeps=0)), "substeps must be in [1, 1024]"),
    (dict(plant=dict(substeps=1025)), "substeps must be in [1, 1024]"),
    (dict(plant=dict(mass=0.0)), "mass and J must be positive"),
    (dict(plant=dict(J=(0.03, 0.0, 0.06))), "mass and J must be positive"),
    (dict(plant=dict(u_min=2.0)), "u_min <= u_max, both finite, required"),
    (dict(plant=dict(u_max=INF)), "u_min <= u_max, both finite, required"),
    (dict(plant=dict(drag=2)), "drag must be 0 or 1"),
    (dict(plant=dict(dt=0.0, substeps=0)), "dt must be positive and finite"),                     # the order within the block
    (dict(plant=dict(substeps=0, mass=0.0)), "substeps must be in [1, 1024]"),
    (dict(plant=dict(u_min=2.0, drag=2)), "u_min <= u_max, both finite, required"),
]
# the quadrotor's counterparts of OBSERVE_PARAMS in tests/test_fleet_refusals.py; regressor 0 has one feature, 7, over [-9, 9] in 32 bins
OBSERVE_PARAMS = [
    (dict(obs=None), "the observe parameters are not set"),
    (dict(obs=dict(dt=0.0)), "dt must be positive and finite"),
    (dict(obs=dict(dt=INF)), "dt must be positive and finite"),
    (dict(obs=dict(substeps=0)), "substeps must be in [1, 64]"),
    (dict(obs=dict(substeps=65)), "substeps must be in [1, 64]"),
    (dict(obs=dict(n_gp=0)), "n_gp must be in [1, 3]"),
    (dict(obs=dict(n_gp=4)), "n_gp must be in [1, 3]"),
    (dict(gp=dict(n_feat=0)), "regressor 0: n_feat must be in [1, 3]"),
    (dict(gp=dict(n_feat=4)), "regressor 0: n_feat must be in [1, 3]"),
    (dict(gp=dict(feat=(6, 0, 0))), "regressor 0: feat must be in [7, 16]"),
    (dict(gp=dict(feat=(17, 0, 0))), "regressor 0: feat must be in [7, 16]"),
    (dict(gp=dict(out=6)), "regressor 0: out must be in [7, 9]"),
    (dict(gp=dict(out=10)), "regressor 0: out must be in [7, 9]"),
    (dict(gp=dict(nb=(0, 1, 1))), "regressor 0: nb must be >= 1, and 1 for an unused feature"),
    (dict(gp=dict(nb=(8, 2, 1))), "regressor 0: nb must be >= 1, and 1 for an unused feature"),
    (dict(gp=dict(nb=(33, 1, 1))), "regressor 0: the product of nb must not exceed 32"),
    (dict(gp=dict(hi=(-9.0, 0.0, 0.0))), "regressor 0: lo and hi must be finite, hi > lo"),
    (dict(gp=dict(sigma_f=0.0)), "regressor 0: sigma_f must be positive and finite"),
    (dict(gp=dict(length=(0.0, 0.0, 0.0))), "regressor 0: length must be positive and finite"),
    (dict(gp=dict(noise=0.0)), "regressor 0: noise must be positive and finite"),
    (dict(gp=dict(count_noise=-1.0)), "regressor 0: count_noise must not be negative"),
    (dict(gp1=dict(out=6)), "regressor 1: out must be in [7, 9]"),
    (dict(obs=dict(dt=0.0, substeps=0, n_gp=9)), "dt must be positive and finite"),               # the order: dt, substeps, n_gp
    (dict(obs=dict(substeps=0, n_gp=9)), "substeps must be in [1, 64]"),
    (dict(obs=dict(n_gp=0), gp=dict(out=6)), "n_gp must be in [1, 3]"),
    (dict(gp=dict(n_feat=0, feat=(6, 0, 0))), "regressor 0: n_feat must be in [1, 3]"),           # the order within a regressor
    (dict(gp=dict(feat=(6, 0, 0), out=6)), "regressor 0: feat must be in [7, 16]"),
    (dict(gp=dict(out=6, nb=(0, 1, 1))), "regressor 0: out must be in [7, 9]"),
    (dict(gp=dict(nb=(33, 1, 1), hi=(-9.0, 0.0, 0.0))), "regressor 0: the product of nb must not exceed 32"),
    (dict(gp=dict(hi=(-9.0, 0.0, 0.0), sigma_f=0.0)), "regressor 0: lo and hi must be finite, hi > lo"),
    (dict(gp=dict(sigma_f=0.0, length=(0.0, 0.0, 0.0))), "regressor 0: sigma_f must be positive and finite"),
    (dict(gp=dict(length=(0.0, 0.0, 0.0), noise=0.0)), "regressor 0: length must be positive and finite"),
    (dict(gp=dict(noise=0.0, count_noise=-1.0)), "regressor 0: noise must be positive and finite"),
    (dict(gp=dict(noise=0.0), gp1=dict(out=6)), "regressor 0: noise must be positive and finite"),
]
# what the plain rollout refuses up to its arrays, in the order of its checks; `sqp` is a handle with sqp_iters = 3
ROLLOUT_HEAD = [
    (dict(s=None), "null solver"),
    (dict(s="sqp"), "a solver in SQP mode (sqp_iters > 1) is not served: the rollout is the RTI loop"),
    (dict(bank=None), "null bank"),
] + PLANT_PARAMS + [
    (dict(over=0), "over must be at least 1"),
    (dict(B=-1), "negative batch"),
    (dict(T=-1), "T must be in [0, 4096]"),
    (dict(T=4097), "T must be in [0, 4096]"),
    (dict(s=None, bank=None), "null solver"),
    (dict(s="sqp", bank=None), "a solver in SQP mode (sqp_iters > 1) is not served: the rollout is the RTI loop"),
    (dict(bank=None, plant=None), "null bank"),
    (dict(plant=None, over=0), "the plant parameters are not set"),
    (dict(plant=dict(substeps=0), over=0), "substeps must be in [1, 1024]"),
    (dict(over=0, B=-1), "over must be at least 1"),
    (dict(B=-1, T=-1), "negative batch"),
    (dict(T=-1, x=None), "T must be in [0, 4096]"),                                               # T before the arrays
    (dict(T=4097, x=None), "T must be in [0, 4096]"),
    (dict(T=-1, B=0), "T must be in [0, 4096]"),                                                  # and before the no-op
]
ROLLOUT_ARRAYS = ("traj_of", "idx", "x", "x_opt", "w_opt", "yref", "yref_e", "status")          # cost, iters and the records may be null


def _rows(prefix, pairs, code=EINVAL):
    return [(over, code, prefix + what) for over, what in pairs]


def _nulls(prefix, names, what="null array argument", **also):
    return [(dict({k: None}, **also), EINVAL, prefix + what) for k in names]


# the rows that need neither a handle nor a device
HOST = {
    "plant": _rows(PLANT, PLANT_PARAMS + [
        (dict(B=-1), "negative batch"),
        (dict(plant=None, B=-1), "the plant parameters are not set"),
        (dict(plant=dict(substeps=0), B=-1), "substeps must be in [1, 1024]"),
        (dict(B=-1, u=None), "negative batch"),
        (dict(u=None, stride=3), "null array argument"),
        (dict(x=None), "null array argument"),
        (dict(stride=3), "u_stride must be at least 4"),
    ]),
    "latch": _rows(LATCH, [(dict(B=-1), "negative batch"), (dict(B=-1, x=None), "negative batch")]) + _nulls(LATCH, ["x", "prev"]),
    "observe": _rows(OBSERVE, OBSERVE_PARAMS + PLANT_PARAMS + [
        (dict(obs=None, plant=None), "the observe parameters are not set"),
        (dict(obs=dict(substeps=0), plant=None), "substeps must be in [1, 64]"),
        (dict(plant=None, model=None), "the plant parameters are not set"),
        (dict(plant=dict(substeps=0), model=None), "substeps must be in [1, 1024]"),
        (dict(plant=None, B=-1), "the plant parameters are not set"),
    ]),
    "fit": _rows(FIT, OBSERVE_PARAMS + [
        (dict(min_count=0), "min_count must be at least 1"),
        (dict(obs=dict(substeps=0), min_count=0), "substeps must be in [1, 64]"),
        (dict(obs=dict(dt=0.0), min_count=0, bins=None), "dt must be positive and finite"),
        (dict(min_count=0, bins=None), "min_count must be at least 1"),
    ]) + _nulls(FIT, ["bins", "gp_dev", "info"]),
}
HOST_EMPTY = {
    "plant": [dict(B=0), dict(B=0, u=None), dict(B=0, u=None, x=None, stride=3)],
    "latch": [dict(B=0), dict(B=0, x=None, prev=None)],
}
# the rows that need a handle or a device; `nominal` is the fleet's model handle, created without GPs
DEVICE = {
    "plant": [(dict(dev=99), ENODEV, "no such device"), (dict(dev=-1), ENODEV, "no such device")],
    "chunk": _rows(CHUNK, [
        (dict(bank=None), "null bank"),
        (dict(B=-1), "negative batch"),
        (dict(N=1), "N must be in [2, 24]"),
        (dict(N=25), "N must be in [2, 24]"),
        (dict(over=0), "over must be at least 1"),
        (dict(bank=None, B=-1), "null bank"),
        (dict(B=-1, N=1), "negative batch"),
        (dict(N=1, over=0), "N must be in [2, 24]"),
        (dict(over=0, yref=None), "over must be at least 1"),
    ]) + _nulls(CHUNK, ["traj_of", "idx", "yref", "yref_e"]),
    "rollout": _rows(ROLL, ROLLOUT_HEAD) + _nulls(ROLL, ROLLOUT_ARRAYS) + _nulls(ROLL, ROLLOUT_ARRAYS, tally=None) + _rows(ROLL, [
        (dict(tally=None), "null tally or counts"),
        (dict(counts=None), "null tally or counts"),
    ]),
    "observe": _rows(OBSERVE, [
        (dict(model=None), "null model"),
        (dict(model=None, B=-1), "null model"),
        (dict(B=-1), "negative batch"),
        (dict(B=-1, u=None), "negative batch"),
        (dict(u=None, stride=3), "null array argument"),
        (dict(stride=3), "u_stride must be at least 4"),
    ]) + _nulls(OBSERVE, ["u", "x", "prev", "samples", "bins", "dropped"]),
    "install": _rows(INSTALL, [
        (dict(s=None), "null solver"),
        (dict(s=None, n_gp=0), "null solver"),
        (dict(s="nominal"), "n_gp = 3, but the handle was created with 0 GPs (create it with placeholder GPs of n_points = 0)"),
        (dict(s="nominal", gp_dev=None), "n_gp = 3, but the handle was created with 0 GPs (create it with placeholder GPs of n_points = 0)"),
        (dict(s="nominal", n_gp=0), "n_gp = 0, but the handle was created with 0 GPs (create it with placeholder GPs of n_points = 0)"),
        (dict(n_gp=2, gp_dev=None), "n_gp = 2, but the handle was created with 3 GPs (create it with placeholder GPs of n_points = 0)"),
        (dict(n_gp=0, gp_dev=None), "n_gp = 0, but the handle was created with 3 GPs (create it with placeholder GPs of n_points = 0)"),
        (dict(n_gp=4), "n_gp = 4, but the handle was created with 3 GPs (create it with placeholder GPs of n_points = 0)"),
    ]) + _nulls(INSTALL, ["gp_dev", "installed"]),
    # the observed rollout: its own parameters and model first; then the plain rollout's refusals up to its arrays, under the plain
    # rollout's name; its arrays, tally and counts among them, last and under its own name
    "observed": _rows(OBSERVED, OBSERVE_PARAMS + [
        (dict(model=None), "null model"),
        (dict(obs=None, model=None), "the observe parameters are not set"),
        (dict(obs=dict(substeps=0), model=None), "substeps must be in [1, 64]"),
        (dict(obs=None, s=None), "the observe parameters are not set"),
        (dict(model=None, s=None), "null model"),
        (dict(model=None, B=-1), "null model"),
    ]) + _rows(ROLL, ROLLOUT_HEAD + [
        (dict(T=-1, tally=None), "T must be in [0, 4096]"),
        (dict(B=-1, x=None), "negative batch"),
    ]) + _nulls(OBSERVED, ROLLOUT_ARRAYS + ("tally", "counts", "prev", "samples", "bins", "dropped")) + _rows(OBSERVED, [
        (dict(x=None, tally=None), "null array argument"),
    ]),
}
# an empty batch and a rollout of no step return 0 behind the other checks and before those of the arrays
DEVICE_EMPTY = {
    "chunk": [dict(B=0), dict(B=0, yref=None, traj_of=None)],
    "rollout": [dict(B=0), dict(T=0), dict(B=0, x=None), dict(T=0, x=None, tally=None)],
    "observe": [dict(B=0), dict(B=0, u=None, x=None), dict(B=0, u=None, stride=3)],
    "observed": [dict(B=0), dict(T=0), dict(B=0, x=None, prev=None), dict(T=0, x=None, prev=None), dict(T=0, tally=None, samples=None)],
}


def _changed(struct, fields):
    """A copy of a ctypes structure with some fields set (a tuple sets an array field)."""
    s = type(struct).from_buffer_copy(bytes(struct))
    for k, v in fields.items():
        setattr(s, k, type(getattr(s, k))(*v) if isinstance(v, tuple) else v)
    return s


class _Caller:
    """Calls an entry point by name with `base` changed by a row's overrides."""

    def __init__(self, L, base, blocks, handles, stream):
        self.L, self.base, self.blocks, self.handles, self.stream = L, base, blocks, handles, stream
        self.keep = []                                                  # the changed parameter blocks, alive while the library reads them

    def args(self, over):
        a, over = dict(self.base), dict(over)
        gps = {g: over.pop(k) for g, k in enumerate(("gp", "gp1")) if k in over}
        if gps:                                                         # regressors of the observe parameters
            obs = self.blocks["obs"]
            gp = tuple(_changed(b, gps.get(g, {})) for g, b in enumerate(obs.gp))
            over["obs"] = dict(over.get("obs") or {}, gp=gp)
        for k, blk in self.blocks.items():
            v = over.pop(k, {})
            self.keep.append(None if v is None else _changed(blk, v))
            a[k] = None if v is None else C.byref(self.keep[-1])
        for k, v in over.items():
            a[k] = self.handles[v] if isinstance(v, str) else v
        return a

    def __call__(self, entry, over):
        a, L, st = self.args(over), self.L, self.stream
        roll = (a["s"], a["bank"], a["plant"], a["over"], a["B"], a["T"], a["traj_of"], a["idx"], a["x"], a["x_opt"], a["w_opt"], a["yref"],
                a["yref_e"], a["cost"], a["status"], a["iters"], a["tally"], a["counts"], None, None)
        if entry == "plant":
            return L.admpc_quad_plant_step_batch(a["plant"], a["dev"], a["B"], a["u"], a["stride"], a["x"], st)
        if entry == "chunk":
            return L.admpc_quad_ref_chunk_batch(a["bank"], a["B"], a["N"], a["over"], a["traj_of"], a["idx"], a["yref"], a["yref_e"], None, st)
        if entry == "rollout":
            return L.admpc_quad_rollout_batch(*roll, st)
        if entry == "latch":
            return L.admpc_quad_observe_latch_batch(a["dev"], a["B"], a["x"], a["prev"], st)
        if entry == "observe":
            return L.admpc_quad_observe_batch(a["model"], a["plant"], a["obs"], a["B"], a["u"], a["stride"], a["x"], a["prev"], a["samples"],
                                              a["bins"], a["dropped"], st)
        if entry == "fit":
            return L.admpc_quad_gp_fit(a["dev"], a["obs"], a["min_count"], a["bins"], a["gp_dev"], a["info"], st)
        if entry == "install":
            return L.admpc_quad_gp_install(a["s"], a["n_gp"], a["gp_dev"], a["installed"], st)
        assert entry == "observed", entry
        return L.admpc_quad_rollout_observe_batch(*roll, a["model"], a["obs"], a["prev"], a["samples"], a["bins"], a["dropped"], st)

    def wrong(self, table, empty):
        """The rows of `table` that are not refused by their code and whole message, and the no-ops of `empty` that do not return 0."""
        bad = []
        for entry, rows in table.items():
            for over, code, msg in rows:
                rc = self(entry, over)
                got = self.L.admpc_last_error().decode()
                if (rc, got) != (code, msg):
                    bad.append((entry, over, rc, got, msg))
        for entry, overs in empty.items():
            for over in overs:
                rc = self(entry, over)
                if rc != 0:
                    bad.append((entry, over, rc, self.L.admpc_last_error().decode(), "0"))
        return bad


def _blocks():
    from ad_mpc_amd.quad_config import AdmpcQuadObserveParams, SimQuad, quad_learn_bins, quad_plant_params
    bins, n_gp = quad_learn_bins(QL.EXP_LEARN)
    return dict(plant=quad_plant_params(SimQuad(drag=True), 5e-4, 0.02), obs=AdmpcQuadObserveParams(dt=0.02, substeps=1, n_gp=n_gp, gp=bins))


def _report(wrong):
    return "\n".join("%s %r: %d %r, expected %r" % w for w in wrong)


def test_the_refusals_that_need_neither_a_handle_nor_a_device():
    """HOST over host buffers, every handle null: no call gets as far as the device it names."""
    import torch  # noqa: F401  (in front of the library: where this process goes on to the GPU, the library loaded first finds no HIP device)
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    d, i = (C.c_double * (B * N * 17))(), (C.c_int32 * 16)()
    base = dict(s=None, bank=None, model=None, dev=0, B=B, T=T, N=N, over=5, stride=N * 4, min_count=1, n_gp=3, gp_dev=d, info=i, installed=i)
    base.update({k: d for k in ("u", "x", "x_opt", "w_opt", "yref", "yref_e", "cost", "tally", "prev", "samples", "bins")})
    base.update({k: i for k in ("traj_of", "idx", "status", "iters", "counts", "dropped")})
    call = _Caller(L, base, _blocks(), {}, None)
    wrong = call.wrong(HOST, HOST_EMPTY)
    assert not wrong, _report(wrong)
    assert not any(d) and not any(i)


def _bank_rows(L):
    """admpc_quad_traj_bank_create over host arrays: (what, return code, message, the handle it left)."""
    x, u = np.zeros((2, 13)), np.zeros((2, 4))
    tp, up, none = (C.c_void_p * 1)(x.ctypes.data), (C.c_void_p * 1)(u.ctypes.data), (C.c_void_p * 1)(None)
    two, zero = (C.c_int32 * 1)(2), (C.c_int32 * 1)(0)
    rows = [
        (dict(M=None), EINVAL, BANK + "null argument"),
        (dict(traj=None), EINVAL, BANK + "null argument"),
        (dict(u=None), EINVAL, BANK + "null argument"),
        (dict(bank=None), EINVAL, BANK + "null argument"),
        (dict(K=0), EINVAL, BANK + "K must be at least 1"),
        (dict(M=zero), EINVAL, BANK + "every trajectory needs M >= 1 rows"),
        (dict(traj=none), EINVAL, BANK + "null trajectory"),
        (dict(u=none), EINVAL, BANK + "null trajectory"),
        (dict(dev=99), ENODEV, "no such device"),
        (dict(dev=-1), ENODEV, "no such device"),
        (dict(M=None, K=0), EINVAL, BANK + "null argument"),                                      # the order
        (dict(K=0, M=zero), EINVAL, BANK + "K must be at least 1"),
        (dict(M=zero, traj=none), EINVAL, BANK + "every trajectory needs M >= 1 rows"),
        (dict(traj=none, dev=99), EINVAL, BANK + "null trajectory"),
    ]
    wrong = []
    for over, code, msg in rows:
        h = C.c_void_p(0)
        a = dict(dev=0, K=1, M=two, traj=tp, u=up, bank=C.byref(h))
        a.update(over)
        rc = L.admpc_quad_traj_bank_create(a["dev"], a["K"], a["M"], a["traj"], a["u"], a["bank"])
        got = L.admpc_last_error().decode()
        if (rc, got) != (code, msg) or h.value:
            wrong.append(("bank", {k: "..." for k in over}, rc, got, msg))
    L.admpc_quad_traj_bank_destroy(None)
    return wrong, len(rows)


@pytest.mark.gpu
def test_every_refusal_by_code_and_whole_message():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import test_quad_fleet_gpu as TQ
    import test_quad_learn_gpu as TG
    from ad_mpc_amd.engine import QuadBatchSolver
    from ad_mpc_amd.quad_config import default_quad_config
    trajs = TQ._circles(N, 3.0)
    traj_of, idx0 = np.zeros(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    fl = TG._learning_fleet(B, N, trajs, traj_of, idx0, None)
    sqp_cfg = default_quad_config(); sqp_cfg.sqp_iters = 3
    sqp = QuadBatchSolver(sqp_cfg)
    L, p = fl.lib, TQ._p
    try:
        base = dict(s=fl._eng._h, bank=fl._bank, model=fl._nominal._h, dev=0, B=B, T=T, N=N, over=5, stride=N * 4, min_count=1, n_gp=3,
                    u=p(fl.w_opt), prev=p(fl._prev), gp_dev=p(fl._gp_dev), info=p(fl.fit_info))
        base.update({k: p(getattr(fl, k)) for k in ROLLOUT_ARRAYS + ("cost", "iters", "tally", "counts", "samples", "bins", "dropped", "installed")})
        call = _Caller(L, base, dict(plant=fl._plant, obs=fl._obs), dict(sqp=sqp._h, nominal=fl._nominal._h), fl._stream())
        watched = TQ.STATE + ("tally", "cost", "iters", "fit_info", "installed", "_gp_dev") + TG.LEARN_STATE
        torch.cuda.synchronize()
        before = {k: getattr(fl, k).cpu().numpy().copy() for k in watched}
        wrong = call.wrong(HOST, HOST_EMPTY) + call.wrong(DEVICE, DEVICE_EMPTY)
        bank_wrong, n_bank = _bank_rows(L)
        rows = sum(len(r) for t in (HOST, DEVICE) for r in t.values()) + sum(len(r) for t in (HOST_EMPTY, DEVICE_EMPTY) for r in t.values()) + n_bank
        print("%d rows" % rows)
        assert not wrong + bank_wrong, _report(wrong + bank_wrong)
        torch.cuda.synchronize()
        for k, v in before.items():
            TQ._bits(getattr(fl, k).cpu().numpy(), v, "%s after refused calls" % k)
    finally:
        fl.close(); sqp.close()
