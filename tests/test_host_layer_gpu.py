"""The Python host layer on the device: the AcadosOcpSolver-shaped seam through its one staging buffer against the batch engine, bit for
bit, and the argument checks in front of every solve entry of the four solver classes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from ad_mpc_amd.config import default_config, NX, NU  # noqa: E402
from ad_mpc_amd.quad_config import default_quad_config, QNX, QNU, QNY  # noqa: E402
from ad_mpc_amd.scenarios import grid_gp, random_scenarios  # noqa: E402


@pytest.mark.parametrize("shift", [None, "rollout"])
@pytest.mark.parametrize("N", [20, 5])          # (N + 1) * 7 = 147 and 42 doubles: both padded to the next multiple of 32
def test_seam_equals_the_engine_bit_for_bit(N, shift):
    """AdmpcOcpSolver.solve (B = 1 on addresses into its staging buffer) against BatchSolver.solve_with_multipliers on tensors of their
    own: iterate, multipliers, cost, status and iteration count are equal bit for bit, and so is a second solve from the iterate the
    first one left in the buffer.  With shift_iterate = "rollout": against BatchSolver.shift followed by the step."""
    import torch
    from ad_mpc_amd.engine import BatchSolver
    from ad_mpc_amd.ocp_solver import AdmpcOcpSolver
    cfg = default_config(N=N)
    s = random_scenarios(1, N, seed=100 + N)
    sol, eng = AdmpcOcpSolver(cfg), BatchSolver(cfg)
    sol.shift_iterate = shift
    for k in range(N):
        sol.set(k, "yref", s["yref"][0, k]); sol.set(k, "u", s["ubar"][0, k])
    sol.set(N, "yref", s["yref_e"][0])
    sol.set(0, "lbx", s["x0"][0]); sol.set(0, "ubx", s["x0"][0])
    for k in range(N + 1):
        sol.set(k, "p", np.array([s["p"][0]])); sol.set(k, "x", s["xbar"][0, k])
    d = eng.to_device
    x0, yref, yref_e, p, xb, ub = (d(s[k]) for k in ("x0", "yref", "yref_e", "p", "xbar", "ubar"))
    cost = torch.empty(1, dtype=torch.float64, device=eng.device); st = torch.empty(1, dtype=torch.int32, device=eng.device); it = torch.empty_like(st)
    for step in range(2):                        # the second step starts from what the first one left behind, on both sides
        status = sol.solve()
        if shift is not None:
            eng.shift(xb, ub, p, rollout=True)
        pi, ineq = eng.solve_with_multipliers(x0, yref, yref_e, p, xb, ub, cost, st, it)
        torch.cuda.synchronize()
        assert int(st[0]) == 0, "the scenario must solve: a failed step adopts no iterate"
        assert status == sol.get_stats("status") == int(st[0]) and sol.get_stats("qp_iter") == int(it[0])
        assert sol.get_cost() == float(cost[0])
        for name, got, want in (("x", sol._x, xb), ("u", sol._u, ub), ("pi", sol._pi, pi), ("ineq", sol._ineq, ineq)):
            assert np.array_equal(got, want[0].cpu().numpy()), "%s differs at step %d" % (name, step)
        assert np.abs(sol._u - s["ubar"][0]).max() > 1e-3          # the iterate moved
    eng.close()


def _assert_rejected(call, args, name, bad, outputs):
    """`call(**args)` with `args[name]` replaced by `bad` raises ValueError before any kernel runs: every output keeps its sentinel."""
    import torch
    before = [t.clone() for t in outputs]
    with pytest.raises(ValueError, match="expected contiguous"):
        call(**dict(args, **{name: bad}))
    torch.cuda.synchronize()
    for t, b in zip(outputs, before):
        assert torch.equal(t, b)
    if name == "status":
        assert (bad == -7).all()


def _sentinels(B, N, nx, nu):
    import torch
    f = lambda *shape: torch.full(shape, 7.25, dtype=torch.float64, device="cuda")
    i = lambda: torch.full((B,), -7, dtype=torch.int32, device="cuda")
    return dict(xbar=f(B, N + 1, nx), ubar=f(B, N, nu), cost=f(B), status=i(), iters=i())


def _reject_both(call, args, yref_shape, outputs=None):
    import torch
    outputs = [args[k] for k in ("xbar", "ubar", "cost", "status", "iters") if k in args] if outputs is None else outputs
    _assert_rejected(call, args, "yref", torch.zeros(yref_shape, dtype=torch.float64, device="cuda"), outputs)
    if "status" in args:
        _assert_rejected(call, args, "status", torch.full((args["status"].shape[0],), -7, dtype=torch.int64, device="cuda"), outputs)


B, N = 3, 5


def _car_args():
    import torch
    s = random_scenarios(B, N, seed=5)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return dict(x0=d(s["x0"]), yref=d(s["yref"]), yref_e=d(s["yref_e"]), p=d(s["p"]), **_sentinels(B, N, NX, NU))


def _quad_args():
    import torch
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    return dict(x0=z(B, QNX), yref=z(B, N, QNY), yref_e=z(B, QNX), **_sentinels(B, N, QNX, QNU))


def test_batch_solver_rejects_a_wrong_tensor_on_every_solve_entry():
    import torch
    from ad_mpc_amd.engine import BatchSolver
    eng = BatchSolver(default_config(N=N))
    a = _car_args()
    _reject_both(eng.solve, a, (B, N + 1, 9))
    _reject_both(eng.solve_with_multipliers, a, (B, N, 8))          # its cost / status / iters are checked like solve's
    for k, bad in (("cost", torch.zeros(B + 1, dtype=torch.float64, device="cuda")), ("iters", torch.zeros(B, dtype=torch.int64, device="cuda"))):
        _assert_rejected(eng.solve_with_multipliers, a, k, bad, [a[k] for k in ("xbar", "ubar", "cost", "status", "iters")])
    r = {k: a[k] for k in ("x0", "yref", "yref_e", "p", "xbar", "ubar")}
    r.update(pi=torch.full((B, N + 1, NX), 7.25, dtype=torch.float64, device="cuda"), ineq=torch.full((B, N, 20), 7.25, dtype=torch.float64, device="cuda"))
    _reject_both(eng.nlp_residuals, r, (B, N), outputs=[])
    eng.close()


def test_ensemble_solver_rejects_a_wrong_tensor():
    import torch
    from ad_mpc_amd.engine import EnsembleBatchSolver
    from ad_mpc_amd.gp_loader import GPEnsemble
    ens = EnsembleBatchSolver(default_config(N=N), GPEnsemble([grid_gp(seed=1), grid_gp(seed=2)], [[4.0], [10.0]], 3))
    assert len(ens.solvers) == 2 and ens.N == N
    a = dict(_car_args(), gp_ind=torch.zeros(B, dtype=torch.int32, device="cuda"))
    _reject_both(ens.solve, a, (B, N, 8))
    ens.close()


def _quad_gps(seed):
    rng = np.random.default_rng(seed)
    return [dict(feat=7 + i, out=7 + i, Z=np.linspace(-3, 3, 15), alpha=0.3 * rng.standard_normal(15), length_scale=1.0, sigma_f=1.0, ymean=0.01 * i)
            for i in range(3)]


def test_quad_solver_rejects_a_wrong_tensor():
    from ad_mpc_amd.engine import QuadBatchSolver
    cfg = default_quad_config(N=N)
    eng = QuadBatchSolver(cfg)
    _reject_both(eng.solve, _quad_args(), (B, N, QNX))
    eng.close()


def test_quad_ensemble_solver_rejects_a_wrong_tensor():
    import torch
    from ad_mpc_amd.engine import QuadEnsembleBatchSolver
    cfg = default_quad_config(N=N)
    ens = QuadEnsembleBatchSolver(cfg, [_quad_gps(1), _quad_gps(2)], [[-1.0], [1.0]], [7])
    assert len(ens.solvers) == 2 and ens.N == N
    a = dict(_quad_args(), gp_ind=torch.zeros(B, dtype=torch.int32, device="cuda"))
    _reject_both(ens.solve, a, (B, N, QNX))
    ens.close()
