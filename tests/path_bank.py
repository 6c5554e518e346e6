"""Shared pieces of test_path_bank_cpu.py / test_path_bank_gpu.py: the rule of admpc_argmin_groups restated in numpy, the launch
lines of its kernel that the GPU tests' sizes mirror, and the layout of the control step's workspace."""
import numpy as np

# (source file under ad_mpc_amd/csrc, line): test_path_bank_cpu.py fails if one changes, as test_batch_regimes_cpu.py does for its own
LAUNCH_LINES = (
    ("admpc_kernels.hip", "#define ARGMIN_GROUPS_WAVES 4"),
    ("admpc_kernels.hip", "#define ARGMIN_GROUPS_GRID 256"),
    ("admpc_kernels.hip", "const bool packed = group <= 16;"),
    ("admpc_kernels.hip", "const int per_wave = packed ? 4 : 1;"),
    ("admpc_kernels.hip", "if (grid > ARGMIN_GROUPS_GRID) grid = ARGMIN_GROUPS_GRID;"),
)
ARGMIN_GROUPS_WAVES, ARGMIN_GROUPS_GRID, PACKED_MAX = 4, 256, 16


def groups_per_round(group):
    """Groups the largest grid of admpc_argmin_groups_kernel takes before its stride loop starts."""
    return ARGMIN_GROUPS_GRID * ARGMIN_GROUPS_WAVES * (4 if group <= PACKED_MAX else 1)


def groups_past(group):
    return groups_per_round(group) + 37


def group_argmin(cost, group):
    """The rule of admpc_argmin_groups: NaN is read as +inf, the lower cost wins, equal costs (-0.0 == 0.0, +inf == +inf) -> the lower
    index; val as read, idx into the batch.  numpy's argmin returns the first position of the minimum."""
    cost = np.asarray(cost, dtype=np.float64)
    G = cost.size // group
    assert G * group == cost.size
    c = np.where(np.isnan(cost), np.inf, cost).reshape(G, group)
    j = np.argmin(c, axis=1) if G else np.zeros(0, dtype=np.int64)
    return c[np.arange(G), j], (np.arange(G, dtype=np.int64) * group + j).astype(np.int64)


def step_work_views(work, B, N):
    """x0 [B,7], yref [B,N,9], yref_e [B,7], p [B] of the control step's workspace (StepWork of admpc_step.hip: ref [B][6][N], err [B][3],
    x0, yref, yref_e, p, each region rounded up to 32 doubles)."""
    al = lambda n: -(-n // 32) * 32
    o = al(B * 6 * N) + al(B * 3)
    out = []
    for shape in ((B, 7), (B, N, 9), (B, 7), (B,)):
        n = int(np.prod(shape))
        out.append(work[o:o + n].view(*shape))
        o += al(n)
    return out
