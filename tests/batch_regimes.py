"""The batch sizes at which the solve kernels change regime, mirrored from their launch code.

Each formula below copies one launch line of the library; LAUNCH_LINES names them, and test_batch_regimes_cpu.py fails if one of
them changes, so that the boundary cases of test_batch_regimes.py cannot drift to the wrong side quietly.

Where the grid depends on the LDS footprint of a kernel (kernel S, the quadrotor kernels), `lds` may be None: the helpers then
return the smallest and largest grid any footprint allows, and the tests pick batches below the smallest (no work order, no
tickets, no stride) or above what the largest allows (work order / tickets for every footprint).
"""

LDS_BYTES = 160 * 1024

# (source file under ad_mpc_amd/csrc, function, line of that function that a formula here copies)
LAUNCH_LINES = (
    ("admpc_fused20.hip", "admpc_fused20_launch", "int grid = num_cu * 8; if (grid > B) grid = B;"),
    ("admpc_fused20.hip", "admpc_fused20_launch", "const int kcap = grid == B ? 0 : cap;"),
    ("admpc_seg.hip", "seg_launch", "int per_cu = (160 * 1024) / lds;"),
    ("admpc_seg.hip", "seg_launch", "if (per_cu > 8 / S) per_cu = 8 / S;"),
    ("admpc_seg.hip", "seg_launch", "if (per_cu < 1) per_cu = 1;"),
    ("admpc_seg.hip", "seg_launch", "int grid = num_cu * per_cu; if (grid > B) grid = B;"),
    ("admpc_seg.hip", "seg_launch", "const int kcap = grid == B ? 0 : cap;"),
    ("admpc_quad.hip", "quad_solve", "int per_cu = (160 * 1024) / ldsb; if (per_cu > (seg20 ? 4 : 8)) per_cu = seg20 ? 4 : 8; if (per_cu < 1) per_cu = 1;"),
    ("admpc_quad.hip", "quad_solve", "int grid = s->num_cu * per_cu; if (grid > B) grid = B;"),
    ("admpc_quad.hip", "quad_solve", "int* ticket = B > 8 * grid ? s->d_ticket : nullptr;"),
    ("admpc_quad.hip", "admpc_quad_solve_batch_ex", "int gridS = s->num_cu * 2; if (gridS > B) gridS = B;"),
    ("admpc_kernels.hip", "solve_rows", "hipLaunchKernelGGL(admpc_nlp_res_kernel<T>, dim3(nb < s->num_cu * 32 ? nb : s->num_cu * 32)"),
    ("admpc_kernels.hip", "admpc_nlp_residuals_batch", "hipLaunchKernelGGL(admpc_nlp_res_kernel<double>, dim3(B < s->num_cu * 32 ? B : s->num_cu * 32)"),
    ("admpc_kernels.hip", "admpc_waypoints_batch", "int grid = B < 4096 ? B : 4096;"),
)


def num_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def f_grid(nc, B):
    """Kernel F (admpc_fused20_launch): eight one-wave workgroups per CU."""
    return min(nc * 8, B)


def _per_cu(lds, cap):
    return max(1, min(LDS_BYTES // lds, cap))


def s_grid(nc, B, S, lds=None):
    """Kernel S (seg_launch) with S waves per instance: (smallest, largest) grid over every LDS footprint when lds is None."""
    if lds is not None:
        g = min(nc * _per_cu(lds, 8 // S), B)
        return g, g
    return min(nc, B), min(nc * (8 // S), B)


def work_ordered(grid, B):
    """admpc_fused20_launch / seg_launch: the pre-pass and the bins run when the batch outgrows the grid."""
    return grid != B


def quad_grid(nc, B, seg20, lds=None):
    """quad_solve: (smallest, largest) grid; seg20 is the two-wave kernel of N = 20."""
    cap = 4 if seg20 else 8
    if lds is not None:
        g = min(nc * _per_cu(lds, cap), B)
        return g, g
    return min(nc, B), min(nc * cap, B)


def quad_tickets(grid, B):
    return B > 8 * grid


def quad_shoot_grid(nc, B):
    """admpc_quad_shoot_kernel in SQP mode: a stride loop over the batch beyond two workgroups per CU."""
    return min(nc * 2, B)


def nlp_res_grid(nc, B):
    return min(nc * 32, B)


def waypoints_grid(B):
    return min(B, 4096)


# batch sizes on the two sides of each switch, for any LDS footprint
def s_below(nc):
    return nc


def s_past(nc, S):
    return nc * (8 // S) + nc // 2 + 37


def f_past(nc):
    return nc * 8 + nc // 2 + 37


def quad_below(nc):
    """No tickets for any footprint: B <= 8 nc <= 8 grid."""
    return nc * 8


def quad_past(nc, seg20=False):
    """Tickets for any footprint: B > 8 * (largest grid)."""
    return nc * 8 * (4 if seg20 else 8) + 37


def nlp_res_past(nc):
    return nc * 32 + nc // 2 + 37


WAYPOINTS_PAST = 2 * 4096 + 901
