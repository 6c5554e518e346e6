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
    ("admpc_rowqp.hip", "rowqp_inst_stride", "int s = RQ_HDR + N * RQ_RS;"),
    ("admpc_rowqp.hip", "rowqp_inst_stride", "s += s & 1;"),
    ("admpc_rowqp.hip", "rowqp_inst_stride", "while (s % (2 * half) != half) s += 2;"),
    ("rowqp_core.h", "", "#define RQ_HDR 16"),
    ("rowqp_core.h", "", "#define RQ_RS 31"),
    ("admpc_rowqp.hip", "admpc_rowqp_plan", "const int cap = 160 * 1024;"),
    ("admpc_rowqp.hip", "admpc_rowqp_plan", "int r = 4;"),
    ("admpc_rowqp.hip", "admpc_rowqp_plan", "while (r > 1 && r * stride * elem > cap) r >>= 1;"),
    ("admpc_rowqp.hip", "admpc_rowqp_plan", "int per_cu = cap / (r * stride * elem);"),
    ("admpc_rowqp.hip", "admpc_rowqp_plan", "while (r > 1 && (B + r - 1) / r < num_cu * 4 && (B + r / 2 - 1) / (r / 2) <= num_cu * 4) r >>= 1;"),
    ("admpc_rowqp.hip", "admpc_rowqp_plan", "if (per_cu > 4) per_cu = 4;"),
    ("admpc_kernels.hip", "rowqp_split", "return (s->split_mode == 1 || nquads > grid) ? s->d_split : nullptr;"),
    # appended, never inserted: the position of an entry is part of its test's id
    ("admpc_step.hip", "step_tail", "hipLaunchKernelGGL(admpc_step_command_kernel, dim3(B < 65536 ? B : 65536), dim3(WAVE)"),
    ("admpc_step.hip", "admpc_step_command_kernel", "for (int b = blockIdx.x; b < B; b += gridDim.x) {"),
    ("admpc_step.hip", "step_tail", "const long nP = (long)B * (N + 1);"),
    # the dispatch of quad_solve that quad_routed_spec.quad_kernel mirrors
    ("admpc_quad.hip", "quad_solve", "const bool seg20 = s->cfg.N == 20 && !s->wide20;"),
    ("admpc_quad.hip", "quad_solve", "else if (s->cfg.N * QU > 64)"),
    ("admpc_quad.hip", "quad_solve", "else if (s->cfg.N * QU == 40 && !s->generic)"),
    # the dispatch of admpc_create / solve_impl that car_routed_spec.car_kernel, split_mode and chunks mirror, and the routed skip of kernel R
    ("admpc_kernels.hip", "admpc_create", 's->use_dense = (cfg->N == 20) && !(e && strcmp(e, "riccati") == 0);'),
    ("admpc_kernels.hip", "admpc_create", 's->use_seg = admpc_seg_supports(cfg->N) && (cfg->n_gp == 0 ? !(e && strcmp(e, "riccati") == 0) : (e && strcmp(e, "seg") == 0));'),
    ("admpc_kernels.hip", "solve_impl", "const bool dense = s->use_dense && !snap && !(nsqp > 1 && s->cfg.sqp_tol > 0.0);"),
    ("admpc_kernels.hip", "solve_impl", "if (s->use_seg && !snap && !(nsqp > 1 && s->cfg.sqp_tol > 0.0)) {"),
    ("admpc_kernels.hip", "rowqp_chunk", "if (s->row_chunk > 0 && (unsigned long long)s->row_chunk < m) m = (unsigned long long)s->row_chunk;"),
    ("admpc_kernels.hip", "rowqp_chunk", "const unsigned long long per = (unsigned long long)(N + 1) * 42ull * (unsigned long long)elem;"),
    ("admpc_kernels.hip", "admpc_create", "s->split_mode = e && e[0] == '0' ? 0 : (e && e[0] == '1' ? 1 : -1);"),
    ("admpc_kernels.hip", "admpc_create", "s->row_chunk = c ? atoi(c) : 0;"),
    ("admpc_seg.hip", "admpc_seg_supports", "return N == 40 || N == 60 || N == 80;"),
    ("admpc_kernels.hip", "solve_rows", "const int first = (sq == 0 && !routed) ? 1 : 0;"),
    ("admpc_kernels.hip", "solve_rows", "first ? (const int32_t*)nullptr : (const int32_t*)cst, (T*)s->d_GT, (T*)s->d_bl, s->d_sched);"),
    ("admpc_rowqp.hip", "admpc_rowqp_kernel", "if (!first_pass) valid = valid && statusg[ic] == 0;"),
    ("admpc_rowqp.hip", "admpc_rowqp_kernel", "int ic = inst < total && has_lds ? inst : total - 1;"),
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


def command_grid(B):
    """admpc_step_command_kernel (admpc_control_step_batch): one wave per vehicle up to 65536 workgroups, a stride loop past it."""
    return min(B, 65536)


COMMAND_PAST = 65536 + 300


# ---- kernel R (admpc_rowqp_plan, rowqp_split).  rowqp_rows / rowqp_splits assume a horizon whose LDS footprint allows four instances per
# wave and four waves per CU; rowqp_lds_rows / rowqp_per_cu state that footprint, and the tests assert it for the horizon they use
RQ_HDR, RQ_RS = 16, 31


def rowqp_inst_stride(N):
    """Values of T per instance in LDS (rowqp_inst_stride: the records, padded to an odd multiple of 16 values)."""
    s = RQ_HDR + N * RQ_RS
    s += s & 1
    while s % 32 != 16:
        s += 2
    return s


def rowqp_lds_rows(N, elem):
    """Instances per wave the LDS allows (the first loop of admpc_rowqp_plan); 0: the horizon does not fit."""
    r = 4
    while r > 1 and r * rowqp_inst_stride(N) * elem > LDS_BYTES:
        r >>= 1
    return r if r * rowqp_inst_stride(N) * elem <= LDS_BYTES else 0


def rowqp_per_cu(N, elem, rows):
    return min(4, LDS_BYTES // (rows * rowqp_inst_stride(N) * elem))


def rowqp_rows(nc, B):
    """Instances per wave: 4, halved while the batch would not fill one wave per SIMD (4 per CU) with the smaller count either."""
    r = 4
    while r > 1 and (B + r - 1) // r < nc * 4 and (B + r // 2 - 1) // (r // 2) <= nc * 4:
        r >>= 1
    return r


def rowqp_splits(nc, B, rows):
    """Two phases (trial for all, interior point for the deferred) when the batch is more than one round of waves."""
    return (B + rows - 1) // rows > nc * 4


def rowqp_sizes(nc):
    """One batch per regime: 1, 2, 4 instances per wave in one round, and 4 per wave past one round (split)."""
    return {"rows1": nc * 4, "rows2": nc * 4 + nc // 2 + 37, "rows4": nc * 8 + nc // 2 + 37, "split": nc * 16 + nc // 2 + 37}
