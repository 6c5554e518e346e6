"""Host-side pieces of the fleet control step that need no GPU: the C structs of admpc_control_step_batch, the refusal of a call
without a solver, and the OCP the fleet shares with ROSGPMPC."""
import ctypes as C
import os

import numpy as np
import pytest

from ad_mpc_amd import _lib
from ad_mpc_amd.config import AdmpcPath, AdmpcStepParams


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_step_structs_match_the_header_layout():
    assert C.sizeof(AdmpcPath) == 4 + 4 + 8 + 7 * 8
    assert AdmpcPath.dt.offset == 8 and AdmpcPath.vel.offset == 16 and AdmpcPath.curv.offset == 64
    assert C.sizeof(AdmpcStepParams) == 4 * 8 + 2 * 4
    assert AdmpcStepParams.resample.offset == 32 and AdmpcStepParams.threshold.offset == 36


def test_step_without_solver_is_refused(lib):
    prm = AdmpcStepParams(blend_min=100.0, blend_max=110.0, acc_max=5.0, resample_dt=0.05, resample=1, threshold=10)
    rc = lib.admpc_control_step_batch(None, None, C.byref(prm), 1, *([None] * 7), *([None] * 5), None, *([None] * 4), None)
    assert rc == -1 and b"null solver" in lib.admpc_last_error()
    n = C.c_size_t(0)
    assert lib.admpc_control_step_workspace(None, 1, C.byref(n)) == -1


def test_fleet_ocp_is_the_ros_surface_ocp():
    """FleetController builds its problem with ocp_config, the function AD3DOptimizer uses: ROSGPMPC's SQP_RTI problem."""
    from ad_mpc_amd import config as _c
    from ad_mpc_amd.ad_3d import AD3D
    from ad_mpc_amd.ad_3d_optimizer import ocp_config
    ad = AD3D(noisy=False, noisy_input=False)
    cfg = ocp_config(ad, 1.0, 20, np.array(_c.Q_DIAG_ROS), np.array(_c.R_DIAG_ROS), "SQP_RTI")
    exp = _c.default_config(N=20, Ts=0.05, q=_c.Q_DIAG_ROS, r=_c.R_DIAG_ROS, terminal_scale=_c.TERMINAL_SCALE, sqp_iters=1, sqp_tol=0.0)
    exp.lbu[0], exp.lbu[1], exp.ubu[0], exp.ubu[1] = ad.acc_min, ad.steering_rate_min, ad.acc_max, ad.steering_rate_max
    exp.lbx_delta, exp.ubx_delta = ad.steering_min, ad.steering_max
    exp.mass, exp.L_F, exp.L_R, exp.Iz, exp.Cf, exp.Cr = ad.mass, ad.L_F, ad.L_R, ad.Iz, ad.Cf, ad.Cr
    assert bytes(cfg) == bytes(exp)
    with pytest.raises(Exception, match="unknown solver_type"):
        ocp_config(ad, 1.0, 20, np.array(_c.Q_DIAG_ROS), np.array(_c.R_DIAG_ROS), "DDP")
