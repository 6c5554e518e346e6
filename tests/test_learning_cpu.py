"""The learning side the two fleets share (ad_mpc_amd/learning.py) without a GPU: the decode of fitted AdmpcGp records into the dicts
set_gp / set_quad_gp take, against records those two functions wrote, and the methods FleetController and QuadFleet have in common."""
import ctypes as C

import numpy as np
import pytest

from ad_mpc_amd.config import AdmpcGp, GP_MAX, GP_MAX_POINTS, default_config, set_gp
from ad_mpc_amd.learning import decode_gps, placeholder_gps
from ad_mpc_amd.quad_config import QUAD_GP_MAX, default_quad_config, set_quad_gp

# the vehicle's empty-record index (the first feature and row its ranges admit), how its records are written, its GP capacity
VEHICLES = {3: (default_config, set_gp, GP_MAX), 7: (default_quad_config, set_quad_gp, QUAD_GP_MAX)}
both = pytest.mark.parametrize("empty", [3, 7])


def _gp(feat, out, n, length_scale, sigma_f=1.0, ymean=0.0, shift=0.0):
    """A record of n points with a different value in every entry of Z and of alpha."""
    nf = len(feat)
    Z = (np.arange(n * nf, dtype=np.float64).reshape(n, nf) + 1.0) / 7.0 + shift
    return dict(feat=list(feat), out=out, Z=Z, alpha=-(np.arange(n, dtype=np.float64) + 1.0) / 3.0 - shift, length_scale=length_scale,
                sigma_f=sigma_f, ymean=ymean)


def _learn(gps):
    return [dict(feat=d["feat"], out=d["out"], length_scale=d["length_scale"], sigma_f=d["sigma_f"]) for d in gps]


def _records(empty, gps):
    """The config of vehicle `empty` with gps installed; bytes(cfg.gp) are its AdmpcGp records."""
    config, install, cap = VEHICLES[empty]
    return install(config(), gps)


def _same(got, want):
    assert list(got) == ["feat", "out", "Z", "alpha", "length_scale", "sigma_f", "ymean"]
    for k in ("feat", "out", "length_scale", "sigma_f", "ymean"):
        assert got[k] == want[k] and type(got[k]) is type(want[k]), k
    n, nf = len(want["alpha"]), len(want["feat"])
    assert got["Z"].shape == (n, nf) and got["alpha"].shape == (n,) and got["Z"].dtype == got["alpha"].dtype == np.float64
    assert got["Z"].tobytes() == want["Z"].tobytes() and got["alpha"].tobytes() == want["alpha"].tobytes()       # the decode copies doubles


def _round_trip(empty, gps):
    got = decode_gps(bytes(_records(empty, gps).gp), _learn(gps), empty)
    assert len(got) == len(gps)
    for g, w in zip(got, gps):
        _same(g, w)


def test_round_trip_of_the_cars_records():
    _round_trip(3, [_gp([3], 3, 1, [2.0]), _gp([3, 7], 4, 5, [2.0, 0.5], sigma_f=1.5, ymean=0.25)])


def test_round_trip_of_the_quadrotors_records():
    _round_trip(7, [_gp([7], 7, 1, [2.0]), _gp([7, 13], 8, 5, [2.0, 0.5], sigma_f=1.5, ymean=0.25)])


@both
def test_a_record_of_no_features_is_the_placeholder(empty):
    learn = [dict(feat=empty, out=empty, length_scale=1.0), dict(feat=[empty, empty + 1], out=empty + 1, length_scale=[0.5, 4.0], sigma_f=2.5)]
    got = decode_gps(bytes(2 * C.sizeof(AdmpcGp)), learn, empty)
    assert got == [dict(feat=empty, out=empty, Z=[], alpha=[], length_scale=1.0, sigma_f=1.0, ymean=0.0),
                   dict(feat=[empty, empty + 1], out=empty + 1, Z=[], alpha=[], length_scale=[0.5, 4.0], sigma_f=2.5, ymean=0.0)]
    assert got == [dict(d, ymean=0.0) for d in placeholder_gps(learn)]
    assert learn[0] == dict(feat=empty, out=empty, length_scale=1.0)                                             # the entries are not written to


def _poison(gp, where, value):
    slot, *idx = where
    if not idx:
        setattr(gp, slot, value)
    elif len(idx) == 1:
        getattr(gp, slot)[idx[0]] = value
    else:
        getattr(gp, slot)[idx[0]][idx[1]] = value


# record 1 below has 2 features and 3 points: Z[k][i] and alpha[i] are read for k < 2 and i < 3, inv_l2[k] for k < 2
USED = [("sigma_f",), ("ymean",), ("inv_l2", 1), ("alpha", 2), ("Z", 1, 2), ("Z", 0, 0)]
UNUSED = [("inv_l2", 2), ("alpha", 3), ("alpha", GP_MAX_POINTS - 1), ("Z", 2, 0), ("Z", 0, 3), ("Z", 1, GP_MAX_POINTS - 1)]


@both
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_a_record_the_install_refuses_is_the_empty_gp(empty, value):
    gps = [_gp([empty], empty, 4, [1.0]), _gp([empty, empty + 1], empty + 1, 3, [2.0, 0.5], sigma_f=1.5, ymean=0.25)]
    for where in USED:
        cfg = _records(empty, gps)
        _poison(cfg.gp[1], where, value)
        got = decode_gps(bytes(cfg.gp), _learn(gps), empty)
        _same(got[0], gps[0])                                                                                    # its neighbour is not disturbed
        assert got[1] == dict(feat=empty, out=empty, Z=[], alpha=[], length_scale=1.0, sigma_f=0.0, ymean=0.0), where
    for where in UNUSED:                                                                                         # slots the solve never reads
        cfg = _records(empty, gps)
        _poison(cfg.gp[1], where, value)
        got = decode_gps(bytes(cfg.gp), _learn(gps), empty)
        _same(got[0], gps[0])
        _same(got[1], gps[1])


@both
def test_a_full_record_in_the_last_slot_decodes(empty):
    cap = VEHICLES[empty][2]
    assert C.sizeof(AdmpcGp) == 1088                                                                             # record g begins at g * 1088
    gps = [_gp([empty + g], empty, 1, [1.0 + g], shift=float(g)) for g in range(cap - 1)]
    gps.append(_gp([empty, empty + 1, empty + 2], empty + 1, GP_MAX_POINTS, [2.0, 0.5, 3.0], sigma_f=0.7, ymean=-1.25))
    assert len(bytes(_records(empty, gps).gp)) == cap * 1088
    _round_trip(empty, gps)


def test_the_fleets_share_one_learning_side():
    from ad_mpc_amd.fleet import FleetController
    from ad_mpc_amd.learning import FleetLearning
    from ad_mpc_amd.quad_fleet import QuadFleet
    for name in ("fit_gp", "learned_gps", "set_observer", "observe_reset", "_learns"):
        assert getattr(FleetController, name) is getattr(QuadFleet, name) is getattr(FleetLearning, name), name
    for name in ("search_gp", "learned_hyper"):
        assert hasattr(FleetController, name) and not hasattr(QuadFleet, name) and not hasattr(FleetLearning, name), name
    assert (FleetController._EMPTY, QuadFleet._EMPTY) == (3, 7) and (FleetController._GP_CAP, QuadFleet._GP_CAP) == (GP_MAX, QUAD_GP_MAX)
