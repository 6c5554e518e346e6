"""The Python host layer without a GPU: the layout of the staging buffer (engine.packed_layout) and the prototype table of
ad_mpc_amd/_lib.py against the declarations of the nine headers under include/."""
import ctypes as C
import os
import re

import pytest

from ad_mpc_amd import _lib
from ad_mpc_amd.config import NX, NU, NY
from ad_mpc_amd.engine import packed_layout
from ad_mpc_amd.quad_config import QNX, QNU, QNY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _car_fields(N):
    """The field list of AdmpcOcpSolver's staging buffer."""
    return ((("x0", (1, NX)), ("yref", (1, N, NY)), ("yref_e", (1, NX)), ("p", (1,)), ("x", (1, N + 1, NX)), ("u", (1, N, NU))),
            (("cost", (1,)), ("pi", (1, N + 1, NX)), ("ineq", (1, N, 20))))


def test_layout_of_the_car_seam_at_n20():
    off, n_in, total = packed_layout(*_car_fields(20))
    assert {k: o for k, (o, n) in off.items()} == dict(x0=0, yref=32, yref_e=224, p=256, x=288, u=448, cost=512, pi=544, ineq=704)
    assert {k: n for k, (o, n) in off.items()} == dict(x0=7, yref=180, yref_e=7, p=1, x=147, u=40, cost=1, pi=147, ineq=400)
    assert list(off) == ["x0", "yref", "yref_e", "p", "x", "u", "cost", "pi", "ineq"]
    assert n_in == 512 and total == 1120


@pytest.mark.parametrize("N", [2, 20, 128])
def test_every_field_starts_on_a_256_byte_boundary(N):
    off, n_in, total = packed_layout(*_car_fields(N))
    assert all(o % 32 == 0 for o, n in off.values()) and n_in % 32 == 0 and total % 32 == 0
    spans = sorted(off.values())
    assert all(o0 + n0 <= o1 for (o0, n0), (o1, n1) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= total     # no overlap
    assert n_in == off["cost"][0]


def test_layout_of_the_quadrotor_optimizer_at_n10():
    """The numbers PackedIO computed for Quad3DOptimizer's field list before the layout became a function of its own."""
    N = 10
    fields_in = (("x0", (1, QNX)), ("yref", (1, N, QNY)), ("yref_e", (1, QNX)), ("gp", (1, QNX)), ("x", (1, N + 1, QNX)), ("u", (1, N, QNU)))
    off, n_in, total = packed_layout(fields_in, (("cost", (1,)),))
    assert off == {"x0": (0, 13), "yref": (32, 170), "yref_e": (224, 13), "gp": (256, 13), "x": (288, 143), "u": (448, 40), "cost": (512, 1)}
    assert n_in == 512 and total == 544
    assert packed_layout(fields_in, ()) == ({k: v for k, v in off.items() if k != "cost"}, 512, 512)        # no outputs: everything is input


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _declared_arity(header):
    """name -> number of parameters, from one header under include/: both kinds of comment stripped, the parameter list split on commas,
    (void) is zero."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    return {name: 0 if params.strip() in ("", "void") else len(params.split(","))
            for name, params in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}


def test_every_export_has_a_prototype_of_the_declared_arity(lib):
    names = _lib.EXPORTS + _lib.QUAD_EXPORTS
    assert len(set(names)) == len(names) == 34
    assert len(_lib.TABLES) == 9 and list(_lib.TABLES)[:2] == ["admpc.h", "admpc_quad.h"]
    assert tuple(_lib.TABLES["admpc.h"]) == _lib.EXPORTS and tuple(_lib.TABLES["admpc_quad.h"]) == _lib.QUAD_EXPORTS
    no_result = {"admpc_destroy", "admpc_quad_destroy", "admpc_quad_default_config", "admpc_path_bank_destroy", "admpc_quad_traj_bank_destroy"}
    strings = {"admpc_last_error", "admpc_version"}
    seen = []
    for header, table in _lib.TABLES.items():
        arity = _declared_arity(header)
        assert set(arity) == set(table), "%s: %s" % (header, set(arity) ^ set(table))
        for name in table:
            fn = getattr(lib, name)
            assert fn.argtypes is not None, "%s: no prototype applied" % name
            want = None if name in no_result else C.c_char_p if name in strings else C.c_int
            assert fn.restype is want, "%s: restype %r" % (name, fn.restype)
            assert len(fn.argtypes) == arity[name], "%s: %d argtypes, %d declared parameters" % (name, len(fn.argtypes), arity[name])
        seen += list(table)
    assert len(set(seen)) == len(seen) == 61                 # no name is declared by two headers


def test_exports_are_the_two_parts_of_the_table():
    assert all(n.startswith("admpc_quad_") for n in _lib.QUAD_EXPORTS) and not any(n.startswith("admpc_quad_") for n in _lib.EXPORTS)
    assert isinstance(_lib.EXPORTS, tuple) and isinstance(_lib.QUAD_EXPORTS, tuple)
