"""The prune of the flight log and the RDRv drag fit (include/admpc_quad_prune.h; ad_mpc_amd/quad_ensemble_fleet.py) without a GPU: the
header, the prototype table, the Makefile and the library agree; the refusals, all of which stand in front of the first device call, come
back in their order; the Python layer refuses before a handle is asked for; and the numpy spec (tests/quad_prune_spec.py), which the GPU
tests hold the kernels against, is pinned to the reference's own prune_dataset and linear_rdrv_fitting through
tests/golden/quad_prune_vectors.json (tests/gen_quad_prune_golden.py writes it where the reference tree is present, and is run live
there) and to np.histogram."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import quad_prune_spec as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "quad_prune_vectors.json")
ARITY = {"admpc_quad_records_prune": 11, "admpc_quad_rdrv_fit": 9, "admpc_quad_rdrv_install": 5}
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from ad_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def last(lib):
    return lib.admpc_last_error().decode()


# ---- 1. the header, the table, the Makefile and the library ------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from ad_mpc_amd import _lib, quad_ensemble_fleet as F
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_prune.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_PRUNE_EXPORTS, tuple) and list(_lib.QUAD_PRUNE_EXPORTS) == list(ARITY)
    assert list(_lib.PRUNE_TABLES) == ["admpc_quad_prune.h"] and tuple(_lib.PRUNE_TABLES["admpc_quad_prune.h"]) == _lib.QUAD_PRUNE_EXPORTS
    known = [t for group in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES, _lib.TARGET_TABLES)
             for t in group.values()]
    assert len(known) == 14 and not set(ARITY) & {n for t in known for n in t}
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n and fn.restype is C.c_int, name
    for name, val, py, spec in (("ADMPC_PRUNE_BINS_MAX", "256", F.PRUNE_BINS_MAX, PS.BINS_MAX), ("ADMPC_PRUNE_PARTIAL", "9", F.PRUNE_PARTIAL, 9),
                                ("ADMPC_RDRV_PARTIAL", "7", F.RDRV_PARTIAL, 7), ("ADMPC_PRUNE_ENOVALID", r"\(-100\)", F.PRUNE_ENOVALID, PS.ENOVALID)):
        assert re.search(r"#define\s+%s\s+%s" % (name, val), hdr), name
        assert py == int(val.strip("\\()")) == spec, name
    assert re.search(r"#define\s+ADMPC_QUAD_REC_PRUNED\s+2\.0", hdr) and F.REC_PRUNED == PS.PRUNED == 2.0
    for cite in ("gp_common.py:64-66, 101-112", "utils.py:458-533", "rdrv_fitting.py:27-33", "comparative_experiment.py", "fit(x_pruned)",
                 "reference call site", "replaced by", "LinearRegression"):
        assert cite in hdr, cite
    offered = hdr[hdr.index("NOT offered"):]
    for words in ("plotting", "utils.py:507, 513", "anything but flags", "QuadFleet", "covariance mode", "SQP mode"):
        assert words in offered, words
    for words in ("WHICH RECORDS TAKE PART", "WHAT IS PRUNED", "CONSTANT column", "DETERMINISM", "No floating-point atomics", "function of M alone",
                  "INTEGER atomics", "Measured on one MI355X"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*=.*\badmpc_quad_prune\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_prune\.h", mk, flags=re.M)
    assert re.search(r"^#\s+admpc_quad_prune\.hip\s", mk, flags=re.M)
    # the learning header points here, and keeps the words tests/test_quad_learn_cpu.py greps for
    learn = open(os.path.join(ROOT, "include", "admpc_quad_learn.h")).read()
    assert "admpc_quad_prune.h" in learn[learn.index("NOT offered"):] and "velocity cap" in learn


# ---- 2. the refusals: every one in front of the first device call, in the listed order -----------------------------------------------------

def test_prune_refusals_in_order(lib):
    one = C.c_void_p(8)                                  # never dereferenced: the call is refused, or M == 0 returns at once
    bad = dict(M=-1, n_bins=0, thresh=2.0, x_cap=0.0, arr=None)
    good = dict(M=4, n_bins=40, thresh=0.001, x_cap=16.0, arr=one)
    order = [("M", "number of records"), ("n_bins", "n_bins"), ("thresh", "thresh"), ("x_cap", "x_cap"), ("arr", "null array")]
    for i, (_, words) in enumerate(order):
        a = dict(good)
        for key, _w in order[i:]:
            a[key] = bad[key]                             # everything from i on is wrong: refusal i is the one that is reported
        rc = lib.admpc_quad_records_prune(0, a["M"], a["arr"], a["x_cap"], a["n_bins"], a["thresh"], a["arr"], a["arr"], a["arr"], a["arr"], None)
        assert rc == EINVAL and "admpc_quad_records_prune" in last(lib) and words in last(lib), (i, last(lib))
    for M in (2 ** 31, -5):
        assert lib.admpc_quad_records_prune(0, M, one, 16.0, 40, 0.001, one, one, one, one, None) == EINVAL
    for n in (-1, 0, 257):
        assert lib.admpc_quad_records_prune(0, 4, one, 16.0, n, 0.001, one, one, one, one, None) == EINVAL and "n_bins" in last(lib)
    for t in (-1e-9, 1.0000001, float("nan")):
        assert lib.admpc_quad_records_prune(0, 4, one, 16.0, 40, t, one, one, one, one, None) == EINVAL and "thresh" in last(lib)
    for cap in (0.0, -1.0, float("nan"), float("-inf")):
        assert lib.admpc_quad_records_prune(0, 4, one, cap, 40, 0.001, one, one, one, one, None) == EINVAL and "x_cap" in last(lib)
    for k in range(5):                                   # each array on its own
        arrs = [one] * 5
        arrs[k] = None
        rc = lib.admpc_quad_records_prune(0, 4, arrs[0], 16.0, 40, 0.001, arrs[1], arrs[2], arrs[3], arrs[4], None)
        assert rc == EINVAL and "null array" in last(lib), k
    # M == 0 is a no-op behind the refusals of the scalars: no array is looked at, no device is asked for
    assert lib.admpc_quad_records_prune(0, 0, None, float("inf"), 256, 0.0, None, None, None, None, None) == 0
    assert lib.admpc_quad_records_prune(0, 0, None, 16.0, 1, 1.0, None, None, None, None, None) == 0
    assert lib.admpc_quad_records_prune(0, 0, None, 16.0, 0, 0.5, None, None, None, None, None) == EINVAL


def test_rdrv_refusals_in_order(lib):
    one = C.c_void_p(8)
    assert lib.admpc_quad_rdrv_fit(0, -1, 0, None, None, None, None, None, None) == EINVAL and "number of records" in last(lib)
    assert lib.admpc_quad_rdrv_fit(0, 2 ** 31, 7, one, one, one, one, one, None) == EINVAL and "number of records" in last(lib)
    for axes in (0, 8, -1):
        assert lib.admpc_quad_rdrv_fit(0, 4, axes, None, None, None, None, None, None) == EINVAL and "axes" in last(lib)
    for k in range(5):
        arrs = [one] * 5
        arrs[k] = None
        assert lib.admpc_quad_rdrv_fit(0, 4, 7, *arrs, None) == EINVAL and "null array" in last(lib), k
    assert lib.admpc_quad_rdrv_fit(0, 0, 5, None, None, None, None, None, None) == 0
    assert lib.admpc_quad_rdrv_fit(0, 0, 0, None, None, None, None, None, None) == EINVAL
    assert lib.admpc_quad_rdrv_install(None, None, None, None, None) == EINVAL and "null solver" in last(lib)


def test_python_layer_refuses_without_a_gpu():
    from ad_mpc_amd import quad_ensemble_fleet as F
    assert F.prune_request(60) == (16.0, 40, 0.001)
    assert F.prune_request(1, None, 256, 0.0) == (float("inf"), 256, 0.0)
    for kw in (dict(steps=0), dict(steps=3, bins=0), dict(steps=3, bins=257), dict(steps=3, bins=2.5), dict(steps=3, thresh=-0.1),
               dict(steps=3, thresh=1.5), dict(steps=3, thresh=float("nan")), dict(steps=3, x_cap=0.0), dict(steps=3, x_cap=-2.0),
               dict(steps=3, x_cap=float("nan"))):
        with pytest.raises(ValueError):
            F.prune_request(**kw)
    assert F.rdrv_axes((7, 8, 9)) == 7 and F.rdrv_axes([9]) == 4 and F.rdrv_axes(8) == 2 and F.rdrv_axes((9, 7)) == 5
    for axes in ((), (6,), (10,), (7, 7), (0, 1, 2)):
        with pytest.raises(ValueError):
            F.rdrv_axes(axes)


# ---- 3. the spec against the reference (through the golden file) and against np.histogram ---------------------------------------------------

def test_golden_file_is_what_the_spec_lists(golden):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert [(c["kind"], c["M"], c["n_bins"], c["thresh"], c["x_cap"], c["seed"]) for c in golden] == [tuple(c) for c in PS.GOLDEN_CASES]
    assert all(c["M"] <= 2000 and set(c) == {"kind", "M", "n_bins", "thresh", "x_cap", "seed", "kept", "drag"} for c in golden)
    assert {c["n_bins"] for c in golden} >= {1, 3, 8, 40, 128} and {c["kind"] for c in golden} == set(PS.KINDS) - {"one"}
    for c in golden:                                      # no thresh of the form k / M
        assert abs(c["thresh"] * c["M"] - round(c["thresh"] * c["M"])) > 1e-4 * max(1.0, c["thresh"] * c["M"]) or c["M"] < 100, c["seed"]


def test_spec_keeps_what_the_reference_keeps(golden):
    pruned_some = 0
    for c in golden:
        S = PS.records(c["kind"], c["M"], c["seed"], dirty=False)
        r = PS.prune(S, c["x_cap"], c["n_bins"], c["thresh"])
        # the precondition that keeps the norm's double normalisation out of play
        assert r["margin"] > 1e-6, (c["seed"], r["margin"])
        assert np.nonzero(r["kept"])[0].tolist() == c["kept"], c["seed"]
        assert r["info"][0] == 0 and r["info"][1] == c["M"] and r["info"][2] == len(c["kept"])
        assert np.array_equal(r["records"][:, :13], S[:, :13]) and set(np.unique(r["records"][:, 13])) <= {1.0, 2.0}
        pruned_some += int(r["info"][4:].sum() > 0)
        D, sums, n_used, status = PS.rdrv(r["records"])
        if c["drag"] is None:
            assert n_used == 0 and status == -1
        else:
            assert status == 0 and n_used == len(c["kept"])
            assert np.all(np.abs(D - np.array(c["drag"])) <= 1e-12 * np.abs(c["drag"])), c["seed"]
    assert pruned_some >= 10                              # the histograms, not the cap alone, are at work in the fixtures


def test_golden_is_what_the_reference_gives_now(golden):
    """Where the reference tree is present: its functions, taken live, give the committed file."""
    import gen_quad_prune_golden as G
    if not G.reference_present():
        pytest.skip("no reference tree on this machine: tests/golden/quad_prune_vectors.json stands in")
    prune_dataset, fit = G.load_reference()
    for c in golden:
        kept, drag = G.run_case(prune_dataset, fit, c["kind"], c["M"], c["n_bins"], c["thresh"], c["x_cap"], c["seed"])
        assert kept == c["kept"] and drag == c["drag"], c["seed"]


@pytest.mark.parametrize("kind", PS.KINDS)
def test_spec_counts_and_edges_are_np_histograms(kind):
    for M, n_bins in ((1, 1), (1, 8), (63, 2), (65, 3), (257, 40), (1000, 255), (5000, 256), (4096, 128)):
        S = PS.records(kind, M, seed=3)
        r = PS.prune(S, 16.0, n_bins, 0.0137)
        part = PS.take_part(S)
        assert r["info"][1] == part.sum() > 0
        cols = PS.columns(S[part, 10:13])
        for j in range(4):
            h, e = np.histogram(cols[:, j], bins=n_bins)
            assert np.array_equal(h, r["counts"][j, :n_bins]) and not r["counts"][j, n_bins:].any(), (M, n_bins, j)
            assert np.array_equal(e, r["edges"][j]) and r["lo"][j] == e[0] and r["hi"][j] == e[-1], (M, n_bins, j)
        assert np.array_equal(cols[:, 3], np.sqrt(np.sum(S[part, 10:13] ** 2, 1)))          # utils.py:503
        # who does not take part is left as it is
        assert np.array_equal(r["records"][~part], S[~part], equal_nan=True) and not r["kept"][~part].any()


def test_spec_properties():
    S = PS.records("heavy", 3000, seed=5)
    a = PS.prune(S, 9.0, 40, 0.00137)
    assert 0 < a["info"][2] < a["info"][1] < 3000 and a["info"][3] > 0 and a["info"][4:].min() > 0
    b = PS.prune(a["records"], 9.0, 40, 0.00137)                                        # twice is once
    assert np.array_equal(a["records"], b["records"], equal_nan=True) and np.array_equal(a["info"], b["info"])
    c = PS.prune(a["records"], None, 40, 0.0)                                           # restore
    part = PS.take_part(S)
    assert (c["records"][part, 13] == 1.0).all() and c["info"][2] == c["info"][1] and not c["info"][3:].any()
    # a constant column prunes everything for an even n_bins, and nothing on its own for an odd one
    K = PS.records("constant", 400, seed=1, dirty=False)
    assert PS.prune(K, None, 8, 0.0137)["info"][5] == 400 and PS.prune(K, None, 8, 0.0137)["info"][2] == 0
    assert PS.prune(K, None, 3, 0.0137)["info"][5] == 0
    # nobody takes part
    Z = S.copy()
    Z[:, 13] = 0.0
    z = PS.prune(Z)
    assert z["info"].tolist() == [PS.ENOVALID, 0, 0, 0, 0, 0, 0, 0] and np.array_equal(z["records"], Z, equal_nan=True)
    # the drag fit: the closed form, the mask, the failures
    R = PS.records("heavy", 500, seed=2, dirty=False)
    D, sums, n, st = PS.rdrv(R, 5)
    assert st == 0 and n == 500 and D[1] == 0.0 and not sums[1].any()
    assert D[0] == (R[:, 0] * R[:, 10]).sum() / (R[:, 0] ** 2).sum()
    R[:, 2] = 0.0
    assert PS.rdrv(R, 7)[3] == -3 and PS.rdrv(R, 3)[3] == 0
    R[7, 10] = np.nan
    assert PS.rdrv(R, 7)[3] == -1
