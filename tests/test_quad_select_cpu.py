"""The selection of the GP training points from a flight log (include/admpc_quad_select.h; ad_mpc_amd/quad_ensemble_fleet.py) without a
GPU: the header, the prototype table, the Makefile and the library agree; the refusal that needs no object comes back under the entry's
name; the request check of the Python layer; and the numpy spec (tests/quad_select_spec.py), which the GPU tests hold the kernels
against, is pinned to the reference's own distance_maximizing_points_1d through tests/golden/quad_select_vectors.json
(tests/gen_quad_select_golden.py writes it where the reference tree is present, and is run live there).

The selection is a rule of decisions: every comparison is of indices, integer for integer.  The one place the reference is not
compared is a bin without a member, where it draws a random record and the rule gives no point; the fixtures are held to have few such
bins (at most one in ten) and to have some (at least two fixtures), so that neither side of the difference passes unseen."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import quad_learn_spec as QL
import quad_select_spec as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "quad_select_vectors.json")
ARITY = {"admpc_quad_ensemble_select_points": 11}
EINVAL = -1
VARIANTS = ("keep_last", "highest", "hi_in_last", "formula", "low_byte")


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


# ---- 1. the header, the table, the Makefile and the library ------------------------------------------------------------------------------

def test_header_table_and_library_agree(lib):
    from ad_mpc_amd import _lib, quad_ensemble_fleet as F
    hdr = open(os.path.join(ROOT, "include", "admpc_quad_select.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = {n: (0 if p.strip() in ("", "void") else len(p.split(","))) for n, p in re.findall(r"\b(admpc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}
    assert decl == ARITY
    assert isinstance(_lib.QUAD_SELECT_EXPORTS, tuple) and list(_lib.QUAD_SELECT_EXPORTS) == list(ARITY)
    assert list(_lib.SELECT_TABLES) == ["admpc_quad_select.h"] and tuple(_lib.SELECT_TABLES["admpc_quad_select.h"]) == _lib.QUAD_SELECT_EXPORTS
    known = [t for group in (_lib.TABLES, _lib.MORE_TABLES, _lib.ENSEMBLE_TABLES, _lib.CLUSTER_TABLES, _lib.HYPER_TABLES, _lib.TARGET_TABLES,
                             _lib.PRUNE_TABLES, _lib.EVAL_TABLES, _lib.TRAJ_TABLES, _lib.POLY_TRAJ_TABLES) for t in group.values()]
    assert not set(ARITY) & {n for t in known for n in t}                          # no name is declared by two headers
    for name, n in ARITY.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n == len(_lib.SELECT_TABLES["admpc_quad_select.h"][name][1]) and fn.restype is C.c_int, name
    slots = 8 * 3 * 32
    work = 4 * slots + 32 + 2 * 32 + 2 * 32 + 2 * slots + 256 * slots                # THE WORK AREA, as the unit lays it out
    for name, val, py in (("ADMPC_SELECT_WORK", str(work), F.SELECT_WORK), ("ADMPC_SELECT_ENOVALID", r"\(-100\)", F.SELECT_ENOVALID),
                          ("ADMPC_SELECT_PASSES", "8", 8)):
        assert re.search(r"#define\s+%s\s+%s" % (name, val), hdr), name
        assert py == int(val.strip("\\()")), name
    assert SS.ENOVALID == F.SELECT_ENOVALID
    for cite in ("gp_fitting.py:230-249", "utils.py:621-626", "utils.py:536-581", "reference call site", "replaced by"):
        assert cite in hdr, cite
    offered = hdr[hdr.index("NOT offered"):hdr.index("THE RULE")]
    for words in ("random draw", "above ADMPC_GP_MAX_POINTS", "dense-GP", "sample_random_points", "k-means", "PCA", "y_mean", "top-2", "SQP", "QuadFleet"):
        assert words in offered, words
    for words in ("THE RULE", "WHAT IS WRITTEN", "THE WORK AREA", "THE CHAIN", "DETERMINISM", "Integer atomics only", "compacted", "re-bin"):
        assert words in hdr, words
    mk = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "Makefile")).read()
    assert re.search(r"^UNITS\s*[:+]?=.*\badmpc_quad_select\b", mk, flags=re.M) and re.search(r"^HDRS\s*=.*admpc_quad_select\.h", mk, flags=re.M)
    assert re.search(r"^#\s+admpc_quad_select\.hip\s", mk, flags=re.M)
    src = open(os.path.join(ROOT, "ad_mpc_amd", "csrc", "admpc_quad_select.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomicAdd(" in code and not re.search(r"atomic\w*\s*\(\s*\(?\s*(double|float)", code)      # integer atomics only
    assert "hipMalloc" not in code and "Synchronize" not in code and "hipMemcpy" not in code
    # the headers that spoke of the selection as missing point here
    for other in ("admpc_quad_eval.h",):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "admpc_quad_select.h" in text[text.index("NOT offered"):], other


def test_null_ensemble_is_refused_first(lib):
    one = C.c_void_p(8)                                  # never dereferenced: the call is refused
    assert lib.admpc_quad_ensemble_select_points(None, -1, None, None, None, None, None, None, None, None, None) == EINVAL
    assert lib.admpc_last_error().decode() == "admpc_quad_ensemble_select_points: null ensemble"
    n = (C.c_int32 * 3)(20, 20, 20)
    assert lib.admpc_quad_ensemble_select_points(None, 0, one, n, one, one, one, one, one, one, None) == EINVAL      # in front of the M == 0 no-op
    assert "null ensemble" in lib.admpc_last_error().decode()


# ---- 2. the request check of the Python layer ------------------------------------------------------------------------------------------------

def _blocks(learn):
    from ad_mpc_amd.quad_ensemble_fleet import ensemble_layout
    return ensemble_layout(np.zeros((len(learn), 1)), [7], learn)[2]


def test_the_request_is_checked_without_a_gpu():
    from ad_mpc_amd.quad_config import select_request
    three = [[dict(d) for d in QL.EXP_LEARN] for _ in range(2)]                    # bins 32, 32, 32 in both clusters
    assert select_request(_blocks(three)) == [32, 32, 32]
    assert select_request(_blocks(three), 20) == [20, 20, 20] and select_request(_blocks(three), [1, 7, 32]) == [1, 7, 32]
    assert select_request(_blocks(three), np.int64(5)) == [5, 5, 5]
    narrow = [[dict(d) for d in QL.EXP_LEARN[:2]] for _ in range(2)]
    narrow[1][1]["bins"] = [8]                                                     # the clusters are free in their bins: the smaller one holds
    assert select_request(_blocks(narrow)) == [32, 8, 0] and select_request(_blocks(narrow), [32, 8]) == [32, 8, 0]
    for blocks, n, words in ((three, 0, "must be in 1 .. 32"), (three, 33, "must be in 1 .. 32"), (three, [20, 20], "one value per regressor"),
                             (three, [20, 20, 20, 20], "one value per regressor"), (three, 2.5, "whole numbers"), (narrow, 9, "regressor 1 must be in 1 .. 8"),
                             (narrow, [33, 8], "regressor 0")):
        with pytest.raises(ValueError, match=words):
            select_request(_blocks(blocks), n)
    two = [[dict(feat=[7, 8], out=7, lo=[-9.0, -9.0], hi=[9.0, 9.0], bins=[4, 4], length_scale=[2.0, 2.0], noise=1e-4)]]
    with pytest.raises(ValueError, match="more than one feature"):
        select_request(_blocks(two), 4)


# ---- 3. the spec against the reference -----------------------------------------------------------------------------------------------------------

def test_the_golden_file_holds_the_cases_of_the_spec(golden):
    assert [(c["kind"], c["N"], c["n_points"], c["seed"]) for c in golden] == SS.GOLDEN_CASES
    assert all(len(c["index"]) == c["n_points"] and set(c) == {"kind", "N", "n_points", "seed", "index"} for c in golden)
    assert os.path.getsize(GOLDEN) < 16384
    kinds = {c[0] for c in SS.GOLDEN_CASES}
    assert kinds == {"normal", "uniform", "eighths", "signs", "lowbits", "constant", "few"}
    assert {c[2] for c in SS.GOLDEN_CASES} >= {1, 2, 7, 20, 32} and {c[1] for c in SS.GOLDEN_CASES if c[0] == "few"} == {2, 3}


def test_the_spec_picks_the_references_index_in_every_bin_that_has_a_member(golden):
    bins = empty = with_empty = 0
    for c in golden:
        z = SS.values(c["kind"], c["N"], c["seed"])
        got, want = SS.select_1d(z, c["n_points"]), np.asarray(c["index"])
        assert np.array_equal(got, want), (c["kind"], c["N"], c["n_points"], got.tolist(), want.tolist())
        bins, empty, with_empty = bins + got.size, empty + int((got < 0).sum()), with_empty + int((got < 0).any())
    print("bins %d, empty %d, fixtures with an empty bin %d" % (bins, empty, with_empty))
    assert 10 * empty <= bins and with_empty >= 2                                  # neither vacuous nor blind to the difference


def test_golden_is_what_the_reference_gives_now(golden):
    """Where the reference tree is present: its function, taken live, gives the committed file."""
    import gen_quad_select_golden as G
    if not G.reference_present():
        pytest.skip("no reference tree on this machine: tests/golden/quad_select_vectors.json stands in")
    pick = G.load_reference()
    for c in golden:
        assert G.run_case(pick, c["kind"], c["N"], c["n_points"], c["seed"]) == c["index"], c


def test_the_fixtures_reach_what_they_are_there_for():
    z = SS.values("signs", 1500, 13)
    assert (np.signbit(z) & (z == 0.0)).any() and (~np.signbit(z) & (z == 0.0)).any() and (z < 0).any() and (z > 0).any()
    z = SS.values("lowbits", 800, 15)
    assert len(np.unique(z.view(np.uint64) >> np.uint64(8))) == 8 and len(np.unique(z)) > 400
    z = SS.values("eighths", 4000, 11)
    assert len(np.unique(z)) < 80
    e = SS.edges(0.625, 0.625, 3)
    assert e[0] == 0.125 and e[3] == 1.125 and SS.select_1d(SS.values("constant", 300, 17), 3).tolist() == [-1, 0, -1]
    # a member equal to hi is in no bin; two points leave one
    assert SS.select_1d([0.5, -1.25], 1).tolist() == [1] and SS.select_1d([0.5, -1.25, 0.75], 2).tolist() == [1, 0]


def test_each_wrong_rule_differs_from_the_reference_on_some_fixture(golden):
    hit = {v: 0 for v in VARIANTS}
    for c in golden:
        z = SS.values(c["kind"], c["N"], c["seed"])
        for v in VARIANTS:
            hit[v] += int((SS.select_1d(z, c["n_points"], v) != np.asarray(c["index"])).sum())
    print(hit)
    assert all(n > 0 for n in hit.values()), hit


def test_the_pick_by_hand():
    """Bins of 1, 2, 3 and 4 members over [0, 4], and the point equal to hi.  n = 4: the edges are 0, 1, 2, 3, 4."""
    #               bin 0        bin 1              bin 2                     bin 3                         hi
    z = np.array([0.0,          1.5, 1.25,         2.5, 2.0, 2.75,           3.5, 3.25, 3.5, 3.0,          4.0])
    # bin 1: the last (1.25, index 2) is set aside, the median of {1.5} is index 1
    # bin 2: the median of {2.5, 2.0, 2.75} is 2.5, index 3
    # bin 3: 3.0 (index 9) is set aside; the median of {3.5, 3.25, 3.5} is 3.5, the lowest index that equals it is 6
    assert SS.select_1d(z, 4).tolist() == [0, 1, 3, 6]
    # the member set aside is the lowest index that equals the median when it comes last but ties: bin 3 = {3.5 (6), 3.25, 3.75, 3.5}
    z2 = np.array([0.0, 4.0, 3.25, 3.75, 3.5, 3.1, 3.9, 3.5])
    # members of bin 3 in index order: 3.25, 3.75, 3.5, 3.1, 3.9, 3.5: six, the last (index 7) set aside; the median of the five left is
    # 3.5 (index 4).  Both 4 and 7 equal it: the lowest is 4
    assert SS.select_1d(z2, 4).tolist() == [0, -1, -1, 4]
    z3 = np.array([0.0, 4.0, 3.5, 3.25, 3.75, 3.5])                               # four members; 3.5 (5) set aside; median of the rest 3.5: index 2
    assert SS.select_1d(z3, 4).tolist() == [0, -1, -1, 2]
    z4 = np.array([0.0, 4.0, 3.25, 3.5])                                          # two members: 3.5 set aside, the median is 3.25
    assert SS.select_1d(z4, 4, None).tolist() == [0, -1, -1, 2] and SS.select_1d(z4, 4, "keep_last").tolist() == [0, -1, -1, 2]
    # -0.0 == 0.0: the lowest index that compares equal wins, whatever its sign
    assert SS.select_1d(np.array([-1.0, -0.0, 0.0, 0.0, 1.0]), 1).tolist() == [1]


def test_select_log_lays_out_what_the_header_says():
    rng = np.random.default_rng(3)
    log = rng.normal(size=(300, SS.REC))
    log[:, 13] = 1.0
    log[::7, 13], log[::11, 13] = 0.0, 2.0
    log[5, 0], log[6, 10] = np.nan, np.inf
    log[:, 3] = np.where(np.arange(300) % 3 == 0, -5.0, 5.0)                      # feature 10 routes: a third to cluster 0, none to cluster 2
    bins, sel, info = SS.select_log(log, [[-5.0], [5.0], [50.0]], [10], [(7, 7), (8, 9)], [20, 7])
    assert bins.shape == (3, 3, 32, 5) and sel.shape == (3, 3, 32) and info.shape == (3, 3, 4)
    assert info[2, 0].tolist() == [0, 0, 20, SS.ENOVALID] and not bins[2].any() and (sel[2] == -1).all() and info[:, 2].tolist() == [[0] * 4] * 3
    for c in range(2):
        for g, (f, o) in enumerate([(7, 7), (8, 9)]):
            n, took, empty, status = info[c, g]
            idx = sel[c, g][sel[c, g] >= 0]
            assert status == 0 and n == idx.size and n + empty == (20, 7)[g] and (sel[c, g, (20, 7)[g]:] == -1).all()
            assert (log[idx, 13] == 1.0).all() and (np.where(log[idx, 3] < 0, 0, 1) == c).all()
            assert np.array_equal(bins[c, g, :n, 1], log[idx, f - 7]) and np.array_equal(bins[c, g, :n, 4], log[idx, 3 + o])
            assert (bins[c, g, :n, 0] == 1.0).all() and not bins[c, g, :n, 2:4].any() and not bins[c, g, n:].any()
            assert (np.diff(bins[c, g, :n, 1]) > 0).all()                          # ascending bins: ascending values
    assert 5 not in sel[:, 0] and 6 not in sel[:, 0]
