"""The launch lines that tests/batch_regimes.py mirrors are still the library's: if one changes, the boundary cases of
test_batch_regimes.py would test the wrong side of a switch without noticing, so this fails first."""
import os
import re

import pytest

from batch_regimes import LAUNCH_LINES, f_grid, s_grid, quad_grid, quad_tickets, quad_shoot_grid, nlp_res_grid, waypoints_grid, \
    s_below, s_past, f_past, quad_below, quad_past, nlp_res_past, WAYPOINTS_PAST, rowqp_rows, rowqp_splits, rowqp_sizes, \
    rowqp_inst_stride, rowqp_lds_rows, rowqp_per_cu, command_grid, COMMAND_PAST

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ad_mpc_amd", "csrc")


def _body(src, fn):
    """Text of the definition of `fn` (signature to the closing brace in column 0)."""
    m = re.search(r"^[^\n;]*\b%s\s*\([^;{]*\)\s*\{" % re.escape(fn), src, re.M)
    assert m, "no definition of %s" % fn
    end = src.find("\n}", m.end())
    return src[m.start():end]


@pytest.mark.parametrize("fname,fn,line", LAUNCH_LINES, ids=["%s:%s:%d" % (f, g, i) for i, (f, g, _) in enumerate(LAUNCH_LINES)])
def test_mirrored_launch_line_is_the_librarys(fname, fn, line):
    with open(os.path.join(CSRC, fname)) as f:
        src = f.read()
    if not fn:                                                   # a definition at file scope
        assert re.search(r"^%s\s*$" % re.escape(line), src, re.M), "%s no longer holds `%s`: update tests/batch_regimes.py" % (fname, line)
        return
    assert line in _body(src, fn), "%s:%s no longer holds `%s`: update tests/batch_regimes.py" % (fname, fn, line)


def test_sizes_sit_on_the_stated_side_of_every_switch():
    """The batches the GPU module picks are on the intended side for every CU count and LDS footprint."""
    for nc in (1, 38, 80, 104, 228, 256, 304):
        for lds in range(4096, 160 * 1024 + 1, 4096):
            assert f_grid(nc, f_past(nc)) < f_past(nc)
            for S in (2, 3, 4):
                assert s_grid(nc, s_past(nc, S), S, lds)[0] < s_past(nc, S)
                assert s_grid(nc, s_below(nc), S, lds)[0] == s_below(nc)
            for seg20 in (False, True):
                g = quad_grid(nc, quad_past(nc, seg20), seg20, lds)[0]
                assert quad_tickets(g, quad_past(nc, seg20))
                g = quad_grid(nc, quad_below(nc), seg20, lds)[0]
                assert not quad_tickets(g, quad_below(nc))
        assert quad_shoot_grid(nc, quad_past(nc)) < quad_past(nc)
        assert nlp_res_grid(nc, nlp_res_past(nc)) < nlp_res_past(nc)
        if nc >= 38:
            sz = rowqp_sizes(nc)
            assert [rowqp_rows(nc, sz[k]) for k in ("rows1", "rows2", "rows4", "split")] == [1, 2, 4, 4]
            assert [rowqp_splits(nc, sz[k], rowqp_rows(nc, sz[k])) for k in ("rows1", "rows2", "rows4", "split")] == [False, False, False, True]
    # the footprint rowqp_rows / rowqp_splits assume holds at the horizon of the fp32 regime test, and the mirror knows where it ends
    assert rowqp_inst_stride(20) == 656 and rowqp_lds_rows(20, 4) == 4 and rowqp_per_cu(20, 4, 4) == 4
    assert rowqp_lds_rows(128, 8) == 4 and rowqp_per_cu(128, 8, 4) == 1 and rowqp_per_cu(80, 4, 4) == 4 and rowqp_per_cu(128, 4, 4) == 2
    assert waypoints_grid(WAYPOINTS_PAST) < WAYPOINTS_PAST and waypoints_grid(4096) == 4096
    assert command_grid(COMMAND_PAST) < COMMAND_PAST and command_grid(COMMAND_PAST // 2) == COMMAND_PAST // 2 and COMMAND_PAST % 2 == 0

