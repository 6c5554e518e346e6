"""The BUDGET rows of tests/test_fp32_path.py: 4 x the float emulator's distance from the fp64 oracle on each batch of
tests/fp32_path.py:ROWS (CPU only; the float oracle's linearisation), rounded up to two digits, with the emulator's values below.

    python scripts/fp32_budget_table.py [row ...]               # prints the rows
    python scripts/fp32_budget_table.py --write                 # rewrites the block between BUDGET-BEGIN / BUDGET-END in the test file;
                                                                # the `device (MI355X)` line of a row that has one is kept
    python scripts/fp32_budget_table.py --device-log LOG        # no CPU work: sets every row's device line from the output of
                                                                # `pytest -s -m gpu tests/test_fp32_path.py` (its `F32 <row> device ...` lines)
"""
import os
import re
import sys
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def fmt(t):
    return "(" + ", ".join("%.1e" % v for v in t) + ")"


def one(name):
    import fp32_path as F
    from ad_mpc_amd.config import default_config, tight_ipm
    from emu.emu import Emu
    from oracle.oracle import Oracle
    o64, o32, emu = Oracle(), Oracle(variant="f32"), Emu()
    if name.startswith("sqp_tol_N"):
        N = int(name[9:])
        s, ref = F.sqp_tol_batch(o64, N, nthreads=1)
        cfg = tight_ipm(default_config(N=N, sqp_iters=20, sqp_tol=F.SQP_TOL))
        x, u, st, nqp = F.emu_sqp_tol(emu, o64, cfg, s, F.cpu_lineariser(o32, cfg))
        assert (st == 0).all()
        su, sx = F.stats((x, u), ref)
    else:
        cfg, s = F.row(name)
        o = F.oracle_solve(o64, cfg, s, nthreads=1)
        g = F.emu_passes(emu, cfg, s, F.cpu_lineariser(o32, cfg))
        F.batch_conditions(o, g, cfg)
        su, sx = F.stats(g, o)
    bu = tuple(F.round_up(F.BUDGET_FACTOR * v) for v in su); bx = tuple(F.round_up(F.BUDGET_FACTOR * v) for v in sx)
    return '    "%s": (%s, %s),\n    #   emulator (CPU): |du| %.1e / %.1e / %.1e; |dx| %.1e / %.1e / %.1e' % ((name, fmt(bu), fmt(bx)) + su + sx)


TEST = os.path.join(ROOT, "tests", "test_fp32_path.py")
DEV = "    #   device (MI355X): "
NOT_MEASURED = DEV + "not measured"


def block():
    src = open(TEST).read()
    i = src.index("\n", src.index("    # BUDGET-BEGIN")) + 1
    j = src.index("    # BUDGET-END")
    return src, i, j


def device_lines(text):
    """row -> its device line in a BUDGET block"""
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r'    "(\S+)": \(\(', line)
        if m:
            cur = m.group(1)
        elif line.startswith(DEV) and cur:
            out[cur] = line
    return out


def rewrite(rows, dev):
    """rows: [(name, text of the row with its emulator line)]; every row gets its device line, or says that it has none"""
    src, i, j = block()
    body = "".join("%s\n%s\n" % (text, dev.get(name, NOT_MEASURED)) for name, text in rows)
    open(TEST, "w").write(src[:i] + body + src[j:])


def from_log(path):
    log = open(path).read()
    dev = {m.group(1): DEV + "|du| %s / %s / %s; |dx| %s / %s / %s" % m.groups()[1:]
           for m in re.finditer(r"F32 (\S+)\s+device\s+\|du\| (\S+) / (\S+) / (\S+)\s+\|dx\| (\S+) / (\S+) / (\S+)", log)}
    src, i, j = block()
    rows, cur = [], None
    for line in src[i:j].rstrip("\n").split("\n"):
        m = re.match(r'    "(\S+)": \(\(', line)
        if m:
            rows.append([m.group(1), line])
        elif not line.startswith(DEV):
            rows[-1][1] += "\n" + line
    kept = device_lines(src[i:j])
    kept.update(dev)
    rewrite(rows, kept)
    print("device lines set for %d of %d rows" % (len(dev), len(rows)))


if __name__ == "__main__":
    import fp32_path as F
    argv = sys.argv[1:]
    if argv[:1] == ["--device-log"]:
        from_log(argv[1])
        sys.exit(0)
    write = argv[:1] == ["--write"]
    names = ([] if write else argv) or list(F.ROWS) + ["sqp_tol_N20", "sqp_tol_N40"]
    rows = []
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, text in zip(names, pool.imap(one, names)):
            rows.append((name, text))
            if not write:
                print(text, flush=True)
    if write:
        src, i, j = block()
        rewrite(rows, device_lines(src[i:j]))
