"""Instruction budget of kernel F (admpc_fused20.hip) per phase, from the compiled gfx950 listing.

The kernel is bound by instruction issue (kernel F, "What bounds it now"): what a stage chain rebuilds from literals, a
select that computes nothing or a block of register copies is time.  This test compiles the unit to a listing with the flags the
Makefile ships (taken from `make -n`, not repeated here) plus `-S -DF20_MARKS --cuda-device-only`, counts the instructions of the
`<7>` instantiation between its `; MARK_after<k>` comments and asserts per phase

    vector instructions <= the count of the build this test came with + 2 %

(the slack lets an unrelated edit pass; losing one of the cuts below does not fit in it), and from the kernel's metadata scratch 0 and
at most 256 VGPRs.  Opcodes are classed by prefix only (`v_`, `ds_`, `s_`).

Vector instructions per phase, the build before the per-lane addresses of phases C and E were formed once per instance -> this build:
    C (condensing, behind stamp 2)            1921 -> 1593
    trial (behind stamp 3)                    1433 -> 1433
    interior-point loop (behind stamp 4)      2370 -> 2370
    E (expansion, behind stamp 5)              642 ->  593
"""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ad_mpc_amd", "csrc")
UNIT = "admpc_fused20"

# vector instructions of the <7> instantiation per region (the code behind stamp k): achieved, the bound is achieved + 2 %
ACHIEVED = {"MARK_after2": ("C", 1593), "MARK_after3": ("trial", 1433), "MARK_after4": ("interior-point loop", 2370), "MARK_after5": ("E", 593)}
SLACK = 1.02


def _shipped_command():
    """The hipcc command line of the unit's object as the Makefile would run it (dry run, forced)."""
    out = subprocess.run(["make", "-C", CSRC, "-n", "-B", "HIPCC=hipcc", "_build/%s.o" % UNIT], check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if (UNIT + ".hip") in l and " -c " in l]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


def _listing(tmp_path):
    cmd = _shipped_command()
    i = cmd.index("-c")
    assert cmd[i + 1] == "-o"
    out = str(tmp_path / (UNIT + ".s"))
    cmd[i:i + 3] = ["-S", "-DF20_MARKS", "--cuda-device-only", "-o", out]
    subprocess.run(cmd, check=True, cwd=CSRC, capture_output=True)
    return open(out).read().split("\n")


def _phase_counts(lines, mangled_fragment):
    start = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + mangled_fragment + r"\w*:", l)]
    assert len(start) == 1
    start = start[0]
    end = start + [i for i, l in enumerate(lines[start:]) if ".amdhsa_kernel" in l][0]
    cur, stats = "PRE", {}
    for l in lines[start:end]:
        m = re.search(r"; (MARK_\w+)", l)
        if m:
            cur = m.group(1)
        st = stats.setdefault(cur, dict(v=0, ds=0, s=0))
        t = l.strip().split(" ")[0] if l.strip() else ""
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        for pre in ("v_", "ds_", "s_"):
            if t.startswith(pre):
                st[pre[:-1]] += 1
    return stats


def _metadata(lines, mangled_fragment):
    """.vgpr_count and .private_segment_fixed_size of the kernel's entry in the amdhsa.kernels metadata."""
    text = "\n".join(lines)
    for entry in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        if re.match(r"^_Z\w*" + mangled_fragment + r"\w*$", name):
            return int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
    raise AssertionError("kernel metadata not found")


@pytest.mark.skipif(shutil.which("hipcc") is None or shutil.which("make") is None, reason="hipcc / make not available")
def test_vector_instructions_per_phase_and_resources(tmp_path):
    lines = _listing(tmp_path)
    key = "fused20_kernelILi7E"
    stats = _phase_counts(lines, key)
    for mark, (name, achieved) in ACHIEVED.items():
        st = stats[mark]
        print("%-22s vector %5d (bound %5d)  LDS %4d  scalar %4d" % (name, st["v"], int(achieved * SLACK), st["ds"], st["s"]))
    vgprs, scratch = _metadata(lines, key)
    print("VGPRs %d scratch %d" % (vgprs, scratch))
    for mark, (name, achieved) in ACHIEVED.items():
        assert stats[mark]["v"] <= int(achieved * SLACK), "phase %s: %d vector instructions, budget %d" % (name, stats[mark]["v"], int(achieved * SLACK))
    assert scratch == 0 and vgprs <= 256
