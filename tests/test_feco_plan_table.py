"""The FeCo k-means launchers' CHOICES, pinned on the CPU.

Every choice the launcher of the FeCo k-means makes gives the same bits (DESIGN.md "The FeCo k-means": chunks merge in ascending
centroid order, paired blocks run the same k-means redundantly), so a launcher that cut no chunks, never paired, never dealt the
units or kept the frames out of LDS passes every GPU test -- and gives back the time those choices earned.
``feco_cos_asan_driver --plan-table`` (the sanitizer build of the library's host half on the host-memory double of the HIP
runtime, tests/native/) prints one line per FeCo launch: kernel name with template arguments, grid, block, dynamic LDS and, for
the base kernels, x_in_lds, fast_lists, JC, the unit table of block 0 (per wave ``ft:lo-hi:jc,...``: frame tile, centroid tiles
[lo, hi), chunk), the pairing switch, the owner mask, block 1's table and the fault-injection flag.  One process per device /
knob setting; together they must be, byte for byte, tests/native/feco_plan_table.expected: the default run in full, and of every
other run its number of lines and those of its lines that the default run does not print; where the default run has a line
with the same label, only the fields that differ from it.

After an INTENDED change of the plan: ``python tests/test_feco_plan_table.py --record`` and review the diff.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "asan", "feco_cos_asan_driver")
TABLE = os.path.join(ROOT, "tests", "native", "feco_plan_table.expected")

# (driver mode, environment): the default device, three other CU counts, and the context after sg_feco_set_two_cu(ctx, 0)
VARIANTS = [("default", {})]
VARIANTS += [("default", {"HIPDOUBLE_CUS": str(n)}) for n in (304, 120, 8)]
VARIANTS += [("two_cu0", {})]


def _walk(variant):
    mode, knobs = variant
    env = {k: v for k, v in os.environ.items() if not k.startswith(("SG_", "HIPDOUBLE_"))}
    env.update(knobs, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "--plan-table", mode], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "%s %s: exit %d\n%s" % (mode, knobs, r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(set(lines)) == len(lines), "%s %s: a line is printed twice" % (mode, knobs)
    return lines


def _table():
    r = subprocess.run(["make", "-j4", EXE[len(ROOT) + 1:]], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    with ThreadPoolExecutor(5) as pool:
        runs = list(pool.map(_walk, VARIANTS))
    default = dict(line.split(" | ") for line in runs[0])
    out = ["## default: 256 CUs, two CUs per instance where they fit (<case> | launch or refusal)"] + runs[0]
    for (mode, knobs), lines in zip(VARIANTS[1:], runs[1:]):
        name = " ".join("%s=%s" % kv for kv in knobs.items()) or "sg_feco_set_two_cu(ctx, 0)"
        out.append("## %s: %d lines, of which the default run does not print" % (name, len(lines)))
        for label, launch in (line.split(" | ") for line in lines):
            was = default.get(label, "").split()
            if launch.split() != was:
                same_form = len(was) == len(launch.split())
                out.append(label + " | " + " ".join(t for t, w in zip(launch.split(), was) if t != w) if same_form else label + " | " + launch)
    return "\n".join(out) + "\n"


def test_feco_plan_table_is_the_recorded_one():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs make and hipcc")
    got = _table().splitlines()
    with open(TABLE) as f:
        want = f.read().splitlines()
    if got == want:
        return
    i = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    section = [line for line in want[:i + 1] if line.startswith("## ")][-1:]
    pytest.fail("line %d of %d (%d printed), in %s\n  recorded: %s\n  now:      %s" % (
        i + 1, len(want), len(got), section, want[i] if i < len(want) else "<end>", got[i] if i < len(got) else "<end>"))


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with open(TABLE, "w") as f:
        f.write(_table())
