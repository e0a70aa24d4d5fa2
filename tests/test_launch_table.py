"""The contraction launcher's CHOICE of kernel, pinned on the CPU.

Every stream-K kind and every tile kernel gives the same bits (tests/test_gpu_conv.py, tests/test_gpu_layers.py), so a
launcher that picks a slower kernel passes every GPU test.  ``abi_asan_driver --launch-table`` (the sanitizer build of the
library's host half on the host-memory double of the HIP runtime, tests/native/) prints one line per ``conv_gemm*`` launch:
kernel name with template arguments, grid, block, dynamic LDS, the ConvGemmArgs fields the launcher fills and the scalar
kernel arguments.  One process per device / knob setting (the knobs are read once per process); together they must be,
byte for byte, tests/native/conv_launch_table.expected: the default run in full, and of every other run its number of lines
and those of its lines that the default run does not print (every line carries its case label and is unique in its run);
where the default run has a line with the same label, only the fields that differ from it.

After an INTENDED change of the launcher's choice: ``python tests/test_launch_table.py --record`` and review the diff.
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "asan", "abi_asan_driver")
TABLE = os.path.join(ROOT, "tests", "native", "conv_launch_table.expected")

# (driver mode, environment).  "all": every kernel x epilogue at every isolated shape, the whole models, fault injection.
# The other runs are thinned, or the recording would be too large to read: the launcher's own choice at every isolated shape,
# the forced kernels at the eleven shapes of tests/test_gpu_conv.py::SHAPES; "device" with the whole models, "isolated" without.
VARIANTS = [("all", {})]
VARIANTS += [("device", {"HIPDOUBLE_CUS": str(n)}) for n in (304, 120, 8)]
VARIANTS += [("device", {"HIPDOUBLE_OCCUPANCY": str(n)}) for n in (1, 0)]
VARIANTS += [("isolated", {k: str(v)}) for k, v in [
    ("SG_STREAMK", 0), ("SG_STREAMK_W16", 0), ("SG_STREAMK_MID", 0), ("SG_STREAMK_MID9", 1), ("SG_STREAMK_DEEP", 0),
    ("SG_STREAMK_WS", 0), ("SG_STREAMK_WS_MINCHUNKS", 16), ("SG_STREAMK_WS_MINCHUNKS", 200), ("SG_STREAMK_MINCHUNKS", 4),
    ("SG_STREAMK_KIND", 5), ("SG_STREAMK_KIND", 6), ("SG_STREAMK_KIND", 7), ("SG_STREAMK_KIND", 8), ("SG_STREAMK_KIND", 9),
    ("SG_TILE32", 0), ("SG_QUADFEED", 0), ("SG_S16_MAX_BLOCKS", 0), ("SG_STREAMK_XCD", 0), ("SG_STREAMK_XCD", 1)]]


def _walk(variant):
    mode, knobs = variant
    env = {k: v for k, v in os.environ.items() if not k.startswith(("SG_", "HIPDOUBLE_"))}
    env.update(knobs, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "--launch-table", mode], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "%s: exit %d\n%s" % (knobs, r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(set(lines)) == len(lines), "%s: a line is printed twice" % knobs
    return lines


def _table():
    r = subprocess.run(["make", "-j4", EXE[len(ROOT) + 1:]], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    with ThreadPoolExecutor(8) as pool:
        runs = list(pool.map(_walk, VARIANTS))
    default = dict(line.split(" | ") for line in runs[0])
    out = ["## default: 256 CUs, occupancy answer 2, no knob (k<kernel> e<epilogues> | launch, E: the epilogue asked for)"] + runs[0]
    for (mode, knobs), lines in zip(VARIANTS[1:], runs[1:]):
        (knob, value), = knobs.items()
        out.append("## %s=%s (%s): %d lines, of which the default run does not print" % (knob, value, mode, len(lines)))
        for label, launch in (line.split(" | ") for line in lines):
            was = default.get(label, "").split()
            if launch.split() != was:
                same_form = len(was) == len(launch.split())
                out.append(label + " | " + " ".join(t for t, w in zip(launch.split(), was) if t != w) if same_form else label + " | " + launch)
    return "\n".join(out) + "\n"


def test_launch_table_is_the_recorded_one():
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
