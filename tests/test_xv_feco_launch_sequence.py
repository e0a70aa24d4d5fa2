"""The launch SEQUENCE of sg_xv_pgd_run_feco, pinned on the CPU.

``xv_feco_asan_driver`` (tests/native/, a stand-alone program of the sanitizer build of the library's host half on the host-memory
double of the HIP runtime) walks the loop at level 1 and level 2 in every form a pass can take -- deterministic; only the defense
random, its repeats as one group and as full groups plus a smaller tail group; a dithered front-end with every repeat a row, as
one group, as groups with a tail and one repeat per pass, with random and with even init; the final pass alone -- and every
refusal.  It prints one line per kernel launch, in order, and one line per refused call; the driver itself checks that no
refusal launched anything, that the trace carries the new stage tags and that nothing allocated is left.  The output must be,
byte for byte, tests/native/xv_feco_launch_sequence.expected, and the run must end clean under AddressSanitizer + UBSan.
(The loops without FeCo: tests/test_loop_launch_sequence.py, whose table this pull request does not move.)

After an INTENDED change of the sequence: ``python tests/test_xv_feco_launch_sequence.py --record`` and review the diff.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "asan", "xv_feco_asan_driver")
TABLE = os.path.join(ROOT, "tests", "native", "xv_feco_launch_sequence.expected")
REFUSED = ("feco NULL", "level 0", "level 3", "B 1", "k 0", "k F+1", "k 31 below the TDNN context", "FeCo max_iter 0",
           "F 5000 k 2500 past the k-means kernel's LDS", "eot 4 in batches of 3", "3000 x 48000 past the 2 GiB activation bound",
           "max_iter -1")


def _table():
    r = subprocess.run(["make", "-j4", EXE[len(ROOT) + 1:]], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    # the driver sets SG_TUNE and SG_EOT_MAX_ROWS itself, case by case: nothing of the caller's environment counts
    env = {k: v for k, v in os.environ.items() if not k.startswith(("SG_", "HIPDOUBLE_"))}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "exit %d\n%s" % (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(set(line.split(" | ")[0] for line in lines)) == len(lines), "a label is printed twice"
    refused = [line for line in lines if " | rc=" in line]
    assert [line.split(" | ")[0] for line in refused] == ["refused: " + what for what in REFUSED]
    assert all(" | rc=1 " in line for line in refused)  # SG_ERR_ARG, every one
    return "## 256 CUs, no knob but SG_EOT_MAX_ROWS where the label says max_rows (call #launch | kernel, grid, block, dynamic LDS)\n" + \
        "\n".join(lines) + "\n"


def test_xv_feco_launch_sequence_is_the_recorded_one():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs make and hipcc")
    got = _table().splitlines()
    with open(TABLE) as f:
        want = f.read().splitlines()
    if got == want:
        return
    i = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    pytest.fail("line %d of %d (%d printed)\n  recorded: %s\n  now:      %s" % (
        i + 1, len(want), len(got), want[i] if i < len(want) else "<end>", got[i] if i < len(got) else "<end>"))


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with open(TABLE, "w") as f:
        f.write(_table())
