"""The device-resident PGD loops' launch SEQUENCE, pinned on the CPU.

Every form a loop can take -- EOT repeats as one pass, as full groups, with a smaller tail group; a chain whose backward is
the identity on shared rows, a chain with a backward of its own on one row per repeat; the waveform ping-pong or the
repeat-sum update; FeCo behind a chain -- gives the same bits (tests/test_gpu_defended_loop.py,
tests/test_gpu_an_defended_loop.py), so a wrong choice passes every GPU parity test.  ``abi_asan_driver --loop-sequence``
(the sanitizer build of the library's host half on the host-memory double of the HIP runtime, tests/native/) walks
sg_xv_pgd_run, sg_xv_pgd_run_defended and sg_an_pgd_run_defended and prints one line per kernel launch, in order: kernel
name with template arguments, grid, block, dynamic LDS and, for the fused CNN kernels, the planned fields of AnFusedArgs.
The output must be, byte for byte, tests/native/loop_launch_sequence.expected.  (sg_an_pgd_run and sg_an_pgd_run_feco:
tests/test_an_launch_sequence.py.)  Only kernel launches are recorded: the asynchronous copies -- labels, the replicated
iterate, the copy home -- are the business of the GPU bit-equality tests and of the sanitizer drivers' exact-extent buffers.

After an INTENDED change of the sequence: ``python tests/test_loop_launch_sequence.py --record`` and review the diff.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "asan", "abi_asan_driver")
TABLE = os.path.join(ROOT, "tests", "native", "loop_launch_sequence.expected")


def _table():
    r = subprocess.run(["make", "-j4", EXE[len(ROOT) + 1:]], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    # the driver sets SG_TUNE and SG_EOT_MAX_ROWS itself, case by case: nothing of the caller's environment counts
    env = {k: v for k, v in os.environ.items() if not k.startswith(("SG_", "HIPDOUBLE_"))}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "--loop-sequence"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "exit %d\n%s" % (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(set(line.split(" | ")[0] for line in lines)) == len(lines), "a label is printed twice"
    assert not [line for line in lines if " | rc=" in line], "a call was refused: %s" % [line for line in lines if " | rc=" in line][:3]
    return "## 256 CUs, no knob but SG_EOT_MAX_ROWS where the label says max_rows (call #launch | kernel, grid, block, dynamic LDS; an_cnn_*: the plan)\n" + \
        "\n".join(lines) + "\n"


def test_loop_launch_sequence_is_the_recorded_one():
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
