"""The launch SEQUENCE of the entry points for batches of unequal lengths, pinned on the CPU.

``ragged_asan_driver`` (tests/native/, a stand-alone program of the sanitizer build of the library's host half on the host-memory
double of the HIP runtime) walks sg_xv_forward_ragged, sg_xv_loss_grad_ragged and sg_xv_pgd_run_ragged: every refusal at each
entry; a context that goes from a uniform call to a ragged one and back; the device loop for 3 utterances and 2 steps without
dither, with dither and EOT repeats as one group and as one repeat per pass, the final pass alone, and 12 utterances whose
overlap-add owns four samples per thread; two contexts.  It prints one line per kernel launch, in order, and one line per
refused call; the driver itself checks that no refusal launched or allocated anything, that the workspace stops growing and
that nothing allocated is left.  The output must be, byte for byte, tests/native/ragged_launch_sequence.expected, and the run
must end clean under AddressSanitizer + UBSan.

A call with lengths launches the ``*_ragged_kernel`` symbols, on the grids of their uniform counterparts; the uniform calls in
the same walk launch the kernels of old -- and the tables of the uniform loops (tests/test_loop_launch_sequence.py,
tests/test_launch_table.py) do not move.

After an INTENDED change of the sequence: ``python tests/test_ragged_launch_sequence.py --record`` and review the diff.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "asan", "ragged_asan_driver")
TABLE = os.path.join(ROOT, "tests", "native", "ragged_launch_sequence.expected")
FRONT_END = ("mfcc_fwd", "mfcc_bwd", "frames_to_wave", "cmvn_fwd", "cmvn_bwd", "pool_fwd", "pool_bwd")


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
    assert len(refused) == 22 and all(line.startswith("refused: ") and " | rc=1 " in line for line in refused)  # SG_ERR_ARG, every one
    # which symbols a call launches: with lengths every per-utterance stage is a *_ragged_kernel, without them none is
    for line in lines:
        if " | rc=" in line:
            continue
        label, kernel = line.split(" | ")
        stage = [s for s in FRONT_END if kernel.startswith(s)]
        if stage:
            assert kernel.startswith(stage[0] + "_ragged_kernel") != label.startswith("uniform"), line
    return "## 256 CUs, no knob but SG_EOT_MAX_ROWS where the label says max_rows (call #launch | kernel, grid, block, dynamic LDS)\n" + \
        "\n".join(lines) + "\n"


def test_ragged_launch_sequence_is_the_recorded_one():
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
