"""The AudioNet entry points' launch SEQUENCE, pinned on the CPU.

The CNN runs in one of four launch forms -- per layer, fused forward and backward with a separate an_tail, the head inside the
backward, forward + head + backward as one launch -- and all four give the same bits (tests/test_gpu_audionet.py), so a wrong
choice passes every GPU parity test.  ``abi_asan_driver --an-sequence`` (the sanitizer build of the library's host half on
the host-memory double of the HIP runtime, tests/native/) walks sg_an_forward / sg_an_loss_grad / sg_an_pgd_run /
sg_an_pgd_run_feco and prints one line per kernel launch, in order: kernel name with template arguments, grid, block, dynamic
LDS and, for the fused CNN kernels, the planned fields of AnFusedArgs.  One process per device / knob setting; together they
must be, byte for byte, tests/native/an_launch_sequence.expected: the default run's calls in full; what differs from them,
call by call, in the same process after sg_an_configure and in every other run (the device that refuses the LDS: from the
SG_AN_FUSED=0 run), as replacements: every distinct pair (launches removed, launches put in their place) once, with the
places (call #position in the run's sequence) where it applies.

After an INTENDED change of the sequence: ``python tests/test_an_launch_sequence.py --record`` and review the diff.
"""
import difflib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "asan", "abi_asan_driver")
TABLE = os.path.join(ROOT, "tests", "native", "an_launch_sequence.expected")

TUNE = {"SG_TUNE": "1"}  # the knobs count only behind it
# (driver mode, environment, index of the run it is compared with); "all": with the sg_an_configure cases
VARIANTS = [("all", {}, None)]
VARIANTS += [("passes", dict(TUNE, **knobs), 0) for knobs in (
    {"SG_AN_FUSED": "0"}, {"SG_AN_HEAD": "0"}, {"SG_AN_ONE": "1"}, {"SG_AN_ONE": "1", "SG_AN_SLICES": "1"},
    {"SG_AN_SLICES": "7"}, {"SG_AN_SLICES": "1000"})]
VARIANTS += [("passes", {"HIPDOUBLE_CUS": "8"}, 0), ("passes", {"HIPDOUBLE_CUS": "304"}, 0), ("passes", {"HIPDOUBLE_REFUSE_LDS": "1"}, 1)]
CONFIGURED = " fft="  # label suffix of a call made after sg_an_configure: " fft=32 cache=-1 ola=0"


def _walk(variant):
    mode, knobs, _ = variant
    env = {k: v for k, v in os.environ.items() if not k.startswith(("SG_", "HIPDOUBLE_"))}
    env.update(knobs, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([EXE, "--an-sequence", mode], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "%s: exit %d\n%s" % (knobs, r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(set(line.split(" | ")[0] for line in lines)) == len(lines), "%s: a label is printed twice" % knobs
    return lines


def _cases(lines):
    """{call label: [launch, ...]} in order ("label #n | launch")"""
    cases = {}
    for line in lines:
        label, launch = line.split(" | ")
        cases.setdefault(label[:label.rindex(" #")], []).append(launch)
    return cases


def _delta(base, lines):
    """`lines` against the calls of `base` with the same label (a configured call: the label without its settings)"""
    base, run = _cases(base), _cases(lines)
    blocks = {}  # (launches removed, launches in their place) -> places
    for label, now in run.items():
        was = base.get(label.split(CONFIGURED)[0], [])
        for op, i0, i1, j0, j1 in difflib.SequenceMatcher(None, was, now, autojunk=False).get_opcodes():
            if op != "equal":
                blocks.setdefault((tuple(was[i0:i1]), tuple(now[j0:j1])), []).append("%s #%d" % (label, j0 + 1))
    out = []
    for (removed, added), places in blocks.items():
        out += ["@ " + "; ".join(places[i:i + 6]) for i in range(0, len(places), 6)]
        out += ["- " + launch for launch in removed] + ["+ " + launch for launch in added]
    return out


def _table():
    r = subprocess.run(["make", "-j4", EXE[len(ROOT) + 1:]], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    with ThreadPoolExecutor(4) as pool:
        runs = list(pool.map(_walk, VARIANTS))
    configured = [line for line in runs[0] if CONFIGURED in line.split(" | ")[0]]
    runs[0] = [line for line in runs[0] if line not in configured]
    names = ["default"] + [" ".join("%s=%s" % kv for kv in knobs.items() if kv[0] != "SG_TUNE") for _, knobs, _ in VARIANTS[1:]]
    legend = "(@ places, - launches there, + launches here)"
    out = ["## default: 256 CUs, no knob (call #launch | kernel, grid, block, dynamic LDS; an_cnn_*: the plan)"] + runs[0]
    out.append("## after sg_an_configure, same process: %d lines; against the same calls of default %s" % (len(configured), legend))
    out += _delta(runs[0], configured)
    for name, (_, _, base), lines in zip(names[1:], VARIANTS[1:], runs[1:]):
        out.append("## %s: %d lines; against %s %s" % (name, len(lines), names[base], legend))
        out += _delta(runs[base], lines)
    return "\n".join(out) + "\n"


def test_an_launch_sequence_is_the_recorded_one():
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
