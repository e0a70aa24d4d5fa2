"""Test infrastructure (like tests/stoi_cases.py): move the buffers a caller hands to the C-ABI.

include/speakerguard_hip.h asks a device pointer for no more than the alignment of its element type, and the host layer hands
row slices of a batch straight to the library, so a waveform of odd length reaches the kernels 4, 8 or 12 bytes off a 16-byte
boundary.  Fresh allocations never do: torch's allocator aligns them to 256 bytes and rounds them up to 512, which also hides a
store that runs a few elements past a ragged row, or a load that starts before one.

  ``window(t, k)``      a contiguous copy of `t` that starts `k` elements after a 16-byte boundary inside a larger buffer
                        whose `guard` elements on either side hold a poison value;
  ``intact(w)``         both guards still hold the poison, bit for bit;
  ``same(exp, got, w)`` the judge: every output bit-equal, every guard intact; names the first offender;
  ``Relocated(k)``      a context manager that puts every device tensor the host layer (or a test) names to ``Context.call``
                        through ``_native._ptr`` through ``window``, inputs, outputs and in-place buffers alike, and copies
                        the windows back after the call, so a whole public-API call runs on moved buffers without knowing it;
  ``placed(t)``         for the pointers ``_ptr`` never sees -- the ones the host layer writes into a descriptor struct with a
                        bare ``data_ptr()`` (``sg_dither.noise_dev``, ``sg_wav_defense.noise_dev``, ``sg_loss_spec.coef_dev``)
                        or hands over as a bare ``c_void_p`` (iv_plda's delta -> CMVN route): inside ``Relocated`` the tensor
                        itself becomes a window (read-only inputs, so nothing is copied back), outside it stays as it is.

Float poison is 2**100, large and finite: fmaxf / fminf drop a NaN, so a NaN that a range kernel reads past the end of a row
would stay invisible.  Integer buffers carry a fixed bit pattern.
"""
import torch

GUARD = 64
FLOAT_POISON = 2.0 ** 100
INT_POISON = {torch.int8: 0x5A, torch.uint8: 0xA5, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
_BITS = {torch.float32: torch.int32, torch.float64: torch.int64}
DTYPES = (torch.float32, torch.float64, torch.int16, torch.int32, torch.int64, torch.uint8)


def poison_of(dtype):
    if dtype in _BITS:
        return FLOAT_POISON
    return INT_POISON[dtype]


def bits(t):
    """the integer view of a tensor: what "bit-equal" compares (-0.f != 0.f, a NaN equals itself)"""
    return t.view(_BITS[t.dtype]) if t.dtype in _BITS else t


def residue(dtype, k):
    """where ``window(., k)`` starts, in bytes past a 16-byte boundary: k elements of the type"""
    return (k * torch.empty(0, dtype=dtype).element_size()) % 16


def window(t, k, guard=GUARD):
    """A contiguous tensor equal to `t`, inside a larger buffer, ``data_ptr() % 16 == residue(t.dtype, k)``; `guard` poisoned
    elements lie on each side of it.  The frame travels with the result (``w.cb_frame``) for ``intact`` / ``guard_report``."""
    if t.dtype not in INT_POISON and t.dtype not in _BITS:
        raise TypeError("no poison for %s" % t.dtype)
    n, size = t.numel(), t.element_size()
    buf = torch.full((n + 2 * guard + 16,), poison_of(t.dtype), dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % size == 0
    want = residue(t.dtype, k)
    start = guard
    while (buf.data_ptr() + start * size) % 16 != want:
        start += 1
    assert start < guard + 16
    w = buf[start:start + n].view(t.shape)
    with torch.no_grad():
        w.copy_(t)
    w.cb_frame = (buf, start, n, guard)
    assert w.is_contiguous() and w.data_ptr() % 16 == want
    return w


def guard_report(w):
    """None when both guards of `w` hold the poison bit for bit, else where the first damaged element lies"""
    buf, start, n, guard = w.cb_frame
    want = bits(torch.full((guard,), poison_of(buf.dtype), dtype=buf.dtype, device=buf.device))
    for name, lo in (("before", start - guard), ("after", start + n)):
        bad = (bits(buf[lo:lo + guard]) != want).nonzero()
        if bad.numel():
            i = int(bad[0 if name == "after" else -1])
            where = i + 1 if name == "after" else guard - i
            return "guard %s the window damaged, %d element(s) %s its %s" % (
                name, where, "past" if name == "after" else "before", "end" if name == "after" else "start")
    return None


def intact(w):
    return guard_report(w) is None


def first_difference(a, b):
    """None when `a` and `b` are bit-equal, else a description of the first element that is not"""
    if a is None or b is None:
        return None if a is b else "one of the two is missing"
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape / dtype %s %s against %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    bad = (bits(a) != bits(b)).nonzero()
    if not bad.numel():
        return None
    i = int(bad[0])
    return "%d of %d elements differ, the first at %d: expected %r, got %r" % (bad.numel(), a.numel(), i, a[i].item(), b[i].item())


def same(expected, got, windows):
    """The judge.  `expected`, `got`: dicts name -> tensor (or None); `windows`: the windows the call under test ran on, as
    tensors or as (label, tensor) pairs.  -> (True, "bit-equal, guards intact") or (False, what differed, first offender)."""
    if sorted(expected) != sorted(got):
        return False, "outputs %s against %s" % (sorted(expected), sorted(got))
    for name in expected:
        d = first_difference(expected[name], got[name])
        if d:
            return False, "output %s: %s" % (name, d)
    for i, w in enumerate(windows):
        label, w = w if isinstance(w, tuple) else ("window %d" % i, w)
        r = guard_report(w)
        if r:
            return False, "%s (%s, %d bytes off a 16-byte boundary): %s" % (label, w.dtype, w.data_ptr() % 16, r)
    return True, "bit-equal, guards intact"


_ACTIVE = []  # the Relocated block that is open, if any


def placed(t):
    """`t` as a caller would hold it where ``Relocated`` cannot reach: inside an open block a window of its own (guards checked
    with the block's other windows), else `t`.  For input tensors whose pointer travels inside a struct or as a bare address."""
    if not _ACTIVE:
        return t
    reloc = _ACTIVE[-1]
    k = reloc.k if reloc.k != "mixed" else (len(reloc.windows) + 1) % 4
    w = window(t, k)
    reloc.windows.append(("placed input %d" % len(reloc.windows), w))
    reloc.placed += 1
    return w


class Relocated:
    """While active, every device tensor handed to ``speakerguard_amd._native._ptr`` -- which is how the host layer and the tests
    name a buffer to ``Context.call`` -- is replaced by ``window(tensor, k)`` for the length of that call, and copied back after
    it (on the call's stream, behind the call): inputs, outputs and in-place buffers all lie k elements off a 16-byte
    boundary, between poisoned guards.  Pointers that do not pass ``_ptr`` (a ``data_ptr()`` written into a descriptor struct,
    a bare ``c_void_p``) stay where they are: a test moves those itself, with ``placed``.
    A tensor named twice in one call (an output that aliases an input) keeps one window.
    `k`: 0..3, or "mixed": consecutive buffers of a call take 1, 2, 3, 0, 1, ...  The windows stay alive until the block ends
    (a table the library reads until a later call clears it stays valid), ``windows`` lists them with the entry and the
    position they were handed to; ``entries`` counts the windows per entry point."""

    def __init__(self, k, host_too=False):
        self.k = k
        self.host_too = host_too  # (the CPU tests of this class: host tensors stand in for device tensors)
        self.windows = []
        self.entries = {}
        self.placed = 0  # inputs a test moved itself (``placed``)
        self._pending = []

    def _k(self):
        return self.k if self.k != "mixed" else (len(self._pending) + 1) % 4

    def __enter__(self):
        from speakerguard_amd import _native as N
        self._N, self._ptr, self._call = N, N._ptr, N.Context.call
        reloc = self

        def ptr(t):
            if t is None or (t.device.type == "cpu" and not reloc.host_too):
                return reloc._ptr(t)
            assert t.is_contiguous(), "the host layer hands contiguous tensors over"
            for src, w in reloc._pending:
                if src.data_ptr() == t.data_ptr() and src.dtype == t.dtype and src.numel() == t.numel():
                    return reloc._ptr(w)
            w = window(t, reloc._k())
            reloc._pending.append((t, w))
            return reloc._ptr(w)

        def flush(name, pending):
            with torch.no_grad():
                for i, (t, w) in enumerate(pending):
                    t.copy_(w)
                    reloc.windows.append(("%s buffer %d" % (name, i), w))
            reloc.entries[name] = reloc.entries.get(name, 0) + len(pending)

        def call(ctx, name, *args):
            pending, reloc._pending = reloc._pending, []
            try:
                return reloc._call(ctx, name, *args)
            finally:
                flush(name, pending)

        def check(ctx, rc, what):
            """(a caller that reads the return code itself goes through ``lib.<entry>`` and then ``check``: WarpedFeCoDefense)"""
            if reloc._pending:
                pending, reloc._pending = reloc._pending, []
                flush(what, pending)
            return reloc._check(ctx, rc, what)

        self._check = N.Context.check
        N._ptr, N.Context.call, N.Context.check = ptr, call, check
        _ACTIVE.append(self)
        return self

    def __exit__(self, *exc):
        _ACTIVE.remove(self)
        self._N._ptr, self._N.Context.call, self._N.Context.check = self._ptr, self._call, self._check
        assert not self._pending or exc[0] is not None, "buffers were named to _ptr and no call took them"
        return False
