"""TEST INFRASTRUCTURE (checker only; never imported by the product).

The down-/up-sampling defense ``DS`` (reference defense/frequency_domain.py:8-31: two torchaudio 0.6.0 ``Resample`` calls,
Kaldi's LinearResample) restated three ways:

  * float64: the tables from the formula and the direct sums, forward and adjoint -- the truth the kernels are judged by,
    and what ``scipy.signal.upfirdn`` corroborates through unrelated code;
  * float32: the contract of speakerguard_amd/csrc/k_resample.hip, fmaf for fmaf -- what the kernels must reproduce bit for bit;
  * torch ``conv1d`` in float64 -- the form autograd differentiates.

A stage's tables: dict(in_unit, out_unit, W, first (out_unit,), weight (out_unit, W)); output m = u out_unit + p is
sum_j weight[p][j] x[first[p] + u in_unit + j], x zero outside [0, n)."""
import math

import numpy as np

from time_domain_restate import fmaf

F32 = np.float32
U = 2.0 ** -24  # unit round-off of float32
WIDTH = 6


def units(fi, fo):
    g = math.gcd(int(fi), int(fo))
    return int(fi) // g, int(fo) // g


def out_len(n, fi, fo):
    """the reference's tick arithmetic, as written"""
    tick = fi * fo // math.gcd(fi, fo)
    L = n * (tick // fi)
    last = L // (tick // fo)
    if L % (tick // fo) == 0:
        last -= 1
    return last + 1


def kernel64(delta, fi, fo):
    """the continuous filter at time offsets delta (seconds), divided by fi: the weight of a tap"""
    cutoff = 0.99 * 0.5 * min(fi, fo)
    w = WIDTH / (2 * cutoff)
    delta = np.asarray(delta, np.float64)
    safe = np.where(delta == 0, 1.0, delta)
    s = np.where(delta == 0, 2 * cutoff, np.sin(2 * np.pi * cutoff * safe) / (np.pi * safe))
    h = 0.5 * (1 + np.cos(2 * np.pi * cutoff / WIDTH * delta)) * s / fi
    return np.where(np.abs(delta) < w, h, 0.0)


def tables64(fi, fo, first=None, W=None):
    """float64 tables from the formula; with first / W given, the formula evaluated on THOSE windows"""
    fi, fo = int(fi), int(fo)
    in_unit, out_unit = units(fi, fo)
    cutoff = 0.99 * 0.5 * min(fi, fo)
    w = WIDTH / (2 * cutoff)
    t = np.arange(out_unit, dtype=np.float64) / fo
    if first is None:
        first = np.ceil((t - w) * fi).astype(np.int64)
        last = np.floor((t + w) * fi).astype(np.int64)
        W = int((last - first + 1).max())
    first = np.asarray(first, np.int64)
    delta = (first[:, None] + np.arange(W)[None]) / fi - t[:, None]
    return dict(in_unit=in_unit, out_unit=out_unit, W=int(W), first=first, weight=kernel64(delta, fi, fo))


def stage_len(n, tab):
    return -((-int(n) * tab["out_unit"]) // tab["in_unit"])


def _index(n_out, tab):
    m = np.arange(n_out)
    u, p = m // tab["out_unit"], m % tab["out_unit"]
    return p, np.asarray(tab["first"], np.int64)[p] + u * tab["in_unit"]


def _padded(x, base, W):
    """x (B, n) with zeros either side so that every base + j indexes it; -> (padded, offset)"""
    n = x.shape[1]
    lo = max(0, -int(base.min())) if len(base) else 0
    hi = max(0, int(base.max()) + W - n) if len(base) else 0
    return np.pad(x, ((0, 0), (lo, hi))), lo


# ---------------------------------------------------------------- float64
def stage64(x, tab):
    x = np.atleast_2d(np.asarray(x, np.float64))
    n_out = stage_len(x.shape[1], tab)
    p, base = _index(n_out, tab)
    xp, lo = _padded(x, base, tab["W"])
    w = np.asarray(tab["weight"], np.float64)
    out = np.zeros((x.shape[0], n_out))
    for j in range(tab["W"]):
        out += w[p, j][None] * xp[:, base + lo + j]
    return out


def adjoint64(g, tab, n_in):
    """stage64's transpose: (B, n_out) -> (B, n_in)"""
    g = np.atleast_2d(np.asarray(g, np.float64))
    n_out = stage_len(n_in, tab)
    assert g.shape[1] == n_out
    p, base = _index(n_out, tab)
    w = np.asarray(tab["weight"], np.float64)
    out = np.zeros((g.shape[0], n_in))
    for j in range(tab["W"]):
        i = base + j
        ok = (i >= 0) & (i < n_in)
        for b in range(g.shape[0]):
            np.add.at(out[b], i[ok], w[p[ok], j] * g[b, ok])
    return out


def ds64(x, down, up, same_size=True):
    x = np.atleast_2d(np.asarray(x, np.float64))
    y = stage64(stage64(x, down), up)
    return y[:, :x.shape[1]] if same_size else y


def ds_adjoint64(g, down, up, T, same_size=True):
    g = np.atleast_2d(np.asarray(g, np.float64))
    n_low = stage_len(T, down)
    n_up = stage_len(n_low, up)
    gp = np.zeros((g.shape[0], n_up))
    gp[:, :g.shape[1]] = g
    assert g.shape[1] == (T if same_size else n_up)
    return adjoint64(adjoint64(gp, up, n_low), down, T)


# ---------------------------------------------------------------- float32: the kernels' contract
def stage32(x, tab):
    """every output one fmaf chain from 0 over the W taps in ascending order, zero-padded taps included"""
    x = np.atleast_2d(np.asarray(x, F32))
    n_out = stage_len(x.shape[1], tab)
    p, base = _index(n_out, tab)
    xp, lo = _padded(x, base, tab["W"])
    w = np.asarray(tab["weight"], F32)
    acc = np.zeros((x.shape[0], n_out), F32)
    for j in range(tab["W"]):
        acc = fmaf(w[p, j][None], xp[:, base + lo + j], acc)
    return acc


def pair_lists(tab):
    """per residue r of the input index: [(toff, weight)] in ascending toff -- input i = v in_unit + r takes weight * g[v
    out_unit + toff]; derived from the definition, pair by pair"""
    iu, ou = tab["in_unit"], tab["out_unit"]
    lists = [[] for _ in range(iu)]
    for p in range(ou):
        for j in range(tab["W"]):
            s = int(tab["first"][p]) + j
            du = s // iu  # (floor)
            lists[s - du * iu].append((p - du * ou, tab["weight"][p][j]))
    return [sorted(l, key=lambda e: e[0]) for l in lists]


def adjoint32(g, tab, n_in):
    """every input sample one fmaf chain from 0 over the outputs whose window holds it, in ascending output index; outputs
    outside [0, n_out) enter as zeros"""
    g = np.atleast_2d(np.asarray(g, F32))
    n_out = stage_len(n_in, tab)
    assert g.shape[1] == n_out
    iu, ou = tab["in_unit"], tab["out_unit"]
    lists = pair_lists(tab)
    toffs = [t for l in lists for t, _ in l]
    lo = max(0, -min(toffs))
    hi = max(0, ((n_in - 1) // iu) * ou + max(toffs) + 1 - n_out)
    gp = np.pad(g, ((0, 0), (lo, hi)))
    out = np.zeros((g.shape[0], n_in), F32)
    for r, l in enumerate(lists):
        v = np.arange(r, n_in, iu) // iu
        if not len(v):
            continue
        acc = np.zeros((g.shape[0], len(v)), F32)
        for toff, w in l:
            acc = fmaf(F32(w), gp[:, v * ou + toff + lo], acc)
        out[:, r::iu] = acc
    return out


def ds32(x, down, up, same_size=True):
    x = np.atleast_2d(np.asarray(x, F32))
    y = stage32(stage32(x, down), up)
    return y[:, :x.shape[1]].copy() if same_size else y


def ds_adjoint32(g, down, up, T, same_size=True):
    g = np.atleast_2d(np.asarray(g, F32))
    n_low = stage_len(T, down)
    n_up = stage_len(n_low, up)
    assert g.shape[1] == (T if same_size else n_up)
    gp = np.zeros((g.shape[0], n_up), F32)
    gp[:, :g.shape[1]] = g
    return adjoint32(adjoint32(gp, up, n_low), down, T)


# ---------------------------------------------------------------- a-priori error bounds of the float32 contract
def gamma(k):
    return k * U / (1 - k * U)


def _abs(tab, weight=None):
    return dict(tab, weight=np.abs(np.asarray(tab["weight"] if weight is None else weight, np.float64)))


def forward_bound(x, down, up, same_size=True):
    """|ds32(x) - ds64(x; float64 tables)| elementwise, from first principles.  With D, U the float32 tables, D*, U* the
    float64 formula on the same windows, low = fl(D x), y = fl(U low):
        |y - U* D* x| <= gamma_Wu |U||low|              (the Up chain: W_u fmafs, Higham 3.5 with fused terms)
                       + |U| (gamma_Wd |D||x|)           (the Down chain's error, carried through |Up|)
                       + |U| (|D - D*||x|)               (Down's table rounding, likewise)
                       + |U - U*| |D* x|                 (Up's table rounding)"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    d64 = tables64(down["fi"], down["fo"], down["first"], down["W"])
    u64 = tables64(up["fi"], up["fo"], up["first"], up["W"])
    low32 = stage32(x.astype(F32), down).astype(np.float64)
    e_low = gamma(down["W"]) * stage64(np.abs(x), _abs(down)) + stage64(np.abs(x), _abs(down, np.asarray(down["weight"], np.float64) - d64["weight"]))
    b = (gamma(up["W"]) * stage64(np.abs(low32), _abs(up)) + stage64(e_low, _abs(up))
         + stage64(np.abs(stage64(x, d64)), _abs(up, np.asarray(up["weight"], np.float64) - u64["weight"])))
    return b[:, :x.shape[1]] if same_size else b


def backward_bound(g, down, up, T, same_size=True):
    """the same four terms for gx = D^T U^T g; a chain has as many terms as the longest pair list of the stage"""
    g = np.atleast_2d(np.asarray(g, np.float64))
    n_low = stage_len(T, down)
    n_up = stage_len(n_low, up)
    gp = np.zeros((g.shape[0], n_up))
    gp[:, :g.shape[1]] = g
    d64 = tables64(down["fi"], down["fo"], down["first"], down["W"])
    u64 = tables64(up["fi"], up["fo"], up["first"], up["W"])
    ku, kd = (max(len(l) for l in pair_lists(t)) for t in (up, down))
    glow32 = adjoint32(gp.astype(F32), up, n_low).astype(np.float64)
    e_low = gamma(ku) * adjoint64(np.abs(gp), _abs(up), n_low) + adjoint64(np.abs(gp), _abs(up, np.asarray(up["weight"], np.float64) - u64["weight"]), n_low)
    return (gamma(kd) * adjoint64(np.abs(glow32), _abs(down), T) + adjoint64(e_low, _abs(down), T)
            + adjoint64(np.abs(adjoint64(gp, u64, n_low)), _abs(down, np.asarray(down["weight"], np.float64) - d64["weight"]), T))


def class_tables(param=0.5, fs=16000):
    """(down, up) as the product's table builder makes them, with the rates attached (the bounds need the formula)"""
    from speakerguard_amd.defense.frequency_domain import ds_tables
    new = int(fs * param)
    return dict(ds_tables(fs, new), fi=fs, fo=new), dict(ds_tables(new, fs), fi=new, fo=fs)


# ---------------------------------------------------------------- torch, for autograd
def stage_torch(x, tab):
    """(B, n) float64 tensor -> (B, n_out): one strided conv1d per phase, interleaved"""
    import torch
    n = x.shape[1]
    n_out = stage_len(n, tab)
    iu, ou, W = tab["in_unit"], tab["out_unit"], tab["W"]
    n_units = -(-n_out // ou)
    first = [int(f) for f in tab["first"]]
    lo = max(0, -min(first))
    hi = max(0, max(first) + (n_units - 1) * iu + W - n)
    xp = torch.nn.functional.pad(x, (lo, hi))
    w = torch.as_tensor(np.asarray(tab["weight"], np.float64))
    cols = []
    for p in range(ou):
        seg = xp[:, first[p] + lo:first[p] + lo + (n_units - 1) * iu + W]
        cols.append(torch.nn.functional.conv1d(seg[:, None, :], w[p].view(1, 1, W), stride=iu)[:, 0, :])
    return torch.stack(cols, 2).reshape(x.shape[0], n_units * ou)[:, :n_out]


def ds_torch(x, down, up, same_size=True):
    """the reference's DS on a (B, T), (B, 1, T) or (T,) tensor, in float64, differentiable"""
    shape = x.shape
    rows = x.reshape(-1, shape[-1]).double()
    y = stage_torch(stage_torch(rows, down), up)
    if same_size:
        y = y[:, :shape[-1]]
    return y.reshape(tuple(shape[:-1]) + (y.shape[1],))
