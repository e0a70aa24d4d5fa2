"""TEST INFRASTRUCTURE (never imported by the product): csrc/k_pso.hip restated in plain torch / numpy on the CPU --
``RestatedSwarm`` has the three operations of ``EngineOps`` (``pso_init`` / ``pso_select`` / ``pso_move``) with the same
arguments, the row list and the per-row flags, and works on a ``SwarmState`` whose tensors live on the CPU.

Every float32 operation is the reference's (attack/SirenAttack.py:66-86, :115-132, :163-174): torch elementwise operators, one
rounding each.  The library's own draws are restated on oracle/philox.py: one Philox4x32-10 call per (t, particle, global
utterance), counter (t, particle, g lo, g hi), key = the draw's key; word 0 -> position or r1, word 1 -> velocity or r2.
"""
import numpy as np
import torch

from oracle import philox as ph

MAX_ROWS, MAX_PARTICLES = 256, 1024


def uniforms(key, g, P, T):
    """(u0, u1), each (P, T) float32 in (0, 1): the two uniforms of every (particle, sample) of global utterance `g`"""
    k0, k1 = ph._key(key)
    t, p = np.arange(T)[None, :], np.arange(P)[:, None]
    w0, w1, _, _ = ph.philox4x32_10(t, p, int(g) & 0xFFFFFFFF, (int(g) >> 32) & 0xFFFFFFFF, k0, k1)
    return torch.from_numpy(ph._uniform(w0)), torch.from_numpy(ph._uniform(w1))


def _f32(v, shape):
    return None if v is None else torch.as_tensor(v, dtype=torch.float32).cpu().reshape(shape)


def check_rows(n, P, T, rows):
    """what the entry points refuse about the shape and the row list"""
    if not (1 <= n <= MAX_ROWS and 1 <= P <= MAX_PARTICLES and T >= 1):
        raise ValueError("shape")
    if not 1 <= len(rows) <= n or len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= n:
        raise ValueError("rows")


class RestatedSwarm:

    def pso_init(self, st, x, lower, upper, rows, epoch, best_index, key, index_base=0, pos_in=None, vel_in=None):
        n, P, T = st.loc.shape
        rows = [int(r) for r in rows]
        check_rows(n, P, T, rows)
        carry = 1 if epoch > 0 else 0
        if carry and any(not 0 <= int(b) < P for b in best_index):
            raise ValueError("best_index")
        pos_in, vel_in = _f32(pos_in, (len(rows), P - carry, T)), _f32(vel_in, (len(rows), P, T))
        queries = torch.empty(len(rows) * P, 1, T, dtype=torch.float32)
        for k, slot in enumerate(rows):
            lo, hi, xv = lower[slot, 0], upper[slot, 0], x[slot, 0]
            u0, u1 = uniforms(key, index_base + slot, P, T)
            if pos_in is not None:
                fresh = pos_in[k]
            else:
                fresh = torch.min(torch.max(lo + (hi - lo) * u0[carry:], lo), hi)
            if vel_in is not None:
                vel = vel_in[k]
            else:
                v_hi = torch.abs(lo - hi)
                v_lo = -v_hi
                vel = torch.min(torch.max(v_lo + (v_hi - v_lo) * u1, v_lo), v_hi)
            if carry:
                b = int(best_index[k])
                best_loc, best_val = st.pbest_loc[slot, b].clone(), st.pbest[slot, b].clone()
                st.pbest_loc[slot] = torch.cat((best_loc.unsqueeze(0), fresh), 0)
                st.pbest[slot] = np.inf
                st.pbest[slot, 0] = best_val
            else:
                st.pbest_loc[slot] = fresh
                st.pbest[slot] = np.inf
            st.loc[slot] = st.pbest_loc[slot]
            st.vel[slot] = vel
            queries[k * P:(k + 1) * P, 0] = st.loc[slot] + xv
        return queries

    def pso_select(self, st, loss, rows):
        n, P, _ = st.loc.shape
        rows = [int(r) for r in rows]
        check_rows(n, P, 1, rows)
        loss = loss.reshape(len(rows), P)
        improved = torch.zeros(len(rows), P, dtype=torch.uint8)
        g_rows, argmin, gbest_from = [], [], []
        for k, slot in enumerate(rows):
            imp = loss[k] < st.pbest[slot]
            st.pbest[slot] = torch.where(imp, loss[k], st.pbest[slot])
            improved[k] = imp.to(torch.uint8)
            at = int(torch.argmin(st.pbest[slot]))
            upd = bool(st.pbest[slot, at] < st.gbest[slot])
            if upd:
                st.gbest[slot] = st.pbest[slot, at]
            g_rows.append(float(st.gbest[slot]))
            argmin.append(at)
            gbest_from.append(at if upd else -1)
        st.improved = improved.reshape(-1)
        return np.array(g_rows, np.float32), np.array(argmin, np.int32), np.array(gbest_from, np.int32)

    def pso_move(self, st, x, lower, upper, rows, gbest_from, cont, do_move, w, c1, c2, key, index_base=0, r1_in=None, r2_in=None):
        n, P, T = st.loc.shape
        rows = [int(r) for r in rows]
        check_rows(n, P, T, rows)
        if any(not -1 <= int(g) < P for g in gbest_from):
            raise ValueError("gbest_from")
        improved = st.improved.reshape(len(rows), P).bool()
        going = [k for k in range(len(rows)) if cont[k]] if do_move else []
        r1_in, r2_in = _f32(r1_in, (len(going), P, T)), _f32(r2_in, (len(going), P, T))
        queries = torch.empty(len(going) * P, 1, T, dtype=torch.float32) if going else None
        w, c1, c2 = (torch.tensor(v, dtype=torch.float32) for v in (w, c1, c2))  # the caller's doubles, rounded once
        for k, slot in enumerate(rows):
            st.pbest_loc[slot] = torch.where(improved[k].unsqueeze(1), st.loc[slot], st.pbest_loc[slot])
            if gbest_from[k] >= 0:
                st.gbest_loc[slot] = st.pbest_loc[slot, int(gbest_from[k])]
            if k not in going:
                continue
            q = going.index(k)
            u0, u1 = uniforms(key, index_base + slot, P, T)
            r1 = r1_in[q] if r1_in is not None else u0 + np.float32(1e-5)
            r2 = r2_in[q] if r2_in is not None else u1 + np.float32(1e-5)
            loc = st.loc[slot]
            vel = (w * st.vel[slot] + c1 * r1 * (st.pbest_loc[slot] - loc)) + c2 * r2 * (st.gbest_loc[slot].unsqueeze(0) - loc)
            loc = loc + vel
            loc = torch.min(torch.max(loc, lower[slot]), upper[slot])
            st.vel[slot], st.loc[slot] = vel, loc
            queries[q * P:(q + 1) * P, 0] = loc + x[slot, 0]
        return queries
