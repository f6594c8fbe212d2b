"""A plain statement of the SBF-transformer attention (include/x2g.h, x2g_sbf_attention_fwd) in torch on
the CPU, float64 by default: the truth the HIP attention kernels are compared with.

    kk_t = k[src] + e_t,  u_t = v[src] + e_t,  l_t,h = <q[dst]_h, kk_t,h> / sqrt(C),
    a = softmax over the triplets of a destination: exp(l - max) / (sum exp(l - max) + 1e-16),
    out[d] = sum_{t into d} u_t * S_t * a_t,h + skip[d]

as oracle/ref_cpu.py:SBFTransformerConv.forward states it (scatter-max shift, exp, /(sum + 1e-16)).  The
gradients come from torch.autograd; everything the kernels call by another name (g, rho, the folded lin_sbf
gradient G, the per-destination / per-atom / per-table-row edge gradients, the P rows) is a plain index sum
over them.  Nothing here is shared with x2gnn beyond index arrays.

The segment maximum is taken as a constant of the backward (the softmax does not depend on the shift
except through the 1e-16, which moves a gradient by less than 1e-16 of itself).
"""
import math

import torch

SOFTMAX_EPS = 1e-16


def _idx(t):
    return torch.as_tensor(t).long().cpu()


def project(sbf, w, b):
    """S = sbf W^T + b (lin_sbf)."""
    return sbf @ w.t() + b


def sbf_from_factors(radial, y, trip_src, nsph=7):
    """sbf[t, R l + n] = radial[src(t), R l + n] * Y_l(t): [T, nsph * R] from radial [E, nsph * R], y [T, >= nsph]."""
    T = y.shape[0]
    r = radial.index_select(0, _idx(trip_src)).view(T, nsph, -1)
    return (r * y[:, :nsph, None]).reshape(T, -1)


def p_rows(w, radial, nsph=7):
    """P[s, l, c] = sum_n W[c, R l + n] radial[s, R l + n]: [E, nsph, D]."""
    D, E = w.shape[0], radial.shape[0]
    return torch.einsum("cln,sln->slc", w.view(D, nsph, -1), radial.view(E, nsph, -1))


def s_from_p(p, b, y, trip_src):
    """S_t = b + sum_l Y_l(t) P_src(t)[l]."""
    nsph = p.shape[1]
    return b + (p.index_select(0, _idx(trip_src)) * y[:, :nsph, None]).sum(1)


def attention_ref(q, k, v, skip, S, trip_src, trip_dst, heads, channels, e_t=None, dout=None,
                  dtype=torch.float64, lin=None):
    """The operation in ``dtype`` on the CPU.  ``e_t`` [T, HC] or None; ``S`` [T, HC], or None with
    ``lin`` = (sbf [T, K], W [HC, K], b [HC]): then S = lin_sbf(sbf) = sbf W^T + b.

    Returns a dict: out, logits [T, H], seg_max [E, H] (-inf without triplets), seg_den [E, H] (no epsilon),
    prob [T, H], row_stats [E, 2], S; with ``dout`` also dq, dk, dv, dskip, dS, de_t, dlogit, g [T, H] =
    sum_c dout (v[src] + e) S, seg_rho [E, H] = sum_t a_t g_t (and dW, db with ``lin``)."""
    H, C = int(heads), int(channels)
    src, dst = _idx(trip_src), _idx(trip_dst)
    want = dout is not None

    def leaf(t):
        t = torch.as_tensor(t).detach().cpu().to(dtype).clone()
        return t.requires_grad_(True) if want else t

    q, k, v, skip = leaf(q), leaf(k), leaf(v), leaf(skip)
    E, T, D = q.shape[0], src.shape[0], H * C
    e = leaf(e_t) if e_t is not None else None
    w = b = None
    if S is None:
        w, b = leaf(lin[1]), leaf(lin[2])
        S = project(torch.as_tensor(lin[0]).detach().cpu().to(dtype), w, b)
        if want:
            S.retain_grad()
    else:
        S = leaf(S)
    kk = k.index_select(0, src)
    u = v.index_select(0, src)
    if e is not None:
        kk, u = kk + e, u + e
    logits = (q.index_select(0, dst).view(T, H, C) * kk.view(T, H, C)).sum(-1) / math.sqrt(C)
    if want:
        logits.retain_grad()
    seg_max = torch.full((E, H), -math.inf, dtype=dtype)
    seg_max = seg_max.scatter_reduce(0, dst[:, None].expand(T, H), logits.detach(), reduce="amax", include_self=True)
    ex = (logits - seg_max.index_select(0, dst)).exp()
    seg_den = torch.zeros(E, H, dtype=dtype).index_add(0, dst, ex)
    prob = ex / (seg_den.index_select(0, dst) + SOFTMAX_EPS)
    msg = u.view(T, H, C) * S.view(T, H, C) * prob[:, :, None]
    out = torch.zeros(E, D, dtype=dtype).index_add(0, dst, msg.reshape(T, D)) + skip
    mean = out.mean(1, keepdim=True)
    row_stats = torch.cat([mean, ((out - mean) ** 2).sum(1, keepdim=True)], 1)
    r = dict(out=out, logits=logits, seg_max=seg_max, seg_den=seg_den, prob=prob, row_stats=row_stats, S=S)
    if want:
        d = torch.as_tensor(dout).detach().cpu().to(dtype)
        out.backward(d)
        g = (d.index_select(0, dst).view(T, H, C) * u.view(T, H, C) * S.view(T, H, C)).sum(-1)
        r.update(dq=q.grad, dk=k.grad, dv=v.grad, dskip=skip.grad, dS=S.grad, dlogit=logits.grad, g=g,
                 seg_rho=torch.zeros(E, H, dtype=dtype).index_add(0, dst, prob * g),
                 de_t=e.grad if e is not None else None)
        if w is not None:
            r.update(dW=w.grad, db=b.grad)
    return {n: (t.detach() if t is not None else None) for n, t in r.items()}


def symmetric_edges(pairs):
    """edge_index [2, E] int64, (src, dst)-sorted, with both directions of every pair."""
    import numpy as np

    ed = sorted({(a, b) for a, b in pairs} | {(b, a) for a, b in pairs})
    return np.array(ed, dtype=np.int64).T


def edge_case_graph(hub=40):
    """(edge_index, num_atoms): a path a-b-c, an atom without edges in the middle of the index range (3) and
    one at the end, a star whose hub (atom 4) has ``hub`` neighbours, a triangle, a 6-atom chain."""
    t = 5 + hub
    pairs = [(0, 1), (1, 2)] + [(4, 5 + i) for i in range(hub)] + [(t, t + 1), (t + 1, t + 2), (t, t + 2)] + \
        [(t + 3 + i, t + 4 + i) for i in range(5)]
    return symmetric_edges(pairs), t + 10


REGIMES = ("unit", "peaked", "offset")


def make_inputs(regime, E, T, D, seed, table_rows=10):
    """Seeded fp32 host inputs of one case, every tensor drawn in a fixed order whatever the case uses:
    q, k, v, skip, dout [E, D]; S, e_trip [T, D]; table [rows, D]; radial [E, 42]; y [T, 8] (y[:, 7] = 1);
    W [D, 42], b [D].  ``unit``: randn.  ``peaked``: q and k scaled by 5.5 (|logit| reaches 130-190).
    ``offset``: every k row = one random row + 0.05 randn, q = 40 randn, the edge terms scaled by 0.05 (the
    logits of a (destination, head) lie within a few units of a common value of either sign up to ~200)."""
    g = torch.Generator().manual_seed(int(seed))

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float32)

    d = dict(q=rn(E, D), k=rn(E, D), v=rn(E, D), skip=rn(E, D), dout=rn(E, D), S=rn(T, D), e_trip=rn(T, D),
             table=rn(table_rows, D), radial=rn(E, 42), y=rn(T, 8), W=0.2 * rn(D, 42), b=0.1 * rn(D))
    row = rn(1, D)
    d["y"][:, 7] = 1.0
    if regime == "peaked":
        d["q"], d["k"] = 5.5 * d["q"], 5.5 * d["k"]
    elif regime == "offset":
        d["k"] = row + 0.05 * d["k"]
        d["q"] = 40.0 * d["q"]
        d["e_trip"], d["table"] = 0.05 * d["e_trip"], 0.05 * d["table"]
    elif regime != "unit":
        raise ValueError(regime)
    return {n: t.contiguous() for n, t in d.items()}


def rows_sum(x, key, rows):
    """out[r] = sum of the rows x[i] with key[i] == r."""
    return torch.zeros((int(rows),) + tuple(x.shape[1:]), dtype=x.dtype).index_add(0, _idx(key), x)


def fold_g(dS, y, trip_src, num_edges, nsph=7):
    """G [E, nsph + 1, HC]: G[s, l] = sum_{t: src = s} dS[t] Y_l(t) for l < nsph, G[s, nsph] = sum dS[t]."""
    yy = torch.cat([y[:, :nsph].to(dS.dtype), torch.ones(y.shape[0], 1, dtype=dS.dtype)], 1)
    return rows_sum(dS[:, None, :] * yy[:, :, None], trip_src, num_edges)


def wgrad_from_g(G, radial):
    """(dW [HC, R nsph], db [HC]) = (sum_s radial[s, R l + n] G[s, l, c], sum_s G[s, nsph, c])."""
    E, n1, D = G.shape
    dw = torch.einsum("sln,slc->cln", radial.to(G.dtype).view(E, n1 - 1, -1), G[:, :n1 - 1]).reshape(D, -1)
    return dw, G[:, n1 - 1].sum(0)
