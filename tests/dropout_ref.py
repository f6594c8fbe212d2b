"""The attention dropout's mask (include/x2g_staged.h) restated in numpy uint32, and the SBF-transformer
attention with that mask in torch on the CPU, float64 by default: the truth the dropout kernels are compared
with.  No tests in here.

    out_d    = sum_t a_t r_t u_t S_t + skip_d
    g_t      = r_t sum_c dout_d u_t S_t,   rho_d = sum_t a_t g_t,   dlogit_t = a_t (g_t - rho_d)
    dv_s    += a_t r_t dout_d S_t,         dS_t = a_t r_t dout_d u_t

with a_t the softmax weight of attention_ref.attention_ref (the mask enters neither the maximum nor the
denominator), u_t = v[src] + e_t.  The forward and every gradient are written out (no autograd), each from the
lines above; with r = 1 everywhere the result is attention_ref.attention_ref's.
"""
import math

import numpy as np
import torch

from attention_ref import SOFTMAX_EPS, _idx, project

M32 = np.uint64(0xFFFFFFFF)


def mix(x):
    """The 32-bit finaliser on a uint32 array (arithmetic in uint64, masked: no overflow warnings)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def keys(seed, step, salt):
    """(k0, k1) of int64 words ``seed``, ``step`` (their bits read as uint64) and the uint32 ``salt``."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    u = lambda v: np.uint64(v & 0xFFFFFFFF)  # noqa: E731
    k0 = mix(u(seed) ^ mix(u(step) ^ u((int(salt) & 0xFFFFFFFF) * 0x9E3779B9)))
    k1 = mix((u(seed >> 32) + mix(u(step >> 32) ^ k0)) & M32)
    return k0, k1


def bits(seed, step, salt, T, H):
    """bits(t, h) [T, H] as uint64 holding uint32 values."""
    k0, k1 = keys(seed, step, salt)
    c = (np.arange(int(T) * int(H), dtype=np.uint64) & M32).reshape(int(T), int(H))
    return mix((mix(c ^ k0) + k1) & M32)


def threshold(p):
    """thr = min(floor(p 2^32 + 0.5), 2^32 - 1), formed in double."""
    return min(int(math.floor(float(p) * 4294967296.0 + 0.5)), 0xFFFFFFFF)


def keep_mask(seed, step, salt, T, H, p):
    """keep [T, H] bool."""
    return bits(seed, step, salt, T, H) >= np.uint64(threshold(p))


def keep_scale(seed, step, salt, T, H, p):
    """r [T, H] float32: keep ? (float)(1 / (1 - (double)p)) : 0.  ``p`` is taken as the double it is: to match
    an entry point, pass the float32 value it receives (``float(np.float32(p))``)."""
    scale = np.float32(1.0 / (1.0 - float(p)))
    return np.where(keep_mask(seed, step, salt, T, H, p), scale, np.float32(0.0)).astype(np.float32)


def attention_dropout_ref(q, k, v, skip, S, trip_src, trip_dst, heads, channels, r, e_t=None, dout=None,
                          dtype=torch.float64, lin=None):
    """attention_ref.attention_ref with the keep scale ``r`` [T, H] on the softmax weights; the same dict
    (out, logits, seg_max, seg_den, prob — the weights BEFORE dropout —, row_stats, S; with ``dout`` dq, dk, dv,
    dskip, dS, de_t, dlogit, g, seg_rho, and dW, db with ``lin``)."""
    H, C = int(heads), int(channels)
    src, dst = _idx(trip_src), _idx(trip_dst)

    def t_(x):
        return torch.as_tensor(x).detach().cpu().to(dtype)

    q, k, v, skip = t_(q), t_(k), t_(v), t_(skip)
    E, T, D = q.shape[0], src.shape[0], H * C
    e = t_(e_t) if e_t is not None else None
    r = t_(r).view(T, H)
    w = b = sbf = None
    if S is None:
        sbf, w, b = t_(lin[0]), t_(lin[1]), t_(lin[2])
        S = project(sbf, w, b)
    else:
        S = t_(S)
    qd = q.index_select(0, dst).view(T, H, C)
    kk = k.index_select(0, src)
    u = v.index_select(0, src)
    if e is not None:
        kk, u = kk + e, u + e
    kk, u, Sv = kk.view(T, H, C), u.view(T, H, C), S.view(T, H, C)
    logits = (qd * kk).sum(-1) / math.sqrt(C)
    seg_max = torch.full((E, H), -math.inf, dtype=dtype)
    seg_max = seg_max.scatter_reduce(0, dst[:, None].expand(T, H), logits, reduce="amax", include_self=True)
    ex = (logits - seg_max.index_select(0, dst)).exp()
    seg_den = torch.zeros(E, H, dtype=dtype).index_add(0, dst, ex)
    prob = ex / (seg_den.index_select(0, dst) + SOFTMAX_EPS)
    ar_ = prob * r  # a_t r_t
    msg = u * Sv * ar_[:, :, None]
    out = torch.zeros(E, D, dtype=dtype).index_add(0, dst, msg.reshape(T, D)) + skip
    mean = out.mean(1, keepdim=True)
    row_stats = torch.cat([mean, ((out - mean) ** 2).sum(1, keepdim=True)], 1)
    res = dict(out=out, logits=logits, seg_max=seg_max, seg_den=seg_den, prob=prob, row_stats=row_stats, S=S)
    if dout is not None:
        d = t_(dout)
        dd = d.index_select(0, dst).view(T, H, C)
        g = r * (dd * u * Sv).sum(-1)
        rho = torch.zeros(E, H, dtype=dtype).index_add(0, dst, prob * g)
        dlogit = prob * (g - rho.index_select(0, dst))
        wl = dlogit[:, :, None] / math.sqrt(C)
        dq = torch.zeros(E, D, dtype=dtype).index_add(0, dst, (wl * kk).reshape(T, D))
        dkk = (wl * qd).reshape(T, D)  # d / d (k[src] + e)
        du = (ar_[:, :, None] * dd * Sv).reshape(T, D)  # d / d (v[src] + e)
        dS = (ar_[:, :, None] * dd * u).reshape(T, D)
        res.update(dq=dq, dk=torch.zeros(E, D, dtype=dtype).index_add(0, src, dkk),
                   dv=torch.zeros(E, D, dtype=dtype).index_add(0, src, du), dskip=d.clone(), dS=dS, dlogit=dlogit,
                   g=g, seg_rho=rho, de_t=(dkk + du) if e is not None else None)
        if w is not None:
            res.update(dW=dS.t() @ sbf, db=dS.sum(0))
    return res
