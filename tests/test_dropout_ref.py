"""The attention dropout's mask definition (include/x2g_staged.h, restated in tests/dropout_ref.py): its
statistics over 2^20 consecutive counters, the threshold's edge cases, the masked fp64 reference against the
plain one, the staged binding tables and the modules' constructor surface.  No GPU.

The mask is a deterministic function, so the statistical bounds either hold always or never: |z| <= 4 for the
overall keep rate and 4.5 for the worst of 16 heads (binomial, n = 2^20 and 2^16), neighbour correlations
<= 6e-3 (sigma = 1 / sqrt(n) ~ 1e-3) and, for two masks that differ only in step, salt or seed, agreement on
0.625 +- 0.003 of the positions at p = 0.25 (independence: 0.75^2 + 0.25^2)."""
import math

import numpy as np
import pytest
import torch

import attention_ref as ar
import dropout_ref as dr

H = 16
N = 1 << 20
T = N // H
TRIPLES = [(0, 0, 0), (1, 1, 0), (1, 2, 0), (1, 1, 1), (1, 1, 2), (1, 1, 3), (0x123456789ABCDEF, 7, 3),
           (2, 1 << 33, 0)]


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("seed,step,salt", TRIPLES)
def test_keep_rate_and_neighbour_correlations(seed, step, salt, p):
    keep = dr.keep_mask(seed, step, salt, T, H, p).astype(np.float64)
    sd = math.sqrt(p * (1 - p))
    z = (keep.mean() - (1 - p)) / (sd / math.sqrt(N))
    zh = (keep.mean(0) - (1 - p)) / (sd / math.sqrt(T))
    c = (keep - (1 - p)) / sd
    corr_t = float((c[1:] * c[:-1]).mean())        # neighbouring triplets, same head
    corr_h = float((c[:, 1:] * c[:, :-1]).mean())  # neighbouring heads, same triplet
    print(f"seed {seed} step {step} salt {salt} p {p}: z {z:.2f}, worst head z {np.abs(zh).max():.2f}, "
          f"corr triplets {corr_t:.2e} heads {corr_h:.2e}")
    assert abs(z) <= 4.0
    assert np.abs(zh).max() <= 4.5
    assert abs(corr_t) <= 6e-3 and abs(corr_h) <= 6e-3


def test_masks_of_different_step_salt_seed_are_independent():
    p = 0.25
    pairs = [((1, 1, 0), (1, 2, 0)),            # step
             ((1, 1, 0), (1, 1, 1)), ((1, 1, 1), (1, 1, 2)), ((1, 1, 2), (1, 1, 3)),  # salt
             ((0, 0, 0), (1, 0, 0)), ((1, 1, 0), (2, 1, 0)),  # seed
             ((2, 1 << 33, 0), (2, 0, 0)), ((1 << 32, 1, 0), (0, 1, 0))]  # the high words alone
    for a, b in pairs:
        agree = float((dr.keep_mask(*a, T, H, p) == dr.keep_mask(*b, T, H, p)).mean())
        print(a, b, f"agreement {agree:.4f}")
        assert 0.622 <= agree <= 0.628, (a, b, agree)


def test_threshold_edge_cases():
    assert dr.threshold(0.0) == 0
    assert dr.keep_mask(3, 4, 5, 64, H, 0.0).all()  # p = 0 keeps everything
    assert np.array_equal(dr.keep_scale(3, 4, 5, 64, H, 0.0), np.ones((64, H), np.float32))
    assert dr.threshold(1.0 - 2.0 ** -33) == 0xFFFFFFFF  # floor(2^32 - 0.5 + 0.5) = 2^32 clamps
    assert dr.threshold(0.5) == 1 << 31
    assert dr.threshold(float(np.float32(0.1))) == int(math.floor(float(np.float32(0.1)) * 2.0 ** 32 + 0.5))
    r = dr.keep_scale(1, 1, 0, 256, H, 0.5)
    assert set(np.unique(r)) == {np.float32(0.0), np.float32(2.0)}
    # the mix finaliser on known words: a bijection with mix(0) = 0
    assert int(dr.mix(np.uint64(0))) == 0 and len(set(int(v) for v in dr.mix(np.arange(4096)))) == 4096


def test_masked_reference_equals_the_plain_one_at_r_1():
    """attention_dropout_ref writes every gradient out; with r = 1 it is attention_ref.attention_ref (autograd)
    to 1e-14 of each output's scale, with S given and with lin_sbf, without and with an edge term."""
    ei, n = ar.edge_case_graph(6)
    from oracle import triplets

    trip = triplets.vertex_to_edge(ei, n)[0]
    E, Tn, Hh, C = ei.shape[1], trip.shape[1], 4, 8
    x = ar.make_inputs("unit", E, Tn, Hh * C, 5)
    sbf = torch.randn(Tn, 42, generator=torch.Generator().manual_seed(1))
    W, b = x["W"][: Hh * C], x["b"][: Hh * C]
    ones = np.ones((Tn, Hh), np.float32)
    for e_t in (None, x["e_trip"]):
        for S, lin in ((x["S"], None), (None, (sbf, W, b))):
            args = (x["q"], x["k"], x["v"], x["skip"], S, trip[0], trip[1], Hh, C)
            want = ar.attention_ref(*args, e_t=e_t, dout=x["dout"], lin=lin)
            got = dr.attention_dropout_ref(*args, ones, e_t=e_t, dout=x["dout"], lin=lin)
            assert sorted(got) == sorted(want)
            for name, w in want.items():
                if w is None:
                    assert got[name] is None
                    continue
                fin = torch.isfinite(w)
                assert torch.equal(got[name][~fin], w[~fin])
                err = float((got[name][fin] - w[fin]).abs().max()) / float(w[fin].abs().max())
                assert err <= 1e-14, (name, err)


def test_mask_enters_the_reference_where_the_arithmetic_puts_it():
    """A dropped (triplet, head) contributes nothing to out, dv and dS and its g is zero; the softmax (prob,
    seg_den) is the undropped one."""
    ei, n = ar.edge_case_graph(6)
    from oracle import triplets

    trip = triplets.vertex_to_edge(ei, n)[0]
    E, Tn, Hh, C = ei.shape[1], trip.shape[1], 4, 8
    x = ar.make_inputs("unit", E, Tn, Hh * C, 6)
    r = dr.keep_scale(9, 1, 0, Tn, Hh, 0.5)
    assert (r == 0).any() and (r > 0).any()
    args = (x["q"], x["k"], x["v"], x["skip"], x["S"], trip[0], trip[1], Hh, C)
    plain = ar.attention_ref(*args, dout=x["dout"])
    got = dr.attention_dropout_ref(*args, r, dout=x["dout"])
    for name in ("logits", "seg_max", "seg_den", "prob"):
        assert torch.equal(got[name], plain[name]), name
    drop = torch.from_numpy(r == 0)
    assert float(got["g"][drop].abs().max()) == 0.0
    assert float(got["dS"].view(Tn, Hh, C)[drop].abs().max()) == 0.0
    rt = torch.from_numpy(r).double()
    assert torch.allclose(got["g"], plain["g"] * rt, rtol=0, atol=1e-12)
    assert torch.allclose(got["dS"].view(Tn, Hh, C), plain["dS"].view(Tn, Hh, C) * rt[:, :, None] , rtol=1e-12, atol=1e-12)


STAGED = ["x2g_attn_dropout_mask", "x2g_sbf_attention_bwd_center_drop", "x2g_sbf_attention_fwd_center_sf_drop",
          "x2g_sbf_attention_fwd_center_sf_tiled_drop"]


def test_staged_tables_hold_the_four_entries_and_the_abi_tables_none():
    import ctypes

    from x2gnn import _lib

    assert sorted(_lib.STAGED_SIGNATURES) == sorted(_lib.STAGED_RESTYPES) == STAGED
    assert not set(STAGED) & set(_lib.SIGNATURES) and not set(STAGED) & set(_lib.RESTYPES)
    tail = [ctypes.c_float, ctypes.c_void_p, ctypes.c_uint32]
    for name in STAGED[1:]:  # the parent's arguments, then drop_p, drop_key, salt
        assert _lib.STAGED_SIGNATURES[name] == _lib.SIGNATURES[name[:-len("_drop")]] + tail, name
        assert _lib.STAGED_RESTYPES[name] is ctypes.c_int
    assert _lib.STAGED_SIGNATURES["x2g_attn_dropout_mask"] == [ctypes.c_int64, ctypes.c_int, ctypes.c_float,
                                                              ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                                              ctypes.c_void_p]


def test_conv_refuses_a_dropout_outside_0_1():
    from x2gnn.sbftransformer_conv import SBFTransformerConv

    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError):
            SBFTransformerConv(128, 8, heads=16, sbf_dim=42, rbf_dim=6, dropout=bad, edge_dim=128)
    assert SBFTransformerConv(128, 8, heads=16, sbf_dim=42, rbf_dim=6, dropout=0.3, edge_dim=128).dropout == 0.3


@pytest.mark.parametrize("kind", ["xgnn_poly", "xgnn_poly_global"])
def test_state_dict_keys_do_not_depend_on_attn_dropout(kind):
    import x2gnn

    cfg = dict(conv_layers=2, sbf_dim=7, rbf_dim=6, in_channels=128, heads=16, embedding_size=128)
    make = getattr(x2gnn, kind)
    torch.manual_seed(0)
    plain = make(**cfg)
    torch.manual_seed(0)
    zero = make(attn_dropout=0.0, **cfg)
    torch.manual_seed(0)
    drop = make(attn_dropout=0.2, dropout_seed=5, **cfg)
    keys = list(plain.state_dict())
    assert list(zero.state_dict()) == keys and list(drop.state_dict()) == keys
    assert not any("dropout" in k for k in keys)
    assert [n for n, _ in drop.named_modules()] == [n for n, _ in plain.named_modules()]
    for a, b in zip(plain.state_dict().values(), drop.state_dict().values()):
        assert torch.equal(a, b)  # the same draws: the dropout arguments consume no random numbers
    st = drop.fin_model.attn_dropout_state
    assert st.dtype == torch.int64 and st.tolist() == [5, 0]
    assert all(c.dropout == 0.2 for c in drop.fin_model.convs) and all(c.dropout == 0 for c in zero.fin_model.convs)
