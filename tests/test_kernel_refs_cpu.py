"""The float64 references and input generators of tests/_kernel_refs.py, checked without a GPU:
each reference against torch's own operator in float64 at the GPU tests' shapes (so a wrong
reference cannot be blamed on a kernel), the generators against the conditions the GPU tests
state for them, and the argument checks of the building-block entries that return before any
HIP call."""
from __future__ import annotations

import math

import torch

import _kernel_refs as R


def _cases(Ls=R.ATT_LS):
    for L in Ls:
        for kind in R.ATT_MASKS:
            for causal in (False, True):
                yield L, kind, causal


def test_attention_ref_matches_sdpa():
    """attention_ref == torch scaled_dot_product_attention in float64 on every row that has a key,
    zeros on the others; vmax is the column maximum over the unmasked keys."""
    B, H = R.ATT_B, R.ATT_H
    for L, kind, causal in _cases((1, 15, 17, 33, 50, 64, 65, 130)):
        for DH in (32, 64):
            mask = R.attention_mask(kind, B, L)
            qkv = R.attention_inputs("peaked" if L % 2 else "flat", B, L, H, DH, mask, causal, seed=L)
            out, empty, vmax = R.attention_ref(qkv, B, L, H, DH, mask, causal)
            x = qkv.double().view(B, L, 3, H, DH).permute(2, 0, 3, 1, 4)
            valid = R.attention_valid(mask, B, L, causal)[:, None]
            sd = torch.nn.functional.scaled_dot_product_attention(x[0], x[1], x[2], attn_mask=valid)
            sd = sd.permute(0, 2, 1, 3).reshape(B * L, H * DH)
            rows = ~empty.reshape(-1)
            assert torch.equal(empty, ~valid.any(-1)[:, 0])
            torch.testing.assert_close(out[rows], sd[rows], rtol=1e-12, atol=1e-12)
            assert bool((out[~rows] == 0).all())
            v = x[2].abs()  # [B][H][L][DH]
            keep = torch.ones(B, L, dtype=torch.bool) if mask is None else mask != 0
            for b in range(B):
                assert torch.equal(vmax[b], v[b][:, keep[b]].amax(1).reshape(-1))


def test_attention_masks_and_empty_rows():
    """Rows without a valid key exist only under causal plus a left / holes mask, and are at most a
    quarter of a case's rows; the left mask skips whole leading blocks and cuts one block, the
    right mask has the lengths L, ceil(L / 2), 1; holes keep every third key."""
    B = R.ATT_B
    for L, kind, causal in _cases():
        mask = R.attention_mask(kind, B, L)
        empty = ~R.attention_valid(mask, B, L, causal).any(-1)
        if not (causal and kind in ("left", "holes")):
            assert not bool(empty.any()), (L, kind, causal)
        assert int(empty.sum()) * 4 <= B * L, (L, kind, causal, int(empty.sum()))
        if mask is not None:
            assert bool((mask.sum(1) >= 1).all())
        if kind == "right":
            assert mask.sum(1).tolist() == [L, (L + 1) // 2, 1]
            assert all(bool((mask[b, :int(mask[b].sum())] == 1).all()) for b in range(B))
        if kind == "left":
            pads = (L - mask.sum(1)).tolist()
            assert all(bool((mask[b, pads[b]:] == 1).all()) for b in range(B))
            if L >= 33:
                assert max(pads) >= 16  # a fully masked (skipped) leading block
                assert any(p % 16 for p in pads)  # and a partly masked one
        if kind == "holes":
            for b in range(B):
                assert mask[b].nonzero().flatten().tolist() == list(range(b % min(3, L), L, 3))
    # causal + left / holes does leave rows without a key somewhere (the zero-row path runs)
    assert bool((~R.attention_valid(R.attention_mask("left", B, 64), B, 64, True).any(-1)).any())
    assert bool((~R.attention_valid(R.attention_mask("holes", B, 64), B, 64, True).any(-1)).any())


def test_attention_regimes():
    """flat: |scores| small; peaked: the planted winner is each query's best key by >= 2 and the
    spread of the scores is >= 6; ramps: the block maxima rise (fall) monotonically, so the
    running maximum changes in every block of the rising ramp."""
    B, H = R.ATT_B, R.ATT_H
    for DH in (32, 64):
        scale = DH ** -0.5
        for L, kind, causal in _cases((1, 16, 17, 33, 49, 64, 77, 130, 512)):
            if L == 512 and (kind not in ("none", "left") or DH == 64):
                continue  # (keeps this test quick; the generator's code does not depend on L)
            mask = R.attention_mask(kind, B, L)
            valid = R.attention_valid(mask, B, L, causal)[:, None]
            win = R.attention_winners(valid[:, 0], H)

            def scores(regime):
                qkv = R.attention_inputs(regime, B, L, H, DH, mask, causal, seed=3 * L + DH)
                x = qkv.double().view(B, L, 3, H, DH).permute(2, 0, 3, 1, 4)
                assert float(x[2].std()) > 0.9 if L > 1 else True  # V ~ N(0, 1)
                return (x[0] @ x[1].transpose(-1, -2)) * scale

            s = scores("flat")
            assert float(s.abs().max()) < 1.5
            s = scores("peaked").masked_fill(~valid, -math.inf)
            has = win >= 0
            assert torch.equal(has, valid.any(-1).expand(B, H, L))
            top = s.argmax(-1)
            assert torch.equal(top[has], win[has]), (L, kind, causal, DH)
            if L > 1:
                top2 = s.topk(2, -1).values
                gap = (top2[..., 0] - top2[..., 1])[has & (valid.sum(-1) > 1).expand(B, H, L)]
                assert gap.numel() == 0 or float(gap.min()) >= 2.0, (L, kind, causal, DH, float(gap.min()))
            if L >= 64 and kind == "none" and not causal:
                assert float(s.std()) >= 6.0
                if math.gcd(7, L) == 1:  # every key (every slot of every block) wins for some query
                    for b in range(B):
                        for h in range(H):
                            assert sorted(win[b, h].tolist()) == list(range(L))
            if L >= 33 and kind == "none" and not causal:
                for regime, sign in (("ramp_up", 1.0), ("ramp_down", -1.0)):
                    s = scores(regime)
                    nb = L // 16
                    bm = s[..., :16 * nb].reshape(B, H, L, nb, 16).amax(-1)  # per-block maxima
                    d = (bm[..., 1:] - bm[..., :-1]) * sign
                    assert float(d.min()) > 0.5, (regime, L, DH, float(d.min()))  # alpha < e^-0.5 per block


def test_layernorm_ref_matches_torch():
    for D in (1, 3, 4, 63, 252, 384, 1023, 1024):
        for rows in (1, 5, 23):
            x, kind = R.layernorm_rows(rows, D, seed=D + rows)
            g = torch.Generator().manual_seed(D)
            gamma = torch.randn(D, generator=g)
            beta = torch.randn(D, generator=g)
            for gather in (None, R.gather_with_repeats(rows + 2, rows, D)):
                ref = R.layernorm_ref(x, gamma, beta, 1e-5, gather)
                xd = x.double() if gather is None else x.double()[gather.long()]
                exp = torch.nn.functional.layer_norm(xd, (D,), gamma.double(), beta.double(), 1e-5)
                # (the shifted rows amplify float64 rounding by |mean| / std ~ 1e3)
                torch.testing.assert_close(ref, exp, rtol=1e-9, atol=1e-9)
                k = kind if gather is None else kind[gather.long()]
                const = k == 2
                if bool(const.any()):  # variance 0: beta exactly, in float64 as in f32
                    assert torch.equal(ref[const], beta.double().expand(int(const.sum()), D))


def test_layernorm_rows_kinds():
    x, kind = R.layernorm_rows(20, 256, seed=1)
    assert sorted(set(kind.tolist())) == [0, 1, 2, 3, 4]
    assert bool((x[kind == 2].abs() == 1.5).all()) and float(x[kind == 2].var(1).max()) == 0.0
    # f32 partial sums of the constant rows are exact: the f32 mean is the value itself
    c = x[kind == 2]
    assert torch.equal(c.cumsum(1)[:, -1] / 256, c[:, 0])
    assert 0.5e-3 < float(x[kind == 1].std()) < 2e-3
    assert 990 < float(x[kind == 3].mean()) < 1010
    assert bool(((x[kind == 4] == 1e4).sum(1) == 1).all())
    gi = R.gather_with_repeats(9, 5, 0)
    assert gi.dtype == torch.int32 and int(gi.min()) >= 0 and int(gi.max()) < 5
    assert len(set(gi.tolist())) < 9 and gi.tolist() != list(range(9))


def test_vit_embed_ln_ref():
    B, T, D = 3, 5, 8
    g = torch.Generator().manual_seed(0)
    patch, cls, pos = torch.randn(B * (T - 1), D, generator=g), torch.randn(D, generator=g), torch.randn(T, D, generator=g)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = R.vit_embed_ln_ref(patch, cls, pos, gamma, beta, B, T, D, 1e-5)
    for b in range(B):
        for t in range(T):
            e = (cls if t == 0 else patch[b * (T - 1) + t - 1]).double() + pos[t].double()
            exp = torch.nn.functional.layer_norm(e, (D,), gamma.double(), beta.double(), 1e-5)
            torch.testing.assert_close(ref[b * T + t], exp, rtol=1e-12, atol=1e-12)


def test_im2col_ref_is_the_conv_unfold():
    """Layout against torch's unfold (K ordered c, kh, kw) and the per-pixel formula against a
    scalar evaluation of every byte value."""
    for B, S, P in ((3, 64, 32), (3, 64, 16), (3, 24, 8)):
        g = torch.Generator().manual_seed(S + P)
        img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
        img[0, 0, 0, 0], img[0, 0, 0, 1] = 0, 255
        ref = R.im2col_ref(img, B, S, P)
        x = (img.double() * (1.0 / 255.0)).float()
        n = (x - torch.tensor(R.CLIP_MEAN)) / torch.tensor(R.CLIP_STD)
        unf = torch.nn.functional.unfold(n.permute(0, 3, 1, 2), kernel_size=P, stride=P)  # [B][3PP][G*G]
        exp = unf.transpose(1, 2).reshape(-1, 3 * P * P).half()
        assert torch.equal(ref.view(torch.int16), exp.view(torch.int16))
    import numpy as np

    v = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()
    ref = R.im2col_ref(v, 1, 16, 16).view(3, 256)
    for c in range(3):
        x = (np.arange(256).astype(np.float64) * (1.0 / 255.0)).astype(np.float32)
        e = ((x - np.float32(R.CLIP_MEAN[c])) / np.float32(R.CLIP_STD[c])).astype(np.float16)
        assert np.array_equal(ref[c].numpy(), e)


def test_small_op_refs():
    g = torch.Generator().manual_seed(4)
    X = torch.randn(4, 7, 12, generator=g)
    mask = torch.tensor([[1] * 7, [1, 1, 1, 0, 0, 0, 0], [0] * 7, [0, 5, 0, 1, 0, 0, 1]], dtype=torch.int32)
    mp = R.mean_pool_ref(X, mask, 4, 7, 12)
    torch.testing.assert_close(mp[0], X[0].double().mean(0))
    torch.testing.assert_close(mp[1], X[1, :3].double().mean(0))
    assert bool((mp[2] == 0).all())
    torch.testing.assert_close(mp[3], X[3, [1, 3, 6]].double().mean(0))
    torch.testing.assert_close(R.mean_pool_ref(X, None, 4, 7, 12), X.double().mean(1))

    ids = torch.tensor([[9, 1, 2, 3], [1, 2, 3, 9], [1, 9, 9, 2], [1, 2, 3, 4], [7, 7, 3, 7]], dtype=torch.int32)
    assert R.eos_rows_ref(ids, 9).tolist() == [0, 7, 9, 12, 16]
    assert R.eos_rows_ref(ids, -1).tolist() == [0, 7, 9, 15, 16]

    vocab, T, D = 10, 4, 8
    tok, pos, tt = torch.randn(vocab, D, generator=g), torch.randn(6, D, generator=g), torch.randn(2, D, generator=g)
    idq = torch.tensor([[-5, 0, 9, vocab + 3]], dtype=torch.int32)
    types = torch.tensor([[0, 1, 7, 0]], dtype=torch.int32)
    te = R.token_embed_ref(idq, tok, pos, tt, types, vocab)
    assert torch.equal(te[0], (tok[0] + pos[0]) + tt[0]) and torch.equal(te[3], (tok[9] + pos[3]) + tt[0])
    assert torch.equal(te[1], (tok[0] + pos[1]) + tt[1]) and torch.equal(te[2], (tok[9] + pos[2]) + tt[1])
    assert torch.equal(R.token_embed_ref(idq, tok, pos, tt, None, vocab)[2], (tok[9] + pos[2]) + tt[0])
    assert torch.equal(R.token_embed_ref(idq, tok, pos, None, None, vocab)[2], tok[9] + pos[2])

    pooled, Wc, bc = torch.randn(3, 63, generator=g), torch.randn(2, 63, generator=g), torch.randn(2, generator=g)
    logits, mag = R.cls_head_ref(pooled, Wc, bc)
    exp = torch.nn.functional.linear(torch.tanh(pooled.double()), Wc.double(), bc.double())
    torch.testing.assert_close(logits, exp, rtol=1e-12, atol=1e-12)
    assert bool((mag >= logits.abs() - 1e-12).all())


def test_gemm_ref_matches_torch():
    """gemm_ref == torch's linear / gelu / x sigmoid(1.702 x) in float64; S bounds |x|."""
    for kind in R.GEMM_KINDS:
        A, W, bias, C0 = R.gemm_real_operands(kind, 37, 128, 192, seed=3)
        for b in (bias, None):
            lin = torch.nn.functional.linear(A.double(), W.double(), b.double() if b is not None else None)
            for epi in range(5):
                ref, x, S = R.gemm_ref(A, W, b, epi, C0)
                torch.testing.assert_close(x, lin, rtol=1e-12, atol=1e-12)
                exp = {1: lin * torch.sigmoid(1.702 * lin), 2: torch.nn.functional.gelu(lin),
                       3: lin + C0.double()}.get(epi, lin)
                torch.testing.assert_close(ref, exp, rtol=1e-12, atol=1e-12)
                mag = A.double().abs() @ W.double().abs().t() + (b.double().abs() if b is not None else 0.0)
                torch.testing.assert_close(S, mag + (C0.double().abs() if epi == 3 else 0.0), rtol=1e-12, atol=1e-12)
                assert bool((S >= x.abs() - 1e-12).all())


def test_gemm_int_operands_are_exact():
    """The integer generator at the largest K any GEMM test uses (3072): every partial sum below
    2^24 (f32 exact in any order), the result below the fp16 maximum, and the fp16 rounding of
    integers up to 2048 the identity."""
    A, W, bias, C0 = R.gemm_int_operands(65, 128, 3072, seed=1)
    for t, lo, hi in ((A, -4, 4), (W, -4, 4), (bias, -64, 64), (C0, -1000, 1000)):
        assert float(t.min()) >= lo and float(t.max()) <= hi and bool((t.double() == t.double().round()).all())
    assert A.dtype == torch.float16 and W.dtype == torch.float16 and bias.dtype == torch.float32
    assert sorted(set(A.flatten().tolist())) == [float(v) for v in range(-4, 5)]
    for epi in (0, 3, 4):
        ref, x, S = R.gemm_ref(A, W, bias, epi, C0)
        assert float(S.max()) < 2 ** 24
        assert float(x.abs().max()) < 65504
        assert bool((ref == ref.round()).all())
        small = ref.abs() <= 2048
        assert bool(small.any()) and torch.equal(ref.half().double()[small], ref[small])
        assert torch.equal(ref.float().double(), ref)
    assert 16 * 3072 + 64 + 1000 < 2 ** 24


def test_gemm_cancel_operands_cancel():
    """cancel: the median |x| / S is below 1e-2 at every K the GPU tests use (plain: it is not)."""
    for K in (64, 192, 384, 512, 704, 768):
        A, W, bias, C0 = R.gemm_real_operands("cancel", 64, 128, K, seed=K)
        _, x, S = R.gemm_ref(A, W, bias, 4)
        assert float((x.abs() / S).median()) < 1e-2, K
        h = K // 2
        assert torch.equal(W[:, h:], -W[:, :h])
        A, W, bias, C0 = R.gemm_real_operands("plain", 64, 128, K, seed=K)
        _, x, S = R.gemm_ref(A, W, bias, 4)
        assert float((x.abs() / S).median()) > 3e-2, K
        assert int((A.float().abs().amax(0) > 40).sum()) == 4  # the four outlier columns


def test_gemm_activation_slopes():
    """|d act / dx| < 1.13 for both activations on [-20, 20] (the factor on the accumulation bound
    of epilogues 1 and 2 in tests/test_gemm_kernels_gpu.py)."""
    x = torch.linspace(-20, 20, 4_000_001, dtype=torch.float64)
    for epi in (1, 2):
        y = R.gemm_act_ref(x, epi)
        slope = ((y[1:] - y[:-1]) / (x[1:] - x[:-1])).abs()
        assert 1.0 < float(slope.max()) < 1.13, (epi, float(slope.max()))
    b = R.gemm_acc_bound(torch.tensor(1.0, dtype=torch.float64), 64)
    assert float(b) == (64 + 2 + 2) * 2.0 ** -23


def test_building_block_argument_checks():
    """The rejections that need no GPU: they return MRAG_ERR_ARG before any HIP call (the pointers
    are never dereferenced on the host)."""
    from app.encoders import _register_signatures

    ERR_ARG = 1  # MRAG_ERR_ARG (include/mrag.h)

    lib = _register_signatures()
    p = 4096  # an aligned non-NULL address
    # in place through a gather: a race between rows, whatever the kernel
    assert lib.mrag_layernorm(p, p + 65536, p, None, p, p, 8, 64, 64, 1e-5, None) == ERR_ARG
    assert b"gather" in lib.mrag_last_error()
    # in place with padded input rows: output row r would land inside input row r - 1
    assert lib.mrag_layernorm(p, None, p, None, p, p, 8, 64, 72, 1e-5, None) == ERR_ARG
    assert lib.mrag_layernorm(None, None, p, None, p, p, 8, 64, 64, 1e-5, None) == ERR_ARG
    assert lib.mrag_layernorm(p, None, None, None, p, p, 8, 64, 64, 1e-5, None) == ERR_ARG
    assert lib.mrag_layernorm(p, None, p, None, p, p, 8, 1028, 1028, 1e-5, None) == ERR_ARG
    # the seq64 attention kernel outside 33 <= L <= 64, an unknown kernel, an unsupported head
    for L in (1, 32, 65, 512):
        assert lib.mrag_attention(p, p, None, 2, L, 2, 64, 0, 0.125, 2, None) == ERR_ARG
        assert b"seq64" in lib.mrag_last_error()
    assert lib.mrag_attention(p, p, None, 2, 40, 2, 64, 0, 0.125, 3, None) == ERR_ARG
    assert lib.mrag_attention(p, p, None, 2, 40, 2, 48, 0, 0.125, 0, None) == ERR_ARG
    assert lib.mrag_attention(p, p, None, 2, 513, 2, 64, 0, 0.125, 0, None) == ERR_ARG
    assert lib.mrag_attention(None, p, None, 2, 40, 2, 64, 0, 0.125, 0, None) == ERR_ARG
    assert lib.mrag_gather_rows(p, p, p, 3, 24, None) == ERR_ARG
    assert b"16" in lib.mrag_last_error()
    assert lib.mrag_vit_im2col(p, p, 1, 64, 12, None) == ERR_ARG
    assert lib.mrag_vit_embed_ln(p, p, p, p, p, p, 1, 2, 6, 1e-5, None) == ERR_ARG
    assert lib.mrag_token_embed(p, p, p, None, None, p, 1, 2, 6, 10, None) == ERR_ARG

    # ---- GEMM: kernel ids as app.encoders.GEMM_KERNELS
    AUTO, K3, K3D, K3S, K3W = range(5)

    def gemm(M, N, K, epi=0, kernel=AUTO, A=p, W=p, bias=p, C=p):
        return lib.mrag_gemm_nt_kernel(A, W, bias, C, M, N, K, epi, kernel, None)

    def gemm_ld(M, N, K, lda, ldc, epi=0, kernel=AUTO):
        return lib.mrag_gemm_nt_ld(p, lda, p, p, p, ldc, M, N, K, epi, kernel, None)

    # K3d keeps 32-bit source offsets: (M - 1) * lda + K > INT_MAX is rejected when it is forced (the
    # ViT fc2 / patch-embedding K at ~14,000 images), one row less passes this check (and fails later,
    # at the launch, on a machine without a GPU: not called here)
    assert (699_051 - 1) * 3072 + 3072 > 2 ** 31 - 1 >= (699_050 - 1) * 3072 + 3072
    assert gemm(699_051, 256, 3072, kernel=K3D) == ERR_ARG
    assert b"offset" in lib.mrag_last_error()
    assert gemm_ld(1100, 256, 64, 1_999_992, 256, kernel=K3D) == ERR_ARG  # the same through lda
    assert b"offset" in lib.mrag_last_error()
    # shape rules of every kernel
    assert gemm(128, 192, 64) == ERR_ARG and gemm(128, 128, 96) == ERR_ARG
    assert lib.mrag_gemm_nt(p, p, p, p, 128, 192, 64, 0, None) == ERR_ARG
    assert gemm(128, 128, 64, bias=p + 8) == ERR_ARG and b"aligned" in lib.mrag_last_error()
    assert gemm(128, 128, 64, C=p + 8) == ERR_ARG and b"aligned" in lib.mrag_last_error()
    assert gemm(128, 128, 64, A=None) == ERR_ARG and gemm(128, 128, 64, kernel=5) == ERR_ARG
    assert gemm(128, 128, 64, epi=5, kernel=K3W) == ERR_ARG
    for shape in ((1023, 256, 64), (1024, 384, 64), (1024, 4352, 64)):
        assert gemm(*shape, kernel=K3D) == ERR_ARG and b"K3d" in lib.mrag_last_error(), shape
    assert gemm(65, 128, 64, kernel=K3S) == ERR_ARG and b"K3s" in lib.mrag_last_error()
    for shape, epi in (((4096, 256, 512), 4), ((4096, 256, 512), 3), ((4096, 256, 256), 0), ((4095, 256, 512), 0),
                       ((4096, 128, 512), 0)):
        assert gemm(*shape, epi=epi, kernel=K3W) == ERR_ARG and b"K3w" in lib.mrag_last_error(), (shape, epi)
    # explicit strides: at least a row, and the vector widths of the loads / stores
    assert gemm_ld(128, 128, 64, 56, 128) == ERR_ARG and b"lda" in lib.mrag_last_error()
    assert gemm_ld(128, 128, 64, 64, 124) == ERR_ARG and b"ldc" in lib.mrag_last_error()
    assert gemm_ld(128, 128, 64, 68, 128) == ERR_ARG and gemm_ld(128, 128, 64, 64, 130) == ERR_ARG
    assert gemm_ld(128, 128, 64, 64, 128, kernel=7) == ERR_ARG
