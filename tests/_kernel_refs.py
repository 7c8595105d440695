"""Plain torch float64 references of the encoder kernels, and the input generators of
tests/test_encoder_kernels_gpu.py.

Everything here is ordinary torch on whatever device its inputs live on, so the CPU suite
(tests/test_kernel_refs_cpu.py) checks the references against torch's own operators and the
generators against the conditions the GPU tests rely on, and the GPU tests run the very same
code next to the kernels.
"""
from __future__ import annotations

import math

import torch

# ---------------------------------------------------------------------------------------
# attention

ATT_B, ATT_H = 3, 3  # odd counts: head and batch offsets, a last workgroup with idle waves
ATT_LS = (1, 15, 16, 17, 31, 32, 33, 48, 49, 50, 63, 64, 65, 77, 130, 257, 512)
ATT_MASKS = ("none", "right", "left", "holes")
ATT_REGIMES = ("flat", "peaked", "ramp_up", "ramp_down")


def attention_mask(kind: str, B: int, L: int):
    """Key mask [B][L] int32 (1 = keep) or None.

    right: sequence lengths L, ceil(L / 2), 1 (then repeating) padded on the right.
    left:  pads 0, 5 L / 8 - 3, L / 8 on the left: whole leading 16-key blocks masked (skipped by
           the kernels) and one block partly masked; the pads sum to less than 3 L / 4, so with
           causal at most a quarter of the query rows are left without a key.
    holes: key k kept when k % 3 == b % min(3, L): every block is partly masked, and with causal
           the first b rows of sequence b have no key.
    """
    if kind == "none":
        return None
    m = torch.zeros(B, L, dtype=torch.int32)
    for b in range(B):
        if kind == "right":
            n = (L, (L + 1) // 2, 1)[b % 3]
            m[b, :n] = 1
        elif kind == "left":
            pad = (0, max(0, 5 * L // 8 - 3), L // 8)[b % 3]
            m[b, pad:] = 1
        elif kind == "holes":
            m[b, (b % min(3, L))::3] = 1
        else:
            raise ValueError(kind)
    return m


def attention_valid(mask, B: int, L: int, causal: bool, device=None):
    """valid[b][q][k]: key k takes part in query q's softmax."""
    dev = mask.device if mask is not None else device
    v = torch.ones(B, L, L, dtype=torch.bool, device=dev)
    if mask is not None:
        v &= (mask != 0)[:, None, :]
    if causal:
        v &= torch.ones(L, L, dtype=torch.bool, device=dev).tril()[None]
    return v


def attention_winners(valid, H: int):
    """winner[b][h][q]: the key planted as query q's best in the peaked regime: the
    ((7 q + h) % n_valid)-th of its valid keys (-1 where it has none)."""
    B, L, _ = valid.shape
    nv = valid.sum(-1)  # [B][L]
    rank = valid.cumsum(-1) - 1  # rank of key k among query q's valid keys
    q = torch.arange(L)[None, None, :]
    h = torch.arange(H)[None, :, None]
    want = (7 * q + h) % nv[:, None, :].clamp_min(1)  # [B][H][L]
    hit = valid[:, None] & (rank[:, None] == want[..., None])  # [B][H][L][L]
    w = hit.int().argmax(-1)
    return torch.where(nv[:, None, :] > 0, w, torch.full_like(w, -1))


def attention_inputs(regime: str, B: int, L: int, H: int, DH: int, mask, causal: bool, seed: int):
    """fp16 qkv [B*L][3*H*DH] (CPU). V rows are independent N(0, 1) draws in every regime, so a key
    weighted wrongly, or a wrong key, moves the output by O(1).

    flat:      q ~ 0.05 N, k ~ N: scores ~ 0.05, an almost uniform softmax.
    peaked:    q ~ 6 N, k ~ N scaled to the length sqrt(DH): scaled scores with a standard
               deviation of ~6; then each query is moved along its planted winner's key
               (attention_winners) just far enough that the winner leads every other valid key
               by >= 2 in the scaled score.
    ramp_up:   scaled score ~ 0.125 * key index (+ noise, slope varying ~ 10 % by query): the
               running maximum rises in every 16-key block (alpha ~ e^-2 each time).
    ramp_down: the same falling: the first block holds the maximum, later blocks add small terms.
    """
    g = torch.Generator().manual_seed(seed)
    scale = DH ** -0.5
    q = torch.randn(B, H, L, DH, generator=g, dtype=torch.float64)
    k = torch.randn(B, H, L, DH, generator=g, dtype=torch.float64)
    v = torch.randn(B, H, L, DH, generator=g, dtype=torch.float64)
    if regime == "flat":
        q *= 0.05
    elif regime == "peaked":
        q = (q * 6.0).half().double()
        # keys of one length (sqrt(DH): unit components), so no key is a longer copy of the
        # winner's direction and the move along the winner always overtakes it
        k = (k / k.norm(dim=-1, keepdim=True) * math.sqrt(DH)).half().double()
        valid = attention_valid(mask, B, L, causal)
        win = attention_winners(valid, H)  # [B][H][L]
        has = win >= 0
        wi = win.clamp_min(0)
        s = q @ k.transpose(-1, -2)  # unscaled [B][H][L][L]
        gram = k @ k.transpose(-1, -2)
        kw = torch.gather(k, 2, wi[..., None].expand(-1, -1, -1, DH))  # winner key of each query
        gw = torch.gather(gram, 2, wi[..., None].expand(-1, -1, -1, L))  # k_w . k_j
        nw = (kw * kw).sum(-1, keepdim=True)
        rho = gw / nw  # moving q by beta k_w / |k_w|^2 adds beta to the winner, beta rho_j to key j
        sw = torch.gather(s, 3, wi[..., None])
        others = valid[:, None] & (torch.arange(L)[None, None, None, :] != wi[..., None])
        margin = 3.0 / scale  # 3 in the scaled score; >= 2 is left after q is rounded to fp16
        need = (s - sw + margin) / (1.0 - rho).clamp_min(0.05)
        beta = torch.where(others, need, torch.zeros_like(need)).amax(-1, keepdim=True).clamp_min(0.0)
        q = torch.where(has[..., None], q + beta * kw / nw, q)
    elif regime in ("ramp_up", "ramp_down"):
        u = (torch.randint(0, 2, (DH,), generator=g).double() * 2 - 1) / math.sqrt(DH)
        t = torch.arange(L, dtype=torch.float64)
        if regime == "ramp_down":
            t = (L - 1) - t
        qa = 4.0
        ka = 0.125 / (qa * scale)
        q = 0.3 * q + qa * u
        k = 0.3 * k + ka * t[None, None, :, None] * u
    else:
        raise ValueError(regime)
    x = torch.stack([q, k, v], 0)  # [3][B][H][L][DH]
    return x.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H * DH).half().contiguous()


def attention_ref(qkv, B: int, L: int, H: int, DH: int, mask=None, causal: bool = False, scale=None):
    """float64 softmax(scale q k^T) v over the valid keys of the fp16 inputs.

    Returns (out [B*L][H*DH] f64 with zeros in rows without a valid key, empty [B][L] bool marking
    those rows, vmax [B][H*DH]: max |v| over the column's keys that pass the mask)."""
    scale = DH ** -0.5 if scale is None else scale
    x = qkv.double().view(B, L, 3, H, DH).permute(2, 0, 3, 1, 4)  # [3][B][H][L][DH]
    q, k, v = x[0], x[1], x[2]
    valid = attention_valid(mask, B, L, causal, qkv.device)[:, None]  # [B][1][L][L]
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~valid, -math.inf)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)  # exp(-inf) = 0 at masked keys
    den = e.sum(-1, keepdim=True)
    p = e / den.clamp_min(1e-300)
    out = (p @ v).permute(0, 2, 1, 3).reshape(B * L, H * DH)
    empty = ~valid.any(-1)[:, 0]  # [B][L]
    keep = torch.ones(B, L, dtype=torch.bool, device=qkv.device) if mask is None else mask != 0
    vmax = (v.abs() * keep[:, None, :, None]).amax(2).reshape(B, H * DH)
    return out, empty, vmax


# ---------------------------------------------------------------------------------------
# LayerNorm

LN_KINDS = ("randn", "small", "const", "shifted", "spike")
LN_WELL = (0, 1)  # kinds under the fixed f32 bound
LN_ILL = (3, 4)   # kinds under the measured bound


def layernorm_rows(rows: int, D: int, seed: int):
    """x [rows][D] f32 (CPU) and kind [rows]: row r is of kind LN_KINDS[(r + seed) % 5].

    const rows hold +-1.5 (alternating by row): every partial sum of up to 1024 copies is exact in
    f32, so the mean is the value itself, the variance 0, and the output beta exactly."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(rows, D, generator=g)
    kind = (torch.arange(rows) + seed) % len(LN_KINDS)
    x[kind == 1] *= 1e-3
    sign = torch.where(torch.arange(rows) % 2 == 0, 1.5, -1.5)
    x = torch.where((kind == 2)[:, None], sign[:, None].expand(rows, D), x)
    x[kind == 3] += 1000.0
    spike_at = torch.randint(0, D, (rows,), generator=g)
    sp = kind == 4
    x[sp, spike_at[sp]] = 1e4
    return x.contiguous(), kind


def layernorm_ref(x, gamma, beta, eps: float, gather=None):
    """float64 LayerNorm (biased variance) of rows x[gather[r]] (or x[r])."""
    xd = x.double()
    if gather is not None:
        xd = xd[gather.long()]
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def layernorm_well_bound(ref):
    """|y32 - ref| allowed on well-conditioned rows: 1e-5 (|ref| + max_row |ref|) — f32 two-pass
    over D <= 1024 (error ~ a few 2^-24 log2 D), with a 10x margin."""
    return 1e-5 * (ref.abs() + ref.abs().amax(-1, keepdim=True))


def gather_with_repeats(rows_out: int, rows_in: int, seed: int):
    """int32 gather [rows_out] into rows_in input rows: a permutation with repeats (every index in
    range, row 0 of the output never its own input unless rows_in == 1)."""
    g = torch.Generator().manual_seed(77 + seed)
    idx = torch.randint(0, rows_in, (rows_out,), generator=g, dtype=torch.int32)
    if rows_out > 1:
        idx[1] = idx[0]  # at least one repeat
    if rows_in > 1 and idx[0] == 0:
        idx[0] = rows_in - 1
    return idx


def vit_embed_ln_ref(patch, cls, pos, gamma, beta, B: int, T: int, D: int, eps: float):
    tok = torch.cat([cls.double().view(1, 1, D).expand(B, 1, D), patch.double().view(B, T - 1, D)], 1)
    return layernorm_ref((tok + pos.double().view(1, T, D)).view(B * T, D), gamma, beta, eps)


# ---------------------------------------------------------------------------------------
# im2col and the small ops

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def im2col_ref(img, B: int, S: int, P: int):
    """u8 [B][S][S][3] -> fp16 [B (S/P)^2][3 P P], K ordered (c, kh, kw); per pixel the
    CLIPImageProcessor arithmetic: u8 -> f64 * (1 / 255) -> f32, (x - mean) / std in f32, -> f16."""
    G = S // P
    x = (img.double() * (1.0 / 255.0)).float()
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32, device=img.device)
    std = torch.tensor(CLIP_STD, dtype=torch.float32, device=img.device)
    y = ((x - mean) / std).half()
    y = y.view(B, G, P, G, P, 3).permute(0, 1, 3, 5, 2, 4)  # b, py, px, c, kh, kw
    return y.reshape(B * G * G, 3 * P * P).contiguous()


def mean_pool_ref(X, mask, B: int, T: int, D: int):
    x = X.double().view(B, T, D)
    m = torch.ones(B, T, dtype=torch.float64, device=X.device) if mask is None else (mask != 0).double()
    return (x * m[:, :, None]).sum(1) / m.sum(1, keepdim=True).clamp_min(1e-9)


def eos_rows_ref(ids, eos_id: int):
    """rows[b] = b T + the first index of eos_id (0 when absent); eos_id < 0: the first argmax."""
    B, T = ids.shape
    out = []
    for b, row in enumerate(ids.tolist()):
        if eos_id >= 0:
            t = row.index(eos_id) if eos_id in row else 0
        else:
            t = row.index(max(row))
        out.append(b * T + t)
    return torch.tensor(out, dtype=torch.int32)


def token_embed_ref(ids, tok, pos, type_tab, types, vocab: int):
    """f32, in the kernel's order: (tok[clamp(id)] + pos[t]) + type_tab[types != 0]."""
    B, T = ids.shape
    x = tok[ids.long().clamp(0, vocab - 1)] + pos[:T][None]
    if type_tab is not None:
        ty = torch.zeros(B, T, dtype=torch.long, device=ids.device) if types is None else (types != 0).long()
        x = x + type_tab[ty]
    return x.view(B * T, -1)


def cls_head_ref(pooled, Wc, bc):
    """float64 logits and the magnitude sum |tanh| |W| + |b| their f32 error scales with."""
    t = torch.tanh(pooled.double())
    return t @ Wc.double().t() + bc.double(), t.abs() @ Wc.double().abs().t() + bc.double().abs()


# ---------------------------------------------------------------------------------------
# GEMM (K3 / K3s / K3d / K3w): C = epilogue(A W^T + bias)

GEMM_QUICK_GELU, GEMM_GELU_ERF, GEMM_RESIDUAL = 1, 2, 3  # epilogue 0: f16 out, 4: f32 out


def gemm_act_ref(x, epi: int):
    """float64 activation of epilogue `epi`: quick-GELU x sigmoid(1.702 x) (1), exact-erf GELU (2),
    the identity otherwise."""
    if epi == GEMM_QUICK_GELU:
        return x * torch.sigmoid(1.702 * x)
    if epi == GEMM_GELU_ERF:
        return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    return x


def gemm_ref(A, W, bias, epi: int, C0=None):
    """float64 reference of one GEMM launch on the inputs' device.

    Returns (ref, x, S): x = A W^T + bias, the pre-activation; ref = act(x) (+ C0 for epilogue 3);
    S = |A| |W|^T + |bias| (+ |C0|), the magnitude the f32 rounding error scales with."""
    Ad, Wd = A.double(), W.double()
    x = Ad @ Wd.t()
    S = Ad.abs() @ Wd.abs().t()
    if bias is not None:
        x = x + bias.double()
        S = S + bias.double().abs()
    ref = gemm_act_ref(x, epi)
    if epi == GEMM_RESIDUAL:
        ref = ref + C0.double()
        S = S + C0.double().abs()
    return ref, x, S


def gemm_int_operands(M: int, N: int, K: int, seed: int, device=None):
    """A [M][K], W [N][K] fp16 integers uniform in [-4, 4], bias [N] f32 integers in [-64, 64],
    C0 [M][N] f32 integers in [-1000, 1000].

    Every product is an integer of magnitude <= 16 and every partial sum, in any order, with the
    bias and C0, an integer of magnitude <= 16 K + 64 + 1000 (50,216 at K = 3072) < 2^24: the f32
    result is exact whatever the accumulation order, and, below 65504, the f16 result is the
    round-to-nearest-even fp16 of the exact integer."""
    g = torch.Generator(device=device or "cpu").manual_seed(seed)
    kw = dict(generator=g, device=device or "cpu")
    A = torch.randint(-4, 5, (M, K), **kw).half()
    W = torch.randint(-4, 5, (N, K), **kw).half()
    bias = torch.randint(-64, 65, (N,), **kw).float()
    C0 = torch.randint(-1000, 1001, (M, N), **kw).float()
    return A, W, bias, C0


GEMM_KINDS = ("plain", "cancel")


def gemm_real_operands(kind: str, M: int, N: int, K: int, seed: int, device=None):
    """fp16 A [M][K], W [N][K], f32 bias [N], f32 C0 [M][N] ~ N(0, 1).

    plain:  A ~ N(0, 1) with four columns scaled by 30 (the outlier features a LayerNorm output
            carries), W ~ 0.05 N, bias ~ 0.1 N.
    cancel: the second half of every W row is the negated first half, the second half of every A
            row the first half times (1 + 2^-9) (rounded to fp16): the two halves of every dot
            product cancel to ~2^-10 of their size, so |x| << S and an error that a max-norm
            comparison hides under the largest element is visible per element. bias ~ 0.01 N
            (the plain kind's 0.1 N would be the whole of x at K = 64)."""
    g = torch.Generator(device=device or "cpu").manual_seed(seed)
    kw = dict(generator=g, device=device or "cpu")
    A = torch.randn(M, K, **kw)
    W = torch.randn(N, K, **kw) * 0.05
    bias = torch.randn(N, **kw) * 0.1
    C0 = torch.randn(M, N, **kw)
    if kind == "plain":
        cols = torch.randperm(K, **kw)[:4]
        A[:, cols] *= 30.0
    elif kind == "cancel":
        h = K // 2
        W[:, h:] = -W[:, :h]
        A = A.half().float()
        A[:, h:] = A[:, :h] * (1.0 + 2.0 ** -9)
        bias = bias * 0.1
    else:
        raise ValueError(kind)
    return A.half().contiguous(), W.half().contiguous(), bias.contiguous(), C0.contiguous()


def gemm_acc_bound(S, K: int):
    """|acc - x| allowed for the f32 accumulator: (K + K / 32 + 2) 2^-23 S. The K products are exact
    in f32 (fp16 x fp16 has 22 significant bits); summing them, the K / 32 chunk results and the
    bias in any order rounds at most K + K / 32 + 1 times, each by at most one ulp (2^-23 relative,
    whatever the rounding mode) of a partial sum of magnitude <= S (1 + small)."""
    return (K + K / 32 + 2) * 2.0 ** -23 * S
