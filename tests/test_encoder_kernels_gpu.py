"""The encoder kernels other than the GEMMs, one launch at a time through the building-block
entries of the C ABI (mrag_attention, mrag_layernorm, ...), each against a plain float64
reference of the same operation (tests/_kernel_refs.py, itself checked on the CPU by
tests/test_kernel_refs_cpu.py) at the shapes, masks and value ranges where such kernels go
wrong. The towers reach these kernels only at their own shapes, on synthetic weights (flat
softmax), through a 1e-4 cosine after 6-12 layers. The GEMM kernels have the same kind of tests
in tests/test_gemm_kernels_gpu.py.

Every launch is tiny; the references run in float64 on the GPU next to the kernels.
"""
from __future__ import annotations

import functools

import pytest
import torch

import _kernel_refs as R
from conftest import record_numerics

pytestmark = pytest.mark.gpu

# ---- attention -----------------------------------------------------------------------------
# |out - ref| <= ATT_TOL * vmax, vmax = max |v| over the (sequence, head, dim) column's unmasked
# keys. From the code: P is rounded to fp16 before the PV MFMA (<= 2^-11 relative per term, and
# the terms' weights sum to 1), the output is rounded to fp16 (<= 2^-11 |out| <= 2^-11 vmax); the
# f32 score / exp / accumulation errors are orders below. Derived: 2 * 2^-11; asserted: twice that.
ATT_TOL = 2.0 ** -9  # observed on MI355X: 5.5e-4 (0.28 of the bound), over all 1088 cases
# ---- LayerNorm -----------------------------------------------------------------------------
# well-conditioned rows (randn, 1e-3 randn): R.layernorm_well_bound, 1e-5 (|ref| + max |ref|);
#   observed 0.051 of it (y32). The fp16 output adds 2^-11 |ref|, its own rounding: observed 0.95
#   of the sum (a half-ulp rounding error reaches its bound; the f32 part is the 0.051 above).
# constant rows: beta exactly.
# ill-conditioned rows (1000 + randn, a 1e4 spike): LN_ILL_FACTOR x the maximum error of torch's own
#   float32 layer_norm on 1023 rows of the same kind, D, gamma and beta (another summation order on
#   the same f32 arithmetic), never below the well-conditioned bound; observed 1.8 x torch's error.
# scalar against vector kernel on the same rows (D = 384): observed 0.011 of the well-conditioned
#   bound, 32 of 67 rows bit-identical. vit_embed_ln: observed 0.014 of the well-conditioned bound.
LN_ILL_FACTOR = 4.0
F16_EPS = 2.0 ** -11
LN_EPS = 1e-5
# ---- small ops -----------------------------------------------------------------------------
# mean_pool: relative to the mean |x| over the kept tokens, the magnitude the sum runs over (relative
# to the result itself is meaningless for a zero-mean sum); a sequential f32 sum over T <= 256 is
# within (T - 1) 2^-24 ~ 1.5e-5 of it in the worst case and ~ 2^-24 sqrt(T) typically.
MEAN_POOL_REL = 1e-6  # observed 1.4e-7
CLS_HEAD_REL = 1e-5   # of sum |tanh| |W| + |b|; observed 4.8e-8
# (every observed figure above is recorded by record_numerics and printed in the numerics section)

def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


@functools.lru_cache(maxsize=None)
def _att_inputs(regime, L, DH, kind, causal):
    mask = R.attention_mask(kind, R.ATT_B, L)
    seed = 16 * L + DH // 32 + 4 * R.ATT_REGIMES.index(regime)
    return R.attention_inputs(regime, R.ATT_B, L, R.ATT_H, DH, mask, causal, seed)


def _att_case(regime, L, DH, kind, causal):
    # only the peaked regime's inputs depend on the mask and the causal flag
    if regime != "peaked":
        kind, causal = "none", False
    return _att_inputs(regime, L, DH, kind, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("DH", [32, 64])
def test_attention_against_float64(cuda, DH, causal):
    """Both attention kernels against float64 softmax(scale q k^T) v of the same fp16 inputs:
    B = H = 3, every L across the 16-key blocks and the 32 / 64 kernel thresholds up to 512,
    no mask / right padding / left padding (leading blocks skipped) / holes, flat, peaked (every
    key slot wins for some query) and ramped scores (the running maximum moves in every block).
    Rows without a valid key are exact zeros; no NaN of the pre-fill survives; qkv is untouched;
    a repeated launch, and for 33 <= L <= 64 the flash16 and seq64 kernels, give the same bytes."""
    from app.encoders import attention

    B, H = R.ATT_B, R.ATT_H
    worst = (-1.0, None)
    for L in R.ATT_LS:
        labels, ratios, flags, keep_for_record = [], [], [], []
        for kind in R.ATT_MASKS:
            mask = R.attention_mask(kind, B, L)
            mask_d = mask.to(cuda) if mask is not None else None
            for regime in R.ATT_REGIMES:
                qkv = _att_case(regime, L, DH, kind, causal).to(cuda)
                before = qkv.clone()
                ref, empty, vmax = R.attention_ref(qkv, B, L, H, DH, mask_d, causal)
                outs = {}
                for name in ("auto", "auto2") + (("flash16", "seq64") if 33 <= L <= 64 else ()):
                    out = _nan((B * L, H * DH), torch.float16, cuda)
                    attention(qkv, out, B, L, H, DH, mask=mask_d, causal=causal, kernel=name.rstrip("2"))
                    outs[name] = out
                out = outs["auto"]
                e = empty.reshape(-1)
                err = (out.double() - ref).abs() / vmax[:, None, :].expand(B, L, H * DH).reshape(B * L, H * DH)
                err = torch.where(e[:, None], torch.zeros_like(err), err)
                same = torch.equal(outs["auto"].view(torch.int16), outs["auto2"].view(torch.int16))
                if "seq64" in outs:
                    same = same and torch.equal(outs["flash16"].view(torch.int16), outs["seq64"].view(torch.int16))
                    same = same and torch.equal(outs["auto"].view(torch.int16), outs["seq64"].view(torch.int16))
                labels.append((L, kind, regime))
                ratios.append(torch.nan_to_num(err, nan=float("inf")).max())
                flags.append(torch.stack([torch.isnan(out).any(), (out[e] != 0).any(),
                                          (qkv.view(torch.int16) != before.view(torch.int16)).any(),
                                          torch.tensor(not same, device=cuda)]))
                keep_for_record.append((out, ref, e))
        ratios_h = torch.stack(ratios).cpu().tolist()
        flags_h = torch.stack(flags).cpu().tolist()
        for lab, r, f, rec in zip(labels, ratios_h, flags_h, keep_for_record):
            print("attention", DH, causal, lab, "max |out - ref| / vmax = %.3g" % r)
            assert not f[0], ("NaN left in out", DH, causal, lab)
            assert not f[1], ("row without a key is not zero", DH, causal, lab)
            assert not f[2], ("qkv modified", DH, causal, lab)
            assert not f[3], ("launches / kernels differ in bytes", DH, causal, lab)
            assert r <= ATT_TOL, ("|out - ref| > 2^-9 vmax", DH, causal, lab, r)
            if r > worst[0]:
                worst = (r, lab, rec)
    r, lab, (out, ref, e) = worst
    record_numerics(f"attention_dh{DH}_causal{int(causal)}", out[~e].double().cpu().numpy(), ref[~e].cpu().numpy(),
                    unit=False, max_err_over_vmax=r, bound=ATT_TOL, worst_case=str(lab))


# ---- LayerNorm ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ln_params(D, dev):
    """gamma, beta of every case at this D, and torch's own f32 layer_norm error on 1023 rows of
    each ill-conditioned kind (the measured part of their bound)."""
    g = torch.Generator().manual_seed(5000 + D)
    gamma = torch.randn(D, generator=g).to(dev)
    beta = torch.randn(D, generator=g).to(dev)
    x, kind = R.layernorm_rows(1023, D, seed=D)
    x, kind = x.to(dev), kind.to(dev)
    ref = R.layernorm_ref(x, gamma, beta, LN_EPS)
    t32 = torch.nn.functional.layer_norm(x, (D,), gamma, beta, LN_EPS)
    err = (t32.double() - ref).abs().amax(1)
    torch_err = {k: float(err[kind == k].max()) for k in R.LN_ILL}
    return gamma, beta, torch_err


class _LnStats:
    def __init__(self):
        self.well32 = self.well16 = self.ill = 0.0

    def record(self, name):
        record_numerics(name, [], [], max_well_err_over_bound_y32=self.well32,
                        max_well_err_over_bound_y16=self.well16, max_ill_err_over_torch_f32_err=self.ill,
                        ill_allowed=LN_ILL_FACTOR)


def _ln_check(y32, y16, ref, kind, D, stats, label):
    """The bounds of the module header on one launch's outputs (kind: the kind of each output row)."""
    gamma, beta, torch_err = _ln_params(D, ref.device)
    well = R.layernorm_well_bound(ref)
    terr = torch.zeros(ref.shape[0], dtype=torch.float64, device=ref.device)
    for k in R.LN_ILL:
        terr = torch.where(kind == k, torch.full_like(terr, torch_err[k]), terr)
    bound = torch.maximum(well, LN_ILL_FACTOR * terr[:, None])
    const = kind == 2
    illrow = (kind == 3) | (kind == 4)
    wellrow = (kind == 0) | (kind == 1)
    for y, extra, exact, which in ((y32, 0.0, beta, "y32"), (y16, F16_EPS, beta.half(), "y16")):
        if y is None:
            continue
        assert not bool(torch.isnan(y).any()), ("NaN left", which, label)
        err = (y.double() - ref).abs()
        b = bound + extra * ref.abs()
        over = (err / b)[~const]
        assert over.numel() == 0 or float(over.max()) <= 1.0, (which, label, float(over.max()))
        if bool(const.any()):  # variance 0: beta exactly
            assert torch.equal(y[const], exact.expand(int(const.sum()), D)), ("constant row != beta", which, label)
        if bool(wellrow.any()):
            w = float((err / (well + extra * ref.abs()))[wellrow].max())
            if which == "y32":
                stats.well32 = max(stats.well32, w)
            else:
                stats.well16 = max(stats.well16, w)
        if which == "y32" and bool(illrow.any()):
            stats.ill = max(stats.ill, float((err.amax(1) / terr.clamp_min(1e-30))[illrow].max()))


def _ln_launch(xbase, rows, D, ldx, gather, combo, cuda, inplace=False):
    """One launch reading from xbase.data_ptr(); returns (y32, y16) as [rows][D] (None when absent)."""
    from app.encoders import layernorm

    gamma, beta, _ = _ln_params(D, cuda)
    y32 = y16 = None
    if inplace:
        y32 = xbase
    elif combo in ("y32", "both"):
        y32 = _nan((rows * D,), torch.float32, cuda)
    if combo in ("y16", "both"):
        y16 = _nan((rows * D,), torch.float16, cuda)
    layernorm(xbase, gamma, beta, rows, D, ldx=ldx, gather=gather, y32=y32, y16=y16, eps=LN_EPS)
    return (y32[:rows * D].view(rows, D) if y32 is not None else None,
            y16.view(rows, D) if y16 is not None else None)


def _ln_strided(x, ldx, cuda, offset=0):
    """x [rows][D] laid out with row stride ldx from a base `offset` floats into a fresh buffer (NaN
    in the padding: a kernel that reads past a row's D floats poisons its output)."""
    rows, D = x.shape
    buf = _nan((rows * ldx + offset + 4,), torch.float32, cuda)
    base = buf[offset:]
    base[:rows * ldx].view(rows, ldx)[:, :D] = x
    return base


def _ln_all(x, kind, D, ldx, cuda, stats, label, offset=0, inplace_too=True):
    """Every output combination, plain / through a gather / in place, of one input."""
    rows = x.shape[0]
    gamma, beta, _ = _ln_params(D, cuda)
    ref = R.layernorm_ref(x, gamma, beta, LN_EPS)
    gi = R.gather_with_repeats(rows, rows, D + rows).to(cuda)
    gref, gkind = ref[gi.long()], kind[gi.long()]
    base = _ln_strided(x, ldx, cuda, offset)
    for combo in ("y32", "y16", "both"):
        y32, y16 = _ln_launch(base, rows, D, ldx, None, combo, cuda)
        _ln_check(y32, y16, ref, kind, D, stats, (label, combo))
        y32, y16 = _ln_launch(base, rows, D, ldx, gi, combo, cuda)
        _ln_check(y32, y16, gref, gkind, D, stats, (label, combo, "gather"))
        if inplace_too and ldx == D and combo != "y16":
            xin = _ln_strided(x, ldx, cuda, offset)
            y32, y16 = _ln_launch(xin, rows, D, ldx, None, combo, cuda, inplace=True)
            _ln_check(y32, y16, ref, kind, D, stats, (label, combo, "in place"))


def test_layernorm_vector_paths(cuda):
    """layernorm_stream_kernel<false> and <true> (gather): D from one float4 to 1024, one row to
    1023 (a ragged last workgroup), dense and padded input rows, in place, every output
    combination, all five row kinds."""
    stats = _LnStats()
    for D in (4, 8, 252, 256, 260, 384, 512, 768, 1020, 1024):
        for rows in (1, 3, 4, 5, 1023):
            x, kind = R.layernorm_rows(rows, D, seed=D // 4 + rows)
            x, kind = x.to(cuda), kind.to(cuda)
            for ldx in (D, D + 8):
                _ln_all(x, kind, D, ldx, cuda, stats, ("vec", D, rows, ldx))
    stats.record("layernorm_vector")


def test_layernorm_stream_walks_rows(cuda):
    """More rows than the persistent grid has waves (4 waves x 4 workgroups per CU): every wave
    walks three rows (r += nw) and the prefetch of the row after its last one clamps to the last
    row of the matrix."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    rows, D = 4 * 4 * cus * 2 + 7, 64
    stats = _LnStats()
    x, kind = R.layernorm_rows(rows, D, seed=3)
    _ln_all(x.to(cuda), kind.to(cuda), D, D, cuda, stats, ("walk", D, rows))
    stats.record("layernorm_stream_walk")


def test_layernorm_scalar_path(cuda):
    """layernorm_kernel (D % 4 != 0, or an unaligned base / row stride), with and without a gather;
    and at D = 384, where misaligning only x sends the same rows down the scalar path, the scalar
    and the vector outputs against each other (recorded, held to the well-conditioned bound)."""
    stats = _LnStats()
    for D in (1, 3, 63, 65, 383, 1023):
        for rows in (1, 5, 67):
            x, kind = R.layernorm_rows(rows, D, seed=D + rows)
            _ln_all(x.to(cuda), kind.to(cuda), D, D, cuda, stats, ("scalar", D, rows))
    D, rows = 384, 67
    x, kind = R.layernorm_rows(rows, D, seed=9)
    x, kind = x.to(cuda), kind.to(cuda)
    _ln_all(x, kind, D, D + 1, cuda, stats, ("scalar unaligned", D, rows, D + 1), offset=1)
    _ln_all(x, kind, D, D, cuda, stats, ("scalar offset base", D, rows, D), offset=1)
    stats.record("layernorm_scalar")
    # the same rows through both kernels
    gamma, beta, _ = _ln_params(D, cuda)
    ref = R.layernorm_ref(x, gamma, beta, LN_EPS)
    ys, _ = _ln_launch(_ln_strided(x, D, cuda, 1), rows, D, D, None, "y32", cuda)
    yv, _ = _ln_launch(_ln_strided(x, D, cuda, 0), rows, D, D, None, "y32", cuda)
    wellrow = (kind == 0) | (kind == 1)
    diff = (ys.double() - yv.double()).abs()
    over = float((diff / R.layernorm_well_bound(ref))[wellrow].max())
    record_numerics("layernorm_scalar_vs_vector_d384", ys.cpu().numpy(), yv.cpu().numpy(), unit=False,
                    max_well_diff_over_bound=over, bit_identical_rows=int((diff.amax(1) == 0).sum()))
    assert over <= 1.0, over


def test_vit_embed_ln(cuda):
    """X = LN(concat(cls, patch) + pos) against float64, under the well-conditioned bound."""
    from app.encoders import vit_embed_ln

    worst = 0.0
    for T in (2, 5, 50):
        for D in (8, 384, 768, 1024):
            B = 3
            g = torch.Generator().manual_seed(T * D)
            patch = torch.randn(B * (T - 1), D, generator=g).to(cuda)
            cls, pos = torch.randn(D, generator=g).to(cuda), torch.randn(T, D, generator=g).to(cuda)
            gamma, beta = torch.randn(D, generator=g).to(cuda), torch.randn(D, generator=g).to(cuda)
            X = _nan((B * T, D), torch.float32, cuda)
            vit_embed_ln(patch, cls, pos, gamma, beta, X, B, T, D, eps=LN_EPS)
            ref = R.vit_embed_ln_ref(patch, cls, pos, gamma, beta, B, T, D, LN_EPS)
            assert not bool(torch.isnan(X).any()), (T, D)
            over = float(((X.double() - ref).abs() / R.layernorm_well_bound(ref)).max())
            assert over <= 1.0, (T, D, over)
            worst = max(worst, over)
    record_numerics("vit_embed_ln", [], [], max_err_over_bound=worst)


# ---- im2col --------------------------------------------------------------------------------

def test_vit_im2col_bit_exact(cuda):
    """Both im2col kernels against the formula reference, bit for bit: P = 32 on an aligned base
    (vit_im2col32_kernel), the same bytes one byte further (the generic kernel), P = 16 and 8."""
    from app.encoders import vit_im2col

    B = 3
    by_base = {}
    for S, P, offset in ((64, 32, 0), (64, 32, 1), (64, 16, 0), (24, 8, 0), (24, 8, 1)):
        g = torch.Generator().manual_seed(S + P)
        img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
        img.view(-1)[:4] = torch.tensor([0, 255, 255, 0], dtype=torch.uint8)
        assert int(img.min()) == 0 and int(img.max()) == 255
        n = img.numel()
        buf = torch.zeros(n + 32, dtype=torch.uint8, device=cuda)
        assert buf.data_ptr() % 16 == 0
        base = buf[offset:offset + n]
        base.copy_(img.view(-1))
        G = S // P
        out = _nan((B * G * G, 3 * P * P), torch.float16, cuda)
        vit_im2col(base, out, B, S, P)
        ref = R.im2col_ref(img.to(cuda), B, S, P)
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (S, P, offset)
        by_base[(S, P, offset)] = out
    assert torch.equal(by_base[(64, 32, 0)].view(torch.int16), by_base[(64, 32, 1)].view(torch.int16))


# ---- small ops -----------------------------------------------------------------------------

def test_mean_pool(cuda):
    """Masked mean over T: no mask, a ragged mask (with holes), one sequence all masked (exactly 0)."""
    from app.encoders import mean_pool

    B, worst = 4, 0.0
    for T in (1, 7, 256):
        for D in (4, 384):
            g = torch.Generator().manual_seed(T + D)
            X = torch.randn(B, T, D, generator=g).to(cuda)
            ragged = torch.zeros(B, T, dtype=torch.int32)
            for b, n in enumerate((T, (T + 1) // 2, 1, max(1, T - 1))):
                ragged[b, :n] = 1
            if T > 2:
                ragged[0, 1] = 0  # a hole
                ragged[3, T - 1] = 5  # any non-zero value keeps the token
            zero_row = ragged.clone()
            zero_row[1] = 0
            for name, mask in (("none", None), ("ragged", ragged), ("zero row", zero_row)):
                md = mask.to(cuda) if mask is not None else None
                out = _nan((B, D), torch.float32, cuda)
                mean_pool(X, out, B, T, D, mask=md)
                ref = R.mean_pool_ref(X, md, B, T, D)
                m = torch.ones(B, T, device=cuda, dtype=torch.float64) if md is None else (md != 0).double()
                mag = (X.double().abs() * m[:, :, None]).sum(1) / m.sum(1, keepdim=True).clamp_min(1)
                assert not bool(torch.isnan(out).any()), (T, D, name)
                if name == "zero row":
                    assert bool((out[1] == 0).all()), (T, D)
                err = (out.double() - ref).abs()
                assert bool((err <= MEAN_POOL_REL * mag).all()), (T, D, name, float((err / mag.clamp_min(1e-30)).max()))
                live = mag > 0
                worst = max(worst, float((err[live] / mag[live]).max()) / MEAN_POOL_REL)
    record_numerics("mean_pool", [], [], max_err_over_bound=worst)


def test_eos_rows(cuda):
    """First EOS (first, last, repeated, absent -> row b T) and the legacy argmax (ties to the first
    index), B = 130: more than two 64-thread groups, the last one ragged."""
    from app.encoders import eos_rows

    B, T, eos = 130, 9, 60
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1, 50, (B, T), generator=g, dtype=torch.int32)
    for b in range(B):
        if b % 4 == 0:
            ids[b, 0] = eos
        elif b % 4 == 1:
            ids[b, T - 1] = eos
        elif b % 4 == 2:
            ids[b, 3] = ids[b, 6] = eos
    ref = R.eos_rows_ref(ids, eos)
    assert ref[:4].tolist() == [0, T + T - 1, 2 * T + 3, 3 * T]
    rows = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    eos_rows(ids.to(cuda), rows, B, T, eos)
    assert torch.equal(rows.cpu(), ref)
    # argmax: a unique maximum anywhere, a tie (the first wins), the maximum first, all equal
    am = torch.randint(1, 50, (B, T), generator=g, dtype=torch.int32)
    for b in range(B):
        if b % 4 == 0:
            am[b, b % T] = 1000
        elif b % 4 == 1:
            am[b, 2] = am[b, 7] = 1000
        elif b % 4 == 2:
            am[b, 0] = 1000
        else:
            am[b] = 7
    ref = R.eos_rows_ref(am, -1)
    assert ref[1].item() == T + 2 and ref[3].item() == 3 * T
    rows = torch.full((B,), -1, dtype=torch.int32, device=cuda)
    eos_rows(am.to(cuda), rows, B, T, -1)
    assert torch.equal(rows.cpu(), ref)


def test_token_embed(cuda):
    """tok[clamp(id)] + pos[t] (+ type row): ids below 0 and past the vocabulary are clamped; no type
    table, a table without types (row 0), types 0 / 1 / 7 (non-zero -> row 1). Exact in f32."""
    from app.encoders import token_embed

    B, T, vocab = 2, 5, 11
    ids = torch.tensor([[-5, 0, 3, vocab + 3, vocab - 1], [10, 1, -1, 7, 2]], dtype=torch.int32)
    types = torch.tensor([[0, 1, 7, 0, 1], [7, 7, 0, 0, 1]], dtype=torch.int32)
    for D in (4, 384, 516):
        g = torch.Generator().manual_seed(D)
        tok = torch.randn(vocab, D, generator=g).to(cuda)
        pos = torch.randn(T + 2, D, generator=g).to(cuda)
        tab = torch.randn(2, D, generator=g).to(cuda)
        for name, tt, ty in (("no table", None, None), ("types null", tab, None), ("types", tab, types.to(cuda))):
            X = _nan((B * T, D), torch.float32, cuda)
            token_embed(ids.to(cuda), tok, pos, X, B, T, D, vocab, type_tab=tt, types=ty)
            ref = R.token_embed_ref(ids.to(cuda), tok, pos, tt, ty, vocab)
            assert torch.equal(X, ref), (D, name)


def test_cls_head(cuda):
    from app.encoders import cls_head

    B, worst = 3, 0.0
    for D in (1, 63, 64, 384):
        for NL in (1, 2, 3):
            g = torch.Generator().manual_seed(D * 4 + NL)
            pooled = (torch.randn(B, D, generator=g) * 1.5).to(cuda)
            Wc, bc = torch.randn(NL, D, generator=g).to(cuda), torch.randn(NL, generator=g).to(cuda)
            out = _nan((B, NL), torch.float32, cuda)
            cls_head(pooled, Wc, bc, out, B, D, NL)
            ref, mag = R.cls_head_ref(pooled, Wc, bc)
            err = (out.double() - ref).abs()
            assert bool((err <= CLS_HEAD_REL * mag).all()), (D, NL, float((err / mag).max()))
            worst = max(worst, float((err / mag).max()) / CLS_HEAD_REL)
    record_numerics("cls_head", [], [], max_err_over_bound=worst)


def test_gather_rows(cuda):
    from app import _native
    from app.encoders import gather_rows

    g = torch.Generator().manual_seed(2)
    rows = torch.tensor([6, 0, 3, 3, 6, 1, 0, 5, 3], dtype=torch.int32, device=cuda)
    for row_bytes in (16, 768, 2048):
        src = torch.randint(0, 256, (7, row_bytes), generator=g, dtype=torch.uint8).to(cuda)
        before = src.clone()
        dst = torch.full((rows.numel(), row_bytes), 0xAB, dtype=torch.uint8, device=cuda)
        gather_rows(src, dst, rows, rows.numel(), row_bytes)
        assert torch.equal(dst, src[rows.long()]), row_bytes
        assert torch.equal(src, before)
    src = torch.zeros(7, 24, dtype=torch.uint8, device=cuda)
    with pytest.raises(_native.NativeError, match="16"):
        gather_rows(src, torch.zeros(9, 24, dtype=torch.uint8, device=cuda), rows, 9, 24)


def test_layernorm_rejects_in_place_gather(cuda):
    """In place through a gather is a race between rows: rejected (MRAG_ERR_ARG), nothing launched,
    the buffer untouched; in place without a gather stays allowed (test_layernorm_vector_paths)."""
    from app import _native
    from app.encoders import layernorm

    rows, D = 8, 64
    gamma, beta, _ = _ln_params(D, cuda)
    x = torch.randn(rows, D, device=cuda)
    before = x.clone()
    gi = torch.arange(rows - 1, -1, -1, dtype=torch.int32, device=cuda)
    with pytest.raises(_native.NativeError, match="gather"):
        layernorm(x, gamma, beta, rows, D, gather=gi, y32=x)
    torch.cuda.synchronize()
    assert torch.equal(x, before)
