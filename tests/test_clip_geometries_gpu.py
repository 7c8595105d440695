"""CLIP geometries beyond ViT-B/32 on the GPU: the padded im2col of patch sizes that are no
multiple of 8 (ViT-L/14), the seqkv attention kernel (65 <= L <= 320) against flash16 byte for
byte, the B/16, L/14 and tiny patch-14 towers against fp32 transformers models holding the same
synthetic weights, batch consistency across the image lanes, and the drop-in classes reading the
geometry from a checkpoint directory's config.json.

Bars: the towers' is tests/test_encoders_gpu.py's (unit rows: 1 - cos <= 1e-4, |diff| <= 1e-3);
attention's is tests/test_encoder_kernels_gpu.py's 2^-9 max |v|. Observed errors are recorded
(conftest.record_numerics) and printed at the end of the run.
"""
from __future__ import annotations

import gc
import json
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import _kernel_refs as R
from conftest import record_numerics

pytestmark = pytest.mark.gpu

COS_ERR_MAX = 1e-4  # tests/test_encoders_gpu.py
ABS_MAX = 1e-3
ATT_TOL = 2.0 ** -9  # tests/test_encoder_kernels_gpu.py
ERR_ARG = 1  # MRAG_ERR_ARG (include/mrag.h)


def _cmp_unit(got, exp, name):
    row = record_numerics(name, got, exp, unit=True)
    print(name, row)
    assert row["max_1_minus_cos"] <= COS_ERR_MAX, row
    assert row["max_abs_diff"] <= ABS_MAX, row


def _unit(x):
    from oracle.models import normalize_rows

    return normalize_rows(np.asarray(x, dtype=np.float32).copy())


def _images(B, S, seed):
    """u8 [B][S][S][3]: uniform noise plus one smooth gradient (a different direction per image)."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 128, (B, S, S, 3))
    y, x = np.mgrid[0:S, 0:S].astype(np.float64) / max(S - 1, 1)
    ramp = np.stack([(np.cos(b) * x + np.sin(b) * y) * 0.5 + 0.5 for b in range(B)])  # in [-0.2, 1.2]
    img = noise + (127.0 * np.clip(ramp, 0.0, 1.0))[..., None]
    return np.clip(img, 0, 255).astype(np.uint8)


# ---- im2col ------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,S,P", [(2, 28, 14), (1, 56, 14), (3, 42, 7), (2, 224, 14)])
def test_im2col_padded_rows_bit_exact(cuda, B, S, P):
    """P % 8 != 0: rows of Kpad = roundup(3 P P, 64) halves. The first 3 P P are the formula
    reference bit for bit, the pad columns exactly +0 over a NaN pre-fill, and 256 guard rows after
    the output keep their bytes."""
    from app.encoders import vit_im2col, vit_patch_kpad

    Kp, Kpad = 3 * P * P, vit_patch_kpad(P)
    assert Kpad % 64 == 0 and 0 < Kpad - Kp < 64 and Kpad == {14: 640, 7: 192}[P]
    g = torch.Generator().manual_seed(S + P)
    img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
    img.view(-1)[:4] = torch.tensor([0, 255, 255, 0], dtype=torch.uint8)
    rows = B * (S // P) ** 2
    GUARD = 256
    buf = torch.full((rows + GUARD, Kpad), float("nan"), dtype=torch.float16, device=cuda)
    guard_before = buf[rows:].view(torch.int16).clone()
    vit_im2col(img.to(cuda), buf, B, S, P)
    ref = R.im2col_ref(img.to(cuda), B, S, P)
    out = buf[:rows]
    assert torch.equal(out[:, :Kp].contiguous().view(torch.int16), ref.view(torch.int16)), "columns differ"
    assert int((out[:, Kp:].contiguous().view(torch.int16) != 0).sum()) == 0, "pad columns are not +0"
    assert torch.equal(buf[rows:].view(torch.int16), guard_before), "rows after the output were written"
    # a second launch over the result gives the same bytes (the pad is written, not assumed)
    buf[:rows, Kp:] = float("inf")
    vit_im2col(img.to(cuda), buf, B, S, P)
    assert int((buf[:rows, Kp:].contiguous().view(torch.int16) != 0).sum()) == 0
    assert torch.equal(buf[rows:].view(torch.int16), guard_before)


@pytest.mark.parametrize("P", [16, 32])
def test_im2col_multiples_of_8_stay_unpadded(cuda, P):
    from app.encoders import vit_im2col, vit_patch_kpad

    B, S = 2, 64
    K = 3 * P * P
    assert vit_patch_kpad(P) == K
    g = torch.Generator().manual_seed(P)
    img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).to(cuda)
    rows = B * (S // P) ** 2
    buf = torch.full((rows * K + 256 * 64,), float("nan"), dtype=torch.float16, device=cuda)
    vit_im2col(img, buf, B, S, P)
    ref = R.im2col_ref(img, B, S, P)
    assert torch.equal(buf[:rows * K].view(torch.int16), ref.view(-1).view(torch.int16))
    assert bool(torch.isnan(buf[rows * K:]).all()), "halves after the unpadded output were written"


# ---- attention: seqkv against flash16 ----------------------------------------------------------

SKV_B, SKV_H = 3, 2
SKV_LS = (65, 79, 80, 81, 197, 257, 320)
SKV_MASKS = ("none", "right", "left", "holes", "one_empty")


def _skv_mask(kind, L):
    if kind == "one_empty":  # ragged padding with one sequence fully masked
        m = R.attention_mask("right", SKV_B, L)
        m[1] = 0
        return m
    return R.attention_mask(kind, SKV_B, L)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("DH", [32, 64])
def test_attention_seqkv_equals_flash16(cuda, DH, causal):
    """kernel=seqkv gives flash16's bytes (and the automatic rule's) at every L across its 16-key
    blocks and staging variants, without a mask, with ragged right / left padding, holes and a
    fully masked sequence, flat and peaked scores; and stays within 2^-9 max |v| of float64."""
    from app.encoders import attention

    B, H = SKV_B, SKV_H
    worst = 0.0
    for L in SKV_LS:
        for kind in SKV_MASKS:
            mask = _skv_mask(kind, L)
            mask_d = mask.to(cuda) if mask is not None else None
            for regime in ("flat", "peaked") if kind in ("none", "right") else ("ramp_up",):
                seed = 16 * L + DH // 32 + 4 * R.ATT_REGIMES.index(regime)
                qkv = R.attention_inputs(regime, B, L, H, DH, mask, causal, seed).to(cuda)
                outs = {}
                for name in ("flash16", "seqkv", "auto"):
                    out = torch.full((B * L, H * DH), float("nan"), dtype=torch.float16, device=cuda)
                    attention(qkv, out, B, L, H, DH, mask=mask_d, causal=causal, kernel=name)
                    outs[name] = out
                lab = (DH, causal, L, kind, regime)
                assert not bool(torch.isnan(outs["seqkv"]).any()), ("NaN left in out", lab)
                assert torch.equal(outs["seqkv"].view(torch.int16), outs["flash16"].view(torch.int16)), \
                    ("seqkv and flash16 differ in bytes", lab)
                assert torch.equal(outs["auto"].view(torch.int16), outs["flash16"].view(torch.int16)), \
                    ("the automatic rule and flash16 differ in bytes", lab)
                ref, empty, vmax = R.attention_ref(qkv, B, L, H, DH, mask_d, causal)
                e = empty.reshape(-1)
                err = (outs["seqkv"].double() - ref).abs() / vmax[:, None, :].expand(B, L, H * DH).reshape(B * L, H * DH)
                err = torch.where(e[:, None], torch.zeros_like(err), err)
                r = float(torch.nan_to_num(err, nan=float("inf")).max())
                print("seqkv", lab, "max |out - ref| / vmax = %.3g" % r)
                assert not bool((outs["seqkv"][e] != 0).any()), ("row without a key is not zero", lab)
                assert r <= ATT_TOL, ("|out - ref| > 2^-9 vmax", lab, r)
                worst = max(worst, r)
    record_numerics(f"attention_seqkv_dh{DH}_causal{int(causal)}", [], [], max_err_over_vmax=worst, bound=ATT_TOL)


def test_attention_seqkv_rejected_outside_its_range(cuda):
    from app.encoders import ATTENTION_KERNELS, _register_signatures

    assert ATTENTION_KERNELS["seqkv"] == 3
    lib = _register_signatures()
    for L in (64, 321):
        qkv = torch.zeros((2 * L, 3 * 2 * 64), dtype=torch.float16, device=cuda)
        out = torch.zeros((2 * L, 2 * 64), dtype=torch.float16, device=cuda)
        assert lib.mrag_attention(qkv.data_ptr(), out.data_ptr(), None, 2, L, 2, 64, 0, 0.125, 3, None) == ERR_ARG
        assert b"seqkv" in lib.mrag_last_error()


# ---- towers against fp32 transformers ----------------------------------------------------------

def _hf_clip(vcfg, tcfg, weights=None):
    """transformers CLIPModel (fp32, CPU) of two EncoderConfigs with their synthetic weights
    (``weights``: those already generated, by name), built on the meta device (no random
    initialisation of weights that are overwritten anyway)."""
    from transformers import CLIPConfig, CLIPModel

    from app.encoders.weights import param_specs, synth_param

    act = {0: "quick_gelu", 1: "gelu"}
    v = dict(hidden_size=vcfg.hidden, intermediate_size=vcfg.intermediate, num_hidden_layers=vcfg.layers,
             num_attention_heads=vcfg.heads, image_size=vcfg.image_size, patch_size=vcfg.patch_size,
             hidden_act=act[vcfg.act], layer_norm_eps=vcfg.ln_eps)
    t = dict(hidden_size=tcfg.hidden, intermediate_size=tcfg.intermediate, num_hidden_layers=tcfg.layers,
             num_attention_heads=tcfg.heads, max_position_embeddings=tcfg.max_positions, vocab_size=tcfg.vocab,
             hidden_act=act[tcfg.act], layer_norm_eps=tcfg.ln_eps, eos_token_id=tcfg.eos_token_id,
             bos_token_id=0, pad_token_id=1)
    cfg = CLIPConfig(text_config=t, vision_config=v, projection_dim=vcfg.proj_dim)
    with torch.device("meta"):
        model = CLIPModel(cfg)
    model = model.to_empty(device="cpu")
    sd = {"logit_scale": torch.tensor(0.0)}
    for c in (vcfg, tcfg):
        for name, shape, kind in param_specs(c):
            have = weights is not None and name in weights
            sd[name] = torch.from_numpy(weights[name] if have else synth_param(name, shape, kind, 0))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    for emb in (model.vision_model.embeddings, model.text_model.embeddings):
        emb.position_ids = torch.arange(emb.position_ids.shape[-1]).unsqueeze(0)  # a non-persistent buffer
    return cfg, model.eval()


def _small_text(proj):
    from app.encoders.weights import EncoderConfig

    return EncoderConfig(kind=2, hidden=128, layers=1, heads=2, intermediate=256, max_positions=77, vocab=512,
                         proj_dim=proj, act=0, eos_token_id=511)


def _small_vision(proj):
    from app.encoders.weights import EncoderConfig

    return EncoderConfig(kind=1, hidden=128, layers=1, heads=2, intermediate=256, proj_dim=proj, image_size=56,
                         patch_size=14, act=0)


def _image_case(cuda, vcfg, B, name):
    from oracle.models import clip_image_embeds

    from app.encoders import GpuEncoder
    from app.encoders.weights import synth_state_dict

    weights = dict(synth_state_dict(vcfg, 0))  # generated once for both sides (9 s at the full L/14 depth)
    _, model = _hf_clip(vcfg, _small_text(vcfg.proj_dim), weights)
    imgs = _images(B, vcfg.image_size, seed=vcfg.patch_size + vcfg.layers)
    exp = clip_image_embeds(model, imgs, normalize=True)
    del model
    enc = GpuEncoder(vcfg, state_dict=weights)
    try:
        got = enc.embed_images(imgs, normalize=True)
        dev = enc.embed_images(torch.from_numpy(imgs).to(cuda), normalize=True).cpu().numpy()
    finally:
        enc.close()
    assert got.shape == (B, vcfg.proj_dim) and np.all(np.isfinite(got))
    assert np.array_equal(got.view(np.int32), dev.view(np.int32)), "host and device pointer calls differ"
    _cmp_unit(got, exp, name)


def test_batch_consistency_l14_lanes(cuda):
    """ViT-L/14 geometry (4 layers): one image's row has the same bytes at B = 1, in a batch of 3 and
    in a batch of 130, which a sole image handle runs as two lanes of 65."""
    from app.encoders import CLIP_VISION_L14, GpuEncoder

    gc.collect()  # handles of earlier tests, so that this one is the process's only image handle
    enc = GpuEncoder(replace(CLIP_VISION_L14, layers=4))
    try:
        base = _images(3, 224, seed=5)
        fill = np.random.default_rng(6).integers(0, 256, (130, 224, 224, 3), dtype=np.uint8)
        fill[77] = base[0]
        big = torch.from_numpy(fill).to(cuda)
        r1 = enc.embed_images(base[:1], normalize=False)
        r3 = enc.embed_images(base, normalize=False)
        r130 = enc.embed_images(big, normalize=False).cpu().numpy()
    finally:
        enc.close()
    assert np.all(np.isfinite(r130)) and float(np.abs(r1).max()) > 0
    assert np.array_equal(r1[0].view(np.int32), r3[0].view(np.int32)), "B = 1 and B = 3 differ"
    assert np.array_equal(r1[0].view(np.int32), r130[77].view(np.int32)), "B = 1 and B = 130 differ"


def test_tower_tiny_patch14(cuda):
    """hidden 128, 2 heads, 2 layers, patch 14 on 56 x 56 images (17 tokens): the padded patch K and
    flash16 at L <= 32."""
    from app.encoders.weights import EncoderConfig

    vcfg = EncoderConfig(kind=1, hidden=128, layers=2, heads=2, intermediate=256, proj_dim=128, image_size=56,
                         patch_size=14, act=0)
    _image_case(cuda, vcfg, 3, "clip_image_tiny_patch14")


def test_tower_b16_two_layers(cuda):
    """ViT-B/16 geometry, two layers: 197 tokens, the seqkv range."""
    from app.encoders import CLIP_VISION_B16

    _image_case(cuda, replace(CLIP_VISION_B16, layers=2), 3, "clip_image_b16_2l")


def test_tower_l14_full_depth(cuda):
    """ViT-L/14, all 24 layers, against fp32 transformers: 257 tokens, hidden 1024, 16 heads."""
    from app.encoders import CLIP_VISION_L14

    _image_case(cuda, CLIP_VISION_L14, 2, "clip_image_l14_24l")


def test_tower_l14_text(cuda):
    """The L/14 text geometry (hidden 768, 12 heads, projection 768), two layers, 4 sequences at 77
    tokens with ragged padding, pooled at the first EOS."""
    from oracle.models import clip_text_embeds

    from app.encoders import CLIP_TEXT_L14, GpuEncoder

    tcfg = replace(CLIP_TEXT_L14, layers=2, vocab=2048, eos_token_id=2047)
    _, model = _hf_clip(_small_vision(tcfg.proj_dim), tcfg)
    rng = np.random.default_rng(3)
    ids = rng.integers(2, 2000, (4, 77)).astype(np.int32)
    mask = np.zeros((4, 77), dtype=np.int32)
    for b, n in enumerate((77, 40, 9, 66)):
        ids[b, n - 1] = 2047
        ids[b, n:] = 1
        mask[b, :n] = 1
    exp = clip_text_embeds(model, ids, mask, normalize=True)
    enc = GpuEncoder(tcfg)
    try:
        got = enc.embed_tokens(ids, mask, normalize=True)
    finally:
        enc.close()
    _cmp_unit(got, exp, "clip_text_l14_2l")


# ---- B/32 bytes are pinned across the automatic rule -------------------------------------------

def test_b32_embedding_independent_of_attention_rule(cuda):
    """The ViT-B/32 tower (50 tokens: seq64, outside seqkv's range) on a fixed batch, against the same
    layers driven from here with attention forced to flash16: the same bytes, so the tower's output
    does not depend on which attention kernel the automatic rule takes. Likewise a 2-layer B/16 tower
    (197 tokens) equals its flash16-forced restatement: adopting seqkv there changed no byte."""
    from app.encoders import (CLIP_VISION_B16, CLIP_VISION_B32, GpuEncoder, attention, gemm_nt, layernorm,
                              vit_embed_ln, vit_im2col)
    from app.encoders.weights import synth_state_dict

    for cfg, B in ((replace(CLIP_VISION_B32, layers=2), 5), (replace(CLIP_VISION_B16, layers=2), 2)):
        sd = {n: torch.from_numpy(a).to(cuda) for n, a in synth_state_dict(cfg, 0)}
        imgs = torch.from_numpy(_images(B, 224, seed=11)).to(cuda)
        enc = GpuEncoder(cfg)
        try:
            got = enc.embed_images(imgs, normalize=False)
        finally:
            enc.close()
        D, I, H, P = cfg.hidden, cfg.intermediate, cfg.heads, cfg.patch_size
        G = 224 // P
        T, K = G * G + 1, 3 * P * P
        pre = "vision_model."
        f16 = lambda n: sd[n].reshape(sd[n].shape[0], -1).half().contiguous()
        col = torch.empty((B * G * G, K), dtype=torch.float16, device=cuda)
        vit_im2col(imgs, col, B, 224, P)
        patch = torch.empty((B * G * G, D), dtype=torch.float32, device=cuda)
        gemm_nt(col, f16(pre + "embeddings.patch_embedding.weight"), None, patch, 4)
        X = torch.empty((B * T, D), dtype=torch.float32, device=cuda)
        vit_embed_ln(patch, sd[pre + "embeddings.class_embedding"], sd[pre + "embeddings.position_embedding.weight"],
                     sd[pre + "pre_layrnorm.weight"], sd[pre + "pre_layrnorm.bias"], X, B, T, D, eps=cfg.ln_eps)
        Hh = torch.empty((B * T, D), dtype=torch.float16, device=cuda)
        for i in range(cfg.layers):
            l = f"{pre}encoder.layers.{i}."
            wqkv = torch.cat([f16(l + f"self_attn.{p}_proj.weight") for p in "qkv"]).contiguous()
            bqkv = torch.cat([sd[l + f"self_attn.{p}_proj.bias"] for p in "qkv"]).contiguous()
            layernorm(X, sd[l + "layer_norm1.weight"], sd[l + "layer_norm1.bias"], B * T, D, y16=Hh, eps=cfg.ln_eps)
            qkv = torch.empty((B * T, 3 * D), dtype=torch.float16, device=cuda)
            gemm_nt(Hh, wqkv, bqkv, qkv, 0)
            att = torch.empty((B * T, D), dtype=torch.float16, device=cuda)
            attention(qkv, att, B, T, H, D // H, kernel="flash16")
            gemm_nt(att, f16(l + "self_attn.out_proj.weight"), sd[l + "self_attn.out_proj.bias"], X, 3)
            layernorm(X, sd[l + "layer_norm2.weight"], sd[l + "layer_norm2.bias"], B * T, D, y16=Hh, eps=cfg.ln_eps)
            F = torch.empty((B * T, I), dtype=torch.float16, device=cuda)
            gemm_nt(Hh, f16(l + "mlp.fc1.weight"), sd[l + "mlp.fc1.bias"], F, 1)
            gemm_nt(F, f16(l + "mlp.fc2.weight"), sd[l + "mlp.fc2.bias"], X, 3)
        pooled = torch.empty((B, D), dtype=torch.float16, device=cuda)
        rows = (torch.arange(B, dtype=torch.int32) * T).to(cuda)
        layernorm(X, sd[pre + "post_layernorm.weight"], sd[pre + "post_layernorm.bias"], B, D, gather=rows, y16=pooled,
                  eps=cfg.ln_eps)
        exp = torch.empty((B, cfg.proj_dim), dtype=torch.float32, device=cuda)
        gemm_nt(pooled, f16("visual_projection.weight"), None, exp, 4)
        assert bool(torch.isfinite(exp).all()) and float(exp.abs().max()) > 0
        assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), f"patch {P}: bytes differ from the flash16 chain"


# ---- through the drop-in -----------------------------------------------------------------------

def _write_checkpoint(d, config, cfgs, extra=None):
    from safetensors.numpy import save_file

    from app.encoders.weights import synth_state_dict

    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(config, f)
    sd = {}
    for c in cfgs:
        sd.update({n: np.ascontiguousarray(a) for n, a in synth_state_dict(c, 0)})
    save_file(sd, os.path.join(d, "model.safetensors"))
    for name, text in (extra or {}).items():
        with open(os.path.join(d, name), "w") as f:
            f.write(text)
    return str(d)


def test_clip_model_reads_b16_checkpoint(cuda, tmp_path):
    """ClipModel on a 2-layer ViT-B/16 checkpoint directory: the towers come from config.json (the
    B/32 constants would fail on the first parameter), give the bytes of directly built encoders of
    those configs, and agree with the transformers model."""
    from oracle.models import clip_image_embeds, clip_text_embeds

    from app.encoders import CLIP_TEXT_B32, CLIP_VISION_B16, GpuEncoder
    from app.encoders.models import ClipModel

    vcfg = replace(CLIP_VISION_B16, layers=2)
    tcfg = replace(CLIP_TEXT_B32, layers=2, vocab=2048, eos_token_id=2047)
    hf_cfg, model = _hf_clip(vcfg, tcfg)
    d = _write_checkpoint(tmp_path / "clip-vit-base-patch16", hf_cfg.to_dict(), (vcfg, tcfg))
    m = ClipModel(d)
    assert m.vision_cfg == vcfg and m.text_cfg == tcfg
    imgs = _images(3, 224, seed=21)
    ids = np.random.default_rng(4).integers(2, 2000, (3, 20)).astype(np.int32)
    mask = np.zeros((3, 20), dtype=np.int32)
    for b, n in enumerate((20, 7, 13)):
        ids[b, n - 1] = 2047
        ids[b, n:] = 1
        mask[b, :n] = 1
    gi = m.get_image_features(images_u8=imgs).cpu().numpy()
    gt = m.get_text_features(input_ids=ids, attention_mask=mask).cpu().numpy()
    assert gi.shape == (3, 512) and gt.shape == (3, 512)
    ev, et = GpuEncoder(vcfg), GpuEncoder(tcfg)
    try:
        di = ev.embed_images(imgs, normalize=False)
        dt = et.embed_tokens(ids, mask, normalize=False)
    finally:
        ev.close()
        et.close()
    assert np.array_equal(gi.view(np.int32), di.view(np.int32)), "image features differ from the direct encoder"
    assert np.array_equal(gt.view(np.int32), dt.view(np.int32)), "text features differ from the direct encoder"
    _cmp_unit(_unit(gi), clip_image_embeds(model, imgs, normalize=True), "dropin_clip_b16_image")
    _cmp_unit(_unit(gt), clip_text_embeds(model, ids, mask, normalize=True), "dropin_clip_b16_text")


def test_minilm_model_reads_12_layer_checkpoint(cuda, tmp_path):
    """MiniLMSentenceModel on a 12-layer MiniLM directory (all-MiniLM-L12-v2's shape, a small
    vocabulary with a minimal vocab.txt): 12 layers run, encode() gives the direct encoder's bytes and
    agrees with transformers' BertModel + mean pooling."""
    from oracle.models import minilm_embeds
    from transformers import BertConfig, BertModel

    from app.encoders import MINILM_L6, GpuEncoder
    from app.encoders.models import MiniLMSentenceModel
    from app.encoders.weights import synth_state_dict

    words = ["the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "a", "search", "image", "text", "model"]
    letters = [chr(c) for c in range(ord("a"), ord("z") + 1)]
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ".", ","] + words + letters + ["##" + c for c in letters]
    cfg = replace(MINILM_L6, layers=12, vocab=128)
    assert len(vocab) <= cfg.vocab
    bc = BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                    num_attention_heads=cfg.heads, intermediate_size=cfg.intermediate,
                    max_position_embeddings=cfg.max_positions, hidden_act="gelu", layer_norm_eps=cfg.ln_eps)
    model = BertModel(bc, add_pooling_layer=False).eval()
    missing, unexpected = model.load_state_dict({n: torch.from_numpy(a) for n, a in synth_state_dict(cfg, 0)},
                                                strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    d = _write_checkpoint(tmp_path / "all-MiniLM-L12-v2", bc.to_dict(), (cfg,), {"vocab.txt": "\n".join(vocab) + "\n"})
    os.makedirs(os.path.join(d, "1_Pooling"))
    with open(os.path.join(d, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": 384, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
                   "pooling_mode_max_tokens": False}, f)
    m = MiniLMSentenceModel(d)
    assert m.cfg == cfg and m.cfg.layers == 12
    sentences = ["the quick brown fox jumps over the lazy dog.", "a search", "image text model, a zebra quiz",
                 "dog", "the model jumps over a lazy image search text"]
    got = m.encode(sentences)
    assert got.shape == (5, 384)
    ids, mask = m.tokenizer(sentences)
    assert ids.max() < cfg.vocab and (ids == 1).sum() == 0, "the minimal vocabulary covers the sentences"
    enc = GpuEncoder(cfg)
    try:
        direct = enc.embed_tokens(ids, mask, normalize=True)
    finally:
        enc.close()
    assert np.array_equal(got.view(np.int32), direct.view(np.int32)), "encode() differs from the direct encoder"
    _cmp_unit(got, minilm_embeds(model, ids, mask, normalize=True), "dropin_minilm_l12")
