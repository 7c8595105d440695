"""GPU encoders: CLIP image towers (ViT-B/32, B/16, L/14 at 224 pixels), CLIP text towers,
BERT sentence encoders (MiniLM-L6 / L12) and cross-encoders — through the
C ABI (``mrag_encoder_*`` in include/mrag.h, kernels in csrc/encoder*.hip).

Replaces the model calls of the reference's ``app/ml/embeddings.py``:
``SentenceTransformer.encode`` (:62-68), ``CLIPModel.get_image_features`` (:86) and
``CLIPModel.get_text_features`` (:102). Host-side work (image decode/resize/crop,
tokenisation) stays on the host as in the reference; everything from pixels / token
ids onward runs on the GPU.
"""
from __future__ import annotations

import ctypes
import os
import time
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np

from app import _native
from app.encoders.weights import (
    CLIP_TEXT_B32,
    CLIP_TEXT_L14,
    CLIP_VISION_B16,
    CLIP_VISION_B32,
    CLIP_VISION_L14,
    MINILM_L6,
    MSMARCO_MINILM_L6_CE,
    EncoderConfig,
    bert_config_from_dir,
    check_supported,
    clip_configs_from_dir,
    encoder_weights,
    param_specs,
    synth_state_dict,
)


class _CConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "kind", "hidden", "layers", "heads", "intermediate", "max_positions", "vocab", "proj_dim",
        "image_size", "patch_size", "act", "eos_token_id")] + [("ln_eps", ctypes.c_float)]


def _register_signatures():
    lib = _native.load()
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    sigs = {
        "mrag_encoder_create": [ctypes.POINTER(_CConfig), i32, ctypes.POINTER(vp)],
        "mrag_encoder_destroy": [vp],
        "mrag_encoder_set_param": [vp, ctypes.c_char_p, vp, i64],
        "mrag_encoder_missing": [vp, ctypes.POINTER(i64)],
        "mrag_encoder_embed_images": [vp, vp, i32, vp, i32, i32, vp],
        "mrag_encoder_embed_tokens": [vp, vp, vp, i32, i32, vp, i32, i32, vp],
        "mrag_gemm_nt": [vp, vp, vp, vp, i32, i32, i32, i32, vp],
        "mrag_gemm_nt_kernel": [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp],
        "mrag_gemm_nt_ld": [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
        "mrag_encoder_score_pairs": [vp, vp, vp, vp, i32, i32, vp, i32, vp],
        # building blocks (tests and timing)
        "mrag_layernorm": [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp],
        "mrag_attention": [vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp],
        "mrag_vit_im2col": [vp, vp, i32, i32, i32, vp],
        "mrag_vit_embed_ln": [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp],
        "mrag_token_embed": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp],
        "mrag_eos_rows": [vp, i32, i32, i32, vp, vp],
        "mrag_mean_pool": [vp, vp, vp, i32, i32, i32, vp],
        "mrag_cls_head": [vp, vp, vp, vp, i32, i32, i32, vp],
        "mrag_gather_rows": [vp, vp, vp, i32, i32, vp],
    }
    for name, args in sigs.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if name in ("mrag_gemm_nt_kernel", "mrag_gemm_nt_ld"):  # timing / test entries, absent from older builds (A/B)
                continue
            raise
        fn.restype = ctypes.c_int32
        fn.argtypes = args
    return lib


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class GpuEncoder:
    """One encoder tower resident on one GPU."""

    def __init__(self, cfg: EncoderConfig, device: int = 0, state_dict=None, seed: int = 0):
        self.lib = _register_signatures()
        self.cfg = cfg
        self.device = int(device)
        c = _CConfig(kind=cfg.kind, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                     intermediate=cfg.intermediate, max_positions=cfg.max_positions, vocab=cfg.vocab,
                     proj_dim=cfg.proj_dim, image_size=cfg.image_size, patch_size=cfg.patch_size, act=cfg.act,
                     eos_token_id=cfg.eos_token_id, ln_eps=cfg.ln_eps)
        h = ctypes.c_void_p()
        _native.check(self.lib.mrag_encoder_create(ctypes.byref(c), self.device, ctypes.byref(h)),
                      "mrag_encoder_create")
        self._h = h
        items = state_dict.items() if state_dict is not None else synth_state_dict(cfg, seed)
        for name, arr in items:
            self.set_param(name, arr)
        missing = ctypes.c_int64(0)
        _native.check(self.lib.mrag_encoder_missing(self._h, ctypes.byref(missing)), "mrag_encoder_missing")
        if missing.value:
            raise RuntimeError(f"{missing.value} encoder parameters missing")

    def set_param(self, name: str, arr) -> None:
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
        _native.check(self.lib.mrag_encoder_set_param(self._h, name.encode(), a.ctypes.data, a.size),
                      f"set_param({name})")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.mrag_encoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @property
    def out_dim(self) -> int:
        return self.cfg.hidden if self.cfg.kind == 3 else self.cfg.proj_dim

    def embed_images(self, images, normalize: bool = True):
        """images: u8 [B, S, S, 3] (numpy host or torch CUDA) -> f32 [B, proj_dim]."""
        if self.cfg.kind != 1:
            raise TypeError("not an image encoder")
        S = self.cfg.image_size
        if _is_torch(images):
            import torch

            x = images.contiguous()
            if x.dtype != torch.uint8 or tuple(x.shape[1:]) != (S, S, 3):
                raise ValueError(f"images must be uint8 [B,{S},{S},3]")
            out = torch.empty((x.shape[0], self.out_dim), dtype=torch.float32, device=x.device)
            stream = torch.cuda.current_stream(x.device).cuda_stream
            _native.check(self.lib.mrag_encoder_embed_images(self._h, x.data_ptr(), x.shape[0], out.data_ptr(),
                                                             int(normalize), _native.MRAG_PTR_DEVICE, stream),
                          "embed_images")
            return out
        x = np.ascontiguousarray(images, dtype=np.uint8)
        if x.ndim != 4 or x.shape[1:] != (S, S, 3):
            raise ValueError(f"images must be uint8 [B,{S},{S},3], got {x.shape}")
        out = np.empty((x.shape[0], self.out_dim), dtype=np.float32)
        _native.check(self.lib.mrag_encoder_embed_images(self._h, x.ctypes.data, x.shape[0], out.ctypes.data,
                                                         int(normalize), _native.MRAG_PTR_HOST, None),
                      "embed_images")
        return out

    def embed_tokens(self, ids, mask=None, normalize: bool = True):
        """ids/mask int [B, T] (numpy host or torch CUDA) -> f32 [B, out_dim]."""
        if self.cfg.kind == 1:
            raise TypeError("not a text encoder")
        if _is_torch(ids):
            import torch

            i = ids.to(torch.int32).contiguous()
            m = mask.to(torch.int32).contiguous() if mask is not None else None
            out = torch.empty((i.shape[0], self.out_dim), dtype=torch.float32, device=i.device)
            stream = torch.cuda.current_stream(i.device).cuda_stream
            _native.check(self.lib.mrag_encoder_embed_tokens(self._h, i.data_ptr(), m.data_ptr() if m is not None else None,
                                                             i.shape[0], i.shape[1], out.data_ptr(), int(normalize),
                                                             _native.MRAG_PTR_DEVICE, stream), "embed_tokens")
            return out
        i = np.ascontiguousarray(ids, dtype=np.int32)
        if i.ndim != 2:
            raise ValueError("ids must be [B, T]")
        m = np.ascontiguousarray(mask, dtype=np.int32) if mask is not None else None
        out = np.empty((i.shape[0], self.out_dim), dtype=np.float32)
        _native.check(self.lib.mrag_encoder_embed_tokens(self._h, i.ctypes.data, m.ctypes.data if m is not None else None,
                                                         i.shape[0], i.shape[1], out.ctypes.data, int(normalize),
                                                         _native.MRAG_PTR_HOST, None), "embed_tokens")
        return out


    def score_pairs(self, ids, type_ids=None, mask=None):
        """Cross-encoder logits: ids / type_ids / mask int [B, T] host arrays -> f32 [B, num_labels]."""
        if self.cfg.kind != 4:
            raise TypeError("not a cross-encoder")
        i = np.ascontiguousarray(ids, dtype=np.int32)
        if i.ndim != 2:
            raise ValueError("ids must be [B, T]")
        t = np.ascontiguousarray(type_ids, dtype=np.int32) if type_ids is not None else None
        m = np.ascontiguousarray(mask, dtype=np.int32) if mask is not None else None
        out = np.empty((i.shape[0], self.cfg.proj_dim), dtype=np.float32)
        _native.check(self.lib.mrag_encoder_score_pairs(self._h, i.ctypes.data, t.ctypes.data if t is not None else None,
                                                        m.ctypes.data if m is not None else None, i.shape[0],
                                                        i.shape[1], out.ctypes.data, _native.MRAG_PTR_HOST, None),
                      "score_pairs")
        return out


GEMM_KERNELS = {"auto": 0, "k3": 1, "k3d": 2, "k3s": 3, "k3w": 4}


def gemm_nt(A, W, bias, C, epilogue: int, kernel: str = "auto", lda: Optional[int] = None,
            ldc: Optional[int] = None):
    """The encoder GEMM on torch CUDA tensors (test / building-block entry): the automatic kernel
    choice of the towers, or one kernel forced (``GEMM_KERNELS``: bit-identity tests, timing).
    With ``lda`` / ``ldc`` (row strides in elements, default K / N) the operands are read from
    ``A.data_ptr()`` / written at ``C.data_ptr()`` with those strides (``A`` and ``C`` still give
    M, K and the base addresses: pass views of the strided buffers)."""
    import torch

    lib = _register_signatures()
    M, K = A.shape
    N = W.shape[0]
    stream = torch.cuda.current_stream(A.device).cuda_stream
    bp = bias.data_ptr() if bias is not None else None
    if lda is not None or ldc is not None:
        _native.check(lib.mrag_gemm_nt_ld(A.data_ptr(), K if lda is None else lda, W.data_ptr(), bp, C.data_ptr(),
                                          N if ldc is None else ldc, M, N, K, epilogue, GEMM_KERNELS[kernel], stream),
                      "mrag_gemm_nt_ld")
    elif kernel == "auto":
        _native.check(lib.mrag_gemm_nt(A.data_ptr(), W.data_ptr(), bp, C.data_ptr(), M, N, K, epilogue, stream),
                      "mrag_gemm_nt")
    else:
        _native.check(lib.mrag_gemm_nt_kernel(A.data_ptr(), W.data_ptr(), bp, C.data_ptr(), M, N, K, epilogue,
                                              GEMM_KERNELS[kernel], stream), "mrag_gemm_nt_kernel")
    return C


# ---- building blocks: one kernel launch each on torch CUDA tensors (tests and timing) --------
# Tensors are passed by their data_ptr (a view's offset base included) and the shape arguments
# are explicit, so a test can hand over strided, offset or aliased buffers. Launches go to the
# current torch stream; nothing is allocated or synchronised here.
ATTENTION_KERNELS = {"auto": 0, "flash16": 1, "seq64": 2, "seqkv": 3}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream(t):
    import torch

    return torch.cuda.current_stream(t.device).cuda_stream


def layernorm(x, gamma, beta, rows: int, D: int, ldx: Optional[int] = None, gather=None, y32=None, y16=None,
              eps: float = 1e-5):
    """K2: LayerNorm of ``rows`` rows of ``D`` floats (``ldx`` apart, default D) read from
    ``x.data_ptr()``, through the optional int32 ``gather``, into ``y32`` (f32) and / or ``y16``."""
    lib = _register_signatures()
    _native.check(lib.mrag_layernorm(_ptr(x), _ptr(gather), _ptr(y32), _ptr(y16), _ptr(gamma), _ptr(beta), rows, D,
                                     D if ldx is None else ldx, eps, _stream(x)), "mrag_layernorm")


def attention(qkv, out, B: int, L: int, H: int, head_dim: int, mask=None, causal: bool = False,
              scale: Optional[float] = None, kernel: str = "auto"):
    """K4: ``out[B*L][H*head_dim]`` from fp16 ``qkv[B*L][3*H*head_dim]``; int32 ``mask[B][L]``
    (1 = keep the key) or None; ``kernel`` one of ``ATTENTION_KERNELS``."""
    lib = _register_signatures()
    sc = head_dim ** -0.5 if scale is None else scale
    _native.check(lib.mrag_attention(_ptr(qkv), _ptr(out), _ptr(mask), B, L, H, head_dim, int(causal), sc,
                                     ATTENTION_KERNELS[kernel], _stream(qkv)), "mrag_attention")
    return out


def vit_im2col(img, out, B: int, S: int, P: int):
    """K1 prologue: u8 ``img[B][S][S][3]`` -> fp16 ``out[B*(S/P)^2][Kpad]`` (CLIP normalisation);
    ``Kpad = 3*P*P``, rounded up to a multiple of 64 with zero pad columns when ``P % 8 != 0``
    (``vit_patch_kpad``)."""
    lib = _register_signatures()
    _native.check(lib.mrag_vit_im2col(_ptr(img), _ptr(out), B, S, P, _stream(img)), "mrag_vit_im2col")
    return out


def vit_patch_kpad(P: int) -> int:
    """Row length of the im2col output (and of the packed patch weight): P = 14 -> 640."""
    return (3 * P * P + 63) // 64 * 64


def vit_embed_ln(patch, cls, pos, gamma, beta, X, B: int, T: int, D: int, eps: float = 1e-5):
    """``X[b*T + t] = LN((t == 0 ? cls : patch[b*(T-1) + t-1]) + pos[t])`` (f32)."""
    lib = _register_signatures()
    _native.check(lib.mrag_vit_embed_ln(_ptr(patch), _ptr(cls), _ptr(pos), _ptr(gamma), _ptr(beta), _ptr(X), B, T, D,
                                        eps, _stream(X)), "mrag_vit_embed_ln")
    return X


def token_embed(ids, tok, pos, X, B: int, T: int, D: int, vocab: int, type_tab=None, types=None):
    """``X[b*T + t] = tok[clamp(ids)] + pos[t] (+ type_tab[types != 0])`` (f32)."""
    lib = _register_signatures()
    _native.check(lib.mrag_token_embed(_ptr(ids), _ptr(tok), _ptr(pos), _ptr(type_tab), _ptr(types), _ptr(X), B, T, D,
                                       vocab, _stream(X)), "mrag_token_embed")
    return X


def eos_rows(ids, rows, B: int, T: int, eos_id: int):
    """``rows[b] = b*T +`` the first ``eos_id`` of int32 ``ids[b]`` (0 when absent; ``eos_id < 0``: the first argmax)."""
    lib = _register_signatures()
    _native.check(lib.mrag_eos_rows(_ptr(ids), B, T, eos_id, _ptr(rows), _stream(ids)), "mrag_eos_rows")
    return rows


def mean_pool(X, out, B: int, T: int, D: int, mask=None):
    """Masked mean over T of f32 ``X[B][T][D]`` (sentence-transformers pooling)."""
    lib = _register_signatures()
    _native.check(lib.mrag_mean_pool(_ptr(X), _ptr(mask), _ptr(out), B, T, D, _stream(X)), "mrag_mean_pool")
    return out


def cls_head(pooled, Wc, bc, out, B: int, D: int, NL: int):
    """``out[b][j] = sum_d tanh(pooled[b][d]) * Wc[j][d] + bc[j]`` (f32)."""
    lib = _register_signatures()
    _native.check(lib.mrag_cls_head(_ptr(pooled), _ptr(Wc), _ptr(bc), _ptr(out), B, D, NL, _stream(out)),
                  "mrag_cls_head")
    return out


def gather_rows(src, dst, rows, B: int, row_bytes: int):
    """``dst[b] = src[rows[b]]`` for rows of ``row_bytes`` bytes (a multiple of 16)."""
    lib = _register_signatures()
    _native.check(lib.mrag_gather_rows(_ptr(src), _ptr(dst), _ptr(rows), B, row_bytes, _stream(src)),
                  "mrag_gather_rows")
    return dst


def load_encoder(cfg: EncoderConfig, model_name: Optional[str] = None, device: int = 0, seed: int = 0,
                 synthetic: Optional[bool] = None) -> GpuEncoder:
    """Encoder for a model name (local directory or cached hub snapshot). Synthetic weights
    only when ``MRAG_SYNTHETIC_WEIGHTS=1``; otherwise an unresolvable name raises before
    the GPU is touched (weights.encoder_weights)."""
    sd, _ = encoder_weights(cfg, model_name, synthetic)
    return GpuEncoder(cfg, device=device, state_dict=sd, seed=seed)


def bench_clip_images(steps: int = 10, warmup: int = 2, batch: int = 256, device: int = 0,
                      inflight: int = 3, streams=None, cfg: Optional[EncoderConfig] = None) -> Dict:
    """BASELINE config 2: CLIP ViT-B/32 image embeds/s on one GPU (batch 256 random
    224x224 u8 images resident in HBM, fp16 MFMA, synthetic weights).

    `inflight` batches run at once, each on its own encoder handle (workspace) and HIP stream,
    fed from this thread (device-pointer calls are stream-ordered, so they return at once):
    the N = 768 GEMMs run 150 persistent tiles on 256 CUs and attention / LayerNorm are
    latency-bound, so other batches' kernels fill what one batch leaves idle, as a serving
    process with concurrent requests does (measured on one box: 1 -> 66.8k, 2 -> 66.8k,
    3 -> 81.9k, 4 -> 81.1k img/s; with two, the batches fall into step and their persistent
    GEMM grids queue behind each other). inflight=1 runs one batch at a time (on its own stream,
    still without a host sync per batch). ``streams``: the HIP streams to run on (a serving
    process creates its request streams once at start-up; bench.py passes streams it made before
    its other legs, so each lands on its own hardware queue, see bench.py _early_streams).
    ``cfg``: another image tower (CLIP_VISION_B16, CLIP_VISION_L14; scripts/encoder_geometry_bench.py)."""
    import torch

    cfg = CLIP_VISION_B32 if cfg is None else cfg

    inflight = max(1, int(inflight))
    dev = torch.device("cuda", device)
    sd = None if cfg is CLIP_VISION_B32 else dict(synth_state_dict(cfg, 0))  # generated once for every handle
    encs = [GpuEncoder(cfg, device=device, state_dict=sd) for _ in range(inflight)]
    del sd
    if streams is None or len(streams) < inflight:
        streams = [torch.cuda.Stream(device=dev) for _ in range(inflight)]
    streams = list(streams)[:inflight]
    g = torch.Generator(device=dev).manual_seed(2)
    imgs = torch.randint(0, 256, (batch, 224, 224, 3), generator=g, dtype=torch.uint8, device=dev)
    outs = [None] * inflight

    def run(n):
        for i in range(n):
            j = i % inflight
            with torch.cuda.stream(streams[j]):
                outs[j] = encs[j].embed_images(imgs)

    torch.cuda.synchronize()
    run(max(warmup, inflight))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    flops_per_img = vit_flops_per_image(cfg)
    ips = batch * steps / dt
    return {
        "metric": "CLIP img-embeds/sec/GPU",
        "value": round(ips, 1),
        "unit": "images/s",
        "batch": batch,
        "steps": steps,
        "batches_in_flight": inflight,
        "ms_per_batch": round(dt / steps * 1e3, 3),
        "dtype": "fp16 MFMA (f32 accumulate, f32 residual stream)",
        "workload": ("BASELINE config 2: CLIP ViT-B/32 image tower, batch 256 random 224x224 u8 images, synthetic weights"
                     if cfg is CLIP_VISION_B32 else
                     f"CLIP ViT image tower (hidden {cfg.hidden}, {cfg.layers} layers, patch {cfg.patch_size}), "
                     f"batch {batch} random 224x224 u8 images, synthetic weights"),
        "roofline": {"bound": "mfma", "achieved": round(flops_per_img * ips / 1e12, 2), "peak": 2500.0,
                     "unit": "TFLOP/s", "frac": round(flops_per_img * ips / 1e12 / 2500.0, 4),
                     "algorithmic_flops_per_image": flops_per_img},
    }


def vit_flops_per_image(cfg: EncoderConfig = CLIP_VISION_B32) -> float:
    D, I, L = cfg.hidden, cfg.intermediate, cfg.layers
    g = cfg.image_size // cfg.patch_size
    T = g * g + 1
    lin = 2 * T * (4 * D * D + 2 * D * I) * L
    attn = 2 * 2 * T * T * D * L
    patch = 2 * (g * g) * (3 * cfg.patch_size ** 2) * D
    proj = 2 * D * cfg.proj_dim
    return float(lin + attn + patch + proj)


def text_flops_per_sequence(cfg: EncoderConfig, L: int) -> float:
    """Algorithmic FLOP of one text-tower forward at sequence length L: the linear layers
    (q, k, v, out, fc1, fc2), attention (QK^T and PV) and, for CLIP text, the projection."""
    D, I = cfg.hidden, cfg.intermediate
    lin = 2 * L * (4 * D * D + 2 * D * I) * cfg.layers
    attn = 2 * 2 * L * L * D * cfg.layers
    proj = 2 * D * cfg.proj_dim if cfg.kind == 2 else 0
    return float(lin + attn + proj)


def smoke_encoders() -> None:
    """One small forward of each tower on cuda:0, finite unit rows."""
    rng = np.random.default_rng(0)
    v = GpuEncoder(CLIP_VISION_B32)
    e = v.embed_images(rng.integers(0, 256, (2, 224, 224, 3), dtype=np.uint8))
    assert e.shape == (2, 512) and np.all(np.isfinite(e)) and np.allclose(np.linalg.norm(e, axis=1), 1, atol=1e-5)
    t = GpuEncoder(MINILM_L6)
    ids = rng.integers(1000, 2000, (3, 12)).astype(np.int32)
    m = np.ones_like(ids)
    m[1, 6:] = 0
    e = t.embed_tokens(ids, m)
    assert e.shape == (3, 384) and np.all(np.isfinite(e))


__all__ = ["GpuEncoder", "load_encoder", "gemm_nt", "layernorm", "attention", "vit_im2col", "vit_embed_ln",
           "token_embed", "eos_rows", "mean_pool", "cls_head", "gather_rows", "bench_clip_images", "smoke_encoders", "CLIP_VISION_B32",
           "CLIP_TEXT_B32", "CLIP_VISION_B16", "CLIP_VISION_L14", "CLIP_TEXT_L14", "MINILM_L6", "EncoderConfig",
           "clip_configs_from_dir", "bert_config_from_dir", "check_supported", "vit_patch_kpad", "param_specs", "vit_flops_per_image",
           "text_flops_per_sequence"]
