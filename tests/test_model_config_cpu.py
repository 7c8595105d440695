"""Encoder geometries read from a checkpoint's ``config.json`` (app/encoders/weights.py:
clip_configs_from_dir, bert_config_from_dir, check_supported): the values of each field for the
CLIP checkpoints the drop-in runs (ViT-B/32, B/16, L/14), transformers' defaults for missing keys,
and a ValueError that names the limit for everything the native encoders do not run. No GPU."""
from __future__ import annotations

import json
import os

import pytest

from app.encoders.weights import (CLIP_TEXT_B32, CLIP_TEXT_L14, CLIP_VISION_B16, CLIP_VISION_B32, CLIP_VISION_L14,
                                  MINILM_L6, MSMARCO_MINILM_L6_CE, EncoderConfig, bert_config_from_dir,
                                  check_supported, clip_configs_from_dir, param_specs)


def _write(d, cfg, name="config.json"):
    os.makedirs(os.path.dirname(os.path.join(d, name)), exist_ok=True)
    with open(os.path.join(d, name), "w") as f:
        json.dump(cfg, f)
    return str(d)


B16 = {"model_type": "clip", "projection_dim": 512,
       "vision_config": {"hidden_size": 768, "intermediate_size": 3072, "num_hidden_layers": 12,
                         "num_attention_heads": 12, "image_size": 224, "patch_size": 16, "hidden_act": "quick_gelu",
                         "layer_norm_eps": 1e-5},
       "text_config": {"hidden_size": 512, "intermediate_size": 2048, "num_hidden_layers": 12,
                       "num_attention_heads": 8, "max_position_embeddings": 77, "vocab_size": 49408,
                       "hidden_act": "quick_gelu", "eos_token_id": 49407}}
L14 = {"model_type": "clip", "projection_dim": 768,
       "vision_config": {"hidden_size": 1024, "intermediate_size": 4096, "num_hidden_layers": 24,
                         "num_attention_heads": 16, "image_size": 224, "patch_size": 14, "hidden_act": "quick_gelu"},
       "text_config": {"hidden_size": 768, "intermediate_size": 3072, "num_hidden_layers": 12,
                       "num_attention_heads": 12, "max_position_embeddings": 77, "vocab_size": 49408,
                       "hidden_act": "quick_gelu", "eos_token_id": 49407}}


def _l14(**vision):
    c = json.loads(json.dumps(L14))
    c["vision_config"].update(vision)
    return c


def test_clip_b32_defaults(tmp_path):
    """Empty sub-configs: every field is transformers' default, the B/32 constants."""
    v, t = clip_configs_from_dir(_write(tmp_path, {"vision_config": {}, "text_config": {}}))
    assert v == CLIP_VISION_B32
    assert t == CLIP_TEXT_B32
    assert (v.kind, v.hidden, v.layers, v.heads, v.intermediate, v.proj_dim, v.image_size, v.patch_size, v.act,
            v.ln_eps) == (1, 768, 12, 12, 3072, 512, 224, 32, 0, 1e-5)
    assert (t.kind, t.hidden, t.layers, t.heads, t.intermediate, t.max_positions, t.vocab, t.proj_dim, t.act,
            t.eos_token_id, t.ln_eps) == (2, 512, 12, 8, 2048, 77, 49408, 512, 0, 49407, 1e-5)
    # no sub-configs at all: the same
    assert clip_configs_from_dir(_write(tmp_path / "bare", {})) == (CLIP_VISION_B32, CLIP_TEXT_B32)


def test_clip_b16(tmp_path):
    v, t = clip_configs_from_dir(_write(tmp_path, B16))
    assert v == CLIP_VISION_B16
    assert (v.hidden, v.layers, v.heads, v.intermediate, v.proj_dim, v.image_size, v.patch_size) == \
        (768, 12, 12, 3072, 512, 224, 16)
    assert t == CLIP_TEXT_B32


def test_clip_l14(tmp_path):
    v, t = clip_configs_from_dir(_write(tmp_path, L14))
    assert v == CLIP_VISION_L14
    assert (v.kind, v.hidden, v.layers, v.heads, v.intermediate, v.proj_dim, v.image_size, v.patch_size, v.act,
            v.ln_eps) == (1, 1024, 24, 16, 4096, 768, 224, 14, 0, 1e-5)
    assert t == CLIP_TEXT_L14
    assert (t.kind, t.hidden, t.layers, t.heads, t.intermediate, t.max_positions, t.vocab, t.proj_dim, t.act,
            t.eos_token_id) == (2, 768, 12, 12, 3072, 77, 49408, 768, 0, 49407)


def test_clip_legacy_eos_and_gelu(tmp_path):
    """eos_token_id 2 (the configs of the original openai uploads) pools at argmax(ids): -1;
    hidden_act gelu is the erf epilogue."""
    c = json.loads(json.dumps(B16))
    c["text_config"]["eos_token_id"] = 2
    c["text_config"]["hidden_act"] = "gelu"
    v, t = clip_configs_from_dir(_write(tmp_path, c))
    assert t.eos_token_id == -1
    assert t.act == 1 and v.act == 0


@pytest.mark.parametrize("cfg,words", [
    (_l14(image_size=336), ("image_size 336", "224")),
    (_l14(hidden_size=1280, num_attention_heads=16), ("hidden size 1280", "1024")),
    (_l14(hidden_act="gelu_new"), ("hidden_act", "gelu_new")),
    (_l14(patch_size=15), ("patch_size 15", "divide")),
    (_l14(num_attention_heads=8), ("head size", "32 or 64")),
    (dict(L14, projection_dim=200), ("projection_dim 200", "128")),
    (dict(L14, model_type="siglip"), ("model_type", "siglip")),
], ids=["l14_336", "hidden_1280", "gelu_new", "patch_15", "head_128", "proj_200", "siglip"])
def test_clip_refusals_name_the_limit(tmp_path, cfg, words):
    d = _write(tmp_path, cfg)
    with pytest.raises(ValueError) as e:
        clip_configs_from_dir(d)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert d in str(e.value)  # the model is named


def test_check_supported_token_limit():
    """(image_size / patch_size)^2 + 1 <= 512, apart from the 224-pixel rule."""
    with pytest.raises(ValueError, match="image_size 336"):
        check_supported(EncoderConfig(kind=1, hidden=1024, layers=24, heads=16, intermediate=4096, proj_dim=768,
                                      image_size=336, patch_size=14), "openai/clip-vit-large-patch14-336")
    with pytest.raises(ValueError, match="785 tokens"):
        check_supported(EncoderConfig(kind=1, hidden=768, layers=12, heads=12, intermediate=3072, proj_dim=512,
                                      image_size=224, patch_size=8))
    for c in (CLIP_VISION_B32, CLIP_VISION_B16, CLIP_VISION_L14, CLIP_TEXT_B32, CLIP_TEXT_L14, MINILM_L6,
              MSMARCO_MINILM_L6_CE):
        assert check_supported(c) is c


MINILM_L12 = {"model_type": "bert", "hidden_size": 384, "num_hidden_layers": 12, "num_attention_heads": 12,
              "intermediate_size": 1536, "max_position_embeddings": 512, "vocab_size": 30522,
              "layer_norm_eps": 1e-12, "hidden_act": "gelu"}
MEAN_POOL = {"word_embedding_dimension": 384, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
             "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}


def test_bert_twelve_layers(tmp_path):
    d = _write(tmp_path, MINILM_L12)
    c = bert_config_from_dir(d, 3)
    assert c.layers == 12
    assert c == EncoderConfig(kind=3, hidden=384, layers=12, heads=12, intermediate=1536, max_positions=512,
                              vocab=30522, act=1, ln_eps=1e-12)
    _write(tmp_path, MEAN_POOL, "1_Pooling/config.json")
    _write(tmp_path, [{"idx": 0, "type": "sentence_transformers.models.Transformer"},
                      {"idx": 1, "type": "sentence_transformers.models.Pooling"},
                      {"idx": 2, "type": "sentence_transformers.models.Normalize"}], "modules.json")
    assert bert_config_from_dir(d, 3) == c
    # the L6 checkpoint's values give the constant
    assert bert_config_from_dir(_write(tmp_path / "l6", dict(MINILM_L12, num_hidden_layers=6)), 3) == MINILM_L6


def test_bert_cross_encoder_labels(tmp_path):
    ce = dict(MINILM_L12, num_hidden_layers=6, id2label={"0": "LABEL_0"}, label2id={"LABEL_0": 0})
    assert bert_config_from_dir(_write(tmp_path / "a", ce), 4) == MSMARCO_MINILM_L6_CE
    assert bert_config_from_dir(_write(tmp_path / "b", dict(MINILM_L12, num_labels=3)), 4).proj_dim == 3


def test_bert_refusals(tmp_path):
    d = _write(tmp_path / "cls", MINILM_L12)
    _write(d, dict(MEAN_POOL, pooling_mode_cls_token=True, pooling_mode_mean_tokens=False), "1_Pooling/config.json")
    with pytest.raises(ValueError, match="pooling_mode_cls_token.*mean pooling"):
        bert_config_from_dir(d, 3)
    d = _write(tmp_path / "max", MINILM_L12)
    _write(d, dict(MEAN_POOL, pooling_mode_max_tokens=True), "1_Pooling/config.json")
    with pytest.raises(ValueError, match="pooling_mode_max_tokens"):
        bert_config_from_dir(d, 3)
    d = _write(tmp_path / "dense", MINILM_L12)
    _write(d, [{"idx": 0, "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "type": "sentence_transformers.models.Dense"}], "modules.json")
    with pytest.raises(ValueError, match="Dense"):
        bert_config_from_dir(d, 3)
    with pytest.raises(ValueError, match="model_type 'mpnet'"):
        bert_config_from_dir(_write(tmp_path / "mpnet", dict(MINILM_L12, model_type="mpnet")), 3)
    with pytest.raises(ValueError, match="model_type 'roberta'"):
        bert_config_from_dir(_write(tmp_path / "roberta", dict(MINILM_L12, model_type="roberta")), 4)
    with pytest.raises(ValueError, match="hidden size 1280"):
        bert_config_from_dir(_write(tmp_path / "wide", dict(MINILM_L12, hidden_size=1280, num_attention_heads=20)), 3)


def test_param_specs_l14_patch_weight():
    specs = {n: s for n, s, _ in param_specs(CLIP_VISION_L14)}
    assert specs["vision_model.embeddings.patch_embedding.weight"] == (1024, 3, 14, 14)
    assert specs["vision_model.embeddings.position_embedding.weight"] == (257, 1024)
    assert specs["visual_projection.weight"] == (768, 1024)
    assert sum(1 for n in specs if ".layers.23." in n) == 16
    b16 = {n: s for n, s, _ in param_specs(CLIP_VISION_B16)}
    assert b16["vision_model.embeddings.position_embedding.weight"] == (197, 768)


def test_model_classes_refuse_before_loading(tmp_path, monkeypatch):
    """The drop-in classes read the geometry first: an unsupported checkpoint raises ValueError from
    check_supported, not a shape mismatch from the weight loader (there are no weights here)."""
    from app.encoders.models import ClipModel, MiniLMSentenceModel

    d = _write(tmp_path / "clip336", _l14(image_size=336))
    with pytest.raises(ValueError, match="image_size 336"):
        ClipModel(d)
    d = _write(tmp_path / "mpnet", dict(MINILM_L12, model_type="mpnet"))
    with open(os.path.join(d, "vocab.txt"), "w") as f:
        f.write("[PAD]\n[UNK]\n[CLS]\n[SEP]\n")
    with pytest.raises(ValueError, match="model_type 'mpnet'"):
        MiniLMSentenceModel(d)
