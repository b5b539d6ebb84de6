"""CPU: the text tower's host side - checkpoint mapping, pooled-row rule, host validation, tokenizer, config defaults -
and the CPU restatement (tests/text_ref.py) pinned against transformers' CLIP models built from config objects."""
import json
import os

import numpy as np
import pytest
import torch

from tests import text_ref as TR


def _tiny_clip(eos_token_id=99):
    from transformers import CLIPConfig, CLIPModel
    torch.manual_seed(0)
    cfg = CLIPConfig(
        text_config=dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                         num_attention_heads=2, max_position_embeddings=16, hidden_act="quick_gelu",
                         layer_norm_eps=1e-5, eos_token_id=eos_token_id, bos_token_id=0, pad_token_id=1),
        vision_config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                           image_size=32, patch_size=8, hidden_act="quick_gelu", layer_norm_eps=1e-5),
        projection_dim=48)
    cfg._attn_implementation = "eager"
    m = CLIPModel(cfg).eval()
    with torch.no_grad():   # non-trivial LayerNorm and bias values, so a swapped name cannot pass
        for n, p in m.named_parameters():
            if "norm" in n or n.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
    return m


def test_clip_state_dict_mapping_shapes_and_forward():
    from vidmem import synthetic
    from vidmem.text import clip_weights_from_state_dict
    from oracle import vit_ref as V
    m = _tiny_clip()
    vision, text = clip_weights_from_state_dict(m.state_dict())
    vspec = V.tiny_spec(image=32, patch=8, hidden=64, layers=2, heads=2, mlp=128, act="quick_gelu", pre_ln=True,
                        patch_bias=False, ln_eps=1e-5, proj_dim=48)
    tspec = TR.tiny_text_spec(hidden=64, layers=2, heads=2, mlp=128, vocab=100, context=16, proj_dim=48, eot_id=99)
    want_v = synthetic.encoder_weight_shapes(vspec)
    want_t = synthetic.text_encoder_weight_shapes(tspec)
    assert {k: v.shape for k, v in vision.items()} == want_v
    assert {k: v.shape for k, v in text.items()} == want_t
    assert all(v.dtype == np.float32 for v in list(vision.values()) + list(text.values()))

    g = torch.Generator().manual_seed(1)
    ids = torch.randint(2, 99, (3, 16), generator=g)
    ids[0, 5] = 99
    ids[1, 15] = 99
    ids[2, 0] = 99
    px = torch.randn(2, 3, 32, 32, generator=g)
    with torch.no_grad():
        out = m(input_ids=ids, pixel_values=px)
    # transformers returns the L2-normalised embeddings from CLIPModel.forward
    got_t = TR.text_forward_ref(tspec, text, ids.numpy(), quant=None)
    got_v = V.vit_forward_ref(vspec, vision, px.numpy(), quant=None)
    assert np.abs(got_t - out.text_embeds.numpy()).max() <= 1e-5
    assert np.abs(got_v - out.image_embeds.numpy()).max() <= 1e-5


@pytest.mark.parametrize("eos", [99, 2])
def test_pooled_position_rule_matches_transformers(eos):
    """eos_token_id != 2: first EOT; the legacy == 2 rule (argmax of the ids) agrees on sequences containing EOT, the
    largest id.  Checked through the pooled text embedding of transformers against our restatement, which pools by
    text.pooled_positions."""
    from vidmem.text import pooled_positions
    tspec = TR.tiny_text_spec(hidden=64, layers=1, heads=1, mlp=128, vocab=100, context=16, proj_dim=32, eot_id=99)
    from vidmem import synthetic
    w = synthetic.text_encoder_weights(tspec, seed=3, std=0.2)
    rng = np.random.default_rng(0)
    ids = rng.integers(2, 99, size=(6, 16))
    for i, p in enumerate([0, 1, 7, 15, 3, 3]):
        ids[i, p] = 99
    ids[5, 9] = 99   # two EOTs: the first one counts
    assert pooled_positions(ids, 99).tolist() == [0, 1, 7, 15, 3, 3]
    want = TR.hf_text_embeds(tspec, w, ids, eos_token_id=eos)
    got = TR.text_forward_ref(tspec, w, ids, quant=None)
    assert np.abs(got - want).max() <= 1e-5
    assert pooled_positions(np.array([[5, 6, 7]]), 99).tolist() == [0]   # no EOT: row 0


def test_host_validation_raises_before_any_launch():
    from vidmem.text import validate_ids
    ok = np.array([[0, 5, 999, 1, 1]])
    assert validate_ids(ok, 1000, 999, 77).tolist() == [2]
    with pytest.raises(ValueError, match="out of range"):
        validate_ids(np.array([[0, 1000, 999]]), 1000, 999, 77)
    with pytest.raises(ValueError, match="out of range"):
        validate_ids(np.array([[-1, 3, 999]]), 1000, 999, 77)
    with pytest.raises(ValueError, match="no EOT"):
        validate_ids(np.array([[0, 3, 4], [0, 999, 1]]), 1000, 999, 77)
    with pytest.raises(ValueError):
        validate_ids(np.zeros((1, 78), np.int64) + 999, 1000, 999, 77)
    with pytest.raises(ValueError):
        validate_ids(np.array([[0.5, 999.0]]), 1000, 999, 77)


def test_text_encoder_encode_ids_validates_without_a_device():
    """TextEncoder.encode_ids runs the host checks before it touches the library (the object is not constructed: no
    device is needed to show that a bad id never reaches a launch)."""
    from vidmem.text import TextEncoder
    enc = TextEncoder.__new__(TextEncoder)
    enc.vocab, enc.eot_id, enc.context = 1000, 999, 77

    def boom(*a, **k):
        raise AssertionError("launched")
    enc.encode_device = boom
    with pytest.raises(ValueError):
        enc.encode_ids([[0, 1000, 999]])
    with pytest.raises(ValueError):
        enc.encode_ids([[0, 1, 2]])


def _tiny_vocab(d):
    vocab = {"<|startoftext|>": 0, "<|endoftext|>": 1}
    for ch in "abcdefghijklmnopqrstuvwxyz":
        vocab[ch] = len(vocab)
        vocab[ch + "</w>"] = len(vocab)
    for tok in ("th", "the</w>", "gl", "glo", "glov", "glove", "gloves</w>"):
        vocab[tok] = len(vocab)
    merges = ["#version: 0.2", "t h", "th e</w>", "g l", "gl o", "glo v", "glov e", "glove s</w>"]
    with open(os.path.join(d, "vocab.json"), "w") as f:
        json.dump(vocab, f)
    with open(os.path.join(d, "merges.txt"), "w") as f:
        f.write("\n".join(merges) + "\n")
    return vocab


def test_clip_tokenizer_on_a_local_vocab(tmp_path):
    from vidmem.text import clip_tokenizer
    vocab = _tiny_vocab(str(tmp_path))
    tok = clip_tokenizer(str(tmp_path))
    ids = tok("The gloves")
    assert ids == [vocab["<|startoftext|>"], vocab["the</w>"], vocab["gloves</w>"], vocab["<|endoftext|>"]]


def test_text_embedder_truncates_with_eot_last():
    from vidmem.text import HipTextEmbedder

    class FakeEnc:
        context, eot_id, out_dim = 8, 999, 16
    emb = HipTextEmbedder(FakeEnc(), lambda s: [0] + [5] * len(s) + [999])
    ids = emb.token_ids(["abcdefghijkl", "ab"])
    assert ids.shape == (2, 8)
    assert ids[0].tolist() == [0, 5, 5, 5, 5, 5, 5, 999]
    assert ids[1, :4].tolist() == [0, 5, 5, 999]


def test_text_encoder_config_defaults_build_nothing():
    from vidmem import config as cfgmod
    from vidmem.extractor import build_text_embedder
    assert cfgmod.TEXT_ENCODER_DEFAULTS == {"arch": None, "dtype": "f16", "weights": None, "seed": 42, "device": 0,
                                            "tokenizer": None}
    assert build_text_embedder(cfgmod.from_dict({})) is None
    assert build_text_embedder(cfgmod.from_dict({"text_encoder": {"dtype": "bf16"}})) is None
    assert "text_encoder" not in cfgmod.from_dict({}).dict()   # configs that do not name it are unchanged


def test_specs():
    from vidmem import specs
    t = specs.TEXT_SPECS["clip_l14_text"]
    assert (t["vocab"], t["context"], t["hidden"], t["layers"], t["heads"], t["mlp"], t["proj_dim"], t["eot_id"]) == \
        (49408, 77, 768, 12, 12, 3072, 768, 49407)
    j = specs.SPECS["clip_l14_336_joint"]
    assert j["proj_dim"] == 768 and {k: v for k, v in j.items() if k not in ("arch", "proj_dim")} == \
        {k: v for k, v in specs.CLIP_L14_336.items() if k not in ("arch", "proj_dim")}
    assert specs.CLIP_L14_336["proj_dim"] == 0
    assert 12.5e9 < specs.text_flops_per_sequence(t) < 13.5e9


def test_safetensors_weights_load(tmp_path):
    from safetensors.torch import save_file
    from vidmem.text import clip_weights_from_state_dict, load_weight_file
    m = _tiny_clip()
    sd = {k: v.contiguous() for k, v in m.state_dict().items()}
    path = str(tmp_path / "clip.safetensors")
    save_file(sd, path)
    vision, text = clip_weights_from_state_dict(sd)
    lv, lt = load_weight_file(path, "vision"), load_weight_file(path, "text")
    assert set(lv) == set(vision) and set(lt) == set(text)
    assert all(np.array_equal(lt[k], text[k]) for k in text)


def test_similarity_rejects_a_mismatched_embedder():
    from types import SimpleNamespace
    from vidmem import _lib
    from vidmem.similarity import HipVectorSearch
    mem = SimpleNamespace(dim=1024)
    with pytest.raises(ValueError, match="memory.dim"):
        HipVectorSearch(mem, SimpleNamespace(out_dim=768), SimpleNamespace(top_k_chunks=3), score_mode=_lib.VM_SCORE_RAW)
    HipVectorSearch(mem, SimpleNamespace(), SimpleNamespace(top_k_chunks=3), score_mode=_lib.VM_SCORE_RAW)  # no out_dim
