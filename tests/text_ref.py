"""CPU restatement of the text tower (test infrastructure, NOT product code), the text-side counterpart of
oracle/vit_ref.py: pinned against ``transformers.CLIPTextModelWithProjection`` built FROM A CONFIG OBJECT (never
from_pretrained) in tests/test_text_cpu.py, and used by tests/test_text_gpu.py as the fp32 answer and as the 16-bit
rounding floor of the device path.

Modes:
  quant=None          fp32 forward
  quant="f16"/"bf16"  the same forward rounded to 16 bit at exactly the points where vm_text_encode stores a 16-bit
                      value (oracle.vit_ref.POINTS minus the patch ones; the two residual-branch outputs always fp16)
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from oracle import vit_ref as V


def tiny_text_spec(hidden=256, layers=2, heads=None, mlp=None, vocab=1000, context=77, proj_dim=128, act="quick_gelu",
                   eot_id=None, ln_eps=1e-5):
    """A small tower of the CLIP text family (the kernels need hidden % 256 == 0 and head dim 64)."""
    return dict(arch="tiny_text", vocab=vocab, context=context, hidden=hidden, layers=layers,
                heads=heads or hidden // 64, mlp=mlp or 4 * hidden, act=act, ln_eps=ln_eps, proj_dim=proj_dim,
                eot_id=vocab - 1 if eot_id is None else eot_id)


def pooled_positions(ids, eot_id):
    ids = np.asarray(ids)
    hit = ids == eot_id
    return np.where(hit.any(axis=1), hit.argmax(axis=1), 0)


@torch.no_grad()
def text_forward_ref(spec: Dict, w: Dict[str, np.ndarray], ids, quant: Optional[str] = None, l2_normalise=True,
                     return_attn_ctx: bool = False):
    """ids: int [B, T].  Returns [B, out_dim] fp32 numpy (or, with return_attn_ctx, layer 0's attention context
    [B, T, H] before its 16-bit rounding)."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    q_ = V._rounder(quant)
    qw = lambda a: q_(t(a), "weights")
    H, heads, L = spec["hidden"], spec["heads"], spec["layers"]
    hd = H // heads
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    B, T = ids.shape
    x = t(w["tok_emb"])[ids] + t(w["pos"])[:T].unsqueeze(0)     # fp32 table + fp32 positions
    scale = 1.0 / math.sqrt(hd)
    causal = torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1)
    for l in range(L):
        p = lambda n: w[f"l{l}.{n}"]
        h = q_(V._layernorm(x, t(p("ln1_g")), t(p("ln1_b")), spec["ln_eps"]), "ln")
        qkv = q_(h @ qw(p("qkv_w")).T + t(p("qkv_b")), "qkv")
        q, k, v = qkv.split(H, dim=-1)
        q = q.reshape(B, T, heads, hd).transpose(1, 2)
        k = k.reshape(B, T, heads, hd).transpose(1, 2)
        v = v.reshape(B, T, heads, hd).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)) * scale
        s = s.masked_fill(causal, float("-inf"))
        s = s - s.max(dim=-1, keepdim=True).values
        e = torch.exp(s)
        den = e.sum(dim=-1, keepdim=True)
        ctx = ((q_(e, "probs") @ v) / den).transpose(1, 2).reshape(B, T, H)
        if return_attn_ctx:
            return ctx.numpy()
        ctx = q_(ctx, "ctx")
        x = x + q_(ctx @ qw(p("proj_w")).T + t(p("proj_b")), "proj_out")
        h = q_(V._layernorm(x, t(p("ln2_g")), t(p("ln2_b")), spec["ln_eps"]), "ln")
        a = q_(V._act(h @ qw(p("fc1_w")).T + t(p("fc1_b")), spec["act"]), "act")
        x = x + q_(a @ qw(p("fc2_w")).T + t(p("fc2_b")), "fc2_out")
    rows = torch.as_tensor(pooled_positions(ids.numpy(), spec["eot_id"]))
    pooled = V._layernorm(x[torch.arange(B), rows], t(w["ln_g"]), t(w["ln_b"]), spec["ln_eps"])
    if spec.get("proj_dim", 0):
        pooled = q_(pooled, "head_in") @ qw(w["proj_w"]).T
    if l2_normalise:
        n = torch.sqrt((pooled * pooled).sum(dim=-1, keepdim=True))
        pooled = pooled / torch.clamp(n, min=1e-12)
    return q_(pooled, "out").numpy()


def hf_text_config(spec: Dict, eos_token_id=None):
    from transformers import CLIPTextConfig
    return CLIPTextConfig(vocab_size=spec["vocab"], hidden_size=spec["hidden"], intermediate_size=spec["mlp"],
                          projection_dim=spec["proj_dim"], num_hidden_layers=spec["layers"],
                          num_attention_heads=spec["heads"], max_position_embeddings=spec["context"],
                          hidden_act=spec["act"], layer_norm_eps=spec["ln_eps"],
                          eos_token_id=spec["eot_id"] if eos_token_id is None else eos_token_id,
                          bos_token_id=0, pad_token_id=1, attn_implementation="eager")


def text_state_dict(w: Dict[str, np.ndarray], layers: int) -> Dict[str, torch.Tensor]:
    """Our named arrays -> CLIPTextModelWithProjection's state-dict names (the inverse of
    text.clip_weights_from_state_dict's text half)."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    sd = {"text_model.embeddings.token_embedding.weight": t(w["tok_emb"]),
          "text_model.embeddings.position_embedding.weight": t(w["pos"]),
          "text_model.final_layer_norm.weight": t(w["ln_g"]), "text_model.final_layer_norm.bias": t(w["ln_b"]),
          "text_projection.weight": t(w["proj_w"])}
    for l in range(layers):
        p = f"text_model.encoder.layers.{l}."
        H = w[f"l{l}.proj_w"].shape[0]
        qw, qb = t(w[f"l{l}.qkv_w"]), t(w[f"l{l}.qkv_b"])
        for i, n in enumerate("qkv"):
            sd[p + f"self_attn.{n}_proj.weight"] = qw[i * H:(i + 1) * H]
            sd[p + f"self_attn.{n}_proj.bias"] = qb[i * H:(i + 1) * H]
        for ours, theirs in (("ln1_g", "layer_norm1.weight"), ("ln1_b", "layer_norm1.bias"),
                             ("proj_w", "self_attn.out_proj.weight"), ("proj_b", "self_attn.out_proj.bias"),
                             ("ln2_g", "layer_norm2.weight"), ("ln2_b", "layer_norm2.bias"),
                             ("fc1_w", "mlp.fc1.weight"), ("fc1_b", "mlp.fc1.bias"),
                             ("fc2_w", "mlp.fc2.weight"), ("fc2_b", "mlp.fc2.bias")):
            sd[p + theirs] = t(w[f"l{l}.{ours}"])
    return sd


@torch.no_grad()
def hf_text_embeds(spec: Dict, w: Dict[str, np.ndarray], ids, eos_token_id=None, l2_normalise=True) -> np.ndarray:
    """transformers' CLIPTextModelWithProjection (built from a config, fp32) on our weights."""
    from transformers import CLIPTextModelWithProjection
    m = CLIPTextModelWithProjection(hf_text_config(spec, eos_token_id)).eval()
    missing, unexpected = m.load_state_dict(text_state_dict(w, spec["layers"]), strict=False)
    assert not [k for k in missing if "position_ids" not in k] and not unexpected, (missing, unexpected)
    out = m(input_ids=torch.as_tensor(np.asarray(ids), dtype=torch.long)).text_embeds
    if l2_normalise:
        out = out / out.norm(dim=-1, keepdim=True)
    return out.numpy()


def rel(a, b) -> np.ndarray:
    """Per-row relative L2 distance."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)
