"""Text questions into the frame memory's space: CLIP's text tower over libvidmem (csrc/encoder.hip vm_text_encode).

Reference call site this stands in for: ``HybridRetriever._vector_search_chunks(session, query: str)``
(src/pipeline/retriever_hybrid.py:284-306) embeds the question with ``aembed_query(query)`` and ranks the stored chunk
embeddings by cosine.  Here the stored rows are CLIP image embeddings (``encoder.arch: clip_l14_336_joint``: the
768-d projected image embedding) and ``HipTextEmbedder.aembed_query`` puts a question into the same joint space.

  * ``TextEncoder``          token ids -> [B, out_dim] 16-bit embeddings (host validation, then one device call)
  * ``HipTextEmbedder``      ``async aembed_query(str)`` / ``aembed_documents(list[str])`` over a tokenizer callable
  * ``clip_tokenizer``       ``transformers.CLIPTokenizer`` from LOCAL vocab.json / merges.txt files
  * ``clip_weights_from_state_dict``  a ``transformers.CLIPModel`` state dict -> (vision, text) arrays of this package
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .memory import _torch_dtype


def _text_weight_order(spec: Dict) -> List[str]:
    names = ["tok_emb", "pos", "ln_g", "ln_b", "proj_w"]
    for l in range(spec["layers"]):
        names += [f"l{l}.{n}" for n in ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ln2_g", "ln2_b",
                                        "fc1_w", "fc1_b", "fc2_w", "fc2_b")]
    return names


_MATRICES = ("proj_w", "qkv_w", "fc1_w", "fc2_w")   # stored in the tower's 16-bit type; tok_emb / pos stay fp32


def pooled_positions(ids: np.ndarray, eot_id: int) -> np.ndarray:
    """Row each sequence is pooled at: the first position whose id is ``eot_id``, 0 when there is none
    (transformers' CLIPTextTransformer for ``eos_token_id != 2``; the device computes the same in vm_text_encode)."""
    ids = np.asarray(ids)
    hit = ids == eot_id
    return np.where(hit.any(axis=1), hit.argmax(axis=1), 0).astype(np.int64)


def validate_ids(ids: np.ndarray, vocab: int, eot_id: int, context: int) -> np.ndarray:
    """Host checks in front of any launch: int ids in [0, vocab), 1 <= T <= context, an EOT in every sequence.
    Returns each sequence's EOT position."""
    ids = np.asarray(ids)
    if ids.ndim != 2 or ids.shape[0] < 1 or not 1 <= ids.shape[1] <= context:
        raise ValueError(f"token ids must be [B, T] with B >= 1 and 1 <= T <= {context}, got {ids.shape}")
    if not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"token ids must be integers, got {ids.dtype}")
    if ids.min() < 0 or ids.max() >= vocab:
        raise ValueError(f"token id out of range [0, {vocab}): min {int(ids.min())}, max {int(ids.max())}")
    has_eot = (ids == eot_id).any(axis=1)
    if not has_eot.all():
        raise ValueError(f"sequence(s) {np.flatnonzero(~has_eot)[:8].tolist()} have no EOT token ({eot_id})")
    return pooled_positions(ids, eot_id)


class TextEncoder:
    """Token ids -> (L2-normalised) 16-bit text embeddings, everything on the device."""

    def __init__(self, spec: Dict, weights: Dict[str, np.ndarray], dtype: str = "f16", device: int = 0):
        self.spec = dict(spec)
        self.ctx = _lib.Context.get(device)
        self.L = self.ctx.L
        self.device = torch.device("cuda", device)
        self.dtype_name = dtype
        self.dtype = _torch_dtype(dtype)
        self.vocab, self.context, self.eot_id = int(spec["vocab"]), int(spec["context"]), int(spec["eot_id"])
        desc = _lib.TextEncoderDesc(
            vocab=self.vocab, context=self.context, hidden=spec["hidden"], layers=spec["layers"], heads=spec["heads"],
            mlp=spec["mlp"], act=_lib.VM_ACT_QUICK_GELU if spec["act"] == "quick_gelu" else _lib.VM_ACT_GELU,
            proj_dim=int(spec.get("proj_dim", 0)), eot_id=self.eot_id, dtype=_lib.DTYPES[dtype],
            ln_eps=float(spec["ln_eps"]))
        staged, ptrs = [], []
        for name in _text_weight_order(spec):
            arr = weights.get(name)
            if arr is None:
                ptrs.append(None)
                continue
            t = torch.as_tensor(np.asarray(arr), dtype=torch.float32)
            if name.split(".")[-1] in _MATRICES:
                t = t.to(self.dtype)
            t = t.to(self.device).contiguous()
            staged.append(t)
            ptrs.append(t.data_ptr())
        arr_t = (C.c_void_p * len(ptrs))(*[C.c_void_p(p) if p else C.c_void_p(0) for p in ptrs])
        h = C.c_void_p()
        torch.cuda.synchronize(self.device)  # uploads done before the library's device-to-device copies
        self.ctx.check(self.L.vm_text_encoder_create(self.ctx.handle, C.byref(desc), arr_t, len(ptrs), C.byref(h)))
        torch.cuda.synchronize(self.device)
        del staged
        self.handle = h
        self.out_dim = int(self.L.vm_text_encoder_out_dim(h))
        self._ws = None

    def close(self):
        if getattr(self, "handle", None):
            self.L.vm_text_encoder_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(self.L.vm_text_encode_workspace_bytes(self.handle, int(B), int(T)))

    def encode_device(self, ids: torch.Tensor, l2_normalise: bool = True, out_flags: Optional[torch.Tensor] = None,
                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """vm_text_encode on device int32 [B, T] ids as they are: no host check, no trimming, no synchronisation
        (capturable).  Ids out of range are clamped on the device and reported in ``out_flags`` (int32 [B])."""
        if ids.dtype != torch.int32 or ids.dim() != 2 or ids.device != self.device:
            raise ValueError(f"ids must be int32 [B, T] on {self.device}")
        ids = ids.contiguous()
        B, T = ids.shape
        need = self.workspace_bytes(B, T)
        if need == 0:
            raise ValueError(f"T = {T} outside 1..{self.context}")
        if workspace is None:
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            workspace = self._ws
        elif workspace.numel() < need:
            raise ValueError(f"caller-owned text workspace {workspace.numel()} < {need} bytes")
        out = torch.empty((B, self.out_dim), dtype=self.dtype, device=self.device)
        flags = C.c_void_p(out_flags.data_ptr()) if out_flags is not None else None
        self.ctx.check(self.L.vm_text_encode(self.handle, C.c_void_p(ids.data_ptr()), B, T, C.c_void_p(out.data_ptr()),
                                             1 if l2_normalise else 0, flags, C.c_void_p(workspace.data_ptr()),
                                             workspace.numel(), _lib.current_stream_ptr()))
        ids.record_stream(torch.cuda.current_stream())
        return out

    def encode_ids(self, ids, l2_normalise: bool = True, trim: bool = True) -> torch.Tensor:
        """[B, T] token ids (host array, list or tensor) -> [B, out_dim].  Validated on the host first (ValueError on
        an id outside [0, vocab) or a sequence without EOT); ``trim``: run only the batch's longest eot + 1 columns
        (the pooled rows do not depend on anything behind their EOT)."""
        a = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        if a.ndim == 1:
            a = a[None]
        eot = validate_ids(a, self.vocab, self.eot_id, self.context)
        if trim:
            a = a[:, : int(eot.max()) + 1]
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
        return self.encode_device(t, l2_normalise)


def clip_tokenizer(directory: str):
    """``transformers.CLIPTokenizer`` built from LOCAL ``vocab.json`` and ``merges.txt`` in ``directory`` (nothing is
    fetched; no vocabulary ships with this package).  Returned as a callable ``str -> list[int]`` with BOS / EOT."""
    from transformers import CLIPTokenizer   # lazy: only this helper needs transformers
    tok = CLIPTokenizer(os.path.join(directory, "vocab.json"), os.path.join(directory, "merges.txt"))

    def encode(text: str) -> List[int]:
        return list(tok(text)["input_ids"])
    encode.tokenizer = tok
    return encode


class HipTextEmbedder:
    """The reference's embedder object for questions: ``async aembed_query(str) -> List[float]`` in the joint space of
    a ``clip_l14_336_joint`` frame memory.  ``tokenizer``: any callable ``str -> list[int]`` that ends a sequence with
    the EOT id (``clip_tokenizer``); sequences longer than the context are cut to it with the EOT kept last, as CLIP
    does."""

    def __init__(self, text_encoder: TextEncoder, tokenizer: Callable[[str], Sequence[int]]):
        self.encoder = text_encoder
        self.tokenizer = tokenizer
        self.out_dim = text_encoder.out_dim

    def token_ids(self, texts: Sequence[str]) -> np.ndarray:
        ctx, eot = self.encoder.context, self.encoder.eot_id
        seqs = []
        for s in texts:
            ids = [int(i) for i in self.tokenizer(s)]
            if len(ids) > ctx:
                ids = ids[: ctx - 1] + [eot]
            seqs.append(ids)
        T = max(len(s) for s in seqs)
        out = np.full((len(seqs), T), eot, dtype=np.int64)   # padding behind the EOT: never read by the pooled row
        for i, s in enumerate(seqs):
            out[i, : len(s)] = s
        return out

    def embed_tensor(self, texts: Sequence[str]) -> torch.Tensor:
        return self.encoder.encode_ids(self.token_ids(texts))

    async def aembed_documents(self, texts: List[str]) -> List[List[float]]:
        if not texts:
            return []
        return self.embed_tensor(texts).float().cpu().tolist()

    async def aembed_query(self, text: str) -> List[float]:
        return (await self.aembed_documents([text]))[0]


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def _np(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().to(torch.float32).cpu().numpy()
    return np.asarray(x, dtype=np.float32)


def _layers(sd, prefix: str, out: Dict[str, np.ndarray]) -> None:
    l = 0
    while f"{prefix}.encoder.layers.{l}.layer_norm1.weight" in sd:
        p = f"{prefix}.encoder.layers.{l}."
        g = lambda n: _np(sd[p + n])
        out[f"l{l}.ln1_g"], out[f"l{l}.ln1_b"] = g("layer_norm1.weight"), g("layer_norm1.bias")
        out[f"l{l}.qkv_w"] = np.concatenate([g(f"self_attn.{n}_proj.weight") for n in "qkv"], axis=0)
        out[f"l{l}.qkv_b"] = np.concatenate([g(f"self_attn.{n}_proj.bias") for n in "qkv"], axis=0)
        out[f"l{l}.proj_w"], out[f"l{l}.proj_b"] = g("self_attn.out_proj.weight"), g("self_attn.out_proj.bias")
        out[f"l{l}.ln2_g"], out[f"l{l}.ln2_b"] = g("layer_norm2.weight"), g("layer_norm2.bias")
        out[f"l{l}.fc1_w"], out[f"l{l}.fc1_b"] = g("mlp.fc1.weight"), g("mlp.fc1.bias")
        out[f"l{l}.fc2_w"], out[f"l{l}.fc2_b"] = g("mlp.fc2.weight"), g("mlp.fc2.bias")
        l += 1


def clip_weights_from_state_dict(sd) -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """A ``transformers.CLIPModel`` state dict (``vision_model.*``, ``visual_projection``, ``text_model.*``,
    ``text_projection``) -> (vision weights of FrameEncoder, text weights of TextEncoder), fp32 arrays named as in
    synthetic.encoder_weight_shapes / text_encoder_weight_shapes.  q / k / v are concatenated in that order; the patch
    conv [H, 3, p, p] becomes [H, 3*p*p] in the k order c*p*p + py*p + px.  Either half is {} when its keys are absent."""
    vision: Dict[str, np.ndarray] = {}
    text: Dict[str, np.ndarray] = {}
    if "vision_model.embeddings.patch_embedding.weight" in sd:
        v = "vision_model."
        pw = _np(sd[v + "embeddings.patch_embedding.weight"])
        vision["patch_w"] = pw.reshape(pw.shape[0], -1)
        vision["patch_b"] = np.zeros(pw.shape[0], np.float32)   # CLIP's patch conv has no bias
        vision["cls"] = _np(sd[v + "embeddings.class_embedding"])
        vision["pos"] = _np(sd[v + "embeddings.position_embedding.weight"])
        vision["pre_ln_g"], vision["pre_ln_b"] = _np(sd[v + "pre_layrnorm.weight"]), _np(sd[v + "pre_layrnorm.bias"])
        vision["ln_g"], vision["ln_b"] = _np(sd[v + "post_layernorm.weight"]), _np(sd[v + "post_layernorm.bias"])
        if "visual_projection.weight" in sd:
            vision["proj_w"] = _np(sd["visual_projection.weight"])
        _layers(sd, "vision_model", vision)
    if "text_model.embeddings.token_embedding.weight" in sd:
        t = "text_model."
        text["tok_emb"] = _np(sd[t + "embeddings.token_embedding.weight"])
        text["pos"] = _np(sd[t + "embeddings.position_embedding.weight"])
        text["ln_g"], text["ln_b"] = _np(sd[t + "final_layer_norm.weight"]), _np(sd[t + "final_layer_norm.bias"])
        if "text_projection.weight" in sd:
            text["proj_w"] = _np(sd["text_projection.weight"])
        _layers(sd, "text_model", text)
    return vision, text


def load_weight_file(path: str, half: str) -> Dict[str, np.ndarray]:
    """Named fp32 arrays from ``.npz`` (this package's names) or ``.safetensors`` (a CLIPModel state dict, mapped by
    clip_weights_from_state_dict, or already this package's names).  half: "vision" | "text"."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file   # torch: also reads bf16 checkpoints
        sd = load_file(path)
        if any(k.startswith(("vision_model.", "text_model.")) for k in sd):
            vision, text = clip_weights_from_state_dict(sd)
            return vision if half == "vision" else text
        return {k: _np(v) for k, v in sd.items()}
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}
