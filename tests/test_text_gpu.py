"""GPU: the text tower (csrc/encoder.hip vm_text_encode) and the joint image spec, end to end into the retriever.

Parity bars are floor-derived, per embedding: the 16-bit device path cannot be closer to the fp32 model than a
restatement that rounds at the same storage points (tests/text_ref.py, oracle/vit_ref.py) - that restatement's
distance to transformers' fp32 output is the embedding's rounding FLOOR, and the device is held to FLOOR_SLACK x it.
Bit-identity properties: a sequence's embedding does not depend on its batch, on tokens behind its EOT, on T, or on
graph capture."""
import asyncio
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import vit_ref as V
from tests import text_ref as TR

pytestmark = pytest.mark.gpu

FLOOR_SLACK = 1.5
EOT_POSITIONS = [0, 1, 15, 16, 17, 76]


def _ids(spec, eots, seed, T=77):
    """[len(eots), T] ids: random non-EOT tokens, the EOT at the given positions, random tokens behind it."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, spec["vocab"] - 1, size=(len(eots), T))
    ids[ids == spec["eot_id"]] = 3
    for i, p in enumerate(eots):
        ids[i, p] = spec["eot_id"]
    return ids


def _encoder(spec, dtype, seed=5, std=0.02):
    from vidmem import synthetic
    from vidmem.text import TextEncoder
    w = synthetic.text_encoder_weights(spec, seed=seed, std=std)
    return TextEncoder(spec, w, dtype=dtype, device=0), w


def _check_floor(got, want32, floor, what):
    err = TR.rel(got, want32)
    ratio = err / floor
    print(f"{what}: err max {err.max():.3e} floor max {floor.max():.3e} ratio max {ratio.max():.3f} "
          f"mean {ratio.mean():.3f}")
    assert np.all(err <= FLOOR_SLACK * floor), (what, err.tolist(), floor.tolist())


@pytest.mark.parametrize("dtype,layers", [("f16", 2), ("bf16", 3)])
def test_tiny_text_tower_parity(dtype, layers):
    spec = TR.tiny_text_spec(hidden=256, layers=layers, vocab=1000, context=77, proj_dim=128)
    enc, w = _encoder(spec, dtype)
    rng = np.random.default_rng(11)
    eots = EOT_POSITIONS + rng.integers(0, 77, size=10).tolist()
    ids = _ids(spec, eots, seed=12)
    got = enc.encode_ids(ids).float().cpu().numpy()
    want32 = TR.hf_text_embeds(spec, w, ids)
    floor = TR.rel(TR.text_forward_ref(spec, w, ids, quant=dtype), want32)
    _check_floor(got, want32, floor, f"tiny text {dtype} L{layers}")


def test_clip_l14_text_parity_f16():
    from vidmem import specs
    spec = specs.CLIP_L14_TEXT
    enc, w = _encoder(spec, "f16")
    rng = np.random.default_rng(21)
    eots = EOT_POSITIONS + rng.integers(0, 77, size=4).tolist()
    ids = _ids(spec, eots, seed=22)
    got = enc.encode_ids(ids).float().cpu().numpy()
    want32 = TR.hf_text_embeds(spec, w, ids)
    floor = TR.rel(TR.text_forward_ref(spec, w, ids, quant="f16"), want32)
    _check_floor(got, want32, floor, "clip_l14_text f16")


@pytest.mark.parametrize("T", [1, 16, 17, 77])
def test_causal_attention_against_torch_causal_softmax(T):
    """1-layer tower, untrimmed T: the EOT rows sit before the end of most sequences, so keys behind them must be masked.
    Reference: torch.nn.functional.scaled_dot_product_attention(is_causal=True) in an fp32 restatement of the layer;
    a non-causal reference is far away wherever the pooled row has later keys (the mask matters)."""
    spec = TR.tiny_text_spec(hidden=256, layers=1, vocab=1000, context=77, proj_dim=128)
    enc, w = _encoder(spec, "f16", std=0.1)   # wide weights: peaked attention rows, so a wrong mask shows
    rng = np.random.default_rng(T)
    eots = sorted(set([0, T - 1] + rng.integers(0, T, size=6).tolist()))
    ids = _ids(spec, eots, seed=100 + T, T=T)
    got = enc.encode_device(torch.from_numpy(ids.astype(np.int32)).cuda()).float().cpu().numpy()
    want32 = _sdpa_forward(spec, w, ids, causal=True)
    floor = TR.rel(TR.text_forward_ref(spec, w, ids, quant="f16"), want32)
    _check_floor(got, want32, floor, f"causal T={T}")
    later = np.asarray(eots) < T - 1
    if later.any():
        wrong = _sdpa_forward(spec, w, ids, causal=False)
        assert np.all(TR.rel(wrong[later], want32[later]) > 3 * FLOOR_SLACK * floor[later])


@torch.no_grad()
def _sdpa_forward(spec, w, ids, causal):
    import torch.nn.functional as F
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    H, heads = spec["hidden"], spec["heads"]
    ids_t = torch.as_tensor(ids, dtype=torch.long)
    B, T = ids_t.shape
    x = t(w["tok_emb"])[ids_t] + t(w["pos"])[:T]
    for l in range(spec["layers"]):
        p = lambda n: t(w[f"l{l}.{n}"])
        h = F.layer_norm(x, (H,), p("ln1_g"), p("ln1_b"), spec["ln_eps"])
        qkv = F.linear(h, p("qkv_w"), p("qkv_b")).reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
        ctx = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], is_causal=causal)
        x = x + F.linear(ctx.transpose(1, 2).reshape(B, T, H), p("proj_w"), p("proj_b"))
        h = F.layer_norm(x, (H,), p("ln2_g"), p("ln2_b"), spec["ln_eps"])
        a = F.linear(h, p("fc1_w"), p("fc1_b"))
        x = x + F.linear(a * torch.sigmoid(1.702 * a), p("fc2_w"), p("fc2_b"))
    rows = torch.as_tensor(TR.pooled_positions(ids, spec["eot_id"]))
    pooled = F.layer_norm(x[torch.arange(B), rows], (H,), t(w["ln_g"]), t(w["ln_b"]), spec["ln_eps"])
    out = F.linear(pooled, t(w["proj_w"]))
    return (out / out.norm(dim=-1, keepdim=True)).numpy()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_embedding_bits_do_not_depend_on_batch_tail_or_T(dtype):
    spec = TR.tiny_text_spec(hidden=256, layers=2, vocab=1000, context=77, proj_dim=128)
    enc, _ = _encoder(spec, dtype)
    rng = np.random.default_rng(7)
    eots = [0, 1, 15, 16, 17, 40, 76] + rng.integers(0, 77, size=30).tolist()   # 37 sequences
    ids = _ids(spec, eots, seed=8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    batch = enc.encode_device(dev(ids)).cpu()
    other = ids.copy()
    for i, p in enumerate(eots):   # arbitrary valid tokens behind every EOT
        other[i, p + 1:] = rng.integers(0, spec["vocab"], size=76 - p)
    batch2 = enc.encode_device(dev(other)).cpu()
    assert torch.equal(batch.view(torch.int16), batch2.view(torch.int16))
    for i in [0, 1, 2, 3, 4, 5, 6, 20, 36]:
        p = eots[i]
        alone77 = enc.encode_device(dev(ids[i:i + 1])).cpu()
        alone_trim = enc.encode_device(dev(ids[i:i + 1, :p + 1])).cpu()
        assert torch.equal(alone77.view(torch.int16), batch[i:i + 1].view(torch.int16)), i
        assert torch.equal(alone_trim.view(torch.int16), batch[i:i + 1].view(torch.int16)), i
    trimmed = enc.encode_ids(ids).cpu()   # encode_ids trims to max(eot) + 1 = 77 here; and for a short batch:
    assert torch.equal(trimmed.view(torch.int16), batch.view(torch.int16))
    short = enc.encode_ids(ids[:4]).cpu()
    assert torch.equal(short.view(torch.int16), batch[:4].view(torch.int16))


def test_graph_capture_replays_to_the_same_bits():
    spec = TR.tiny_text_spec(hidden=256, layers=2, vocab=1000, context=77, proj_dim=128)
    enc, _ = _encoder(spec, "f16")
    ids = torch.from_numpy(_ids(spec, [3, 76, 20, 0], seed=9).astype(np.int32)).cuda()
    eager = enc.encode_device(ids).clone()
    ws = torch.empty(enc.workspace_bytes(4, 77), dtype=torch.uint8, device="cuda")
    flags = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc.encode_device(ids, out_flags=flags, workspace=ws)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = enc.encode_device(ids, out_flags=flags, workspace=ws)
    out.zero_()
    flags.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
    assert flags.tolist() == [0, 0, 0, 0]


def _joint_vision_spec(layers=2):
    from vidmem import specs
    return dict(specs.CLIP_L14_336_JOINT, layers=layers)


def test_joint_image_spec_matches_clip_vision_with_projection():
    """clip_l14_336_joint (2 layers) against transformers' CLIPVisionModelWithProjection (built from a config, fp32):
    weights taken from the HF model through text.clip_weights_from_state_dict."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from vidmem.encoder import FrameEncoder
    from vidmem.text import clip_weights_from_state_dict
    spec = _joint_vision_spec()
    torch.manual_seed(0)
    cfg = CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=2, num_attention_heads=16,
                           image_size=336, patch_size=14, projection_dim=768, hidden_act="quick_gelu",
                           layer_norm_eps=1e-5, attn_implementation="eager")
    m = CLIPVisionModelWithProjection(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n or n.endswith("bias"):
                p.add_(0.05 * torch.randn_like(p))
    w, _ = clip_weights_from_state_dict(m.state_dict())
    px = torch.randn(6, 3, 336, 336, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want32 = m(pixel_values=px).image_embeds
    want32 = (want32 / want32.norm(dim=-1, keepdim=True)).numpy()
    enc = FrameEncoder(spec, w, dtype="f16", device=0)
    assert enc.out_dim == 768
    got = enc.encode_patches(enc.patches_from_pixels(px)).float().cpu().numpy()
    floor = TR.rel(V.vit_forward_ref(spec, w, px.numpy(), quant="f16"), want32)
    _check_floor(got, want32, floor, "clip_l14_336_joint f16 L2")


def test_text_question_searches_a_joint_frame_memory():
    """Joint image tower -> EmbeddingMemory; text tower + HipTextEmbedder (stub tokenizer) -> the retriever's vector leg
    through attach_memory(embedder=...): rows and fp64 scores equal oracle.cref's top-k on the device's own text
    embedding; a memory of another width is refused."""
    from oracle import cref
    from vidmem import _lib, synthetic
    from vidmem.encoder import FrameEncoder
    from vidmem.fusion import HipHybridMixin
    from vidmem.memory import EmbeddingMemory
    from vidmem.text import HipTextEmbedder
    vspec = V.tiny_spec(image=224, patch=16, hidden=256, layers=2, heads=4, mlp=1024, act="quick_gelu", pre_ln=True,
                        patch_bias=False, ln_eps=1e-5, proj_dim=128)
    fenc = FrameEncoder(vspec, synthetic.encoder_weights(vspec, seed=31), dtype="f16", device=0)
    frames = torch.from_numpy(synthetic.frames_u8(32, 40, 224, 224)).cuda()
    emb = fenc.embed_frames(frames)
    mem = EmbeddingMemory(64, fenc.out_dim, "f16")
    n = emb.shape[0]
    mem.append(emb, ids=[f"run_0_{i}" for i in range(n)],
               meta=[{"time": f"00:{i:02d}", "content": f"chunk {i}"} for i in range(n)])
    tspec = TR.tiny_text_spec(hidden=256, layers=2, vocab=1000, context=77, proj_dim=128)
    tenc, _ = _encoder(tspec, "f16", seed=33)

    def stub_tokenizer(s):
        return [0] + [(7 * ord(c)) % 990 + 2 for c in s] + [tspec["eot_id"]]
    embedder = HipTextEmbedder(tenc, stub_tokenizer)

    class Retriever(HipHybridMixin):
        def __init__(self):
            self.config = SimpleNamespace(top_k_chunks=8, compression_threshold=0.7, top_k=5)
            self.embedder = None   # the reference's embedder of the host class: not used once one is passed
    r = Retriever().attach_memory(mem, score_mode=_lib.VM_SCORE_RAW, min_score=-1.0, embedder=embedder)
    question = "What color are the gloves worn by the person in the lab?"
    chunks = asyncio.run(r._vector_search_chunks(None, question))
    q = embedder.embed_tensor([question]).cpu()
    want_rows, want_scores = cref.cosine_topk(q.view(torch.int16).numpy().view(np.uint16),
                                              emb.cpu().view(torch.int16).numpy().view(np.uint16), 8, dtype="f16",
                                              score_mode=0, min_score=-1.0)
    assert [c["id"] for c in chunks] == [f"run_0_{i}" for i in want_rows[0] if i >= 0]
    assert [c["score"] for c in chunks] == [float(s) for s, i in zip(want_scores[0], want_rows[0]) if i >= 0]
    assert len(chunks) == 8
    wide = EmbeddingMemory(16, 256, "f16")
    with pytest.raises(ValueError, match="memory.dim"):
        Retriever().attach_memory(wide, score_mode=_lib.VM_SCORE_RAW, embedder=embedder)
