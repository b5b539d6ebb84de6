"""The novelty-gated append, event-timed and warm, the variants alternating in one process.

  python tools/novelty_probe.py [--pushes 120] [--iters 12] [--out profiles/novelty_probe.json] [--only eager|stream|buys]

1. stream  Streaming push at BASELINE config C5's shape: 16 frames of 1080p, ViT-B/16 f16, top-10 over a 2 M x 768 ring.
           p50 / p99 per push of a gated session against an ungated one (the captured body without the gate), taking
           turns, on a repetitive feed (every source frame shown 1-4 times) and on an all-distinct feed.
2. eager   One vm_memory_append_novel (known given) at look-ahead size, B = 1,760 and 4,096, 768 f16 and 1,024 bf16,
           against cosine_exact(X, X) + append(X): what the extractor's group search runs to learn the same thing.
3. buys    Rows stored per 1,000 frames of a repetitive embedding feed, and topk over the gated against the ungated memory.
`--only eager` under `rocprofv3 --kernel-trace --stats` gives the per-kernel split of the call.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vidmem  # noqa: E402,F401
from vidmem.memory import EmbeddingMemory  # noqa: E402

from scope_probe import alternate  # noqa: E402

TD = {"f16": torch.float16, "bf16": torch.bfloat16}


def runs_feed(n, C, D, sigma, dtype, seed=5):
    """n unit rows in runs of 1-8 around one of C random unit centres + sigma x N(0, 1) per component (device)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn((C, D), generator=g, device="cuda"), dim=1)
    lens = torch.randint(1, 9, (n,), generator=g, device="cuda")
    run_of = torch.repeat_interleave(torch.arange(n, device="cuda"), lens)[:n]
    pick = torch.randint(0, C, (n,), generator=g, device="cuda")[run_of]
    x = centres[pick] + sigma * torch.randn((n, D), generator=g, device="cuda")
    return torch.nn.functional.normalize(x, dim=1).to(TD[dtype])


def eager_case(B, D, dtype, iters):
    x = runs_feed(B, max(1, B // 4), D, 0.01, dtype)
    gated = EmbeddingMemory(1 << 16, D, dtype, ring=True)
    plain = EmbeddingMemory(1 << 16, D, dtype, ring=True)
    ks = torch.zeros(B, dtype=torch.float64, device="cuda")
    kr = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    gated.prepare_append_novel(B)

    def parent():
        plain.cosine_exact(x, x)
        plain.append(x)

    ms = alternate({"gated": lambda: gated.enqueue_append_novel(x, 0.9, known=(ks, kr)), "parent": parent,
                    "pairs_only_parent": lambda: plain.cosine_exact(x, x)}, iters)
    keep, _, count = gated.enqueue_append_novel(x, 0.9, known=(ks, kr))
    rec = {"B": B, "D": D, "dtype": dtype, "kept": int(count.item()), "append_novel_ms": round(ms["gated"], 4),
           "cosine_exact_plus_append_ms": round(ms["parent"], 4), "cosine_exact_ms": round(ms["pairs_only_parent"], 4),
           "ratio": round(ms["gated"] / ms["parent"], 3), "bar": 1.5, "met": bool(ms["gated"] <= 1.5 * ms["parent"])}
    gated.close()
    plain.close()
    return rec


class BlockFeed:
    """Frames made on the device, never the same twice: every source frame is a grid of random colour blocks, shown
    1-4 times in a row (``repeat``) or once, each showing with its own +-1 of pixel noise."""

    def __init__(self, seed, F, H, W, block, repeat):
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.F, self.H, self.W, self.block, self.repeat = F, H, W, block, repeat
        self.left, self.src = 0, None

    def chunk(self):
        out = []
        for _ in range(self.F):
            if self.left == 0:
                b = torch.randint(0, 256, (self.H // self.block, self.W // self.block, 3), generator=self.g,
                                  device="cuda", dtype=torch.int16)
                self.src = b.repeat_interleave(self.block, 0).repeat_interleave(self.block, 1)
                self.left = int(torch.randint(1, 5, (1,), generator=self.g, device="cuda")) if self.repeat else 1
            self.left -= 1
            noise = torch.randint(-1, 2, self.src.shape, generator=self.g, device="cuda", dtype=torch.int16)
            out.append((self.src + noise).clamp_(0, 255).to(torch.uint8))
        return torch.stack(out)


def stream_case(pushes):
    from vidmem import specs, synthetic as syn
    from vidmem.encoder import FrameEncoder
    from vidmem.streaming import StreamingSession
    F, H, W, cap, k = 16, 1080, 1920, 1 << 21, 10
    enc = FrameEncoder(specs.VIT_B16_224, syn.encoder_weights(specs.VIT_B16_224, seed=42), "f16")
    # the threshold: halfway between the repeated-frame and the distinct-frame scores of 128 frames of the repetitive feed
    sample = BlockFeed(2, F, H, W, 120, True)
    emb = torch.cat([enc.embed_frames(sample.chunk()) for _ in range(8)])
    probe_mem = EmbeddingMemory(64, 768, "f16")
    m = probe_mem.cosine_exact(emb, emb)
    m.fill_diagonal_(-1.0)
    top = m.max(dim=1).values
    rep, dist = top[top > 0.999], top[top <= 0.999]
    tau = float((rep.min() + dist.max()) / 2)
    probe_mem.close()
    recs = []
    fill = torch.nn.functional.normalize(torch.randn((1 << 16, 768), device="cuda"), dim=1).half()
    sessions = {}
    for name, thr in (("ungated", None), ("gated", tau)):
        mem = EmbeddingMemory(cap, 768, "f16", ring=True)
        for _ in range(cap >> 16):
            mem.append(fill)
        sessions[name] = (mem, StreamingSession(enc, mem, F, H, W, top_k=k, novelty_threshold=thr))
    for feed_name, repeat in (("repetitive", True), ("distinct", False)):
        feed = BlockFeed(3, F, H, W, 120, repeat)
        times = {n: [] for n in sessions}
        redone = {n: 0 for n in sessions}
        stored0 = {n: s.rows_appended for n, (_, s) in sessions.items()}
        for p in range(pushes + 8):
            chunk = feed.chunk()
            torch.cuda.synchronize()
            for n, (_, s) in sessions.items():     # the two sessions take turns on the same chunk
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(s.stream):
                    a.record()
                s.push(chunk)
                with torch.cuda.stream(s.stream):
                    b.record()
                s.stream.synchronize()
                redone[n] += s.uncertified_last_push
                if p >= 8:
                    times[n].append(a.elapsed_time(b))
        rec = {"feed": feed_name, "threshold": tau, "pushes": pushes, "budget_ms": 33.0}
        for n, t in times.items():
            rec[f"{n}_p50_ms"] = round(float(np.percentile(t, 50)), 4)
            rec[f"{n}_p99_ms"] = round(float(np.percentile(t, 99)), 4)
            rec[f"{n}_rows_stored_per_1000_frames"] = round(
                1000.0 * (sessions[n][1].rows_appended - stored0[n]) / ((pushes + 8) * F), 1)
            rec[f"{n}_queries_redone"] = redone[n]
        rec["added_p50_ms"] = round(rec["gated_p50_ms"] - rec["ungated_p50_ms"], 4)
        rec["p99_inside_budget"] = bool(rec["gated_p99_ms"] <= 33.0)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    for mem, _ in sessions.values():
        mem.close()
    return recs


def buys_case(n, iters):
    D, dtype = 768, "f16"
    x = runs_feed(n, n // 4, D, 0.01, dtype, seed=9)
    plain = EmbeddingMemory(n, D, dtype)
    gated = EmbeddingMemory(n, D, dtype)
    for lo in range(0, n, 65536):
        plain.append(x[lo:lo + 65536])
    for lo in range(0, n, 4096):
        gated.append_novel(x[lo:lo + 4096], 0.9)
    q = x[torch.randint(0, n, (16,), device="cuda")]
    ms = alternate({"gated": lambda: gated.topk(q, 10), "ungated": lambda: plain.topk(q, 10)}, iters)
    rec = {"frames": n, "rows_stored_ungated": len(plain), "rows_stored_gated": len(gated),
           "rows_stored_per_1000_frames": round(1000.0 * len(gated) / n, 1), "topk_Q16_k10_ungated_ms": round(ms["ungated"], 4),
           "topk_Q16_k10_gated_ms": round(ms["gated"], 4)}
    plain.close()
    gated.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=120)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if a.only in (None, "eager"):
        out["eager"] = []
        for D, dtype in ((768, "f16"), (1024, "bf16")):
            for B in (1760, 4096):
                out["eager"].append(eager_case(B, D, dtype, a.iters))
                print(json.dumps(out["eager"][-1]), flush=True)
    if a.only in (None, "buys"):
        out["buys"] = buys_case(1 << 19, a.iters)
        print(json.dumps(out["buys"]), flush=True)
    if a.only in (None, "stream"):
        out["stream"] = stream_case(a.pushes)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
