"""Clip search against the row top-k of the same frames, event-timed and warm, alternating in one process.

  python tools/clip_probe.py [--iters 20] [--rows 1048576] [--out profiles/clip_probe.json] [--lib other/libvidmem.so]

Memory: 1 M x 768 fp16 of scene-structured rows (scenes of 24 - 40 rows, row = normalise(scene centre + 0.5 x unit noise)).
Clips: C in {1, 16} of L = 16 consecutive stored rows plus 0.1 x unit noise, k = 10, min_sep = 16.
"clip" = EmbeddingMemory.topk_clip (vm_topk_cosine_clip, redo included); "rows" = EmbeddingMemory.topk of the same 16 C
frames as independent queries at k = 10 (vm_topk_cosine + vm_topk_redo_flagged).  Per case: both times, their ratio, the
per-category profile (vm_profile_read) of one clip call and the clips the last call sent to the exhaustive redo.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402,F401
import vidmem._lib  # noqa: E402
from vidmem.memory import EmbeddingMemory  # noqa: E402

from scope_probe import alternate, fill  # noqa: E402


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def scene_rows(n, D, seed):
    """fp16 [n, D] on the device, made scene by scene in blocks of 65,536 rows."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sizes = torch.randint(24, 41, (n // 24 + 1,), generator=g, device="cuda")
    scene = torch.repeat_interleave(torch.arange(sizes.numel(), device="cuda"), sizes)[:n]
    centres = unit(torch.randn((int(scene[-1]) + 1, D), generator=g, device="cuda"))
    out = torch.empty((n, D), dtype=torch.float16, device="cuda")
    for c0 in range(0, n, 65536):
        c1 = min(n, c0 + 65536)
        noise = unit(torch.randn((c1 - c0, D), generator=g, device="cuda"))
        out[c0:c1] = unit(centres[scene[c0:c1]] + 0.5 * noise).to(torch.float16)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time")
    a = ap.parse_args()
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    n, D, L, k, sep = a.rows, 768, 16, 10, 16
    rows = scene_rows(n, D, 5)
    mem = fill(EmbeddingMemory(n, D, "f16"), rows)
    g = torch.Generator(device="cuda").manual_seed(9)
    recs = []
    for Cn in (1, 16):
        starts = torch.randint(0, n - L + 1, (Cn,), generator=g, device="cuda")
        idx = starts[:, None] + torch.arange(L, device="cuda")[None, :]
        clips = (rows[idx].float() + 0.1 * unit(torch.randn((Cn, L, D), generator=g, device="cuda"))).to(torch.float16)
        frames = clips.reshape(Cn * L, D).contiguous()
        mem.prepare_topk_clip(Cn, L, k)
        ms = alternate({"clip": lambda: mem.enqueue_topk_clip(clips, k, min_sep=sep),
                        "rows": lambda: mem.topk(frames, k)}, a.iters)
        flagged = int((mem.last_clip_flags[:Cn] != 0).sum())
        s, r = mem.topk_clip(clips, k, min_sep=sep)
        found = int((r[:, 0] == starts).sum())
        torch.cuda.synchronize()
        mem.ctx.profile_enable(4096)
        mem.ctx.profile_read()
        mem.enqueue_topk_clip(clips, k, min_sep=sep)
        prof = {c: round(v[0], 4) for c, v in mem.ctx.profile_read().items() if v[1]}
        mem.ctx.profile_enable(0)
        rec = {"rows": n, "D": D, "dtype": "f16", "C": Cn, "L": L, "k": k, "min_sep": sep,
               "clip_ms": round(ms["clip"], 4), "rows_topk_of_16C_frames_ms": round(ms["rows"], 4),
               "ratio": round(ms["clip"] / ms["rows"], 3), "profile_ms_one_clip_call": prof,
               "flagged_clips_last_call": flagged, "clips_that_found_their_moment_first": found}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
