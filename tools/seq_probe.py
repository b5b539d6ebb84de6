"""Sequence search against the clip search and the row top-k of the same vectors, event-timed and warm, alternating in one
process.

  TOOLS_DEV=1 python tools/seq_probe.py [--iters 20] [--rows 1048576] [--out profiles/seq_probe.json]

Memory: 1 M x 768 fp16 of scene-structured rows (tools/clip_probe.py scene_rows).  Sequences: C in {1, 16} of J stored rows
at cumulative random gaps in 1 .. G plus 0.1 x unit noise, (J, G) in {(4, 1), (4, 8), (16, 1), (16, 16)}, k = 10, min_sep =
min(32, (J - 1) G + 1).  "seq" = EmbeddingMemory.enqueue_topk_seq (vm_topk_cosine_seq, redo and back-trace included);
"clip" = enqueue_topk_clip of the same vectors at L = J and the same min_sep; "rows" = EmbeddingMemory.topk of the C x J
vectors as independent queries.  Per case: the three times, the per-category profile (vm_profile_read) of one sequence call
and of one clip call - topk_scan = pack + scan; topk_finalize = align (the clip search: window), peaks, select, re-score,
rank; topk_exact = redo and back-trace - and the sequences the last call sent to the exhaustive redo.  At G = 1 the
sequence search must return the clip search's answer, rows + J - 1: asserted.

Per STAGE (needs the developer library, TOOLS_DEV=1: its switch VIDMEM_SEQ_STOP ends the call after the scan or after the
align kernel; without it "stages_ms" is null): the same call event-timed whole, ended after the scan and ended after the
align kernel, the three taking turns; scan = pack + scan, align = the second minus the first, redo = the topk_exact
category of one profiled call (redo launches and back-trace), peaks..rank = the whole call minus the other three.

One more case sends its sequence to the redo on purpose - an all-zero sequence, J = 4, G = 8, every chain ties at 0.0 - to
put a number on the exhaustive path at this size.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402,F401
from vidmem.memory import EmbeddingMemory  # noqa: E402

from _dev import maybe_dev  # noqa: E402
from clip_probe import scene_rows, unit  # noqa: E402
from scope_probe import alternate, fill  # noqa: E402


def profile_of(mem, fn):
    torch.cuda.synchronize()
    mem.ctx.profile_enable(4096)
    mem.ctx.profile_read()
    fn()
    prof = {c: round(v[0], 4) for c, v in mem.ctx.profile_read().items() if v[1]}
    mem.ctx.profile_enable(0)
    return prof


def stages(mem, call, iters, exact_ms):
    """-> {scan, align, peaks_to_rank, redo, whole} in ms, or None with the release library."""
    if not os.environ.get("TOOLS_DEV"):
        return None

    def stopped(at):
        def fn():
            os.environ["VIDMEM_SEQ_STOP"] = str(at)
            call()
        return fn
    ms = alternate({"whole": stopped(0), "scan": stopped(1), "scan_align": stopped(2)}, iters)
    os.environ["VIDMEM_SEQ_STOP"] = "0"
    align = ms["scan_align"] - ms["scan"]
    return {"scan": round(ms["scan"], 4), "align": round(align, 4),
            "peaks_to_rank": round(ms["whole"] - ms["scan_align"] - exact_ms, 4), "redo": round(exact_ms, 4),
            "whole": round(ms["whole"], 4), "align_over_scan": round(align / ms["scan"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    maybe_dev()
    n, D, k = a.rows, 768, 10
    rows = scene_rows(n, D, 5)
    mem = fill(EmbeddingMemory(n, D, "f16"), rows)
    g = torch.Generator(device="cuda").manual_seed(9)
    recs = []
    for J, G in ((4, 1), (4, 8), (16, 1), (16, 16)):
        sep = min(32, (J - 1) * G + 1)
        for Cn in (1, 16):
            starts = torch.randint(0, n - (J - 1) * G, (Cn,), generator=g, device="cuda")
            gaps = torch.randint(1, G + 1, (Cn, J), generator=g, device="cuda")
            gaps[:, 0] = 0
            idx = starts[:, None] + torch.cumsum(gaps, dim=1)
            steps = (rows[idx].float() + 0.1 * unit(torch.randn((Cn, J, D), generator=g, device="cuda"))).to(torch.float16)
            vectors = steps.reshape(Cn * J, D).contiguous()
            mem.prepare_topk_seq(Cn, J, k)
            mem.prepare_topk_clip(Cn, J, k)
            ms = alternate({"seq": lambda: mem.enqueue_topk_seq(steps, k, max_step=G, min_sep=sep),
                            "clip": lambda: mem.enqueue_topk_clip(steps, k, min_sep=sep),
                            "rows": lambda: mem.topk(vectors, k)}, a.iters)
            flagged = int((mem.last_seq_flags[:Cn] != 0).sum())
            s, r, sr, _ = mem.topk_seq(steps, k, max_step=G, min_sep=sep)
            found = int((sr[:, 0] == idx).all(dim=1).sum())
            if G == 1:
                cs, cr = mem.topk_clip(steps, k, min_sep=sep)
                assert torch.equal(r, torch.where(cr >= 0, cr + J - 1, cr)), "G = 1 is not the clip search's rows + J - 1"
                assert torch.equal(s.view(torch.int64), cs.view(torch.int64)), "G = 1 is not the clip search's scores"
            call = lambda: mem.enqueue_topk_seq(steps, k, max_step=G, min_sep=sep)  # noqa: E731
            prof = profile_of(mem, call)
            rec = {"rows": n, "D": D, "dtype": "f16", "C": Cn, "J": J, "G": G, "k": k, "min_sep": sep,
                   "seq_ms": round(ms["seq"], 4), "clip_ms_L_eq_J": round(ms["clip"], 4),
                   "rows_topk_of_CJ_vectors_ms": round(ms["rows"], 4), "seq_over_clip": round(ms["seq"] / ms["clip"], 3),
                   "seq_over_rows": round(ms["seq"] / ms["rows"], 3),
                   "stages_ms": stages(mem, call, a.iters, prof.get("topk_exact", 0.0)),
                   "profile_ms_one_seq_call": prof,
                   "profile_ms_one_clip_call": profile_of(mem, lambda: mem.enqueue_topk_clip(steps, k, min_sep=sep)),
                   "flagged_sequences_last_call": flagged, "sequences_whose_first_hit_is_the_planted_chain": found,
                   "equals_clip_search": True if G == 1 else None}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    # the exhaustive path at this size: an all-zero sequence ties everywhere and is redone
    J, G, sep = 4, 8, 25
    zero = torch.zeros((1, J, D), dtype=torch.float16, device="cuda")
    call = lambda: mem.enqueue_topk_seq(zero, k, max_step=G, min_sep=sep)  # noqa: E731
    ms = alternate({"seq": call}, max(2, a.iters // 4))
    flagged = int((mem.last_seq_flags[:1] != 0).sum())
    rec = {"rows": n, "D": D, "dtype": "f16", "C": 1, "J": J, "G": G, "k": k, "min_sep": sep, "all_zero_sequence": True,
           "seq_ms": round(ms["seq"], 4), "profile_ms_one_seq_call": profile_of(mem, call),
           "flagged_sequences_last_call": flagged}
    print(json.dumps(rec), flush=True)
    recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters,
                       "developer_build": bool(os.environ.get("TOOLS_DEV")), "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
