"""Scoped top-k against the row top-k, event-timed and warm, the variants alternating in one process.

  python tools/scope_probe.py [--iters 20] [--out profiles/scope_probe.json] [--lib other/libvidmem.so]

Memory: 1 M x 768 fp16 in 8 contiguous sources of 131,072 rows, clustered rows (a centre per 16 rows + small noise),
queries noisy copies of stored in-scope rows; Q = 1 / 16 at k = 10, and 1 M x 1024 bf16 at Q = 1, k = 20.
Scopes: everything, one source (1/8), a 2,048-row window of one source, and - on a second memory with two sources
interleaved every 16 rows - one of the two (1/2).
"scoped" = EmbeddingMemory.topk_scoped (vm_topk_cosine_scoped, redo included).  Comparators: A = EmbeddingMemory.topk
over the whole memory (vm_topk_cosine + vm_topk_redo_flagged); B = the same on a plain memory that holds only the
in-scope rows (one memory per video: the workaround without tags).  In-scope bytes/s counts the in-scope rows read once.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402
import vidmem._lib  # noqa: E402
from vidmem.memory import SCOPE_ALL, EmbeddingMemory, make_tag, scope_of  # noqa: E402

from group_probe import TD, clustered  # noqa: E402

ROUNDS = 4


def fill(mem, rows, tags=None):
    for c0 in range(0, rows.shape[0], 65536):
        if tags is None:
            mem.append(rows[c0:c0 + 65536])
        else:
            mem.append(rows[c0:c0 + 65536], tag=tags[c0:c0 + 65536])
    return mem


def alternate(fns, iters):
    """Mean ms per call of every variant; the variants take turns, ROUNDS rounds of iters / ROUNDS calls each."""
    per = max(1, (iters + ROUNDS - 1) // ROUNDS)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    total = {name: 0.0 for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per):
                fn()
            b.record()
            torch.cuda.synchronize()
            total[name] += a.elapsed_time(b)
    return {name: t / (ROUNDS * per) for name, t in total.items()}


def run_case(n, D, dtype, Qs, k, iters):
    rows = clustered(n, D, 16, dtype, seed=16)
    per = n // 8
    i = torch.arange(n, device="cuda")
    tags_c = ((i // per) << 40) | ((i % per) * 33)                      # 8 contiguous sources
    tags_i = (((i // 16) % 2) << 40) | (i * 33)                        # 2 sources alternating every 16 rows
    plain = fill(EmbeddingMemory(n, D, dtype), rows)
    contig = fill(EmbeddingMemory(n, D, dtype, tagged=True), rows, tags_c)
    inter = fill(EmbeddingMemory(n, D, dtype, tagged=True), rows, tags_i)
    w0 = 40000
    scopes = [   # name, tagged memory, scope, in-scope row ids
        ("all", contig, SCOPE_ALL, i),
        ("source_1_of_8", contig, scope_of(3), i[3 * per:4 * per]),
        ("window_2048", contig, (make_tag(3, w0 * 33), make_tag(3, (w0 + 2047) * 33)), i[3 * per + w0:3 * per + w0 + 2048]),
        ("interleaved_1_of_2", inter, scope_of(1), i[(i // 16) % 2 == 1]),
    ]
    out = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for name, mem, scope, ids in scopes:
        only = plain if name == "all" else fill(EmbeddingMemory(ids.numel(), D, dtype), rows[ids])
        for Q in Qs:
            pick = ids[torch.randint(0, ids.numel(), (Q,), generator=g, device="cuda")]
            q = (rows[pick].float() + 0.1 * torch.randn((Q, D), generator=g, device="cuda")).to(TD[dtype])
            sc = torch.tensor([scope] * Q, dtype=torch.int64, device="cuda")
            ms = alternate({"scoped": lambda: mem.topk_scoped(q, k, sc), "A": lambda: plain.topk(q, k),
                            "B": lambda: only.topk(q, k)}, iters)
            flagged = int((mem.last_scope_flags[:Q] != 0).sum())
            s1, r1 = mem.topk_scoped(q, k, sc)
            s2, r2 = only.topk(q, k)
            same = bool(torch.equal(ids[r2.clamp(min=0)], r1) and torch.equal(s1, s2))
            rec = {"rows": n, "D": D, "dtype": dtype, "scope": name, "in_scope_rows": int(ids.numel()), "Q": Q, "k": k,
                   "scoped_ms": round(ms["scoped"], 4), "A_whole_memory_topk_ms": round(ms["A"], 4),
                   "B_in_scope_only_memory_topk_ms": round(ms["B"], 4), "ratio_to_A": round(ms["scoped"] / ms["A"], 3),
                   "ratio_to_B": round(ms["scoped"] / ms["B"], 3), "flagged_queries_last_call": flagged,
                   "in_scope_bytes_per_s": ids.numel() * D * 2 / (ms["scoped"] * 1e-3), "equals_B": same}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        if only is not plain:
            only.close()
    for m in (plain, contig, inter):
        m.close()
    del rows
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time (an A/B against a parent commit)")
    a = ap.parse_args()
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    recs = []
    recs += run_case(1 << 20, 768, "f16", [1, 16], 10, a.iters)
    recs += run_case(1 << 20, 1024, "bf16", [1], 20, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
