"""Grouped top-k against the row top-k of the same (Q, k), event-timed and warm, in one process.

  python tools/group_probe.py [--iters 20] [--out profiles/group_probe.json] [--lib other/libvidmem.so]

Cases: 1 M x 768 fp16 in groups of 16 and of 5, Q = 1 / 16 / 64, k = 10; 1 M x 1024 bf16 in groups of 16, Q = 1,
k = 20.  Rows are clustered (a centre per group + small noise), queries are noisy copies of stored rows.  "row" =
EmbeddingMemory.topk (vm_topk_cosine + vm_topk_redo_flagged); "grouped" = EmbeddingMemory.topk_grouped
(vm_topk_cosine_grouped, redo included).  Bytes/s counts the row store read once (n x D x 2) per call.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402
import vidmem._lib  # noqa: E402
from vidmem.memory import EmbeddingMemory  # noqa: E402

HBM_PEAK = 8.0e12
TD = {"f16": torch.float16, "bf16": torch.bfloat16}


def clustered(n, D, size, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = torch.empty((n, D), dtype=TD[dtype], device="cuda")
    step = 65536
    for c0 in range(0, n, step):
        c1 = min(n, c0 + step)
        gid = torch.arange(c0, c1, device="cuda") // size
        ng = int(gid[-1] - gid[0]) + 1
        centres = torch.randn((ng, D), generator=g, device="cuda")
        x = centres[gid - gid[0]] + 0.05 * torch.randn((c1 - c0, D), generator=g, device="cuda")
        rows[c0:c1] = (x / x.norm(dim=1, keepdim=True)).to(TD[dtype])
    return rows


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def run_case(n, D, size, dtype, Qs, k, iters):
    rows = clustered(n, D, size, dtype, seed=size)
    plain = EmbeddingMemory(n, D, dtype)
    grouped = EmbeddingMemory(n, D, dtype, grouped=True)
    keys = torch.arange(n, device="cuda") // size
    for c0 in range(0, n, 65536):
        plain.append(rows[c0:c0 + 65536])
        grouped.append(rows[c0:c0 + 65536], group=keys[c0:c0 + 65536])
    out = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for Q in Qs:
        pick = torch.randint(0, n, (Q,), generator=g, device="cuda")
        q = (rows[pick].float() + 0.1 * torch.randn((Q, D), generator=g, device="cuda")).to(TD[dtype])
        t_row = timed(lambda: plain.topk(q, k), iters)
        t_grp = timed(lambda: grouped.topk_grouped(q, k), iters)
        flagged = int((grouped.last_group_flags[:Q] != 0).sum())
        rec = {"rows": n, "D": D, "dtype": dtype, "group_size": size, "Q": Q, "k": k,
               "row_topk_ms": round(t_row, 4), "grouped_ms": round(t_grp, 4), "ratio": round(t_grp / t_row, 3),
               "grouped_bytes_per_s": n * D * 2 / (t_grp * 1e-3), "grouped_hbm_fraction": round(n * D * 2 / (t_grp * 1e-3) / HBM_PEAK, 3),
               "row_bytes_per_s": n * D * 2 / (t_row * 1e-3), "grouped_flagged_queries_last_call": flagged}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    del plain, grouped, rows
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
    recs += run_case(1 << 20, 768, 16, "f16", [1, 16, 64], 10, a.iters)
    recs += run_case(1 << 20, 768, 5, "f16", [1, 16, 64], 10, a.iters)
    recs += run_case(1 << 20, 1024, 16, "bf16", [1], 20, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
