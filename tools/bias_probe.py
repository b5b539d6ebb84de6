"""Biased top-k against the masked top-k, event-timed and warm.

  python tools/bias_probe.py [--rows 1000000] [--iters 20] [--out profiles/bias_probe.json] [--root other/checkout | --lib other/libvidmem.so]

One process.  Memory: ``--rows`` x 768 fp16 scene-structured rows (a centre per 16 rows + small noise), k = 10.  In the
same process, taking turns: ``EmbeddingMemory.topk_biased`` at Q = 1, 16 and 32 without a mask and with a full mask
(vm_topk_cosine_biased, redo included; queries are noisy copies of stored rows, the bias is linear recency over the row
ids, -0.1 for the oldest row, weight 1.0) and ``EmbeddingMemory.topk_masked`` with a full mask at the same Q.  Every
variant is timed twice (``iters`` calls each); both means are kept: the spread between a variant's two runs is the margin
of a comparison.  After each timing the queries the last call flagged are read: a timed call must flag none.  Then, per
biased variant, the per-category split of one call (vm_profile_read: ``topk_scan`` = pack + scan, ``topk_finalize`` =
cut .. finalize, ``topk_exact`` = redo scan + merge).

``--root``: another built checkout (the parent commit's) whose ``vidmem`` package and library are used instead of this
tree's - the package binds every symbol of its own header when it loads, so a library goes with its package.  Only the
variants that build has are timed: the masked yardstick of the parent and of the new build come from alternating processes.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, DTYPE, K = 768, "f16", 10
QS = (1, 16, 32)        # 32: two query tiles per block, where the biased scan holds 88 registers against the masked 80


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=None, help="another built checkout to import vidmem from (an A/B against a parent "
                    "commit)")
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so with this tree's ABI to time")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else HERE)
    import torch
    import vidmem  # noqa: F401
    import vidmem._lib
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    from vidmem.memory import EmbeddingMemory
    from group_probe import TD, clustered          # these find vidmem already imported
    from mask_probe import timed
    from scope_probe import fill
    n = a.rows
    rows = clustered(n, D, 16, DTYPE, seed=16)
    mem = fill(EmbeddingMemory(n, D, DTYPE), rows)
    has_bias = hasattr(mem.L, "vm_topk_cosine_biased")
    g = torch.Generator(device="cuda").manual_seed(7)

    def near(count):
        pick = torch.randint(0, n, (count,), generator=g, device="cuda")
        return (rows[pick].float() + 0.1 * torch.randn((count, D), generator=g, device="cuda")).to(TD[DTYPE])

    full = ~mem.new_mask()
    fns, flags_of, bias_args = {}, {}, {}
    queries = {Q: near(Q) for Q in QS}
    for Q in QS:
        fns[f"masked Q={Q}"] = lambda q=queries[Q]: mem.topk_masked(q, K, full)
        flags_of[f"masked Q={Q}"] = lambda Q=Q: mem.last_mask_flags[:Q]
    if has_bias:
        bias = mem.new_bias()
        bias[0, :n] = (torch.arange(n, device="cuda", dtype=torch.float64) - (n - 1)).mul_(0.1 / max(n - 1, 1)).float()
        for Q in QS:
            w = torch.ones(Q, dtype=torch.float64, device="cuda")
            for name, mask in (("", None), (" full mask", full)):
                v = f"biased Q={Q}{name}"
                bias_args[v] = (queries[Q], w, mask)
                fns[v] = lambda q=queries[Q], w=w, m=mask: mem.topk_biased(q, K, bias, weight=w, mask=m)
                flags_of[v] = lambda Q=Q: mem.last_bias_flags[:Q]
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {v: [] for v in fns}
    flagged = {v: 0 for v in fns}
    for _ in range(2):                               # every variant twice, taking turns
        for v, fn in fns.items():
            runs[v].append(round(timed(fn, a.iters), 4))
            flagged[v] += int((flags_of[v]() != 0).sum())
    recs = [{"variant": v, "ms": ms, "flagged_queries_after_timing": flagged[v]} for v, ms in runs.items()]
    for v, (q, w, mask) in bias_args.items():        # one profiled call per biased variant
        torch.cuda.synchronize()
        mem.ctx.profile_enable(256)
        mem.topk_biased(q, K, bias, weight=w, mask=mask)
        prof = mem.ctx.profile_read()
        mem.ctx.profile_enable(0)
        rec = next(r for r in recs if r["variant"] == v)
        rec["stages_ms"] = {"pack+scan": round(prof["topk_scan"][0], 4), "cut..finalize": round(prof["topk_finalize"][0], 4),
                            "redo": round(prof["topk_exact"][0], 4)}
        rec["flagged_queries_last_call"] = int((mem.last_bias_flags[:q.shape[0]] != 0).sum())
    for Q in QS:                                     # the yardstick's split, for the scan-to-scan comparison
        torch.cuda.synchronize()
        mem.ctx.profile_enable(256)
        mem.topk_masked(queries[Q], K, full)
        prof = mem.ctx.profile_read()
        mem.ctx.profile_enable(0)
        rec = next(r for r in recs if r["variant"] == f"masked Q={Q}")
        rec["stages_ms"] = {"scan": round(prof["topk_scan"][0], 4), "cut..finalize": round(prof["topk_finalize"][0], 4),
                            "redo": round(prof["topk_exact"][0], 4)}
    for r in recs:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "D": D, "dtype": DTYPE, "k": K, "iters": a.iters,
                       "root": "the parent commit" if a.root else "this tree", "cases": recs}, f, indent=1)
    if any(flagged.values()):
        sys.exit(f"bias_probe: queries were flagged in a timed call: {flagged}")


if __name__ == "__main__":
    main()
