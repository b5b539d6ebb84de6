"""Diverse top-k against the plain and the masked top-k at k = pool, event-timed and warm.

  python tools/diverse_probe.py [--rows 1000000] [--iters 20] [--out profiles/diverse_probe.json] [--root other/checkout]

One process.  Memory: ``--rows`` x 768 fp16 scene-structured rows (a centre per 16 rows + small noise).  In the same
process, taking turns: ``EmbeddingMemory.topk_diverse`` at Q in (1, 16), k = 10, pool in (16, 64), lam = 0.5
(vm_topk_cosine_diverse: pool search with its redo, pairs, greedy) and the yardsticks ``topk(k = pool)`` and
``topk_masked(full mask, k = pool)``.  Every variant is timed twice (``iters`` calls each); both means are kept: the spread
between a variant's two runs is the margin of a comparison.  Then, per diverse variant, the per-category split of one call
(vm_profile_read: ``topk_scan`` = the pool's scan, ``topk_finalize`` = its cut .. finalize PLUS pairs + greedy,
``topk_exact`` = its redo scan + merge), the same split of one ``topk_span`` call with the open span at k = pool - the pool
stage alone, so the difference of the two ``topk_finalize`` figures is pairs + greedy - and the queries the last call
flagged.

``--root``: another built checkout (the parent commit's) whose ``vidmem`` package and library are used instead of this
tree's - the package binds every symbol of its own header when it loads, so a library goes with its package (a ``--lib``
switch as in tools/mask_probe.py cannot load a library that lacks the new symbols).  Only the variants that build has are
timed: the yardsticks of the parent and of the new build come from alternating processes.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, DTYPE, K = 768, "f16", 10
QS = (1, 16)
POOLS = (16, 64)
LAM = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=None, help="another built checkout to import vidmem from (an A/B against a parent "
                    "commit)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else HERE)
    import torch
    import vidmem  # noqa: F401
    from vidmem.memory import EmbeddingMemory
    from group_probe import TD, clustered          # these find vidmem already imported
    from mask_probe import timed
    from scope_probe import fill
    n = a.rows
    rows = clustered(n, D, 16, DTYPE, seed=16)
    mem = fill(EmbeddingMemory(n, D, DTYPE), rows)
    has_diverse = hasattr(mem.L, "vm_topk_cosine_diverse")
    g = torch.Generator(device="cuda").manual_seed(7)

    def near(count):
        pick = torch.randint(0, n, (count,), generator=g, device="cuda")
        return (rows[pick].float() + 0.1 * torch.randn((count, D), generator=g, device="cuda")).to(TD[DTYPE])

    full = ~mem.new_mask()
    fns, queries = {}, {}
    for Q in QS:
        q = queries[Q] = near(Q)
        lam = torch.full((Q,), LAM, dtype=torch.float64, device="cuda")
        for pool in POOLS:
            fns[f"topk Q={Q} k={pool}"] = lambda q=q, pool=pool: mem.topk(q, pool)
            fns[f"masked Q={Q} k={pool}"] = lambda q=q, pool=pool: mem.topk_masked(q, pool, full)
            if has_diverse:
                fns[f"diverse Q={Q} pool={pool}"] = lambda q=q, pool=pool, lam=lam: mem.topk_diverse(q, K, pool=pool, lam=lam)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {v: [] for v in fns}
    for _ in range(2):                               # every variant twice, taking turns
        for v, fn in fns.items():
            runs[v].append(round(timed(fn, a.iters), 4))
    recs = [{"variant": v, "ms": ms} for v, ms in runs.items()]

    def profiled(fn):
        torch.cuda.synchronize()
        mem.ctx.profile_enable(256)
        fn()
        prof = mem.ctx.profile_read()
        mem.ctx.profile_enable(0)
        return {c: round(prof[c][0], 4) for c in ("topk_scan", "topk_finalize", "topk_exact")}

    if has_diverse:
        for Q in QS:
            for pool in POOLS:                       # one profiled call per diverse variant, and one of its pool stage alone
                rec = next(r for r in recs if r["variant"] == f"diverse Q={Q} pool={pool}")
                whole = profiled(fns[f"diverse Q={Q} pool={pool}"])
                rec["flagged_queries_last_call"] = int((mem.last_diverse_flags[:Q] != 0).sum())
                alone = profiled(lambda: mem.topk_span(queries[Q], pool, (None, None)))
                rec["stages_ms"] = {"pool scan": whole["topk_scan"], "cut..finalize + pairs + greedy": whole["topk_finalize"],
                                    "redo": whole["topk_exact"]}
                rec["pool_stage_alone_ms"] = {"scan": alone["topk_scan"], "cut..finalize": alone["topk_finalize"],
                                              "redo": alone["topk_exact"]}
                rec["pairs_plus_greedy_ms"] = round(whole["topk_finalize"] - alone["topk_finalize"], 4)
    for r in recs:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "D": D, "dtype": DTYPE, "k": K, "lam": LAM,
                       "iters": a.iters, "root": a.root or "this tree", "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
