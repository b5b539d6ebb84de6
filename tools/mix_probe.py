"""Mixed-query top-k against the masked top-k, event-timed and warm.

  python tools/mix_probe.py [--rows 1000000] [--iters 20] [--out profiles/mix_probe.json] [--root other/checkout | --lib other/libvidmem.so]

One process.  Memory: ``--rows`` x 768 fp16 scene-structured rows (a centre per 16 rows + small noise), k = 10.  In the
same process, taking turns: ``EmbeddingMemory.topk_mix`` at (C, J) = (1, 1), (1, 4), (1, 16), (16, 4) (vm_topk_cosine_mix,
redo included; terms are noisy copies of stored rows, weights +1, +1, -0.5 repeating) and ``EmbeddingMemory.topk_masked``
with a full mask at Q = 1 and Q = 16.  Every variant is timed twice (``iters`` calls each); both means are kept: the spread
between a variant's two runs is the margin of a comparison.  Then, per mixed variant, the per-category split of one call
(vm_profile_read: ``topk_scan`` = pack + scan, ``topk_finalize`` = cut .. finalize, ``topk_exact`` = redo scan + merge) and
the queries the last call flagged.

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
MIX = ((1, 1), (1, 4), (1, 16), (16, 4))
MASKED_Q = (1, 16)


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
    has_mix = hasattr(mem.L, "vm_topk_cosine_mix")
    g = torch.Generator(device="cuda").manual_seed(7)

    def near(count):
        pick = torch.randint(0, n, (count,), generator=g, device="cuda")
        return (rows[pick].float() + 0.1 * torch.randn((count, D), generator=g, device="cuda")).to(TD[DTYPE])

    full = ~mem.new_mask()
    fns, mix_args = {}, {}
    for Q in MASKED_Q:
        q = near(Q)
        fns[f"masked Q={Q}"] = lambda q=q: mem.topk_masked(q, K, full)
    if has_mix:
        for C, J in MIX:
            terms = near(C * J).reshape(C, J, D).contiguous()
            w = torch.tensor([[(1.0, 1.0, -0.5)[j % 3] for j in range(J)]] * C, dtype=torch.float64, device="cuda")
            mix_args[(C, J)] = (terms, w)
            fns[f"mix C={C} J={J}"] = lambda t=terms, w=w: mem.topk_mix(t, w, K)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {v: [] for v in fns}
    for _ in range(2):                               # every variant twice, taking turns
        for v, fn in fns.items():
            runs[v].append(round(timed(fn, a.iters), 4))
    recs = [{"variant": v, "ms": ms} for v, ms in runs.items()]
    for (C, J), (terms, w) in mix_args.items():      # one profiled call per mixed variant
        torch.cuda.synchronize()
        mem.ctx.profile_enable(256)
        mem.topk_mix(terms, w, K)
        prof = mem.ctx.profile_read()
        mem.ctx.profile_enable(0)
        rec = next(r for r in recs if r["variant"] == f"mix C={C} J={J}")
        rec["stages_ms"] = {"pack+scan": round(prof["topk_scan"][0], 4), "cut..finalize": round(prof["topk_finalize"][0], 4),
                            "redo": round(prof["topk_exact"][0], 4)}
        rec["flagged_queries_last_call"] = int((mem.last_mix_flags[:C] != 0).sum())
    for r in recs:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": n, "D": D, "dtype": DTYPE, "k": K, "iters": a.iters,
                       "root": a.root or "this tree", "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
