"""Any/all top-k against the two-step linking and against the mixed top-k, warm.

  python tools/fold_probe.py [--rows 100000 1000000] [--iters 20] [--out profiles/fold_probe.json] [--root other/checkout | --lib other/libvidmem.so]

One process; one run per value of ``--rows``, one after the other, each on a memory of its own: ``rows`` x 768 fp16
scene-structured rows (a centre per 16 rows + small noise), one id per row.  ``--out`` holds ``{"tool", "runs": [one object
per run]}``.

1. Linking, wall clock with a synchronisation after every call (both routes end in host code): a batch of Q = 16
   embeddings, ``top_k_each`` = ``top_k_final`` = 10.  ``two-step`` is the parent's route and the new function's fallback
   branch, ``merge_batch_similarities(batch_similarities(...))``; ``fold`` is ``similarity.linked_similarities``.  Once for
   1 batch and once for 64 batches, one call per batch (the adapter takes one batch).  The two routes are checked to return
   the same list first.
2. The device calls alone, event-timed: ``topk_fold`` (max and min) against ``topk_mix`` at the same (C, J, k) = (1, 16, 10),
   (64, 16, 10), and against the plain ``topk`` of the same C x J vectors as separate queries (what step one of the
   two-step route launches).  Then the per-category split of one call (vm_profile_read: ``topk_scan`` = pack + scan,
   ``topk_finalize`` = cut .. finalize, ``topk_exact`` = redo scan + merge; the fold's winning-term kernel is in none) and
   the queries the last call flagged.

Every variant is timed twice, taking turns; both means are kept: the spread between a variant's two runs is the margin of a
comparison.

``--root`` / ``--lib``: another built checkout, or another build of the library with this tree's ABI, to time instead
(mix_probe.py's options: an A/B against a parent commit, one process per side).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D, DTYPE, K = 768, "f16", 10
SHAPES = ((1, 16), (64, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=None, help="another built checkout to import vidmem from (an A/B against a parent "
                    "commit)")
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so with this tree's ABI to time")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else HERE)
    import vidmem  # noqa: F401
    import vidmem._lib
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    runs = [run(n, a.iters) for n in a.rows]
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/fold_probe.py", "root": a.root or "this tree", "lib": a.lib or "its own",
                       "runs": runs}, f, indent=1)


def run(n, iters):
    """One memory of ``n`` rows: both parts of the probe -> the run's record."""
    import torch
    from vidmem.memory import EmbeddingMemory
    from vidmem.similarity import batch_similarities, linked_similarities, merge_batch_similarities
    from group_probe import TD, clustered          # these find vidmem already imported
    from mask_probe import timed
    from scope_probe import fill
    rows = clustered(n, D, 16, DTYPE, seed=16)
    mem = fill(EmbeddingMemory(n, D, DTYPE), rows)
    mem.ids = [str(i) for i in range(n)]
    g = torch.Generator(device="cuda").manual_seed(7)

    def near(count):
        pick = torch.randint(0, n, (count,), generator=g, device="cuda")
        return (rows[pick].float() + 0.1 * torch.randn((count, D), generator=g, device="cuda")).to(TD[DTYPE])

    # ---- 1. linking ----------------------------------------------------------------------------------------------------
    batches = [list(near(16)) for _ in range(64)]

    def two_step(b):
        return merge_batch_similarities(batch_similarities(mem, b, K), K)

    def fold(b):
        return linked_similarities(mem, b, K, K)

    same = sum(two_step(b) == fold(b) for b in batches[:8])
    same_scores = sum([s for _, s in two_step(b)] == [s for _, s in fold(b)] for b in batches[:8])

    def wall(fn, bs, reps):
        for b in bs[:2]:
            fn(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            for b in bs:
                fn(b)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / reps, 4)

    link = {}
    for _ in range(2):
        for name, fn in (("two-step", two_step), ("fold", fold)):
            link.setdefault(f"{name}, 1 batch", []).append(wall(fn, batches[:1], iters))
            link.setdefault(f"{name}, 64 batches", []).append(wall(fn, batches, max(1, iters // 10)))
    recs = [{"variant": v, "ms": ms} for v, ms in link.items()]
    recs.append({"variant": "routes agree on 8 batches", "lists": same, "score lists": same_scores})

    # ---- 2. the device calls ---------------------------------------------------------------------------------------------
    fns, args = {}, {}
    for C, J in SHAPES:
        terms = near(C * J).reshape(C, J, D).contiguous()
        w = torch.ones((C, J), dtype=torch.float64, device="cuda")
        flat = terms.reshape(C * J, D)
        args[(C, J)] = (terms, w)
        fns[f"fold max C={C} J={J}"] = lambda t=terms, w=w: mem.topk_fold(t, K, op="max", weights=w)
        fns[f"fold min C={C} J={J}"] = lambda t=terms, w=w: mem.topk_fold(t, K, op="min", weights=w)
        fns[f"mix C={C} J={J}"] = lambda t=terms, w=w: mem.topk_mix(t, w, K)
        fns[f"topk Q={C * J}"] = lambda q=flat: mem.topk(q, K)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {v: [] for v in fns}
    for _ in range(2):                               # every variant twice, taking turns
        for v, fn in fns.items():
            runs[v].append(round(timed(fn, iters), 4))
    dev = [{"variant": v, "ms": ms} for v, ms in runs.items()]
    for (C, J), (terms, w) in args.items():          # one profiled call per variant
        for name, call, flags in (("fold max", lambda: mem.topk_fold(terms, K, op="max", weights=w), "last_fold_flags"),
                                  ("fold min", lambda: mem.topk_fold(terms, K, op="min", weights=w), "last_fold_flags"),
                                  ("mix", lambda: mem.topk_mix(terms, w, K), "last_mix_flags")):
            torch.cuda.synchronize()
            mem.ctx.profile_enable(256)
            call()
            prof = mem.ctx.profile_read()
            mem.ctx.profile_enable(0)
            rec = next(r for r in dev if r["variant"] == f"{name} C={C} J={J}")
            rec["stages_ms"] = {"pack+scan": round(prof["topk_scan"][0], 4),
                                "cut..finalize": round(prof["topk_finalize"][0], 4), "redo": round(prof["topk_exact"][0], 4)}
            rec["flagged_queries_last_call"] = int((getattr(mem, flags)[:C] != 0).sum())
    recs += dev
    for r in recs:
        print(json.dumps(r), flush=True)
    mem.close()
    return {"device": torch.cuda.get_device_name(0), "rows": n, "D": D, "dtype": DTYPE, "k": K, "iters": iters, "cases": recs}


if __name__ == "__main__":
    main()
