"""The range search against the two yardsticks the memory had before it, event-timed and warm, the variants alternating
in one process.

  python tools/range_probe.py [--rounds 3] [--out profiles/range_probe.json] [--quick] [--lib other/libvidmem.so]

Memories: 1 M x 768 fp16 and 1 M x 1024 bf16, clusters of 16 rows, tagged as 16 contiguous sources.  Q in {1, 16, 64};
queries = stored rows plus 0.1 noise.  Thresholds: taken from the exact scores of query 0 so that it has 16, 1,000 and
100,000 hits (the midpoint between the two scores at that rank); the other queries of a call get roughly as many.  One
more run is scoped to the source of each query's own row (1/16 of the memory) at the 1,000-hit threshold.
Per point:
  range    = EmbeddingMemory.enqueue_range (vm_range_cosine) with max_hits = the largest count of the call, i.e. the
             filling call of range_search; "count" = the count-only call (max_hits = 0) that precedes it there.
             rescored / hits = out_rescored and out_counts summed over the queries.
  P        = the only route to the same answer before: cosine_exact(q, rows_tensor()), the threshold, the scope mask and
             nonzero in torch.  It ends in the same (query, row) pairs (checked once per point).
  topk     = topk(q, 10) with its redo stage at the same Q: the price of one scan of the same memory.
"empty" = two events with nothing between them.  --quick: the fp16 memory and Q in {1, 16} only.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402, F401
import vidmem._lib  # noqa: E402
from vidmem.memory import EmbeddingMemory, _tensor_from_ptr  # noqa: E402

from group_probe import TD, clustered  # noqa: E402

SOURCES = 16


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(variants, rounds):
    """{name: [ms of each round]}: one warm call each, then the variants take turns, one call per round."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(one_call(fn))
    return ms


def run_memory(n, D, dtype, qs, rounds):
    rows = clustered(n, D, 16, dtype, seed=21)
    per = n // SOURCES
    i = torch.arange(n, device="cuda")
    tags = ((i // per) << 40) | ((i % per) * 33)
    mem = EmbeddingMemory(n, D, dtype, tagged=True)
    mem.append(rows, tag=tags)
    tag_col = _tensor_from_ptr(mem.L.vm_memory_tags(mem.handle), (n,), torch.int64, mem.device)
    g = torch.Generator(device="cuda").manual_seed(22)
    pick = torch.randint(0, n, (max(qs),), generator=g, device="cuda")
    q_all = (rows[pick].float() + 0.1 * torch.randn((max(qs), D), generator=g, device="cuda")).to(TD[dtype])
    own = ((pick // per) << 40)
    own_scope = torch.stack([own, own | ((1 << 40) - 1)], dim=1).contiguous()          # [Q, 2]
    ranked = torch.sort(mem.cosine_exact(q_all[:1], mem.rows_tensor())[0], descending=True).values
    cut_at = lambda hits: float((ranked[hits - 1] + ranked[hits]) / 2)
    cases = [("hits_16", cut_at(16), False), ("hits_1000", cut_at(1000), False), ("hits_100000", cut_at(100000), False),
             ("scoped_1_of_16", cut_at(1000), True)]
    del ranked
    out = []
    for Q in qs:
        q = q_all[:Q].contiguous()
        mem.prepare_topk(Q, 10)
        for name, tau, scoped in cases:
            sc = own_scope[:Q].contiguous() if scoped else None
            counts = mem.enqueue_range(q, tau, scope=sc, max_hits=0).counts.cpu()
            width = int(counts.max())
            scratch = mem.prepare_range(Q, width)

            def route_p():
                s = mem.cosine_exact(q, mem.rows_tensor())
                m = s > tau
                if scoped:
                    col = tag_col[None, :]
                    m &= (col >= sc[:, :1]) & (col <= sc[:, 1:])
                return torch.nonzero(m), s[m]

            hits = mem.enqueue_range(q, tau, scope=sc, max_hits=width, scratch=scratch)
            rescored = int(mem.last_range_rescored[:Q].sum())
            pairs, p_scores = route_p()
            live = hits.rows >= 0
            same = bool(int(live.sum()) == pairs.shape[0] and torch.equal(hits.rows[live], pairs[:, 1])
                        and torch.equal(hits.scores[live], p_scores))
            del pairs, p_scores, live
            ms = alternate({"range": lambda: mem.enqueue_range(q, tau, scope=sc, max_hits=width, scratch=scratch),
                            "count": lambda: mem.enqueue_range(q, tau, scope=sc, max_hits=0, scratch=scratch),
                            "P": route_p, "topk": lambda: mem.topk(q, 10), "empty": lambda: None}, rounds)
            mean = {k: sum(v) / len(v) for k, v in ms.items()}
            rec = {"rows": n, "D": D, "dtype": dtype, "Q": Q, "case": name, "min_score": tau, "scoped": scoped,
                   "hits": int(counts.sum()), "max_hits_per_query": width, "rescored": rescored,
                   "range_ms": round(mean["range"], 4), "count_ms": round(mean["count"], 4),
                   "P_ms": round(mean["P"], 4), "topk_ms": round(mean["topk"], 4), "empty_ms": round(mean["empty"], 4),
                   "ratio_to_P": round(mean["range"] / mean["P"], 4), "ratio_to_topk": round(mean["range"] / mean["topk"], 3),
                   "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "equals_P": same}
            print(json.dumps(rec), flush=True)
            out.append(rec)
            torch.cuda.empty_cache()
    mem.close()
    del rows
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the fp16 memory and Q in {1, 16} only")
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time (an A/B against a parent commit)")
    a = ap.parse_args()
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    qs = (1, 16) if a.quick else (1, 16, 64)
    recs = run_memory(1 << 20, 768, "f16", qs, a.rounds)
    if not a.quick:
        recs += run_memory(1 << 20, 1024, "bf16", qs, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "points": recs}, f, indent=1)


if __name__ == "__main__":
    main()
