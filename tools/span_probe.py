"""Span top-k against the scoped and the row top-k of the same build, and a recall-links pass, event-timed and warm
(DESIGN.md 25).

  python tools/span_probe.py --rows 1000000 [--queries 1 16] [--iters 20] [--out profiles/span_probe_1m.json] [--lib other/libvidmem.so]
  python tools/span_probe.py --links 100000 [--block 256] [--out profiles/span_probe_links_100k.json]

``--rows``: one process per memory size.  Memory: ``--rows`` x 768 fp16, clustered rows (a centre per 16 rows + small
noise), tagged with tag = row id so that a span is also one scope; queries are noisy copies of stored rows of the span;
Q = 1 and 16 (``--queries``) at k = 10.  Spans: every row, the newest 10 %, 2,048 rows.  "span" = EmbeddingMemory.topk_span
(vm_topk_cosine_span, redo included).  Yardsticks from the same process: EmbeddingMemory.topk_scoped on the same ranges,
EmbeddingMemory.topk for every row.  Every variant is timed twice (``iters`` calls each), the variants taking turns; both
means are kept: the spread between a yardstick's two runs is the margin of the comparison.

``--links``: EmbeddingMemory.recall_links over ``--links`` x 768 fp16 rows, k = 10, min_gap = 16, pages of ``--block``
rows: rows per second of one whole-memory pass, and the same pages with every span left open (no triangular skip: every
page scans every tile) as its denominator.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: F401,E402
import vidmem._lib  # noqa: E402
from vidmem.memory import EmbeddingMemory  # noqa: E402

from group_probe import TD, clustered  # noqa: E402
from mask_probe import timed  # noqa: E402
from scope_probe import fill  # noqa: E402

D, DTYPE, K = 768, "f16", 10


def spans_probe(n, iters, queries):
    rows = clustered(n, D, 16, DTYPE, seed=16)
    ids = torch.arange(n, device="cuda")
    mem = fill(EmbeddingMemory(n, D, DTYPE, tagged=True), rows, ids)
    tenth, window = n // 10, min(2048, n)
    start = n // 3 // 16 * 16
    selections = [("all", (0, n - 1)), ("newest 10%", (n - tenth, n - 1)), ("2048 rows", (start, start + window - 1))]
    recs = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for Q in queries:
        for name, (lo, hi) in selections:
            pick = torch.randint(lo, hi + 1, (Q,), generator=g, device="cuda")
            q = (rows[pick].float() + 0.1 * torch.randn((Q, D), generator=g, device="cuda")).to(TD[DTYPE])
            sp = torch.tensor([(lo, hi)] * Q, dtype=torch.int64, device="cuda")
            fns = {"span": lambda: mem.topk_span(q, K, sp), "scoped": lambda: mem.topk_scoped(q, K, sp)}
            if name == "all":
                fns["topk"] = lambda: mem.topk(q, K)
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            runs = {v: [] for v in fns}
            for _ in range(2):                       # every variant twice, taking turns
                for v, fn in fns.items():
                    runs[v].append(round(timed(fn, iters), 4))
            s1, r1 = mem.topk_span(q, K, sp)
            flagged = int((mem.last_span_flags[:Q] != 0).sum())
            s2, r2 = mem.topk_scoped(q, K, sp)
            rec = {"rows": n, "D": D, "dtype": DTYPE, "Q": Q, "k": K, "span": name, "rows_in_span": hi - lo + 1,
                   "span_ms": runs["span"], "scoped_ms": runs["scoped"], "topk_ms": runs.get("topk"),
                   "flagged_queries_last_call": flagged, "equals_scoped": bool(torch.equal(r1, r2) and torch.equal(s1, s2))}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    return recs


def links_probe(n, block):
    rows = clustered(n, D, 16, DTYPE, seed=16)
    mem = EmbeddingMemory(n, D, DTYPE)
    for c0 in range(0, n, 65536):
        mem.append(rows[c0:c0 + 65536])
    mem.prepare_topk_span(block, K)
    table = mem.rows_tensor()

    def open_pass():                                 # the same pages and queries, every span open: no tile is skipped
        for b0 in range(0, n, block):
            mem.topk_span(table[b0:b0 + block], K, (None, None))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    mem.recall_links(first_row=0, n_rows=2 * block, k=K, min_gap=16, block=block)      # warm
    before = mem.span_uncertified_count
    t_links, (s, r) = wall(lambda: mem.recall_links(k=K, min_gap=16, block=block))
    redone = mem.span_uncertified_count - before
    t_open, _ = wall(open_pass)
    rec = {"rows": n, "D": D, "dtype": DTYPE, "k": K, "min_gap": 16, "block": block, "links_s": round(t_links, 4),
           "links_rows_per_s": round(n / t_links, 1), "open_spans_s": round(t_open, 4),
           "open_rows_per_s": round(n / t_open, 1), "links_over_open": round(t_links / t_open, 4),
           "queries_redone": int(redone), "rows_with_k_links": int((r[:, K - 1] >= 0).sum())}
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--links", type=int, default=None, help="rows of the recall-links pass")
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 16], help="the Q of --rows; above 16 the scan takes two "
                    "query tiles per block")
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time")
    a = ap.parse_args()
    if (a.rows is None) == (a.links is None):
        ap.error("give --rows or --links")
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    recs = spans_probe(a.rows, a.iters, a.queries) if a.rows else links_probe(a.links, a.block)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
