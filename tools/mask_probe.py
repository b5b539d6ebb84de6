"""Masked top-k against the scoped and the row top-k of the same build, event-timed and warm.

  python tools/mask_probe.py --rows 100000 [--iters 20] [--out profiles/mask_probe_100k.json] [--lib other/libvidmem.so]

One process per memory size.  Memory: ``--rows`` x 768 fp16, clustered rows (a centre per 16 rows + small noise), tagged
with tag = row id so that a contiguous selection is also one scope; queries are noisy copies of stored selected rows;
Q = 1 and 16 at k = 10.  Selections: 100 %, 10 % contiguous, 10 % scattered (one row in ten: nearly every 16-row tile
holds a selected row), 0.1 % contiguous.  "masked" = EmbeddingMemory.topk_masked (vm_topk_cosine_masked, redo included).
Yardsticks from the same process: EmbeddingMemory.topk_scoped on the same contiguous selections, EmbeddingMemory.topk for
100 %; the scattered case has none.  Every variant is timed twice (``iters`` calls each), the variants taking turns; both
means are kept: the spread between a yardstick's two runs is the margin of the comparison.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: F401,E402
import vidmem._lib  # noqa: E402
from vidmem.memory import EmbeddingMemory  # noqa: E402

from group_probe import TD, clustered  # noqa: E402
from scope_probe import fill  # noqa: E402

D, DTYPE, K = 768, "f16", 10


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time (an A/B against a parent commit)")
    a = ap.parse_args()
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    n = a.rows
    rows = clustered(n, D, 16, DTYPE, seed=16)
    ids = torch.arange(n, device="cuda")
    mem = fill(EmbeddingMemory(n, D, DTYPE, tagged=True), rows, ids)
    tenth, thousandth, start = n // 10, max(n // 1000, 16), n // 3 // 16 * 16
    selections = [   # name, selected row ids, the scope that says the same (or None)
        ("100%", ids, (0, n - 1)),
        ("10% contiguous", ids[start:start + tenth], (start, start + tenth - 1)),
        ("10% scattered", ids[::10], None),
        ("0.1% contiguous", ids[start:start + thousandth], (start, start + thousandth - 1)),
    ]
    recs = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for Q in (1, 16):
        for name, sel, scope in selections:
            pick = sel[torch.randint(0, sel.numel(), (Q,), generator=g, device="cuda")]
            q = (rows[pick].float() + 0.1 * torch.randn((Q, D), generator=g, device="cuda")).to(TD[DTYPE])
            mask = mem.mask_of_rows(sel)
            fns = {"masked": lambda: mem.topk_masked(q, K, mask)}
            if scope is not None:
                sc = torch.tensor([scope] * Q, dtype=torch.int64, device="cuda")
                fns["scoped"] = lambda: mem.topk_scoped(q, K, sc)
            if name == "100%":
                fns["topk"] = lambda: mem.topk(q, K)
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            runs = {v: [] for v in fns}
            for _ in range(2):                       # every variant twice, taking turns
                for v, fn in fns.items():
                    runs[v].append(round(timed(fn, a.iters), 4))
            s1, r1 = mem.topk_masked(q, K, mask)
            flagged = int((mem.last_mask_flags[:Q] != 0).sum())
            rec = {"rows": n, "D": D, "dtype": DTYPE, "Q": Q, "k": K, "selection": name, "selected_rows": int(sel.numel()),
                   "masked_ms": runs["masked"], "scoped_ms": runs.get("scoped"), "topk_ms": runs.get("topk"),
                   "flagged_queries_last_call": flagged}
            if scope is not None:
                s2, r2 = mem.topk_scoped(q, K, sc)
                rec["equals_scoped"] = bool(torch.equal(r1, r2) and torch.equal(s1, s2))
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
