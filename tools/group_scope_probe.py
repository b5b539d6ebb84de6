"""Scoped grouped top-k against the grouped top-k, event-timed and warm, the two alternating in one process
(DESIGN.md 19).

  python tools/group_scope_probe.py [--iters 20] [--out run.json] [--lib other/libvidmem.so]
  python tools/group_scope_probe.py --merge profiles/group_scope_probe.json parent_a=pa.json new_a=na.json ...

Memory: 1 M x 768 fp16 in groups of 16, clustered rows (a centre per group + small noise) - tools/group_probe.py's rows,
keys and, for the whole-memory scope, queries, so that its `grouped_ms` from another build of the library (a parent
commit's tree runs its own group_probe.py) is the same work.  Q = 1 / 16 at k = 10.  Scopes:
  all                  [INT64_MIN, INT64_MAX]: the grouped search's row traffic plus 8 bytes of tag per row
  contiguous_1_of_16   one of 16 contiguous sources of 65,536 rows: 15 of 16 tiles are skipped on their tags
  interleaved_1_of_16  the same share with the source changing every row: every tile and every group holds one in-scope
                       row, nothing can be skipped
"grouped_scoped" = EmbeddingMemory.topk_grouped_scoped (vm_topk_cosine_grouped_scoped, redo included); "grouped" =
EmbeddingMemory.topk_grouped on the same memory (vm_topk_cosine_grouped: every group, whatever the scope).

profiles/group_scope_probe.json is four runs in four processes on one device, in the order parent_a, new_a, parent_b,
new_b: "new" = this probe with --out; "parent" = tools/group_probe.py's run_case(1 << 20, 768, 16, "f16", [1, 16], 10,
20) from a checkout of the parent commit with its own built library, its records saved as {"cases": [...]}.  The two
parent runs give the parent's run-to-run spread.  --merge assembles the runs into that one file.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402,F401
import vidmem._lib  # noqa: E402
from vidmem.memory import SCOPE_ALL, EmbeddingMemory, scope_of  # noqa: E402

from group_probe import TD, clustered  # noqa: E402
from scope_probe import alternate  # noqa: E402


def fill(mem, rows, keys, tags):
    for c0 in range(0, rows.shape[0], 65536):
        mem.append(rows[c0:c0 + 65536], group=keys[c0:c0 + 65536], tag=tags[c0:c0 + 65536])
    return mem


def run_case(n, D, size, dtype, Qs, k, iters):
    rows = clustered(n, D, size, dtype, seed=size)
    i = torch.arange(n, device="cuda")
    keys = i // size
    per = n // 16
    contig = fill(EmbeddingMemory(n, D, dtype, grouped=True, tagged=True), rows, keys, ((i // per) << 40) | ((i % per) * 33))
    inter = fill(EmbeddingMemory(n, D, dtype, grouped=True, tagged=True), rows, keys, ((i % 16) << 40) | (i * 33))
    scopes = [   # name, memory, scope, in-scope row ids
        ("all", contig, SCOPE_ALL, i),
        ("contiguous_1_of_16", contig, scope_of(5), i[5 * per:6 * per]),
        ("interleaved_1_of_16", inter, scope_of(5), i[i % 16 == 5]),
    ]
    out = []
    for name, mem, scope, ids in scopes:
        g = torch.Generator(device="cuda").manual_seed(7)      # "all": tools/group_probe.py's queries, in its order
        for Q in Qs:
            pick = ids[torch.randint(0, ids.numel(), (Q,), generator=g, device="cuda")]
            q = (rows[pick].float() + 0.1 * torch.randn((Q, D), generator=g, device="cuda")).to(TD[dtype])
            sc = torch.tensor([scope] * Q, dtype=torch.int64, device="cuda")
            ms = alternate({"grouped": lambda: mem.topk_grouped(q, k),
                            "grouped_scoped": lambda: mem.topk_grouped_scoped(q, k, sc)}, iters)
            flagged = int((mem.last_group_scope_flags[:Q] != 0).sum())
            fast = mem.topk_grouped_scoped(q, k, sc)
            same = all(torch.equal(a, b) for a, b in zip(fast, mem.topk_grouped_scoped(q, k, sc, exact=True)))
            rec = {"rows": n, "D": D, "dtype": dtype, "group_size": size, "scope": name,
                   "in_scope_rows": int(ids.numel()), "Q": Q, "k": k, "grouped_scoped_ms": round(ms["grouped_scoped"], 4),
                   "grouped_ms": round(ms["grouped"], 4), "ratio_to_grouped": round(ms["grouped_scoped"] / ms["grouped"], 3),
                   "flagged_queries_last_call": flagged, "redo_share": round(flagged / Q, 3),
                   "in_scope_bytes_per_s": ids.numel() * D * 2 / (ms["grouped_scoped"] * 1e-3),
                   "equals_exact_entry": bool(same)}
            if name == "all":
                rec["equals_grouped"] = all(torch.equal(a, b) for a, b in zip(fast, mem.topk_grouped(q, k)))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    for m in (contig, inter):
        m.close()
    del rows
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time (an A/B against a parent commit)")
    ap.add_argument("--merge", nargs="+", metavar=("OUT", "NAME=RUN_JSON"), default=None,
                    help="no measurement: collect runs written with --out (and the parent's) into OUT")
    a = ap.parse_args()
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    if a.merge:
        runs = {name: json.load(open(path)) for name, path in (m.split("=", 1) for m in a.merge[1:])}
        device = next((r["device"] for r in runs.values() if "device" in r), None)
        with open(a.merge[0], "w") as f:
            json.dump({"device": device, "order": list(runs), "runs": {n: r["cases"] for n, r in runs.items()}}, f, indent=1)
        return
    recs = run_case(1 << 20, 768, 16, "f16", [1, 16], 10, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
