"""Group summaries against the event segmentation of the same memory - one pass over the rows - event-timed and warm,
the variants alternating in one process.

  TOOLS_DEV=1 python tools/summary_probe.py [--rounds 30] [--out profiles/summary_probe.json] [--quick]

Memories: n = 100 k and 1 M rows of 768 fp16 and of 1024 bf16, grouped in chunks of 16 rows; every group is in the
window.  Per point, the median ms over ``rounds`` calls (at least 20) after a warm call of every variant:
  summaries        = vm_memory_summaries with every output: bounds, sum and normalise, score, select (two passes)
  centroids        = the same call with both key outputs NULL: bounds, sum and normalise (one pass)
  summaries_simple = the call with the score kernel's simple form (every lane runs the reference dot on global memory),
                     which only the developer build reaches: under TOOLS_DEV=1 the probe loads libvidmem_dev.so and
                     flips VIDMEM_SUMMARY_SIMPLE between calls; without it this is null
  events           = vm_memory_events over the same memory (out_links NULL, out_event_of and 4,096 first rows): the
                     yardstick for one pass over the rows
GB/s: centroids and events over n x D x 2 bytes, summaries over twice that.  "empty" = two events with nothing between.
One more line: a single group of 10,000 rows (768 fp16), which one workgroup streams alone.
--quick: the 100 k memories only.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402, F401
from _dev import maybe_dev  # noqa: E402

maybe_dev()

from vidmem.memory import EmbeddingMemory  # noqa: E402

from event_probe import alternate  # noqa: E402
from group_probe import clustered  # noqa: E402

DEV = bool(os.environ.get("TOOLS_DEV"))
SWITCH = "VIDMEM_SUMMARY_SIMPLE"
MAX_EVENTS = 4096


def simple(fn):
    """``fn`` with the developer switch set for the duration of the call (the library reads it at every call)."""
    def run():
        os.environ[SWITCH] = "1"
        try:
            return fn()
        finally:
            os.environ[SWITCH] = "0"
    return run


def run_memory(n, D, dtype, rounds, size=16):
    rows = clustered(n, D, size, dtype, seed=31)
    mem = EmbeddingMemory(n, D, dtype, grouped=True)
    for c0 in range(0, n, 1 << 16):
        part = rows[c0:c0 + (1 << 16)]
        mem.append(part, group=(torch.arange(c0, c0 + part.shape[0], device="cuda") // size))
    torch.cuda.synchronize()
    mem.sync()
    groups = (n + size - 1) // size
    scratch = mem.prepare_summaries(groups)
    ev_scratch = mem.prepare_events(MAX_EVENTS)

    def summaries():
        return mem.enqueue_summaries(0, groups, key_frames=True, scratch=scratch)

    def centroids():
        return mem.enqueue_summaries(0, groups, key_frames=False, scratch=scratch)

    def events():
        return mem.enqueue_events(0.5, max_events=MAX_EVENTS, scratch=ev_scratch)

    os.environ[SWITCH] = "0"
    out = summaries()
    count = int(out.count.item())
    cent, krows, kscores = out.centroids.clone(), out.key_rows.clone(), out.key_scores.clone()
    same_cent = bool(torch.equal(centroids().centroids.view(torch.int16), cent.view(torch.int16)))
    same = None
    variants = {"summaries": summaries, "centroids": centroids}
    if DEV:
        out = simple(summaries)()
        same = bool(torch.equal(out.key_rows, krows) and torch.equal(out.key_scores.view(torch.int64),
                                                                      kscores.view(torch.int64)))
        variants["summaries_simple"] = simple(summaries)
    variants.update({"events": events, "empty": lambda: None})
    ms = alternate(variants, rounds)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}
    one_pass = n * D * 2
    gbs = lambda b, t: round(b / (t * 1e-3) / 1e9, 1)
    rec = {"rows": n, "D": D, "dtype": dtype, "group_rows": size, "groups": count, "rounds": rounds,
           "developer_build": DEV, "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": spread,
           "summaries_gbs": gbs(2 * one_pass, med["summaries"]), "centroids_gbs": gbs(one_pass, med["centroids"]),
           "summaries_simple_gbs": gbs(2 * one_pass, med["summaries_simple"]) if DEV else None,
           "events_gbs": gbs(one_pass, med["events"]),
           "centroids_over_events": round(med["centroids"] / med["events"], 3),
           "summaries_over_two_events": round(med["summaries"] / (2 * med["events"]), 3),
           "key_pass_over_events": round((med["summaries"] - med["centroids"]) / med["events"], 3),
           "simple_over_shipped": round(med["summaries_simple"] / med["summaries"], 3) if DEV else None,
           "simple_equals_shipped": same, "centroids_equal_without_key_frames": same_cent}
    print(json.dumps(rec), flush=True)
    mem.close()
    del rows
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="the 100 k memories only")
    a = ap.parse_args()
    rounds = max(20, a.rounds)
    recs = []
    for n in (100_000,) if a.quick else (100_000, 1_000_000):
        recs.append(run_memory(n, 768, "f16", rounds))
        recs.append(run_memory(n, 1024, "bf16", rounds))
    recs.append(run_memory(10_000, 768, "f16", rounds, size=10_000))       # one long group
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": rounds, "points": recs}, f, indent=1)


if __name__ == "__main__":
    main()
