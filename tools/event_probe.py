"""Event segmentation against the rate a streaming read of the same memory reaches, event-timed and warm, the variants
alternating in one process.

  TOOLS_DEV=1 python tools/event_probe.py [--rounds 30] [--out profiles/event_probe.json] [--quick]

Memories: n = 100 k and 1 M rows of 768 fp16 and of 1024 bf16, clusters of 16 rows (one event each at threshold 0.5),
grouped.  Per point, the median ms over ``rounds`` calls (at least 20) after a warm call of every variant:
  events   = vm_memory_events with out_links NULL, out_event_of and 4,096 first rows written
  regroup  = vm_memory_regroup_events over the whole memory
  *_simple = the same two calls with the link kernel's simple form (every lane runs the reference dot on global memory
             instead of reading its rows from LDS), which only the developer build reaches: under TOOLS_DEV=1 the probe
             loads libvidmem_dev.so and flips VIDMEM_EVENTS_SIMPLE between calls; without it these are null
  topk     = topk(q, 10) at Q = 16 without its redo stage: the scan of the same memory, the yardstick for what a
             streaming read reaches here
GB/s: events, regroup over n x D x 2 + n x 8 bytes; topk over n x D x 2.  "empty" = two events with nothing between.
--quick: the 100 k memories only.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402, F401
from _dev import maybe_dev  # noqa: E402

maybe_dev()

from vidmem import _lib  # noqa: E402
from vidmem.memory import EmbeddingMemory  # noqa: E402

from group_probe import TD, clustered  # noqa: E402

DEV = bool(os.environ.get("TOOLS_DEV"))
SWITCH = "VIDMEM_EVENTS_SIMPLE"
MAX_EVENTS = 4096


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


def simple(fn):
    """``fn`` with the developer switch set for the duration of the call (the library reads it at every call)."""
    def run():
        os.environ[SWITCH] = "1"
        try:
            return fn()
        finally:
            os.environ[SWITCH] = "0"
    return run


def run_memory(n, D, dtype, rounds):
    rows = clustered(n, D, 16, dtype, seed=31)
    mem = EmbeddingMemory(n, D, dtype, grouped=True)
    first = C.c_int64(0)
    # the raw append: keys NULL, every row its own group until the regroup
    for c0 in range(0, n, 1 << 16):
        part = rows[c0:c0 + (1 << 16)]
        mem.ctx.check(mem.L.vm_memory_append(mem.handle, C.c_void_p(part.data_ptr()), part.shape[0], C.byref(first),
                                             _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    mem.sync()
    g = torch.Generator(device="cuda").manual_seed(32)
    pick = torch.randint(0, n, (16,), generator=g, device="cuda")
    q = (rows[pick].float() + 0.1 * torch.randn((16, D), generator=g, device="cuda")).to(TD[dtype])
    mem.prepare_topk(16, 10)
    scratch = mem.prepare_events(MAX_EVENTS)

    def events():
        return mem.enqueue_events(0.5, max_events=MAX_EVENTS, scratch=scratch)

    def regroup():
        return mem.enqueue_regroup_events(0.5, scratch=scratch)

    os.environ[SWITCH] = "0"
    out = events()
    count, event_of = int(out.count.item()), out.event_of[:n].clone()
    regroup()
    keys = torch.from_numpy(mem.group_keys_host())
    same = None
    variants = {"events": events, "regroup": regroup}
    if DEV:
        out = simple(events)()
        same = bool(int(out.count.item()) == count and torch.equal(out.event_of[:n], event_of))
        simple(regroup)()
        same = same and bool(torch.equal(torch.from_numpy(mem.group_keys_host()), keys))
        variants.update({"events_simple": simple(events), "regroup_simple": simple(regroup)})
    variants.update({"topk": lambda: mem.topk(q, 10, redo=False), "empty": lambda: None})
    ms = alternate(variants, rounds)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}
    ev_bytes, scan_bytes = n * D * 2 + n * 8, n * D * 2
    gbs = lambda b, t: round(b / (t * 1e-3) / 1e9, 1)
    rec = {"rows": n, "D": D, "dtype": dtype, "events": count, "rounds": rounds, "developer_build": DEV,
           "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_max_ms": spread,
           "events_gbs": gbs(ev_bytes, med["events"]), "regroup_gbs": gbs(ev_bytes, med["regroup"]),
           "events_simple_gbs": gbs(ev_bytes, med["events_simple"]) if DEV else None,
           "regroup_simple_gbs": gbs(ev_bytes, med["regroup_simple"]) if DEV else None,
           "topk_q16_scan_gbs": gbs(scan_bytes, med["topk"]),
           "events_fraction_of_scan_rate": round(gbs(ev_bytes, med["events"]) / gbs(scan_bytes, med["topk"]), 3),
           "simple_over_shipped": round(med["events_simple"] / med["events"], 3) if DEV else None,
           "simple_equals_shipped": same}
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
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rounds": rounds, "points": recs}, f, indent=1)


if __name__ == "__main__":
    main()
