"""Erase against the route the memory had before it, event-timed and warm, the variants alternating in one process
(DESIGN.md 14).

  python tools/erase_probe.py [--iters 8] [--out profiles/erase_probe.json] [--lib other/libvidmem.so]
                              [--segments 0,32768,16384] [--quick] [--dev-variants]

Memories: 1 M x 768 fp16 tagged with 8 contiguous sources of 131,072 rows, and 1 M x 1024 bf16 tagged the same way; a
second tagging of the fp16 rows puts two sources in turns of 16 rows.  Cases: erase one source of 8 from the middle; the
first source (everything moves); the last source (nothing moves); a seeded random 10 % of the rows (by id); one of the
two interleaved sources.
"erase" = EmbeddingMemory.enqueue_erase (vm_memory_erase_scoped / vm_memory_erase_rows) with the workspace of
--segments' first entry (0 = the library's default); the other entries are timed on the fp16 memory beside it.
Yardstick P = the route without erase, on the device: the in-scope test, a torch gather of the survivors and their tags
from rows_tensor(), reset, append (one call).  It ends in the same memory (checked once per case).
Yardstick C = one device-to-device copy of exactly the bytes that had to move (the rows and side columns of every
survivor whose id changed).  "empty" = two events with nothing between them.
Every timed call starts from the full memory: between calls the memory is rebuilt by reset + append, outside the events.
--quick: the fp16 memory only, no search comparison.  --dev-variants (with --lib = the developer build, which reads
VIDMEM_ERASE_DIRECT and VIDMEM_ERASE_SEGMENT at every call): erase without the direct-copy branch and erase with a
131,072-row default segment take their turns beside the others.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402
import vidmem._lib  # noqa: E402
from vidmem.memory import EmbeddingMemory, EraseScratch, _tensor_from_ptr, scope_of  # noqa: E402

from group_probe import TD, clustered  # noqa: E402

ROUNDS = 4
DEV_SEGMENT = 131072     # a default segment above the release build's, reachable only through the developer build


def rebuild(mem, rows, tags):
    mem.reset()
    mem.append(rows, tag=tags)


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(variants, restore, iters):
    """{name: (mean ms, [mean ms of each round])}: the variants take turns, ROUNDS rounds of iters / ROUNDS calls each;
    ``restore`` runs before every call of a variant whose entry is (fn, True), outside the events."""
    per = max(1, (iters + ROUNDS - 1) // ROUNDS)
    for fn, dirty in variants.values():       # warm
        if dirty:
            restore()
        fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, (fn, dirty) in variants.items():
            t = 0.0
            for _ in range(per):
                if dirty:
                    restore()
                    torch.cuda.synchronize()
                t += one_call(fn)
            rounds[name].append(t / per)
    return {name: (sum(r) / len(r), r) for name, r in rounds.items()}


def with_env(name, value, fn):
    def call():
        os.environ[name] = value
        try:
            fn()
        finally:
            del os.environ[name]
    return call


def run_memory(n, D, dtype, segments, iters, interleaved, search, dev=False):
    rows = clustered(n, D, 16, dtype, seed=16)
    per = n // 8
    i = torch.arange(n, device="cuda")
    tags_c = ((i // per) << 40) | ((i % per) * 33)
    tags_i = (((i // 16) % 2) << 40) | (i * 33)
    g = torch.Generator(device="cuda").manual_seed(10)
    tenth = torch.nonzero(torch.rand(n, generator=g, device="cuda") < 0.1).flatten()
    mem = EmbeddingMemory(n, D, dtype, tagged=True)
    tag_col = _tensor_from_ptr(mem.L.vm_memory_tags(mem.handle), (n,), torch.int64, mem.device)
    scratches = {s: EraseScratch.for_(mem, s) for s in segments}
    if dev:
        os.environ["VIDMEM_ERASE_SEGMENT"] = str(DEV_SEGMENT)
        scratches["dev"] = EraseScratch.for_(mem, 0)
        del os.environ["VIDMEM_ERASE_SEGMENT"]
    default_rows = (scratches[segments[0]].ws.numel() - int(mem.L.vm_memory_erase_workspace_bytes(mem.handle, 256))) \
        // (2 * D + 28) + 256
    cases = [("source_1_of_8_middle", tags_c, scope_of(3), None), ("first_source", tags_c, scope_of(0), None),
             ("last_source", tags_c, scope_of(7), None), ("random_tenth", tags_c, None, tenth)]
    if interleaved:
        cases.append(("interleaved_1_of_2", tags_i, scope_of(1), None))
    out = []
    for name, tags, scope, ids in cases:
        restore = lambda: rebuild(mem, rows, tags)
        if scope is not None:
            sc = torch.tensor([scope], dtype=torch.int64, device="cuda")
            drop = (tags >= scope[0]) & (tags <= scope[1])
        else:
            drop = torch.zeros(n, dtype=torch.bool, device="cuda")
            drop[ids] = True
        keep = ~drop
        new_id = torch.cumsum(keep, 0) - 1
        moved = int((keep & (new_id != i)).sum())
        moved_bytes = moved * (2 * D + 8 + 4 + 8)          # rows, norm64, rnorm32, tag
        src = torch.empty(max(moved_bytes, 16), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def erase_with(s):
            if scope is not None:
                return lambda: mem.enqueue_erase(scope=sc, scratch=scratches[s])
            return lambda: mem.enqueue_erase(rows=ids, scratch=scratches[s])

        def route_p():
            col = tag_col[:n]
            if scope is not None:
                idx = torch.nonzero(~((col >= scope[0]) & (col <= scope[1]))).flatten()
            else:
                m = torch.ones(n, dtype=torch.bool, device="cuda")
                m[ids] = False
                idx = torch.nonzero(m).flatten()
            r, t = mem.rows_tensor()[idx], col[idx]
            mem.reset()
            mem.append(r, tag=t)

        # once: both routes end in the same memory
        restore()
        erase_with(segments[0])()
        mem.sync()
        n_new = len(mem)
        got = (mem.rows_tensor().clone(), tag_col[:n_new].clone())
        restore()
        route_p()
        same = bool(len(mem) == n_new and torch.equal(got[0], mem.rows_tensor()) and torch.equal(got[1], tag_col[:n_new]))
        del got
        variants = {"erase": (erase_with(segments[0]), True), "P": (route_p, True),
                    "C": ((lambda: dst.copy_(src)) if moved else (lambda: None), False), "empty": (lambda: None, False)}
        if interleaved:                                     # the fp16 memory: the alternative segment sizes beside it
            for s in segments[1:]:
                variants[f"erase_segment_{s}"] = (erase_with(s), True)
            if dev:                                         # the developer build reads its switches at every call
                variants["erase_no_direct"] = (with_env("VIDMEM_ERASE_DIRECT", "0", erase_with(segments[0])), True)
                variants[f"erase_segment_{DEV_SEGMENT}"] = (
                    with_env("VIDMEM_ERASE_SEGMENT", str(DEV_SEGMENT), erase_with("dev")), True)
        ms = alternate(variants, restore, iters)
        e, p, c = ms["erase"][0], ms["P"][0], ms["C"][0]
        rec = {"rows": n, "D": D, "dtype": dtype, "case": name, "erased_rows": int(drop.sum()), "moved_rows": moved,
               "moved_bytes": moved_bytes, "segment_rows": int(default_rows), "erase_ms": round(e, 4), "P_ms": round(p, 4),
               "C_ms": round(c, 4), "empty_ms": round(ms["empty"][0], 4), "ratio_to_P": round(e / p, 3),
               "ratio_to_C": round(e / c, 3) if moved else None,
               "moved_bytes_per_s": moved_bytes / (e * 1e-3) if moved else None,
               "erase_rounds_ms": [round(x, 4) for x in ms["erase"][1]], "P_rounds_ms": [round(x, 4) for x in ms["P"][1]],
               "equals_P": same}
        for name_v, (mean, _) in ms.items():
            if name_v.startswith("erase_"):
                rec[f"{name_v}_ms"] = round(mean, 4)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del src, dst
    if search:   # topk over the erased memory against topk over a fresh memory of the survivors
        tags, scope = tags_c, scope_of(3)
        rebuild(mem, rows, tags)
        mem.erase(scope=scope)
        keep = ~((tags >= scope[0]) & (tags <= scope[1]))
        fresh = EmbeddingMemory(n, D, dtype, tagged=True)
        fresh.append(rows[keep], tag=tags[keep])
        pick = torch.randint(0, n, (16,), generator=g, device="cuda")
        q = (rows[pick].float() + 0.1 * torch.randn((16, D), generator=g, device="cuda")).to(TD[dtype])
        for Q in (1, 16):
            ms = alternate({"erased": (lambda: mem.topk(q[:Q], 10), False), "fresh": (lambda: fresh.topk(q[:Q], 10), False)},
                           None, 4 * iters)
            a, b = mem.topk(q[:Q], 10), fresh.topk(q[:Q], 10)
            rec = {"rows": len(mem), "D": D, "dtype": dtype, "case": "topk_after_erase", "Q": Q, "k": 10,
                   "erased_memory_ms": round(ms["erased"][0], 4), "fresh_memory_ms": round(ms["fresh"][0], 4),
                   "erased_rounds_ms": [round(x, 4) for x in ms["erased"][1]],
                   "fresh_rounds_ms": [round(x, 4) for x in ms["fresh"][1]],
                   "same_answer": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        fresh.close()
    mem.close()
    del rows
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time")
    ap.add_argument("--segments", default="0,32768,16384", help="segment rows: the first is 'erase', the others alternatives")
    ap.add_argument("--quick", action="store_true", help="the fp16 memory only, no search comparison")
    ap.add_argument("--dev-variants", action="store_true",
                    help="--lib is the developer build: also time erase without the direct-copy branch and with a "
                         f"{DEV_SEGMENT}-row default segment")
    a = ap.parse_args()
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    segments = [int(s) for s in a.segments.split(",")]
    recs = run_memory(1 << 20, 768, "f16", segments, a.iters, True, not a.quick, dev=a.dev_variants)
    if not a.quick:
        recs += run_memory(1 << 20, 1024, "bf16", segments[:1], a.iters, False, False)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "lib": a.lib or "release",
                       "segments": segments, "env": {k: v for k, v in os.environ.items() if k.startswith("VIDMEM_ERASE")},
                       "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
