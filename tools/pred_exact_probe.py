"""The exhaustive (``exact=True``) entries of the scoped, the masked and the scoped grouped search, event-timed and warm:
the callers of topk_redo_scan_kernel under the TagScope and MaskScope predicates and of group_redo_scan_kernel under
TagScope; and those of the mixed, the any/all and the biased search, the callers of
mix_redo_scan_kernel and bias_redo_scan_kernel.

  python tools/pred_exact_probe.py [--iters 5] [--out run.json] [--lib other/libvidmem.so]

Memory: 100,000 x 768 fp16, clustered rows in groups of 16, tag = row id; Q = 16, k = 10.  Row sets: everything, and a
contiguous tenth, each as a tag range (topk_scoped, topk_grouped_scoped) and as the mask of that range (topk_masked).  The
scored searches run on the same memory: ``topk_mix`` and ``topk_fold`` (max) at C = 4, J = 4, ``topk_biased`` at Q = 16 with
one bias column, over everything without a mask (NoScope) and over the tenth under its mask (MaskScope).  The variants
take turns (scope_probe.py's ``alternate``).
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
from scope_probe import alternate  # noqa: E402

N, D, DTYPE, Q, K = 100_000, 768, "f16", 16, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libvidmem.so to time (an A/B against a parent commit)")
    a = ap.parse_args()
    if a.lib:
        vidmem._lib.LIB_PATH = os.path.abspath(a.lib)
    rows = clustered(N, D, 16, DTYPE, seed=16)
    ids = torch.arange(N, device="cuda")
    mem = EmbeddingMemory(N, D, DTYPE, grouped=True, tagged=True)
    for c0 in range(0, N, 65536):
        mem.append(rows[c0:c0 + 65536], group=ids[c0:c0 + 65536] // 16, tag=ids[c0:c0 + 65536])
    g = torch.Generator(device="cuda").manual_seed(7)
    bias = mem.new_bias()
    bias[0, :N] = torch.rand(N, generator=g, device="cuda") * 0.25
    recs = []
    for name, (lo, hi) in (("100%", (0, N - 1)), ("10% contiguous", (N // 3, N // 3 + N // 10 - 1))):
        pick = torch.randint(lo, hi + 1, (Q,), generator=g, device="cuda")
        q = (rows[pick].float() + 0.1 * torch.randn((Q, D), generator=g, device="cuda")).to(TD[DTYPE])
        sc = torch.tensor([(lo, hi)] * Q, dtype=torch.int64, device="cuda")
        mask = mem.mask_of_scope((lo, hi))
        terms = q.reshape(4, 4, D).contiguous()
        w = torch.tensor([[1.0, 1.0, -0.5, 1.0]] * 4, dtype=torch.float64, device="cuda")
        sm = None if name == "100%" else mask
        ms = alternate({"scoped_exact": lambda: mem.topk_scoped(q, K, sc, exact=True),
                        "masked_exact": lambda: mem.topk_masked(q, K, mask, exact=True),
                        "grouped_scoped_exact": lambda: mem.topk_grouped_scoped(q, K, sc, exact=True),
                        "mix_exact": lambda: mem.topk_mix(terms, w, K, mask=sm, exact=True),
                        "fold_exact": lambda: mem.topk_fold(terms, K, op="max", weights=w, mask=sm, exact=True),
                        "biased_exact": lambda: mem.topk_biased(q, K, bias, mask=sm, exact=True)}, a.iters)
        s0, r0 = mem.topk_scoped(q, K, sc, exact=True)
        s1, r1 = mem.topk_masked(q, K, mask, exact=True)
        rec = {"rows": N, "D": D, "dtype": DTYPE, "selection": name, "Q": Q, "k": K,
               "scoped_exact_ms": round(ms["scoped_exact"], 4), "masked_exact_ms": round(ms["masked_exact"], 4),
               "grouped_scoped_exact_ms": round(ms["grouped_scoped_exact"], 4),
               "mix_exact_ms": round(ms["mix_exact"], 4), "fold_exact_ms": round(ms["fold_exact"], 4),
               "biased_exact_ms": round(ms["biased_exact"], 4),
               "equal": bool(torch.equal(r0, r1) and torch.equal(s0, s1))}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
