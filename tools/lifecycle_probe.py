"""The lifecycle scripts of tests/test_lifecycle_gpu.py once more outside pytest, timed, with the queries every
checkpoint sent to the exhaustive redo.

  python tools/lifecycle_probe.py [--out profiles/lifecycle.json] [--parent parent.json]

Per script and dtype: the wall time from the memory's creation to its close, the number of checkpoints, and after every
checkpoint the ``*_uncertified_count`` of each reader (cumulative per memory) - the masked, span, mixed, diverse, biased,
any/all and sequence searches included; the span counter also counts the pages of ``recall_links``.  The counts are recorded, not asserted;
what the checkpoint asserts is the per-query flag wherever a feature's oracle condition says the fast path must certify.
``--parent``: the file this tool wrote at the parent commit on the same machine in the same session; its seconds are
recorded beside the new ones as ``parent_seconds``.
"""
import argparse
import json
import os
import pathlib
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vidmem  # noqa: E402,F401
from tests import lifecycle_ref as LC  # noqa: E402
from tests.test_lifecycle_gpu import run_life  # noqa: E402

LIVES = [("test_linear_life", LC.linear_script, 1600, False), ("test_ring_life", LC.ring_script, 600, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/lifecycle.json")
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    tests = {}
    with tempfile.TemporaryDirectory() as tmp:
        for warm in (True, False):          # the first pass loads every kernel and builds the data pools
            for name, script, cap, ring in LIVES:
                for dtype in ("f16", "bf16"):
                    record = run_life(script, dtype, cap, ring, pathlib.Path(tmp))[2]
                    if not warm:
                        tests[f"{name}[{dtype}]"] = record
    if args.parent:
        with open(args.parent) as f:
            parent = json.load(f)["tests"]
        tests = {name: {"seconds": rec["seconds"], "parent_seconds": parent[name]["seconds"],
                        **{k: v for k, v in rec.items() if k != "seconds"}} for name, rec in tests.items()}
    out = {"device": torch.cuda.get_device_name(0),
           "note": "uncertified = queries (clips) each reader's fp32 stage sent to the exhaustive redo since the memory "
                   "was created, read after every checkpoint; recorded, not asserted (the checkpoint asserts the "
                   "per-query flags of the masked, span, mixed, diverse, biased, any/all and sequence searches where "
                   "their oracle conditions say the fast path must certify).  seconds = one warm run of the script, memory creation to close, the "
                   "host oracle's time included; parent_seconds = the same at the parent commit (fourteen readers), same "
                   "machine, same session.",
           "tests": tests}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["seconds"], v["checkpoints"]) for k, v in tests.items()}))


if __name__ == "__main__":
    main()
