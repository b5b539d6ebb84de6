"""Text tower probe: one JSON record for the CLIP-L/14 text tower (specs.CLIP_L14_TEXT, synthetic weights).
  * single-question latency: B = 1, HIP-event-timed vm_text_encode calls (median, p99), at T = 77 and trimmed (T = 16,
    a question of 14 words);
  * throughput: sequences/s at B = 16 and B = 256, T = 77 (event-timed windows of back-to-back calls);
  * the per-category profile (vm_profile_read) of one B = 1 call and one B = 256 call.
   python tools/text_probe.py [dtype=f16] [out.json]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import vidmem  # noqa: F401
from _dev import maybe_dev; maybe_dev()
from vidmem import _lib, specs, synthetic
from vidmem.text import TextEncoder

dtype = sys.argv[1] if len(sys.argv) > 1 else "f16"
out_path = sys.argv[2] if len(sys.argv) > 2 else None
spec = specs.CLIP_L14_TEXT
enc = TextEncoder(spec, synthetic.text_encoder_weights(spec, seed=42), dtype=dtype, device=0)
rng = np.random.default_rng(0)


def ids_of(B, T, eot):
    a = rng.integers(0, spec["vocab"] - 1, size=(B, T)).astype(np.int32)
    a[:, eot] = spec["eot_id"]
    return torch.from_numpy(a).cuda()


def latency(B, T, n=300, warm=30):
    ids = ids_of(B, T, T - 1)
    ws = torch.empty(enc.workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
    for _ in range(warm):
        enc.encode_device(ids, workspace=ws)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:   # one call per event pair; the stream stays busy, so the host's enqueue cost is included
        a.record()
        enc.encode_device(ids, workspace=ws)
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return {"B": B, "T": T, "calls": n, "median_ms": float(np.median(ms)), "p99_ms": float(np.percentile(ms, 99)),
            "min_ms": float(ms.min())}


def throughput(B, T=77, seconds=1.5, reps=3):
    ids = ids_of(B, T, T - 1)
    ws = torch.empty(enc.workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
    for _ in range(5):
        enc.encode_device(ids, workspace=ws)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    enc.encode_device(ids, workspace=ws)
    torch.cuda.synchronize()
    n = max(10, int(seconds / max(time.perf_counter() - t0, 1e-4)))
    rates = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            enc.encode_device(ids, workspace=ws)
        b.record()
        torch.cuda.synchronize()
        rates.append(B * n / (a.elapsed_time(b) / 1e3))
    flops = specs.text_flops_per_sequence(spec, T)
    return {"B": B, "T": T, "calls": n, "seq_per_s": float(np.median(rates)), "seq_per_s_all": rates,
            "tflops": float(np.median(rates) * flops / 1e12)}


def profile(B, T=77):
    ids = ids_of(B, T, T - 1)
    ws = torch.empty(enc.workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
    enc.encode_device(ids, workspace=ws)
    enc.ctx.profile_enable(4096)
    enc.ctx.profile_read()
    enc.encode_device(ids, workspace=ws)
    prof = enc.ctx.profile_read()
    enc.ctx.profile_enable(0)
    return {"B": B, "T": T, "categories": {k: {"ms": v[0], "launches": v[1]} for k, v in prof.items() if v[1]}}


rec = {
    "probe": "text_probe", "spec": spec["arch"], "dtype": dtype, "device": torch.cuda.get_device_name(0),
    "gflop_per_seq_T77": specs.text_flops_per_sequence(spec, 77) / 1e9,
    "latency_b1": [latency(1, 77), latency(1, 16)],
    "throughput": [throughput(16), throughput(256)],
    "profile": [profile(1), profile(256)],
}
line = json.dumps(rec)
print(line)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
