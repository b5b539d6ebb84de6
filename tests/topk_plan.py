"""Pure-Python mirror of the cosine top-k dispatch (csrc/topk.hip make_plan / run_topk_kl, csrc/topk_emit.hip,
csrc/topk_gscan.hip): which kernels one ``vm_topk_cosine`` call launches for (Q, k, D, dtype, capacity, CUs).

A test helper, not a conftest.  tests/test_topk_paths_gpu.py pins every case to the path this mirror names (the
profile launch counts must match), and tests/test_topk_plan_cpu.py checks that its case table reaches every kernel
instantiation.  Each rule cites the line of the release build it restates; a retuned rule there must be retuned here.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

SAMPLE_ROWS = 16384       # topk.hip:690
EMIT_CAP = 4096           # vm_internal.h:76 VM_EMIT_CAP (the dense pass's row budget, the first limit's unit)
EM_QPB = 128              # topk_emit.hip:33 queries per superblock (16 per wave, 8 waves)
MAX_K_FAST = 58           # topk.hip vm_topk_cosine: k > 58 -> vm_topk_cosine_exact


def pick_kl(k: int) -> int:
    """topk.hip:697: the per-lane list length, k + 2 / k + 4 / k + 6 of slack."""
    if k + 2 <= 8:
        return 8
    if k + 4 <= 16:
        return 16
    if k + 6 <= 32:
        return 32
    return 64


def pick_qt(Q: int, KL: int, D: int) -> int:
    """topk.hip:698-702: query tiles of 16 per scan block, QT * KL <= 64, the query tile within 144 KiB of LDS."""
    qt_max = min(64 // KL, 4)
    need = (Q + 15) // 16
    qt = 4 if need >= 4 and qt_max >= 4 else (2 if need >= 2 and qt_max >= 2 else 1)
    while qt > 1 and qt * 16 * D * 2 > 144 * 1024:
        qt //= 2
    return qt


def emit_supported(Q: int, KL: int, D: int, cap: int) -> bool:
    """topk_emit.hip:560-571 vm_topk_emit_supported (release build: TOPK_EMIT = EMIT_KL32 = 1)."""
    ks = D // 128
    d_ok = D % 128 == 0 and ks in (1, 2, 4, 6, 8)
    return d_ok and (Q >= 49 or KL >= 32) and KL <= 64 and cap >= 65536


def gscan_supported(Q: int, rows: int, D: int, num_cus: int) -> bool:
    """topk_gscan.hip:406-415 vm_topk_gscan_supported: Q >= 129, >= 16,384 rows in the pass, enough 256 x 256 tiles
    for every CU to walk four; ``rows`` counts from the pass's limits and the capacity, not the rows stored."""
    if Q < 129 or rows < 16384:
        return False
    tiles = ((rows + 255) // 256) * ((Q + 255) // 256)
    return tiles >= 4 * num_cus and D % 128 == 0 and D <= 2048 and num_cus % 8 == 0


def cut_growth(Q: int) -> int:
    """topk.hip:810-812: the cascade's pass limits grow 32-fold for <= 128 queries (one superblock), 8-fold above."""
    return 32 if Q <= 128 else 8


def pass_limits(Q: int, cap: int) -> List[Tuple[int, Optional[int]]]:
    """topk.hip:819-830: the cascade's scan passes after the dense one, as [begin, limit) in physical slots; limit None
    = the last pass (INT64_MAX: up to the end of the stored rows).  The limits go 4096 g, 4096 g^2, ... and the pass
    that starts once a limit reaches the capacity is the last."""
    g = cut_growth(Q)
    out = []
    begin, limit = 0, EMIT_CAP * g
    while True:
        if limit >= cap:
            out.append((begin, None))
            return out
        out.append((begin, limit))
        begin, limit = limit, limit * g


@dataclass
class Pass:
    begin: int
    limit: Optional[int]      # None: to the end of the memory
    kind: str                 # "dense" | "emit" | "gscan"


@dataclass
class Plan:
    family: str               # "list" | "list+prepass" | "cascade" | "exact"
    dtype: str
    D: int
    KL: int = 0
    QT: int = 0
    KS: int = 0
    NG: int = 0
    passes: List[Pass] = field(default_factory=list)
    staged: Optional[bool] = None   # bf16 final finalize with the KL candidate rows in LDS (None: f16 / exact)
    launches: dict = field(default_factory=dict)  # profile category -> launches of one call

    @property
    def limits(self) -> List[int]:
        """The cascade's pass limits below the capacity (the later passes start at these slots)."""
        return [p.limit for p in self.passes if p.kind != "dense" and p.limit is not None]

    @property
    def instantiations(self) -> set:
        """Names of the kernel instantiations one call runs (the coverage check's units)."""
        dt = self.dtype
        if self.family == "exact":
            return {f"exact/{dt}"}
        out = set()
        if self.family in ("list", "list+prepass"):
            out.add(f"scan/{dt}/KL{self.KL}/QT{self.QT}")
        if self.family == "list+prepass":
            out.add(f"prepass/{dt}")
        for p in self.passes:
            out.add(f"gscan/{dt}" if p.kind == "gscan" else f"emit/{dt}/KS{self.KS}/NG{self.NG}")
        kinds = {p.kind for p in self.passes}
        if "gscan" in kinds and "emit" in kinds:
            out.add(f"mixed/{dt}")
        if self.staged is not None:
            out.add(f"finalize/{dt}/{'staged' if self.staged else 'unstaged'}")
        return out


def plan(Q: int, k: int, D: int, dtype: str, cap: int, num_cus: int = 256) -> Plan:
    """The kernels one vm_topk_cosine call launches (EmbeddingMemory.topk with exact=False)."""
    if k > MAX_K_FAST:   # memory.py topk / topk.hip vm_topk_cosine: only the exhaustive kernel
        return Plan("exact", dtype, D, launches={"topk_scan": 0, "topk_finalize": 0})
    KL = pick_kl(k)
    QT = pick_qt(Q, KL, D)
    p = Plan("list", dtype, D, KL=KL, QT=QT)
    # topk.hip:735 make_plan: the emit cascade needs the emit set of D and a memory of >= 4 samples
    if emit_supported(Q, KL, D, cap) and cap >= 4 * SAMPLE_ROWS:
        p.family = "cascade"
        p.KS = D // 128
        p.NG = 2 if p.KS <= 6 and Q > EM_QPB else 1     # topk_emit.hip:546-547 launch_emit_ng
        p.passes.append(Pass(0, None, "dense"))           # topk.hip:821: pass 0 has no cut (never gscan)
        for begin, limit in pass_limits(Q, cap):
            rows = (cap if limit is None else min(cap, limit)) - begin
            gs = begin % 256 == 0 and gscan_supported(Q, rows, D, num_cus)   # topk_emit.hip:585-587
            p.passes.append(Pass(begin, limit, "gscan" if gs else "emit"))
        n = len(p.passes)
        # every pass: one scan launch (emit or gscan: VM_PROF_TOPK_SCAN) and one compact (VM_PROF_TOPK_FINALIZE,
        # topk_emit.hip:606), then the final finalize (topk.hip:856)
        p.launches = {"topk_scan": n, "topk_finalize": n + 1}
    elif QT >= 2 and cap >= 4 * SAMPLE_ROWS:              # topk.hip:834: the sampled pre-pass and its finalize
        p.family = "list+prepass"
        p.launches = {"topk_scan": 2, "topk_finalize": 2}
    else:
        p.launches = {"topk_scan": 1, "topk_finalize": 1}
    if dtype == "bf16":   # topk.hip:858-863: stage the KL candidate rows when they fit in 96 KiB beside the query
        p.staged = D * 2 + KL * (D + 8) * 2 <= 96 * 1024
    return p


def dense_range(n: int, head: int) -> Tuple[int, int]:
    """vm_internal.h:61 dense_newest: physical slots [d0, d1) of the dense pass for n searchable rows, ring head."""
    end = head if head else n
    e_al = end & ~255
    if e_al >= 3840:
        return e_al - 3840, end
    return 0, min(n, 4095)
