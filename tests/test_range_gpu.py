"""GPU: the range search (vm_range_cosine / vm_range_cosine_exact, csrc/range.hip) against tests/range_ref.py.

Bar: rows, fp64 score bits, padding and counts identical to the oracle, for the fast and the exhaustive entry on every
case.  The oracle's score matrix of a data set is computed once (``dataset``) and shared: a fresh memory and a wrapped
ring over the same rows differ only in which columns are live.
"""
import functools

import numpy as np
import pytest
import torch

from tests import range_ref as R
from tests.search_checks import range_check, range_memory, raw_range
from tests.support import ALL, bits, clustered, contiguous_tags, mixed_scopes, queries_near, scope_of, tagged_memory

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def dataset(name):
    """(rows, queries, oracle score matrix [Q, n]) of the two clean-gap sets, made once."""
    if name == "f16":
        n, D, size, Q, seed = 40003, 768, 16, 49, 5
    else:
        n, D, size, Q, seed = 5003, 1024, 5, 130, 6
    sizes = [size] * (n // size) + ([n % size] if n % size else [])
    rows, _ = clustered(sizes, D, name, seed=seed)
    q = queries_near(rows, Q, seed + 1, name)
    return rows, q, R.cref.cosine_matrix(bits(q), bits(rows), dtype=name)


# ---- 1. clean gap --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True], ids=["fresh", "ring"])
@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_clean_gap(name, ring):
    """Clusters with in-cluster scores far above 0.2 and cross-cluster scores far below: no exact score lies within
    4 x cert_eps(D) of the threshold (asserted from the oracle's scores), so a row outside the hit set is provably no
    candidate and the scan may re-score the hits only: out_rescored == out_counts."""
    rows, q_all, matrix = dataset(name)
    n, D = rows.shape
    cap = None if not ring else (30011 if name == "f16" else 4001)        # below the rows appended: a wrapped ring
    mem = range_memory(rows, name, capacity=cap, ring=ring)
    base, host = mem.rows_host()
    assert host.shape[0] == (cap or n) and base == n - host.shape[0]
    assert np.array_equal(host[:3], bits(rows[base:base + 3]))
    live = matrix[:, base:]
    gap = np.abs(live - 0.2).min()
    print(f"{name} ring={ring}: nearest score to 0.2 is {gap / R.cert_eps(D):.0f} x cert_eps away")
    assert gap > 4 * R.cert_eps(D), "precondition: an exact score lies within 4 x cert_eps of the threshold"
    for Q in (1, 17, 49) + ((130,) if name == "bf16" else ()):
        q = q_all[:Q].contiguous()
        want = R.range_from_scores(live[:Q], 0.2, base=base)
        counts, resc = range_check(mem, q, 0.2, want, label=f"{name} Q={Q} 0.2")
        assert counts.sum() > 0 and np.array_equal(resc, counts), (resc[:8], counts[:8])
        everything = R.range_from_scores(live[:Q], -1.0, base=base)
        counts, _ = range_check(mem, q, -1.0, everything, max_hits=100, label=f"{name} Q={Q} -1")
        assert (counts == host.shape[0]).all()
        range_check(mem, q, 2.0, R.range_from_scores(live[:Q], 2.0, base=base), max_hits=5, label=f"{name} Q={Q} 2.0")
    # the Python entry on the same memory: trimmed lists, the full count, -inf = everything
    found = mem.range_search(q_all[:17], 0.2)
    for (r, s, c), got in zip(R.range_from_scores(live[:17], 0.2, base=base), found):
        assert got.count == c and np.array_equal(got.rows.cpu().numpy(), r)
        assert np.array_equal(got.scores.cpu().numpy().view(np.int64), s.view(np.int64))
    assert torch.equal(mem.last_range_rescored[:17].cpu(), torch.tensor([f.count for f in found]))
    cut = mem.range_search(q_all[:2], float("-inf"), max_hits=9, exact=True)
    assert [f.count for f in cut] == [host.shape[0]] * 2 and cut[1].rows.tolist() == list(range(base, base + 9))


# ---- 2. inside the bound ---------------------------------------------------------------------------------------------
def test_threshold_inside_the_fp32_bound():
    """2,000 near-identical rows whose scores all lie within cert_eps of the threshold, about half on each side: fp32
    cannot decide any of them, the exact re-scoring has to."""
    D = 768
    g = torch.Generator(device="cuda").manual_seed(17)
    others, _ = clustered([1] * 3000, D, "f16", seed=18)
    centre = torch.randn(D, generator=g, device="cuda")
    tight = centre[None] + 0.001 * torch.randn(2000, D, generator=g, device="cuda")
    tight = (tight / tight.norm(dim=1, keepdim=True)).to(torch.float16)
    rows = torch.cat([others[:1700], tight, others[1700:]]).contiguous()
    q = (tight[:1].float() + 0.1 * torch.randn(1, D, generator=g, device="cuda")).to(torch.float16)
    m = R.cref.cosine_matrix(bits(q), bits(rows), dtype="f16")
    inside = m[0, 1700:3700]
    tau = float(np.median(inside))
    spread = np.abs(inside - tau).max() / R.cert_eps(D)
    mem = range_memory(rows, "f16")
    want = R.range_from_scores(m, tau)
    counts, resc = range_check(mem, q, tau, want, label="inside the bound")
    print(f"inside the bound: counts={counts.tolist()} rescored={resc.tolist()} spread={spread:.2f} x cert_eps")
    assert 0 < counts[0] < 2000 and (resc >= counts).all()


# ---- 3. the strict `>` -------------------------------------------------------------------------------------------------
def test_strict_threshold_duplicates_and_zero_vectors():
    D = 768
    rows, _ = clustered([5] * 600, D, "f16", seed=23)
    rows = rows.clone()
    dup = list(range(1000, 3000, 20))                 # 100 exact copies of one row
    for r in dup:
        rows[r] = rows[40]
    rows[77] = 0                                      # a zero row
    q = queries_near(rows, 4, 3, "f16").clone()
    q[1] = rows[40]
    q[3] = 0                                          # a zero query
    mem = range_memory(rows, "f16")
    m = R.cref.cosine_matrix(bits(q), bits(rows), dtype="f16")
    for mode in (0, 1):
        for qi, r in ((0, 123), (1, 40), (2, 2999)):
            s = float(R.shown(m[qi, r], mode))
            for tau, present in ((s, False), (float(np.nextafter(s, -np.inf)), True)):
                want = R.range_from_scores(m, tau, score_mode=mode)
                assert (r in want[qi][0].tolist()) == present
                range_check(mem, q, tau, want, score_mode=mode, label=f"strict mode={mode} q={qi}")
                if r == 40:                           # the copies are all in or all out together, in row order
                    got = [x for x in want[1][0].tolist() if x in set(dup + [40])]
                    assert got == ([40] + dup if present else [])
    want = R.range_from_scores(m, -0.5)
    range_check(mem, q, -0.5, want, label="zero row")
    for qi in range(3):
        i = want[qi][0].tolist().index(77)
        assert want[qi][1][i] == 0.0
    assert want[3][0].tolist() == list(range(3000)) and (want[3][1] == 0.0).all()
    assert R.range_from_scores(m, 0.0)[3][2] == 0
    range_check(mem, q, 0.0, R.range_from_scores(m, 0.0), label="zero query at 0.0")
    range_check(mem, q, 0.4, R.range_from_scores(m, 0.4, score_mode=1), score_mode=1, label="zero query, unit interval")


# ---- 4. scopes ---------------------------------------------------------------------------------------------------------
def test_scopes_mixed_null_and_refused():
    from vidmem import _lib
    rows, _ = clustered([5] * 800, 768, "f16", seed=31)
    tags = contiguous_tags(4000, 8)
    mem = tagged_memory(rows, tags, "f16")
    q = queries_near(rows, 16, 7, "f16")
    m = R.cref.cosine_matrix(bits(q), bits(rows), dtype="f16")
    scopes = mixed_scopes(tags, 16, 10)
    for tau in (0.2, -1.0):
        want = R.range_from_scores(m, tau, tags=tags, scopes=scopes)
        counts, _ = range_check(mem, q, tau, want, scopes=scopes, label=f"mixed scopes {tau}")
        assert counts[0] == 0 and counts[1] == 0 and counts[6] > 0
    assert range_check(mem, q, -1.0, R.range_from_scores(m, -1.0, tags=tags, scopes=scopes), scopes=scopes)[0][2] == 1
    # both scopes NULL = [INT64_MIN, INT64_MAX]
    whole = R.range_from_scores(m, 0.2)
    range_check(mem, q, 0.2, whole, scopes=None, label="null scopes")
    range_check(mem, q, 0.2, whole, scopes=ALL, label="whole scope")
    # the Python entry takes what topk_scoped takes
    got = mem.range_search(q, 0.2, scope=scopes)
    for (r, _, c), g in zip(R.range_from_scores(m, 0.2, tags=tags, scopes=scopes), got):
        assert g.count == c and g.rows.tolist() == r.tolist()
    # refusals of the C entry
    lo = torch.zeros(16, dtype=torch.int64, device="cuda")
    plain = range_memory(rows, "f16")
    for exact in (False, True):
        assert raw_range(plain, q, 0.2, lo_hi=(lo, lo), exact=exact)[0] == _lib.VM_ERR_INVALID
        assert raw_range(mem, q, 0.2, lo_hi=(lo, None), exact=exact)[0] == _lib.VM_ERR_INVALID
        assert raw_range(mem, q, 0.2, lo_hi=(None, lo), exact=exact)[0] == _lib.VM_ERR_INVALID
    with pytest.raises(ValueError, match="tagged"):
        plain.range_search(q, 0.2, scope=ALL)
    # a plain and a grouped memory answer the unscoped call
    range_check(plain, q, 0.2, whole, label="plain")
    range_check(range_memory(rows, "f16", grouped=True), q, 0.2, whole, label="grouped")


# ---- 5. truncation and independence -------------------------------------------------------------------------------------
def test_truncation_stride_and_independence_of_the_other_queries():
    from vidmem import _lib
    rows, q_all, matrix = dataset("bf16")
    mem = range_memory(rows, "bf16")
    q = q_all[:49].contiguous()
    want = R.range_from_scores(matrix[:49], 0.2)
    full = np.array([c for _, _, c in want])
    assert full.max() > 1
    for max_hits in (0, 1, 7):                        # 0: a count-only call on NULL output pointers
        counts, _ = range_check(mem, q, 0.2, want, max_hits=max_hits, label=f"max_hits={max_hits}")
        assert np.array_equal(counts, full)
    range_check(mem, q, 0.2, want, stride=8, offset=3, label="stride 8 offset 3")
    # one query alone returns the bits it returns as the 31st of 49
    width = int(full.max()) + 3
    _, r49, s49, c49, x49 = raw_range(mem, q, 0.2, max_hits=width)
    _, r1, s1, c1, x1 = raw_range(mem, q[30:31].contiguous(), 0.2, max_hits=width)
    assert c1[0] == c49[30] and x1[0] == x49[30]
    assert np.array_equal(r1[0], r49[30]) and np.array_equal(s1[0].view(np.int64), s49[30].view(np.int64))
    for exact in (False, True):
        assert raw_range(mem, q, float("nan"), max_hits=4, exact=exact)[0] == _lib.VM_ERR_INVALID
    with pytest.raises(ValueError, match="NaN"):
        mem.range_search(q, float("nan"))


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------
def test_graph_capture_append_and_range_search_replayed():
    from vidmem.memory import EmbeddingMemory
    MS = 33
    rows, _ = clustered([4] * 256, 768, "f16", seed=61)
    mem = EmbeddingMemory(2048, 768, "f16", tagged=True)
    mem.append(rows[:256], tag=torch.arange(256, device="cuda") * MS)          # source 0
    Q, B, H = 4, 128, 16
    scratch = mem.prepare_range(Q, H)
    src = rows[256:256 + B].clone()
    tg = torch.zeros(B, dtype=torch.int64, device="cuda")
    q = queries_near(rows, Q, 6, "f16")
    scope = torch.zeros((Q, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(src, tag=tg)
            hits = mem.enqueue_range(q, 0.2, scope=scope, max_hits=H, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count
    assert len(mem) == 256
    for rep in range(3):
        src.copy_(rows[256 + rep * B:256 + (rep + 1) * B])
        tg.copy_(((rep + 1) << 40) + torch.arange(B, device="cuda") * MS)
        q.copy_(queries_near(rows[:256 + (rep + 1) * B].contiguous(), Q, 10 + rep, "f16"))
        windows = [scope_of(rep + 1), scope_of(0, MS * 10, MS * 100), ALL, (7, 3)]
        scope.copy_(torch.tensor(windows, dtype=torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        assert mem.sync() == 256 + (rep + 1) * B
        base, host_rows = mem.rows_host()
        want = R.range_hits(bits(q), host_rows, 0.2, tags=mem.tags_host(), scopes=windows, dtype="f16", base=base)
        want_r, want_s, want_c = R.padded(want, H)
        assert np.array_equal(hits.counts.cpu().numpy(), want_c)
        assert np.array_equal(hits.rows.cpu().numpy(), want_r)
        assert np.array_equal(hits.scores.cpu().numpy().view(np.int64), want_s.view(np.int64))
        assert want_c[3] == 0 and want_c[2] > 0
        assert (want_r[0][want_r[0] >= 0] >= 256 + rep * B).all()
