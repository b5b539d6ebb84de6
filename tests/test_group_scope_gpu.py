"""GPU: scoped grouped top-k (vm_topk_cosine_grouped_scoped, csrc/topk_group_scope.hip) against tests/group_scope_ref.py.

Bar: rows, keys and fp64 score bits identical to the reference, for the fast and the ``exact=True`` entry on every case.

Section 1 reuses the shapes and scope sets of tests/test_tile_scan_gpu.py (D = 128 / 384, 17 / 33 / 47 rows and a ring of
40 after 57, Q = 1 / 16 / 17 / 33, k = 1) with group keys from its cluster sizes and tags interleaved row by row: every
multi-row group is half in scope, so a group's overall best row is hidden from about half the queries.  There the fast
path must answer alone (every per-query flag 0): the redo would hide a broken scan or select.  That is a demand on the
data, asserted from the oracle's in-scope group maxima before any GPU call: rank k and rank M + 1 more than
4 x cert_eps(D) apart (the certificate needs 2 x), or no rank M + 1.  The rows are test_tile_scan_gpu.dataset's, made
here from a seed of this file's own (SEEDS) so that a case that misses the gap gets another seed, never a skip.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import domain_ref as DR
from tests import group_ref as G
from tests import group_scope_ref as GS
from tests import range_ref as R
from tests import scope_ref as S
from tests.support import ALL, MS, bits, clustered, contiguous_tags, make_tag, mixed_scopes, queries_near, scope_of
from tests.tile_scan_data import CLUSTERS, K, QS, SHAPES, gap_ok, scope_sets, tags_of

pytestmark = pytest.mark.gpu

SEEDS = {}          # (D, dtype, shape) -> seed; default D + rows appended, test_tile_scan_gpu.dataset's


def gs_memory(rows, keys, tags, dtype, capacity=None, ring=False, step=65536):
    """A grouped and tagged memory holding `rows` with one key and one tag per row, appended `step` rows at a time."""
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(capacity or max(rows.shape[0], 16), rows.shape[1], dtype, ring=ring, grouped=True, tagged=True)
    keys = torch.as_tensor(np.asarray(keys, dtype=np.int64), device=rows.device)
    tags = torch.as_tensor(np.asarray(tags, dtype=np.int64), device=rows.device)
    step = min(step, mem.capacity)
    for c0 in range(0, rows.shape[0], step):
        mem.append(rows[c0:c0 + step], group=keys[c0:c0 + step], tag=tags[c0:c0 + step])
    return mem


def keys_of(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)


def compare(mem, q, k, scopes, want, min_score=None, score_mode=0, certified=False, label=""):
    """Fast and exact entry against `want` = (rows, scores, keys).  certified=True: every fast-path flag is 0."""
    out = None
    for exact in (False, True):
        s, r, kk = mem.topk_grouped_scoped(q, k, scopes, min_score=min_score, score_mode=score_mode, exact=exact)
        got_r, got_s, got_k = r.cpu().numpy(), s.cpu().numpy(), kk.cpu().numpy()
        if not exact:
            flags = mem.last_group_scope_flags[:q.shape[0]].cpu().numpy().copy()
            print(f"{label} k={k} Q={q.shape[0]} flagged={int((flags != 0).sum())}")
            out = (got_r, got_s, got_k, flags)
        assert np.array_equal(got_r, want[0]), (label, exact, np.argwhere(got_r != want[0])[:5], got_r[:2], want[0][:2])
        assert np.array_equal(got_k, want[2]), (label, exact)
        assert np.array_equal(got_s.view(np.int64), want[1].view(np.int64)), f"{label}: scores differ, exact={exact}"
        if certified and not exact:
            assert (flags == 0).all(), f"{label}: fast path flagged {int((flags != 0).sum())} of {q.shape[0]}: {flags[:8]}"
    return out


def check(mem, q, k, dtype, scopes, **kw):
    """`compare` with the reference computed from what the memory holds."""
    base, host_rows = mem.rows_host()
    want = GS.group_scoped_topk(bits(q), host_rows, mem.group_keys_host(), mem.tags_host(), scopes, k, dtype=dtype,
                                score_mode=kw.get("score_mode", 0), min_score=kw.get("min_score"), base=base)
    return compare(mem, q, k, scopes, want, **kw)


# ---- 1. small shapes where the scan can go wrong ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dataset(D, dtype, shape):
    """Host side of one shape: (rows, queries, base, cluster sizes, oracle score matrix [33, live rows])."""
    total, cap = SHAPES[shape]
    sizes, left = [], total
    while left:
        sizes.append(min(CLUSTERS[len(sizes) % len(CLUSTERS)], left))
        left -= sizes[-1]
    seed = SEEDS.get((D, dtype, shape), D + total)
    rows, _ = clustered(sizes, D, dtype, seed=seed, device="cpu")
    base = total - cap if cap else 0
    q = queries_near(rows[base:].contiguous(), max(QS), seed + 1, dtype)
    live = R.cref.cosine_matrix(bits(q), bits(rows[base:]), dtype=dtype)
    return rows, q, base, sizes, live


def in_scope_group_maxima(scores, gid, mask):
    """One query's exact maxima over the in-scope rows of every group that has one, descending."""
    return np.sort([scores[mask & (gid == g)].max() for g in np.unique(gid[mask])])[::-1]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_small_shapes_answered_by_the_fast_path_alone(D, dtype, shape):
    rows, q_all, base, sizes, live = dataset(D, dtype, shape)
    total, cap = SHAPES[shape]
    tags, keys = tags_of(total), keys_of(sizes)
    gid = G.group_ids(keys[base:])
    plan = []
    for Q in QS:                     # preconditions of flag 0 first, from the oracle's scores alone: no GPU call yet
        for name, scopes in scope_sets(Q, base, cap).items():
            lo, hi = S.scope_arrays(scopes, Q)
            for i in range(Q):
                maxima = in_scope_group_maxima(live[i], gid, S.scope_mask(tags[base:], lo[i], hi[i]))
                assert gap_ok(maxima, D), f"precondition: {shape} D={D} {dtype} {name} Q={Q} query {i}"
            plan.append((Q, name, scopes))
    mem = gs_memory(rows.cuda(), keys, tags, dtype, capacity=cap, ring=cap is not None, step=19)
    assert mem.rows_host()[0] == base and np.array_equal(mem.tags_host(), tags[base:])
    assert np.array_equal(mem.group_keys_host(), keys[base:])
    q_dev = q_all.cuda()
    for Q, name, scopes in plan:
        want = GS.group_scoped_topk_from_scores(live[:Q], keys[base:], tags[base:], scopes, K, base=base)
        compare(mem, q_dev[:Q].contiguous(), K, scopes, want, certified=True, label=f"{shape} {name}")
        if name == "one_empty":
            assert want[0][Q // 2, 0] == -1
    mem.close()


# ---- 2. identities -------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64))


@pytest.mark.parametrize("score_mode,min_score", [(0, None), (1, 0.65)])
def test_whole_scope_equals_the_grouped_search(score_mode, min_score):
    sizes = [5] * 800
    rows, _ = clustered(sizes, 128, "f16", seed=3)
    mem = gs_memory(rows, keys_of(sizes), contiguous_tags(4000, 8), "f16")
    q = queries_near(rows, 16, 9, "f16")
    for k in (1, 10, 50):
        s0, r0, k0 = mem.topk_grouped(q, k, min_score=min_score, score_mode=score_mode)
        for exact in (False, True):
            s1, r1, k1 = mem.topk_grouped_scoped(q, k, ALL, min_score=min_score, score_mode=score_mode, exact=exact)
            assert torch.equal(r0, r1) and torch.equal(k0, k1) and _bits_equal(s0, s1), (k, exact)


def test_singleton_groups_equal_the_scoped_search():
    rows, _ = clustered([5] * 800, 128, "bf16", seed=4)
    tags = contiguous_tags(4000, 8)
    mem = gs_memory(rows, np.arange(4000), tags, "bf16")
    q = queries_near(rows, 16, 9, "bf16")
    for k in (1, 10, 50):
        scopes = mixed_scopes(tags, 16, k)
        s0, r0 = mem.topk_scoped(q, k, scopes)
        for exact in (False, True):
            s1, r1, k1 = mem.topk_grouped_scoped(q, k, scopes, exact=exact)
            assert torch.equal(r0, r1) and _bits_equal(s0, s1), (k, exact)
            assert torch.equal(k1, torch.where(r1 >= 0, r1, -1))       # key = row id here


# ---- 3. scope meets group -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def events_memory():
    """64 events of 8 frames, one source, a frame every MS milliseconds."""
    sizes = [8] * 64
    rows, _ = clustered(sizes, 128, "f16", seed=5)
    return rows, gs_memory(rows, 100 + keys_of(sizes), np.arange(512) * MS, "f16")


def test_a_window_that_cuts_an_event_in_two():
    rows, mem = events_memory()
    window = (12 * MS, 27 * MS)                  # rows 12 .. 27: the second half of event 1, event 2, half of event 3
    q = torch.stack([rows[9], rows[13], rows[30], rows[20]]).contiguous()      # rows 9 and 30 are outside the window
    r, s, k, flags = check(mem, q, 5, "f16", window, certified=True, label="cut event")
    assert ((r[:, :3] >= 12) & (r[:, :3] <= 27)).all() and all(sorted(x) == [101, 102, 103] for x in k[:, :3].tolist())
    assert k[0, 0] == 101 and 12 <= r[0, 0] <= 15 and k[2, 0] == 103 and 24 <= r[2, 0] <= 27   # only the inside rows count
    assert r[1, 0] == 13 and r[3, 0] == 20
    assert (r[:, 3:] == -1).all() and (s[:, 3:] == 0.0).all() and (k[:, 3:] == -1).all()     # 3 in-scope groups, k = 5


def test_the_best_group_out_of_scope_is_never_returned():
    rows, mem = events_memory()
    q = rows[100:101].clone()                    # event 12 (rows 96 .. 103)
    for scopes in ((0, 95 * MS), (104 * MS, 511 * MS)):
        r, _, k, _ = check(mem, q, 10, "f16", scopes, certified=True, label="best group hidden")
        assert 112 not in k[0].tolist() and not ((r[0] >= 96) & (r[0] <= 103)).any() and (r[0] >= 0).all()


def test_empty_scopes_and_untagged_rows():
    from vidmem.memory import EmbeddingMemory
    rows, mem = events_memory()
    q = rows[40:42].clone()
    r, s, k, flags = check(mem, q, 4, "f16", [(10, 5), (600 * MS, 700 * MS)], certified=True, label="empty scope")
    assert (r == -1).all() and (s == 0.0).all() and (k == -1).all()
    # rows appended without a tag carry INT64_MIN: only a scope that starts there sees them
    mem2 = EmbeddingMemory(64, 128, "f16", grouped=True, tagged=True)
    mem2.append(rows[:16], group=torch.arange(16, device="cuda") // 4, tag=make_tag(0, 5))
    mem2.append(rows[16:32], group=4 + torch.arange(16, device="cuda") // 4)              # no tag
    mem2.append(rows[32:48], group=8 + torch.arange(16, device="cuda") // 4, tag=make_tag(1, 0))
    assert (mem2.tags_host()[16:32] == S.INT64_MIN).all()
    q = rows[20:21].clone()
    r, _, _, _ = check(mem2, q, 6, "f16", ALL, label="untagged/all")
    assert r[0, 0] == 20
    r, _, k, _ = check(mem2, q, 6, "f16", (S.INT64_MIN, S.INT64_MIN), label="untagged/min")
    assert r[0, 0] == 20 and sorted(k[0].tolist()) == [-1, -1, 4, 5, 6, 7]
    r, _, _, _ = check(mem2, q, 6, "f16", (S.INT64_MIN + 1, S.INT64_MAX), label="untagged/excluded")
    assert not ((r[0] >= 16) & (r[0] < 32)).any() and (r[0] >= 0).all()


def test_antiparallel_query_returns_negative_scores_and_no_hidden_group():
    g = torch.Generator(device="cuda").manual_seed(6)
    centre = torch.randn(128, generator=g, device="cuda")
    centre = centre / centre.norm()
    hidden, _ = clustered([8] * 5, 128, "f16", seed=7)                       # source 0: five unrelated events
    shown = centre + 0.02 * torch.randn(40, 128, generator=g, device="cuda")  # source 1: five events around one centre
    shown = (shown / shown.norm(dim=1, keepdim=True)).to(torch.float16)
    rows = torch.stack([hidden, shown], 1).reshape(80, 128).contiguous()      # interleaved row by row
    keys = np.arange(80) // 16                                                # every event: 8 rows of each source
    tags = np.where(np.arange(80) % 2 == 1, make_tag(1, 0), make_tag(0, 0)) + np.arange(80)
    mem = gs_memory(rows, keys, tags, "f16")
    q = (-centre).to(torch.float16)[None].contiguous()
    r, s, k, _ = check(mem, q, 10, "f16", scope_of(1), certified=True, label="antiparallel")
    assert (s[0, :5] < -0.9).all() and (r[0, :5] % 2 == 1).all() and sorted(k[0, :5].tolist()) == [0, 1, 2, 3, 4]
    assert (r[0, 5:] == -1).all() and (s[0, 5:] == 0.0).all() and (k[0, 5:] == -1).all()


@pytest.mark.parametrize("score_mode,min_score", [(0, 0.3), (1, 0.65)])
def test_min_score(score_mode, min_score):
    sizes = [5] * 800
    rows, _ = clustered(sizes, 128, "bf16", seed=8)
    tags = contiguous_tags(4000, 8)
    mem = gs_memory(rows, keys_of(sizes), tags, "bf16")
    q = queries_near(rows, 16, 5, "bf16")
    _, s, _, _ = check(mem, q, 64, "bf16", mixed_scopes(tags, 16, 64), min_score=min_score, score_mode=score_mode,
                       label=f"min_score mode {score_mode}")
    assert (s == 0.0).any() and (s > min_score).any()


def test_exact_duplicates_the_lower_in_scope_representative_wins():
    g = torch.Generator(device="cuda").manual_seed(9)
    rows = torch.randn(64, 128, generator=g, device="cuda").to(torch.float16)
    planted = rows[1].clone()                  # row 1 itself stays out of scope
    for r in (3, 5, 20, 45):
        rows[r] = planted                      # 3 and 5 in event 0, 20 in event 2, 45 in event 5
    mem = gs_memory(rows, np.arange(64) // 8, np.arange(64), "f16")
    r, s, k, _ = check(mem, planted[None].contiguous(), 4, "f16", (3, 40), label="duplicates")
    assert r[0, :2].tolist() == [3, 20] and k[0, :2].tolist() == [0, 2] and s[0, 0] == s[0, 1]
    assert 1 not in r[0].tolist() and 45 not in r[0].tolist()


# ---- 4. every route to the redo stays exact and says why ------------------------------------------------------------
def test_more_tied_groups_than_the_slack_is_a_gap():
    from vidmem import _lib
    g = torch.Generator(device="cuda").manual_seed(2)
    rows = torch.randn(3000, 128, generator=g, device="cuda").to(torch.float16)
    tags = contiguous_tags(3000, 3)
    planted = rows[5].clone()
    dup = list(range(1010, 1970, 24))          # 40 in-scope copies in 40 events of 8: k = 10 keeps 18 candidates
    for r in dup + [100, 2500]:
        rows[r] = planted
    mem = gs_memory(rows, np.arange(3000) // 8, tags, "f16")
    before = mem.group_scoped_uncertified_count
    r, _, k, flags = check(mem, planted[None].contiguous(), 10, "f16", scope_of(1), label="many ties")
    assert r[0].tolist() == dup[:10] and k[0].tolist() == [d // 8 for d in dup[:10]]
    assert flags[0] == _lib.VM_FLAG_GAP and mem.group_scoped_uncertified_count == before + 1


def test_an_in_scope_group_longer_than_the_row_cap_is_an_overflow():
    from vidmem import _lib
    sizes = [8] * 50 + [5000] + [8] * 50
    rows, _ = clustered(sizes, 128, "f16", seed=5, noise=0.02)
    mem = gs_memory(rows, keys_of(sizes), np.arange(5800) * MS, "f16")
    q = torch.stack([rows[3000], rows[10]]).contiguous()
    r, _, k, flags = check(mem, q, 3, "f16", ALL, label="long group")
    assert k[0, 0] == 50 and flags[0] == _lib.VM_FLAG_OVERFLOW
    r, _, k, flags = check(mem, q, 3, "f16", (0, 399 * MS), label="long group hidden")   # the long event is out of scope
    assert 50 not in k.ravel().tolist() and (flags == 0).all()


@functools.lru_cache(maxsize=None)
def long_memory():
    """70,000 rows in 4,375 events of 16, one source, a frame every MS milliseconds: more groups than the select's sample
    of 2,048 and than its compaction buffer of 4,096, and 9 compaction slices."""
    n = 70000
    sizes = [16] * (n // 16)
    rows, _ = clustered(sizes, 128, "f16", seed=99)
    return rows, gs_memory(rows, keys_of(sizes), np.arange(n, dtype=np.int64) * MS, "f16")


@pytest.mark.parametrize("width", [160, 4375])
def test_narrow_scope_keeps_the_cut_above_the_empty_groups(width):
    """A window of 161 rows holds 11 of the 4,375 events - fewer than the M + 1 = 19 the cut asks its sample for, so the
    sampled cut comes out 0 and only the cut-at-least-1 rule keeps the 4,364 empty groups out: a cut of 0 would collect
    every group, overflow the compaction buffer and hand the finalize empty groups as candidates.  The query must be
    answered by the fast path alone (flag 0; 11 candidates are all re-scored, so the certificate asks nothing of the
    data).  A window of 1/16 of the rows (274 events, about 128 of them in the sample) takes the sampled cut."""
    rows, mem = long_memory()
    lo = 35003
    window = (lo * MS, (lo + width) * MS)        # cuts an event at either end
    g = torch.Generator(device="cuda").manual_seed(3)
    pick = lo + torch.randint(0, width, (4,), generator=g, device="cuda")
    q = (rows[pick].float() + 0.1 * torch.randn(4, 128, generator=g, device="cuda")).to(torch.float16)
    r, _, _, flags = check(mem, q, 10, "f16", window, certified=True, label=f"narrow scope {width}")
    assert ((r >= lo) & (r <= lo + width)).all()


def test_more_groups_at_the_cut_than_the_compaction_keeps_takes_the_radix_select():
    """A zero query ties all 4,275 in-scope events at 0.0: more groups at the cut than the compaction buffer of 4,096
    keeps, so the select runs its radix pass over all maxima, the 100 empty groups in front included.  The certificate
    does not apply to a zero query, so the fast path answers it alone: the first in-scope row of the first k in-scope
    events."""
    rows, mem = long_memory()
    q = torch.zeros((2, 128), dtype=torch.float16, device="cuda")
    q[1] = rows[40000]
    r, s, k, flags = check(mem, q, 20, "f16", (1600 * MS, 69999 * MS), label="radix select")
    assert r[0].tolist() == list(range(1600, 1920, 16)) and (s[0] == 0.0).all() and k[0].tolist() == list(range(100, 120))
    assert flags[0] == 0 and k[1, 0] == 2500


@pytest.mark.parametrize("name", DR.OUTSIDE)
def test_bf16_rows_outside_the_norm_domain_take_the_redo(name):
    from vidmem import _lib
    n, D, Q, k = 1500, 128, 16, 10
    ds = DR.domain_set(name, n, D, seed=11, device="cuda", pair_at=[700])
    tags = contiguous_tags(n, 6)
    mem = gs_memory(ds.rows, np.arange(n) // 5, tags, "bf16")
    _, qs, _, _, _ = ds.queries(Q, seed=79)
    _, _, _, flags = check(mem, qs, k, "bf16", mixed_scopes(tags, Q, k), label=f"domain {name}")
    assert (flags == _lib.VM_FLAG_GAP).all(), flags


# ---- 5. ring --------------------------------------------------------------------------------------------------------
def test_ring_wrap_and_overwritten_group():
    sizes = [7] * 73 + [4]           # 515 rows in a 500-row ring: rows 0 .. 14 are overwritten
    rows, _ = clustered(sizes, 128, "f16", seed=21)
    i = np.arange(515, dtype=np.int64)
    tags = (((i // 3) % 2) << 40) | (i * MS)                 # two sources alternating every 3 rows
    mem = gs_memory(rows, keys_of(sizes), tags, "f16", capacity=500, ring=True, step=250)
    keys = mem.group_keys_host()
    assert len(keys) == 500 and keys[0] == keys[5] != keys[6]   # rows 15 .. 20: what is left of the group of 14 .. 20
    # rows 497 .. 503 (group 71) straddle the physical wrap: slots 497 .. 499 and 0 .. 3
    q = torch.stack([rows[499], rows[500], rows[15], rows[499]]).contiguous()
    r, _, k, _ = check(mem, q, 5, "f16", [scope_of(0), scope_of(1), ALL, scope_of(1, MS * 500, MS * 503)], label="ring")
    assert k[0, 0] == 71 and k[1, 0] == 71 and r[2, 0] == 15 and k[3, 0] == 71 and 500 <= r[3, 0] <= 503
    check(mem, queries_near(rows[15:].contiguous(), 16, 2, "f16"), 10, "f16", [scope_of(j % 2) for j in range(16)],
          certified=True, label="ring 16")


# ---- 6. graph capture -----------------------------------------------------------------------------------------------
def test_graph_capture_append_and_search_replayed_with_new_windows():
    from vidmem.memory import EmbeddingMemory
    rows, _ = clustered([4] * 256, 128, "f16", seed=61)
    mem = EmbeddingMemory(2048, 128, "f16", grouped=True, tagged=True)
    mem.append(rows[:256], group=torch.arange(256, device="cuda") // 4, tag=torch.arange(256, device="cuda") * MS)
    Q, k, B = 4, 10, 128
    mem.prepare_topk_grouped_scoped(Q, k)
    src = rows[256:256 + B].clone()
    tg = torch.zeros(B, dtype=torch.int64, device="cuda")
    kg = torch.zeros(B, dtype=torch.int64, device="cuda")
    q = queries_near(rows, Q, 6, "f16")
    scope = torch.zeros((Q, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(src, group=kg, tag=tg)
            out_s, out_r, out_k = mem.topk_grouped_scoped(q, k, scope)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count
    assert len(mem) == 256
    for rep in range(3):
        first = 256 + rep * B
        src.copy_(rows[first:first + B])
        tg.copy_(make_tag(rep + 1, 0) + torch.arange(B, device="cuda") * MS)
        kg.copy_((first + torch.arange(B, device="cuda")) // 4)
        q.copy_(queries_near(rows[:first + B].contiguous(), Q, 10 + rep, "f16"))
        windows = [scope_of(rep + 1), scope_of(0, MS * 10, MS * 100), scope_of(rep + 1, MS * 5, MS * 60), (7, 3)]
        scope.copy_(torch.tensor(windows, dtype=torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        assert mem.sync() == first + B
        base, host_rows = mem.rows_host()
        want = GS.group_scoped_topk(bits(q), host_rows, mem.group_keys_host(), mem.tags_host(), windows, k, base=base)
        assert np.array_equal(out_r.cpu().numpy(), want[0]) and np.array_equal(out_k.cpu().numpy(), want[2])
        assert np.array_equal(out_s.cpu().numpy().view(np.int64), want[1].view(np.int64))
        assert (out_r[0] >= first).all() and (out_r[3] == -1).all()
        eager = mem.topk_grouped_scoped(q, k, scope)
        assert all(torch.equal(a, b) for a, b in zip(eager, (out_s, out_r, out_k)))


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory
    rows, _ = clustered([1] * 64, 128, "f16", seed=71)
    only_grouped = EmbeddingMemory(64, 128, "f16", grouped=True)
    only_grouped.append(rows, group=torch.arange(64, device="cuda") // 4)
    only_tagged = EmbeddingMemory(64, 128, "f16", tagged=True)
    only_tagged.append(rows, tag=torch.arange(64, device="cuda"))
    for m in (only_grouped, only_tagged):
        with pytest.raises(ValueError, match="grouped and tagged"):
            m.topk_grouped_scoped(rows[:1], 3, ALL)
    mem = gs_memory(rows, np.arange(64) // 4, np.arange(64), "f16")
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_grouped_scoped(rows[:2], k, ALL)
    with pytest.raises(ValueError, match="scopes"):
        mem.topk_grouped_scoped(rows[:2], 3, [(0, 1), (0, 1), (0, 1)])
    # the C entry points themselves refuse too, and touch neither the outputs nor the counters
    L = mem.L
    ws = mem.prepare_topk_grouped_scoped(2, 3).ws
    need = int(L.vm_topk_grouped_scoped_workspace_bytes(mem.handle, 2, 3))
    assert need > 0 and L.vm_topk_grouped_scoped_workspace_bytes(mem.handle, 2, 65) == 0
    sc = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    out_s = torch.full((2, 64), 7.0, dtype=torch.float64, device="cuda")
    out_r = torch.full((2, 64), 7, dtype=torch.int64, device="cuda")
    out_k = torch.full((2, 64), 7, dtype=torch.int64, device="cuda")
    unc = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    fl = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = _lib.current_stream_ptr()
    inv, nomem = _lib.VM_ERR_INVALID, _lib.VM_ERR_NOMEM
    cases = [(only_grouped.handle, 3, p(sc[0]), p(sc[1]), need, inv), (only_tagged.handle, 3, p(sc[0]), p(sc[1]), need, inv),
             (mem.handle, 3, None, p(sc[1]), need, inv), (mem.handle, 3, p(sc[0]), None, need, inv),
             (mem.handle, 65, p(sc[0]), p(sc[1]), need, inv), (mem.handle, 0, p(sc[0]), p(sc[1]), need, inv),
             (mem.handle, 3, p(sc[0]), p(sc[1]), need - 1, nomem)]
    for handle, k, lo, hi, nbytes, code in cases:
        rc = L.vm_topk_cosine_grouped_scoped(handle, p(rows), 2, k, lo, hi, 0, 0.0, 0, p(out_s), p(out_r), p(out_k),
                                             p(unc), p(fl), p(ws), nbytes, st)
        assert rc == code, (k, nbytes, rc)
        rc = L.vm_topk_cosine_grouped_scoped_exact(handle, p(rows), 2, k, lo, hi, 0, 0.0, 0, p(out_s), p(out_r),
                                                   p(out_k), p(ws), nbytes, st)
        assert rc == code, (k, nbytes, rc)
    torch.cuda.synchronize()
    assert (out_s == 7.0).all() and (out_r == 7).all() and (out_k == 7).all() and unc.item() == 7 and (fl == 7).all()
    rc = L.vm_topk_cosine_grouped_scoped(mem.handle, p(rows), 2, 3, p(sc[0]), p(sc[1]), 0, 0.0, 0, p(out_s), p(out_r),
                                         p(out_k), p(unc), p(fl), p(ws), need, st)
    assert rc == _lib.VM_OK and out_r[0, 0].item() == 0 and (fl == 0).all()       # the same call, valid: tag 0 is row 0
