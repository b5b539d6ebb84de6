"""GPU: grouped top-k (vm_topk_cosine_grouped, csrc/topk_group.hip) against tests/group_ref.py.

Bar: rows, keys and fp64 scores bit-identical to the oracle, on clustered memories (groups of near-identical rows:
the frames of one chunk) where the fast path must certify or send the query to the exhaustive redo.
"""
import numpy as np
import pytest
import torch

from tests import group_ref as G
from tests.search_checks import grouped_check
from tests.support import clustered, group_sizes, grouped_memory, queries_near

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("size", [1, 5, 16, "ragged"])
def test_group_sizes(dtype, D, size):
    sizes = group_sizes(600 if size != 1 else 4000, size, seed=D)
    rows, _ = clustered(sizes, D, dtype, seed=7 + D)
    mem = grouped_memory(rows, sizes, dtype)
    grouped_check(mem, queries_near(rows, 16, 3, dtype), 10, dtype, certified=True)


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("Q", [1, 16, 64, 300])
def test_k_and_q(k, Q):
    sizes = group_sizes(800, 5, 0)
    rows, _ = clustered(sizes, 768, "f16", seed=11)
    mem = grouped_memory(rows, sizes, "f16")
    grouped_check(mem, queries_near(rows, Q, Q + k, "f16"), k, "f16", certified=True)


@pytest.mark.parametrize("score_mode", [0, 1])
def test_min_score(score_mode):
    sizes = group_sizes(500, "ragged", 4)
    rows, _ = clustered(sizes, 768, "bf16", seed=12)
    mem = grouped_memory(rows, sizes, "bf16")
    q = queries_near(rows, 16, 5, "bf16")
    cut = 0.3 if score_mode == 0 else 0.65
    _, s, _ = grouped_check(mem, q, 64, "bf16", min_score=cut, score_mode=score_mode, certified=True)
    assert (s == 0.0).any() and (s > cut).any()  # the filter cut some lists short


def test_ties_lower_representative_wins():
    D = 768
    base = torch.randn(40, D, device="cuda").to(torch.float16)
    rows = base.clone()
    rows[3] = rows[1]                  # duplicate inside group 0 (rows 0-4): its lower copy represents it
    rows[12] = rows[1]                 # and across groups: group 2 (rows 10-14) ties group 0 exactly
    rows[27] = rows[1]
    sizes = [5] * 8
    mem = grouped_memory(rows, sizes, "f16")
    q = rows[1:2].clone()
    r, s, k = grouped_check(mem, q, 5, "f16")
    assert r[0, :3].tolist() == [1, 12, 27] and s[0, 0] == s[0, 1] == s[0, 2]
    assert k[0, :3].tolist() == [0, 2, 5]


def test_reappearing_key_is_a_new_group():
    rows, _ = clustered([4, 4, 4], 768, "f16", seed=3)
    mem = grouped_memory(rows, [4, 4, 4], "f16", keys=[7, 8, 7])
    r, _, k = grouped_check(mem, rows[:1].clone(), 3, "f16")
    assert k[0].tolist().count(7) == 2  # key 7 is two groups


def test_ring_wrap_and_overwritten_group():
    sizes = [7] * 73 + [4]       # 515 rows in a 500-row ring
    rows, _ = clustered(sizes, 768, "f16", seed=21)
    mem = grouped_memory(rows, sizes, "f16", capacity=500, ring=True)
    keys = mem.group_keys_host()
    assert len(keys) == 500 and keys[0] == keys[5] != keys[6]  # rows 15-20: the surviving part of the group of 14-20
    # rows 497-503 (group 71) straddle the physical wrap: slots 497-499 and 0-3
    grouped_check(mem, torch.stack([rows[499], rows[500], rows[15]]).contiguous(), 5, "f16")
    grouped_check(mem, queries_near(rows[15:].contiguous(), 16, 2, "f16"), 10, "f16", certified=True)


def test_one_group_of_10k_rows():
    sizes = [300, 10000, 300] + [7] * 200
    rows, _ = clustered(sizes, 768, "f16", seed=5, noise=0.02)
    mem = grouped_memory(rows, sizes, "f16")
    grouped_check(mem, queries_near(rows, 16, 1, "f16"), 10, "f16")
    grouped_check(mem, rows[500:501].clone(), 3, "f16")


def test_exact_variant_and_fast_path_agree():
    sizes = group_sizes(400, 16, 0)
    rows, _ = clustered(sizes, 1024, "bf16", seed=2)
    mem = grouped_memory(rows, sizes, "bf16")
    q = queries_near(rows, 16, 8, "bf16")
    a = grouped_check(mem, q, 20, "bf16", certified=True)
    b = grouped_check(mem, q, 20, "bf16", exact=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_singleton_groups_equal_row_topk():
    from vidmem.memory import EmbeddingMemory
    rows, _ = clustered([1] * 20000, 768, "f16", seed=31, noise=0.0)
    plain = EmbeddingMemory(20000, 768, "f16")
    plain.append(rows)
    mem = EmbeddingMemory(20000, 768, "f16", grouped=True)
    mem.append(rows, group=torch.arange(20000, device="cuda"))
    q = queries_near(rows, 16, 4, "f16")
    for k in (1, 10, 50):
        s0, r0 = plain.topk(q, k)
        s1, r1, _ = mem.topk_grouped(q, k)
        assert torch.equal(r0, r1) and np.array_equal(s0.cpu().numpy().view(np.int64), s1.cpu().numpy().view(np.int64))


def test_plain_append_on_grouped_memory_makes_singletons():
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory
    rows, _ = clustered([6], 768, "f16", seed=1)
    mem = EmbeddingMemory(16, 768, "f16", grouped=True)
    first = C_append_plain(mem, rows)
    assert first == 0
    assert mem.group_keys_host().tolist() == [-1, -2, -3, -4, -5, -6]
    _, r, _ = mem.topk_grouped(rows[:1].clone(), 6)
    assert sorted(r[0].tolist()) == list(range(6))
    assert _lib.VM_OK == 0


def C_append_plain(mem, rows):
    import ctypes as C
    from vidmem import _lib
    first = C.c_int64(0)
    mem.ctx.check(mem.L.vm_memory_append(mem.handle, C.c_void_p(rows.data_ptr()), rows.shape[0], C.byref(first),
                                         _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    mem.ids.extend([None] * rows.shape[0])
    mem.meta.extend([None] * rows.shape[0])
    return int(first.value)


def test_one_million_clustered_rows_redo_path():
    """1 M rows in groups of 16 plus planted near-ties: 100 groups hold an exact copy of one row, so every query that
    finds it sees more tied groups than candidate slots - flagged, redone on the device, still exact."""
    sizes = [16] * 62500
    rows, _ = clustered(sizes, 768, "f16", seed=99, noise=0.03)
    planted = rows[123456].clone()
    for g in range(100):
        rows[g * 625 * 16 + 3] = planted
    mem = grouped_memory_bulk(rows, 16)
    q = torch.stack([planted, rows[777], rows[500000], rows[999999]]).contiguous()
    grouped_check(mem, q, 10, "f16")
    flags = mem.last_group_flags[:4].cpu().numpy()
    assert flags[0] != 0 and (flags != 0).sum() >= 1
    assert mem.grouped_uncertified_count > 0


def grouped_memory_bulk(rows, size):
    from vidmem.memory import EmbeddingMemory
    n = rows.shape[0]
    mem = EmbeddingMemory(n, rows.shape[1], "f16", grouped=True)
    keys = torch.arange(n, device=rows.device) // size
    for c0 in range(0, n, 65536):
        mem.append(rows[c0:c0 + 65536], group=keys[c0:c0 + 65536])
    return mem


def test_graph_capture_replays_eager_result():
    from vidmem.memory import EmbeddingMemory
    sizes = [8] * 64
    rows, _ = clustered(sizes, 768, "f16", seed=41)
    q = queries_near(rows, 4, 6, "f16")
    eager = EmbeddingMemory(1024, 768, "f16", grouped=True)
    eager.append(rows[:256], group=torch.arange(256, device="cuda") // 8)
    eager.append(rows[256:], group=torch.arange(256, 512, device="cuda") // 8)
    want = eager.topk_grouped(q, 10)

    mem = EmbeddingMemory(1024, 768, "f16", grouped=True)
    mem.append(rows[:256], group=torch.arange(256, device="cuda") // 8)
    mem.prepare_topk_grouped(4, 10)
    keys2 = (torch.arange(256, 512, device="cuda") // 8).contiguous()
    src = rows[256:].contiguous()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(src, group=keys2)
            out = mem.topk_grouped(q, 10)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count (256)
    assert len(mem) == 256
    graph.replay()
    torch.cuda.synchronize()
    mem.sync()
    assert len(mem) == 512
    for a, b in zip(out, want):
        assert torch.equal(a, b)


def test_snapshot_restore_keeps_groups(tmp_path):
    from vidmem.memory import EmbeddingMemory
    sizes = group_sizes(100, "ragged", 6)
    rows, _ = clustered(sizes, 768, "f16", seed=8)
    mem = grouped_memory(rows, sizes, "f16")
    q = queries_near(rows, 8, 3, "f16")
    want = mem.topk_grouped(q, 10)
    path = str(tmp_path / "g.npz")
    mem.snapshot(path)
    back = EmbeddingMemory.restore(path)
    assert back.grouped
    got = back.topk_grouped(q, 10)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert back.new_group_key() == mem.new_group_key()


def test_reset_clears_group_state():
    from vidmem.memory import EmbeddingMemory
    rows, _ = clustered([4, 4], 768, "f16", seed=13)
    mem = EmbeddingMemory(64, 768, "f16", grouped=True)
    mem.append(rows[:4], group=5)
    mem.reset()
    mem.append(rows[4:], group=5)   # after a reset the same key opens a new group, not the old one
    mem.append(rows[:4], group=5)   # ... which this call continues
    _, r, k = mem.topk_grouped(rows[:1].clone(), 4)
    assert k[0].tolist() == [5, -1, -1, -1]


def test_select_overflow_path_on_a_million_tied_groups():
    """A zero query ties every one of 1 M singleton groups at 0.0: more groups reach the sampled cut than the
    compaction keeps, so the select runs its radix pass over all maxima; the answer is still the first k rows."""
    rows, _ = clustered([1] * (1 << 20), 768, "f16", seed=17, noise=0.0)
    mem = grouped_memory_bulk(rows, 1)
    q = torch.zeros((2, 768), dtype=torch.float16, device="cuda")
    q[1] = rows[4242]
    r, s, _ = grouped_check(mem, q, 20, "f16")
    assert r[0].tolist() == list(range(20)) and (s[0] == 0.0).all()
    assert r[1, 0] == 4242


def test_omitted_group_after_device_keys_opens_a_new_group():
    """An append without `group` is one new group even when the previous call's keys were a device tensor whose last
    key equals the memory's next counter value."""
    from vidmem.memory import EmbeddingMemory
    rows, _ = clustered([3, 3, 3], 768, "f16", seed=19)
    mem = EmbeddingMemory(16, 768, "f16", grouped=True)
    mem.append(rows[:3], group=torch.zeros(3, dtype=torch.int64, device="cuda"))
    mem.append(rows[3:6])
    mem.append(rows[6:9])
    keys = mem.group_keys_host()
    assert len(set(G.group_ids(keys).tolist())) == 3, keys
    _, r, _ = mem.topk_grouped(rows[:1].clone(), 3)
    assert sorted(r[0].tolist())[0] == 0 and len({x // 3 for x in r[0].tolist()}) == 3
