"""GPU: the sequence search through the memory's life - after erase, reset and re-append, and a novelty-gated append it
equals the oracle on ``rows_host()`` / ``tags_host()``; a stale mask after an erase means what its bits now select; a
captured graph is replayed after appends with the steps and the mask rewritten in place (at the default queue setting);
``similarity.seq_similarities`` returns the reference's list shape with the span of every hit."""
import numpy as np
import pytest
import torch

from tests import clip_ref as CL
from tests import mask_ref as MR
from tests import seq_ref as R
from tests.search_checks import make_memory
from tests.support import MS, contiguous_tags, dev_mask, from_bits, scope_of
from tests.test_seq_gpu import check

pytestmark = pytest.mark.gpu


def test_mutations_erase_reset_reappend_and_novel_append():
    n, J, G = 1600, 4, 3
    bits = CL.scene_video(n, 128, "f16", 81)
    tags = contiguous_tags(n, 4)
    mem = make_memory(bits, "f16", tags=tags, capacity=2048)
    chains = np.stack([s + 2 * np.arange(J) for s in (100, 395, 900, 1300)])       # 395 .. 401 crosses into video 1
    steps = R.steps_at(bits, "f16", chains, 2)
    got = check(mem, steps, 5, G, 8, "f16", label="before")
    assert np.array_equal(got[2][0, 0], chains[0]) and not np.array_equal(got[2][1, 0], chains[1])
    # a stale mask: built for rows 880 .. 940, then video 1 (rows 400 .. 799) goes and every later row moves down by 400
    stale = MR.pack_rows(range(880, 941), mem.capacity)[None]
    got = check(mem, steps, 5, G, 8, "f16", masks=stale, label="mask before the erase")
    assert np.array_equal(got[2][2, 0], chains[2])
    assert mem.erase(scope=scope_of(1)).count == 400
    got = check(mem, steps, 5, G, 8, "f16", label="after erase of a video")
    assert np.array_equal(got[2][2, 0], chains[2] - 400) and np.array_equal(got[2][3, 0], chains[3] - 400)
    got = check(mem, steps, 5, G, 8, "f16", masks=stale, label="stale mask after the erase")
    live = got[2][got[2] >= 0]
    assert live.size and (live >= 880).all() and (live <= 940).all()        # the bits speak about the rows now there
    assert mem.erase(rows=[102, 104]).count == 2                            # two rows of the first planted chain
    got = check(mem, steps, 5, G, 8, "f16", label="after erase of rows")
    assert not np.array_equal(got[2][0, 0], chains[0])
    mem.reset()
    got = check(mem, steps, 5, G, 8, "f16", label="after reset")
    assert (got[0] == -1).all()
    mem.append(from_bits(bits[800:1200], "f16"), tag=torch.from_numpy(tags[800:1200]).cuda())
    got = check(mem, steps, 5, G, 8, "f16", label="after re-append")
    assert np.array_equal(got[2][2, 0], chains[2] - 800)
    kept = mem.append_novel(from_bits(bits[1200:1500], "f16"), 0.9, tag=torch.from_numpy(tags[1200:1500]).cuda()).kept
    assert 0 < kept <= 300
    check(mem, steps, 5, G, 8, "f16", label="after a novelty-gated append")
    check(mem, steps, 5, 16, 8, "f16", label="after a novelty-gated append, G=16")


def test_graph_capture_append_and_sequence_search_replayed():
    from vidmem.memory import EmbeddingMemory
    J, G, k, B, Cn = 4, 3, 4, 128, 3
    bits = CL.scene_video(1024, 128, "f16", 61)
    rows = from_bits(bits, "f16")
    mem = EmbeddingMemory(2048, 128, "f16", tagged=True)
    mem.append(rows[:256], tag=torch.arange(256, device="cuda") * MS)                # source 0
    scratch = mem.prepare_topk_seq(Cn, J, k)
    src = rows[256:256 + B].clone()
    tg = torch.zeros(B, dtype=torch.int64, device="cuda")
    q = torch.zeros((Cn, J, 128), dtype=torch.float16, device="cuda")
    mask = mem.new_mask(2)
    index = torch.zeros(Cn, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            mem.append(src, tag=tg)
            got = mem.enqueue_topk_seq(q, k, max_step=G, min_sep=4, mask=mask, mask_index=index, max_gap_ms=100,
                                       scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    mem.sync()                     # the capture advanced only the host mirror: back to the device count
    assert len(mem) == 256
    for rep in range(3):
        n_new = 256 + (rep + 1) * B
        src.copy_(rows[256 + rep * B:n_new])
        tg.copy_(((rep + 1) << 40) + torch.arange(B, device="cuda") * MS)
        chains = np.stack([n_new - 1 - 2 * np.arange(J)[::-1], 100 + 3 * np.arange(J), 250 + 2 * np.arange(J)])
        steps = R.steps_at(bits, "f16", chains, 70 + rep)
        q.copy_(from_bits(steps, "f16"))
        words = np.stack([np.full(mem.mask_words, MR.FULL, np.uint32), MR.pack_rows(range(90 + rep, 120), mem.capacity)])
        mask.copy_(dev_mask(words))
        idx = [0, 1, 0] if rep != 1 else [0, 1, 9]
        index.copy_(torch.tensor(idx, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert mem.sync() == n_new
        base, host_rows = mem.rows_host()
        sel = MR.selection(words, idx, Cn, base, n_new, mem.capacity)
        want = R.seq_topk(steps, host_rows, k, G, 4, "f16", tags=mem.tags_host(), sel=sel, max_gap_ms=100, base=base)
        s_, r_, sr_, ss_ = (t.cpu().numpy() for t in got)
        assert np.array_equal(r_, want[0]) and np.array_equal(s_.view(np.int64), want[1].view(np.int64)), rep
        assert np.array_equal(sr_, want[2]) and np.array_equal(ss_.view(np.int64), want[3].view(np.int64)), rep
        assert np.array_equal(want[2][0, 0], chains[0]) and np.array_equal(want[2][1, 0], chains[1])
        assert not np.array_equal(want[2][2, 0], chains[2])          # 250 .. 256 crosses from source 0 into a new one


def test_similarity_adapter_returns_ids_scores_and_spans():
    from vidmem import similarity
    from vidmem.memory import EmbeddingMemory
    n, J, G = 600, 3, 4
    bits = CL.scene_video(n, 128, "f16", 91)
    mem = EmbeddingMemory(1024, 128, "f16")
    mem.append(from_bits(bits, "f16"), ids=[f"frame-{i}" for i in range(n)])
    chains = np.stack([s + 3 * np.arange(J) for s in (50, 400)])
    steps = from_bits(R.steps_at(bits, "f16", chains, 3), "f16")
    two = from_bits(R.steps_at(bits, "f16", chains[:1, :2], 4), "f16")
    entries = [steps[0], None, steps[1].float().cpu().tolist(), RuntimeError("embedder failed"), two[0]]
    hits, spans = similarity.seq_similarities(mem, entries, 3, max_step=G, min_sep=8)
    assert hits[1] == [] and hits[3] == [] and spans[1] == [] and spans[3] == []
    for i, c in ((0, 0), (2, 1)):
        s, r, sr, _ = mem.topk_seq(steps[c], 3, max_step=G, min_sep=8)
        assert hits[i] == [(f"frame-{int(a)}", float(b)) for a, b in zip(r[0].tolist(), s[0].tolist()) if a >= 0]
        assert spans[i][0] == (f"frame-{chains[c, 0]}", f"frame-{chains[c, -1]}")
        assert [e for _, e in spans[i]] == [h for h, _ in hits[i]]
    assert spans[4][0] == ("frame-50", "frame-53") and len(hits[4]) == 3
    empty = EmbeddingMemory(64, 128, "f16")
    assert similarity.seq_similarities(empty, [steps[0]], 3) == ([[]], [[]])
