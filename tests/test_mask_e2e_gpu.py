"""GPU, end to end: the three uses of a row mask through the public interface - a search within the
results of another search, an exclusion ("next page"), a metadata filter - and the retrieval adapters' ``mask=``, each
against the oracle (tests/mask_ref.py statement (A), oracle.cref)."""
import asyncio
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mask_ref as MR
from tests.support import Embedder, bits, clustered, queries_near

pytestmark = pytest.mark.gpu

D, N = 768, 2000


@pytest.fixture(scope="module")
def world():
    """One memory of 50 scenes of 40 frames with ids and metadata, its host rows, and queries near stored frames."""
    from vidmem.memory import EmbeddingMemory
    rows, _ = clustered([40] * 50, D, "f16", seed=17)
    mem = EmbeddingMemory(N, D, "f16")
    mem.append(rows, ids=[f"frame{r}" for r in range(N)],
               meta=[{"camera": r % 4, "time": f"00:{r // 60:02d}-00:{r // 60:02d}", "content": f"c{r}"} for r in range(N)])
    q = queries_near(rows, 6, 23, "f16")
    return mem, rows, mem.rows_host()[1], q


def _same(got_s, got_r, want_r, want_s):
    assert np.array_equal(got_r.cpu().numpy(), want_r), (got_r[:2], want_r[:2])
    assert np.array_equal(got_s.cpu().numpy().view(np.int64), want_s.view(np.int64))


def test_search_within_the_results_of_a_range_search(world):
    """"The frames that show X, ranked by Y": range_search(qX) -> mask_of_rows on the device -> topk_masked(qY)."""
    mem, rows, host, _ = world
    qx = (rows[805].float() + 0.02 * torch.randn(D, device="cuda", generator=torch.Generator("cuda").manual_seed(1)))
    qx = qx.to(torch.float16)[None].contiguous()
    x = MR.cref.cosine_matrix(bits(qx), host)[0]
    srt = np.sort(x)[::-1]
    gaps = srt[10:200] - srt[11:201]                 # tau in the widest gap that leaves 11 .. 200 hits
    i = 10 + int(np.argmax(gaps))
    tau = float((srt[i] + srt[i + 1]) / 2)
    assert np.abs(x - tau).min() >= 4 * MR.cert_eps(D), "tau lies within 4 x cert_eps of an exact score"
    hit = x > tau
    assert 11 <= hit.sum() <= 200
    qy = queries_near(rows[800:840].contiguous(), 3, 5, "f16")
    hits = mem.enqueue_range(qx, tau, max_hits=256)  # rows [1, 256] on the device, -1 padded: nothing is read on the host
    m = mem.mask_of_rows(hits.rows)
    s, r = mem.topk_masked(qy, 10, m)
    assert mem.rows_of_mask(m) == hit.nonzero()[0].tolist()
    _same(s, r, *MR.masked_topk(bits(qy), host, np.tile(hit, (3, 1)), 10))
    assert hit[r.cpu().numpy()].all()


def test_next_page_by_excluding_the_rows_returned_so_far(world):
    mem, rows, host, q = world
    Q, k = 2, 10
    q = q[:Q].contiguous()
    want_r, want_s = MR.cref.cosine_topk(bits(q), host, 3 * k)
    mask = ~mem.new_mask(Q)                          # one mask per query: everything
    pages = []
    for page in range(3):
        s, r = mem.topk_masked(q, k, mask)
        pages.append((s, r))
        for i in range(Q):                           # "not the rows I have returned": on the device
            mask[i] &= ~mem.mask_of_rows(r[i])
    got_r = torch.cat([r for _, r in pages], dim=1).cpu().numpy()
    got_s = torch.cat([s for s, _ in pages], dim=1).cpu().numpy()
    assert np.array_equal(got_r, want_r), "pages 1-3 are not ranks 1 .. 3k of the exhaustive ranking"
    assert np.array_equal(got_s.view(np.int64), want_s.view(np.int64))
    assert len(mem.rows_of_mask(mask[0])) == N - 3 * k


def test_metadata_filter(world):
    mem, rows, host, q = world
    m = mem.mask_where(lambda row, id_, meta: meta["camera"] == 3 and id_ == f"frame{row}")
    sel = np.arange(N) % 4 == 3
    assert mem.rows_of_mask(m) == sel.nonzero()[0].tolist()
    s, r = mem.topk_masked(q, 20, m, min_score=0.05)
    _same(s, r, *MR.masked_topk(bits(q), host, np.tile(sel, (q.shape[0], 1)), 20, min_score=0.05))
    assert all(mem.meta_of(int(x))["camera"] == 3 for x in r.flatten().tolist() if x >= 0)


def test_adapters_take_a_mask(world):
    from vidmem import _lib
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    mem, rows, host, q = world
    sel = (np.arange(N) % 4 == 1) & (np.arange(N) >= 100)
    m = mem.mask_where(lambda row, id_, meta: meta["camera"] == 1 and row >= 100)
    q16 = q[0]
    vs = HipVectorSearch(mem, Embedder(q16.double().cpu().tolist()), SimpleNamespace(top_k_chunks=6), min_score=-1.0,
                         score_mode=_lib.VM_SCORE_RAW, mask=m)
    got = asyncio.run(vs._vector_search_chunks(None, "q"))
    want_r, want_s = MR.masked_topk(bits(q16[None]), host, sel[None], 6, min_score=-1.0)
    assert [c["id"] for c in got] == [f"frame{int(r)}" for r in want_r[0]] and len(got) == 6
    assert [c["score"] for c in got] == want_s[0].tolist()
    assert [c["content"] for c in got] == [f"c{int(r)}" for r in want_r[0]]
    # the pre-LLM similarity; a wrong-length query lists the first selected rows, a failed one nothing
    sim = HipPreLLMSimilarity(mem, SimpleNamespace(top_k_chunk_with_batch_similarity=3), mask=m)
    got = asyncio.run(sim._calculate_batch_similarities([q16, [0.0] * 5, RuntimeError("embedder"), rows[50]]))
    want_r, want_s = MR.masked_topk(bits(torch.stack([q16, rows[50]])), host, np.tile(sel, (2, 1)), 3)
    assert got[0] == [(f"frame{int(r)}", float(s)) for r, s in zip(want_r[0], want_s[0])]
    assert got[3] == [(f"frame{int(r)}", float(s)) for r, s in zip(want_r[1], want_s[1])]
    assert got[1] == [("frame101", 0.0), ("frame105", 0.0), ("frame109", 0.0)] and got[2] == []
    assert batch_similarities(mem, [q16], 3, mask=m) == got[:1]
    m.zero_()                                        # the adapter keeps the tensor: an emptied mask empties the answer
    assert asyncio.run(vs._vector_search_chunks(None, "q")) == []
