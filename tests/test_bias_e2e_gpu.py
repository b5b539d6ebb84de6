"""GPU, end to end: recency over two tagged synthetic videos (tests/bias_ref.py ``e2e_videos``).

"This, but rather the recent occurrences": ``EmbeddingMemory.bias_of_age`` builds the linear-recency column on the device
from the rows' tags, ``similarity.biased_similarities`` returns the ``(id, score)`` lists of statement (A) of the oracle,
and for at least one query they are not ``topk``'s order - which is asserted from the oracle's scores before any search.
A second round boosts the rows another retrieval leg found, through ``bias_of_rows``."""
import numpy as np
import pytest
import torch

from oracle import cref
from tests import bias_ref as BR
from tests import mask_ref as MR

pytestmark = pytest.mark.gpu


def _lists(want_r, want_s, names):
    return [[(names[r], float(s)) for r, s in zip(rr, ss) if r >= 0] for rr, ss in zip(want_r, want_s)]


def test_recency_reorders_the_hits_and_equals_the_oracle():
    from vidmem import similarity
    from vidmem.memory import EmbeddingMemory
    bits = BR.e2e_videos()
    tags = BR.e2e_tags()
    N, D = BR.E2E_N, BR.E2E_D
    rows = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16).cuda()
    names = [f"A{i}" for i in range(N)] + [f"B{i}" for i in range(N)]
    mem = EmbeddingMemory(256, D, "f16", tagged=True)
    mem.append(rows[:N], ids=names[:N], tag=tags[:N].tolist())
    mem.append(rows[N:], ids=names[N:], tag=tags[N:].tolist())
    g = torch.Generator(device="cuda").manual_seed(5)
    picks = [20, 45, N + 7, N + 52]
    queries = torch.stack([(rows[p].float() + 0.01 * torch.randn(D, device="cuda", generator=g)).to(torch.float16)
                           for p in picks])
    qbits = queries.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
    now_ms, per_ms, k = (N - 1) * BR.E2E_FRAME_MS, 2e-6, 6       # a frame loses 0.12 of score per minute of age
    col = BR.bias_from_tags_ref(tags, 0, 256, now_ms, per_ms, 0.0)
    # from the oracle first: recency changes the order of at least one query's hits, not merely their scores
    plain_r, _ = cref.cosine_topk(qbits, bits, k, dtype="f16")
    want_r, want_s = BR.bias_topk(qbits, bits, col[None], None, [1.0] * 4, None, k, capacity=256)
    assert any(plain_r[i].tolist() != want_r[i].tolist() for i in range(4))
    assert (want_s <= 1.0 + 1e-9).all() and (want_r >= 0).all()
    bias = mem.bias_of_age(now_ms, per_ms)                         # built on the device from the tags
    assert np.array_equal(bias.cpu().numpy().view(np.int32), col.view(np.int32))
    got = similarity.biased_similarities(mem, queries, bias, 1.0, k)
    assert got == _lists(want_r, want_s, names)
    _, topk_rows = mem.topk(queries, k)
    assert np.array_equal(topk_rows.cpu().numpy(), plain_r)
    assert any([i for i, _ in got[q]] != [names[r] for r in plain_r[q]] for q in range(4))
    # weight None is 1.0; a per-query weight, a threshold and the mask of video B
    assert similarity.biased_similarities(mem, queries, bias, None, k) == got
    only_b = mem.mask_of_scope((int(tags[N]), int(tags[-1])))
    sel = np.zeros((4, 2 * N), dtype=bool)
    sel[:, N:] = True
    assert np.array_equal(MR.selection(only_b.cpu().numpy().view(np.uint32), None, 4, 0, 2 * N, 256), sel)
    betas = [0.0, 1.0, 5.0, -1.0]
    for cut in (None, 0.5):
        want_r, want_s = BR.bias_topk(qbits, bits, col[None], None, betas, sel, 64, min_score=cut, capacity=256)
        got = similarity.biased_similarities(mem, queries, bias, betas, 64, mask=only_b, min_score=cut)
        assert got == _lists(want_r, want_s, names)
        assert all(i.startswith("B") for hits in got for i, _ in hits)
    # the graph leg found three chunks: their rows are boosted, nothing is excluded
    found = torch.tensor([3, N + 30, N + 31, -1], dtype=torch.int64, device="cuda")
    prior = mem.bias_of_rows(found, 0.25)
    pcol = BR.bias_from_rows_ref([3, N + 30, N + 31, -1], [0.25] * 4, 0, 2 * N, 256)
    assert np.array_equal(prior.cpu().numpy().view(np.int32), pcol.view(np.int32))
    want_r, want_s = BR.bias_topk(qbits, bits, np.stack([col, pcol]), [1, 0, 1, 1], [1.0] * 4, None, k, capacity=256)
    scores, got_rows = mem.topk_biased(queries, k, torch.stack([bias, prior]), bias_index=[1, 0, 1, 1])
    assert np.array_equal(got_rows.cpu().numpy(), want_r)
    assert np.array_equal(scores.cpu().numpy().view(np.int64), want_s.view(np.int64))
    assert similarity.biased_similarities(EmbeddingMemory(16, D, "f16"), queries, torch.zeros(64, device="cuda"), 1.0, 5) \
        == [[]] * 4
    mem.close()
