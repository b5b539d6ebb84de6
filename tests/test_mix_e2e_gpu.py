"""GPU, end to end: one round of relevance feedback over two synthetic videos (tests/mix_ref.py ``e2e_videos``).

Round one is a plain ``topk`` for a noisy frame of the first video.  Round two asks for "more like hits 2 and 5, less like
hit 3, and nothing I was already shown": ``similarity.feedback_terms`` builds the mixed query, the exclusion is the device
mask ``~mask_of_rows(first round's rows)``, and ``similarity.mix_similarities`` returns the ``(id, score)`` lists of
statement (A) of the oracle."""
import numpy as np
import pytest
import torch

from tests import mask_ref as MR
from tests import mix_ref as XR

pytestmark = pytest.mark.gpu


def test_a_feedback_round_excludes_what_was_shown_and_equals_the_oracle():
    from vidmem import similarity
    from vidmem.memory import EmbeddingMemory
    bits = XR.e2e_videos()
    N, D = XR.E2E_N, XR.E2E_D
    rows = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16).cuda()
    names = [f"A{i}" for i in range(N)] + [f"B{i}" for i in range(N)]
    mem = EmbeddingMemory(256, D, "f16")
    mem.append(rows[:N], ids=names[:N])
    mem.append(rows[N:], ids=names[N:])
    g = torch.Generator(device="cuda").manual_seed(5)
    query = (rows[20].float() + 0.01 * torch.randn(D, device="cuda", generator=g)).to(torch.float16)
    k = 6
    _, first = mem.topk(query[None], k)
    shown = first[0].tolist()
    assert shown[0] == 20 and all(0 <= r < N for r in shown)        # the frame's own neighbourhood in video A
    terms, weights = similarity.feedback_terms(query, positives=[rows[shown[2]], rows[shown[5]]], negatives=[rows[shown[3]]])
    assert terms.shape == (4, D) and weights == [1.0, 0.375, 0.375, -0.15]
    keep = ~mem.mask_of_rows(first)                                 # built on the device: the rows are not read here
    sel = np.ones((1, 2 * N), dtype=bool)
    sel[0, shown] = False
    assert np.array_equal(MR.selection(keep.cpu().numpy().view(np.uint32), None, 1, 0, 2 * N, 256), sel)
    tbits = terms.contiguous().view(torch.int16).numpy().view(np.uint16)[None]
    for top_k, cut in ((8, None), (8, 0.9), (64, None)):
        want_r, want_s = XR.mix_topk(tbits, [weights], bits, sel, top_k, min_score=cut)
        got = similarity.mix_similarities(mem, terms, weights, top_k, mask=keep, min_score=cut)
        assert len(got) == 1
        assert [i for i, _ in got[0]] == [names[r] for r in want_r[0] if r >= 0]
        assert [v for _, v in got[0]] == [v for v, r in zip(want_s[0].tolist(), want_r[0]) if r >= 0]
        assert not {i for i, _ in got[0]} & {names[r] for r in shown}
    assert len(got[0]) == 64                                        # 2 N - k rows were not shown
    # two feedback queries in one call, one mask each; an empty memory yields empty lists
    t2, w2 = similarity.feedback_terms(rows[N + 7], positives=[rows[N + 9]], negatives=[rows[3], rows[N + 30]])
    both = torch.stack([terms, t2])
    masks = torch.stack([keep, ~mem.new_mask()[0]])
    got = similarity.mix_similarities(mem, both, [weights, w2], 5, mask=masks)
    sel2 = np.concatenate([sel, np.ones((1, 2 * N), dtype=bool)])
    want_r, want_s = XR.mix_topk(both.view(torch.int16).numpy().view(np.uint16), [weights, w2], bits, sel2, 5)
    assert [[i for i, _ in hits] for hits in got] == [[names[r] for r in row] for row in want_r.tolist()]
    assert [[v for _, v in hits] for hits in got] == want_s.tolist()
    assert all(i.startswith("B") for i, _ in got[1])                # the second query lives in video B
    assert similarity.mix_similarities(EmbeddingMemory(16, D, "f16"), terms, weights, 5) == [[]]
    mem.close()
