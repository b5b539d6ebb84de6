"""GPU, end to end: a video shown twice is linked to its first showing (tests/span_ref.py ``e2e_videos``; that the data
allows it is proven from the oracle alone in tests/test_span_cpu.py).

Videos A, B, then A' = A plus small noise, one row per frame.  ``recall_links`` over the rows of A' with ``min_gap = 16``
returns the aligned row of A as each frame's best match; ``similarity.recall_links`` lists those rows' ids; and
``batch_similarities(span=...)`` equals the host ranking restricted to the span."""
import numpy as np
import pytest
import torch

from tests import span_ref as SR

pytestmark = pytest.mark.gpu


def _memory():
    from vidmem.memory import EmbeddingMemory
    bits = SR.e2e_videos()
    rows = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16).cuda()
    A, B = SR.E2E_A, SR.E2E_B
    mem = EmbeddingMemory(256, SR.E2E_D, "f16")
    names = [f"A{i}" for i in range(A)] + [f"B{i}" for i in range(B)] + [f"A'{i}" for i in range(A)]
    for c0, c1 in ((0, A), (A, A + B), (A + B, 2 * A + B)):          # three videos, three appends
        mem.append(rows[c0:c1], ids=names[c0:c1])
    return mem, bits, rows, names


def test_a_second_showing_links_to_the_first():
    from vidmem import similarity
    mem, bits, rows, names = _memory()
    A, B = SR.E2E_A, SR.E2E_B
    want_r, want_s = SR.links_ref(bits, 0, 3, first=A + B, count=A, min_gap=SR.E2E_GAP)
    s, r = mem.recall_links(first_row=A + B, n_rows=A, k=3, min_gap=SR.E2E_GAP, block=16)
    assert np.array_equal(r.cpu().numpy(), want_r)
    assert np.array_equal(s.cpu().numpy().view(np.int64), want_s.view(np.int64))
    assert r[:, 0].tolist() == list(range(A))                        # the aligned rows of A
    lists = similarity.recall_links(mem, first_row=A + B, n_rows=A, top_k=3, min_gap=SR.E2E_GAP)
    assert [hits[0][0] for hits in lists] == [f"A{i}" for i in range(A)]
    assert [[i for i, _ in hits] for hits in lists] == [[names[x] for x in row] for row in want_r.tolist()]
    assert [[v for _, v in hits] for hits in lists] == want_s.tolist()
    # every live row: the first frames have no past at this gap, and nothing links forward
    s_all, r_all = mem.recall_links(k=1, min_gap=SR.E2E_GAP)
    assert (r_all[:SR.E2E_GAP] == -1).all() and (r_all[SR.E2E_GAP:, 0] >= 0).all()
    assert (r_all[SR.E2E_GAP:, 0] <= torch.arange(2 * A + B, device="cuda")[SR.E2E_GAP:] - SR.E2E_GAP).all()
    assert similarity.recall_links(mem, first_row=0, n_rows=2, top_k=1, min_gap=SR.E2E_GAP) == [[], []]
    mem.close()


def test_batch_similarities_with_a_span_equals_the_host_ranking():
    from vidmem.similarity import batch_similarities
    mem, bits, rows, names = _memory()
    A, B = SR.E2E_A, SR.E2E_B
    q = rows[A + B + 5:A + B + 9]
    for span in ((A, A + B - 1), (None, A - 1), (A + B, None), (300, 400)):      # video B, video A, A', nothing
        want_r, want_s = SR.span_topk(bits[A + B + 5:A + B + 9], bits, [span] * 4, 5)
        got = batch_similarities(mem, list(q), 5, span=span)
        assert [[i for i, _ in hits] for hits in got] == [[names[x] for x in row if x >= 0] for row in want_r.tolist()]
        assert [[v for _, v in hits] for hits in got] == [[v for v, x in zip(vs, row) if x >= 0]
                                                          for vs, row in zip(want_s.tolist(), want_r.tolist())]
    got = batch_similarities(mem, [q[0], [0.0] * 7, ValueError("embed failed")], 3, span=(A + 2, None))
    assert [i for i, _ in got[1]] == names[A + 2:A + 5] and [v for _, v in got[1]] == [0.0] * 3      # the wrong-length rule
    assert got[2] == [] and got[0][0][0] == "A'5"
    mem.close()
