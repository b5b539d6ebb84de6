"""GPU: a streaming session with ``novelty_threshold`` - the captured graph searches, gates and appends; every push is
held against statement (A) of tests/novelty_ref.py on the session's own embeddings, over enough pushes to wrap a small
ring.  Without a threshold the session is today's."""
import numpy as np
import pytest
import torch

from oracle import cref
from tests import novelty_ref as N
from tests.novelty_feed import feed, threshold_between
from tests.support import bits

pytestmark = pytest.mark.gpu

B, CAP, K, H, W, PUSHES = 16, 48, 5, 224, 224, 10


def _setup():
    from vidmem import specs, synthetic as syn
    from vidmem.encoder import FrameEncoder
    spec = dict(specs.VIT_B16_224, layers=1)
    enc = FrameEncoder(spec, syn.encoder_weights(spec, seed=5), "f16")
    frames, owner = feed(31, 72, H, W)
    frames, owner = frames[:B * PUSHES], owner[:B * PUSHES]
    assert frames.shape[0] == B * PUSHES
    seed_rows = torch.from_numpy(syn.unit_rows(3, "seed", 8, 768)).to(torch.float16)
    return enc, frames, owner, seed_rows


def test_gated_session_matches_the_reference_push_by_push():
    from vidmem.memory import EmbeddingMemory
    from vidmem.streaming import StreamingSession
    enc, frames, owner, seed_rows = _setup()
    all_emb = torch.cat([enc.embed_frames(torch.from_numpy(frames[i:i + B]).cuda()) for i in range(0, len(frames), B)])
    tau = threshold_between(cref.cosine_matrix(bits(all_emb), bits(all_emb)), owner)
    mem = EmbeddingMemory(CAP, 768, "f16", ring=True)
    mem.append(seed_rows)
    sess = StreamingSession(enc, mem, B, H, W, top_k=K, warmup=1, novelty_threshold=tau)
    assert len(mem) == 8 and sess.rows_appended == 8         # warm-up and capture leave the user's memory untouched
    model = N.GatedMemory(768, "f16", capacity=CAP)
    model.rows = bits(seed_rows)
    model.tags = model.keys = np.zeros(8, np.int64)
    for step in range(PUSHES):
        chunk = torch.from_numpy(frames[step * B:(step + 1) * B]).cuda()
        emb, scores, rows = sess.push(chunk)
        kept = sess.kept_last_push                            # synchronises the session stream
        assert torch.equal(emb, all_emb[step * B:(step + 1) * B])
        lo, live = model.window()
        want_r, want_s = cref.cosine_topk(bits(emb), live, K, dtype="f16")
        want_r = np.where(want_r >= 0, want_r + lo, -1)
        assert np.array_equal(rows.cpu().numpy(), want_r), step
        assert np.array_equal(scores.cpu().numpy(), want_s), step
        want_keep, want_row_of = model.append_novel(bits(emb), tau, known=(want_s[:, 0], want_r[:, 0]))
        assert 0.05 <= want_keep.mean() <= 0.95
        assert np.array_equal(sess.keep.cpu().numpy().astype(bool), want_keep), step
        assert np.array_equal(sess.row_of.cpu().numpy(), want_row_of), step
        assert kept == int(want_keep.sum())
        assert sess.rows_appended == model.total
    assert model.total > CAP + 8                              # the ring wrapped
    # first showing of every source frame is what was stored, and nothing else
    first = np.r_[True, owner[1:] != owner[:-1]]
    assert model.total == 8 + int(first.sum())
    assert len(mem) == 8                                      # the host mirror lags until sync()
    assert sess.sync() == model.total and len(mem) == model.total and len(mem.ids) == len(mem)
    base, got = mem.rows_host()
    assert base == model.total - CAP and np.array_equal(got, model.rows[base:])
    # eager calls line up again afterwards
    nov = mem.append_novel(all_emb[:B], tau)
    want_keep, want_row_of = model.append_novel(bits(all_emb[:B]), tau, known=model.known(bits(all_emb[:B])))
    assert np.array_equal(nov.keep.cpu().numpy(), want_keep) and np.array_equal(nov.row_of.cpu().numpy(), want_row_of)


def test_session_without_a_threshold_is_todays():
    from vidmem.memory import EmbeddingMemory
    from vidmem.streaming import StreamingSession
    enc, frames, owner, seed_rows = _setup()
    mem = EmbeddingMemory(CAP, 768, "f16", ring=True)
    mem.append(seed_rows)
    sess = StreamingSession(enc, mem, B, H, W, top_k=K, warmup=1, novelty_threshold=None)
    assert sess.keep is None and sess.row_of is None
    with pytest.raises(ValueError):
        sess.kept_last_push
    hist = [seed_rows.cuda()]
    for step in range(4):
        chunk = torch.from_numpy(frames[step * B:(step + 1) * B]).cuda()
        emb, scores, rows = sess.push(chunk)
        torch.cuda.synchronize()
        assert torch.equal(emb, enc.embed_frames(chunk))
        allrows = torch.cat(hist)
        lo = max(0, allrows.shape[0] - CAP)
        want_r, want_s = cref.cosine_topk(bits(emb), bits(allrows[lo:]), K, dtype="f16")
        assert np.array_equal(rows.cpu().numpy(), np.where(want_r >= 0, want_r + lo, -1))
        assert np.array_equal(scores.cpu().numpy(), want_s)
        hist.append(emb.clone())
        assert sess.rows_appended == 8 + (step + 1) * B      # every frame is stored
    assert sess.sync() == 8 + 4 * B
    base, got = mem.rows_host()
    assert np.array_equal(got, bits(torch.cat(hist))[base:])
