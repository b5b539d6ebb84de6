"""CPU: the two statements of the novelty-gate oracle (tests/novelty_ref.py) against each other on the data recipe, the
host-side rules of the gated append (argument errors, config default, exported symbols) and the extractor's gated path
on host stand-ins."""
import json

import numpy as np
import pytest
import torch

from tests import novelty_ref as N

SEQUENCE = (16, 17, 1, 300, 16, 250, 600)


@pytest.mark.parametrize("sigma,tau", [(0.01, 0.9), (0.02, 0.7), (0.01, 0.95)])
@pytest.mark.parametrize("dtype,D", [("f16", 768), ("bf16", 1024)])
def test_two_statements_agree(dtype, D, sigma, tau):
    """(A) the greedy rule on the batch's own score matrix plus the exact top-1 over the memory before the call, against
    (B) the one-frame-at-a-time loop over the memory as it grows: same keep masks, same memories (bit patterns)."""
    x = N.clip(1200, 300, D, sigma, dtype)
    model = N.GatedMemory(D, dtype)
    off = 0
    fractions = []
    for B in SEQUENCE:
        batch = x[off:off + B]
        keep_b, mem_b = N.gate_loop(batch, tau, dtype, model.rows)
        first = model.total
        keep_a, row_of = model.append_novel(batch, tau, known=model.known(batch))
        assert np.array_equal(keep_a, keep_b), B
        assert np.array_equal(model.rows, mem_b), B
        # row_of: a kept row's own new id, in order; a dropped row names a row that exists and scores above tau
        assert row_of[keep_a].tolist() == list(range(first, model.total))
        assert ((row_of[~keep_a] >= 0) & (row_of[~keep_a] < model.total)).all()
        if B >= 16:
            fractions.append(keep_a.mean())
        off += B
    if tau < 0.95:       # tau inside or below the same-scene score range: no batch keeps or drops everything
        assert all(0.05 <= f <= 0.95 for f in fractions), fractions
    else:                # above it: every frame is new
        assert all(f == 1.0 for f in fractions), fractions


def test_dropped_rows_score_above_the_threshold_against_their_row():
    from oracle import cref
    dtype, D, tau = "bf16", 1024, 0.9
    x = N.clip(400, 100, D, 0.01, dtype)
    model = N.GatedMemory(D, dtype)
    for lo in (0, 150):
        batch = x[lo:lo + 150] if lo == 0 else x[lo:]
        keep, row_of = model.append_novel(batch, tau, known=model.known(batch))
        for i in np.nonzero(~keep)[0]:
            s = cref.cosine_matrix(batch[i:i + 1], model.rows[row_of[i]:row_of[i] + 1], dtype=dtype)[0, 0]
            assert s > tau


def _stand_in(tagged=False):
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory.__new__(EmbeddingMemory)      # host rules only: no device handle
    mem.tagged, mem.grouped, mem.dim = tagged, False, 8
    mem.device, mem.dtype = torch.device("cpu"), torch.float16
    return mem


def test_argument_checks_of_the_gated_append():
    mem = _stand_in()
    rows = torch.zeros((3, 8))
    s, r = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="not both"):
        mem.append_novel(rows, 0.5, against=None, known=(s, r))
    with pytest.raises(ValueError, match="not both"):
        mem.append_novel(rows, 0.5, against=(0, 5), known=(s, r))
    with pytest.raises(ValueError, match="tagged"):
        mem.append_novel(rows, 0.5, against=(0, 5))
    with pytest.raises(ValueError, match="against"):
        mem.append_novel(rows, 0.5, against="batch")
    with pytest.raises(ValueError, match="NaN"):
        mem.append_novel(rows, float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        mem.enqueue_append_novel(rows, float("nan"))
    with pytest.raises(ValueError, match="ids"):
        mem.append_novel(rows, 0.5, ids=["a", "b"])
    with pytest.raises(ValueError, match="meta"):
        mem.append_novel(rows, 0.5, meta=[{}])
    for bad in ((s[:2], r[:2]), (s, r[:2]), (torch.zeros((3, 0), dtype=torch.float64), torch.zeros((3, 0), dtype=torch.int64)),
                (s,), s):
        with pytest.raises(ValueError, match="known"):
            mem.append_novel(rows, 0.5, known=bad)
        with pytest.raises(ValueError, match="known"):
            mem.enqueue_append_novel(rows, 0.5, known=bad)
    with pytest.raises(ValueError, match="dimension"):
        mem.append_novel(torch.zeros((3, 9)), 0.5)
    big = torch.zeros((4097, 8))
    with pytest.raises(ValueError, match="4096"):
        mem.enqueue_append_novel(big, 0.5)
    with pytest.raises(ValueError, match="4096"):
        mem.append_novel(big, 0.5, against=None)
    with pytest.raises(ValueError, match="4096"):
        mem.append_novel(big, 0.5, known=(torch.zeros(4097, dtype=torch.float64), torch.zeros(4097, dtype=torch.int64)))


def test_streaming_session_checks_its_threshold_first():
    from vidmem.streaming import StreamingSession

    class Ring:
        ring = True
    with pytest.raises(ValueError, match="NaN"):
        StreamingSession(object(), Ring(), 16, 8, 8, novelty_threshold=float("nan"))
    with pytest.raises(ValueError, match="top_k"):
        StreamingSession(object(), Ring(), 16, 8, 8, top_k=0, novelty_threshold=0.9)


def test_config_default_is_off():
    from vidmem import config as cfg
    assert cfg.MEMORY_DEFAULTS["novelty_threshold"] is None
    assert cfg.from_dict({}).memory.novelty_threshold is None
    assert cfg.from_dict({"memory": {"novelty_threshold": 0.9}}).memory.novelty_threshold == 0.9
    assert cfg.section(object(), "memory", cfg.MEMORY_DEFAULTS).novelty_threshold is None


def test_library_exports_the_gated_append_and_abi_4():
    from vidmem import _lib
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_novelty_workspace_bytes", "vm_memory_append_novel"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_novelty_workspace_bytes(None, 16) == 0
    assert L.vm_memory_append_novel(None, None, 1, 0.5, None, None, 1, None, None, None, None, None, None, 0,
                                    None) == _lib.VM_ERR_INVALID


class _GateMemory:
    """Host stand-in for EmbeddingMemory whose append_novel is statement (A)."""
    searchable = 0          # the extractor does not search it (top_k = 0): append_novel(against="memory") does

    def __init__(self, D):
        self.model = N.GatedMemory(D, "f16")
        self.ids, self.calls = [], []

    def id_of(self, r):
        return self.ids[r]

    def append(self, emb, ids=None, meta=None):
        raise AssertionError("the gated extractor must not call append")

    def append_novel(self, emb, threshold, against="memory", known=None, ids=None, meta=None):
        from types import SimpleNamespace
        assert against == "memory" and known is None
        batch = emb.to(torch.float16).view(torch.int16).numpy().view(np.uint16)
        keep, row_of = self.model.append_novel(batch, threshold, known=self.model.known(batch))
        self.ids += [ids[i] for i in np.nonzero(keep)[0]]
        self.calls.append(len(ids))
        return SimpleNamespace(keep=torch.from_numpy(keep), row_of=torch.from_numpy(row_of), kept=int(keep.sum()))


@pytest.mark.parametrize("look_ahead", [1, 4])
def test_extractor_gated_path_on_host_stand_ins(tmp_path, monkeypatch, look_ahead):
    monkeypatch.chdir(tmp_path)
    import asyncio
    from types import SimpleNamespace
    from vidmem import extractor as X
    D, tau = 16, 0.95
    table = torch.from_numpy(np.random.default_rng(1).standard_normal((256, D)).astype(np.float32)).to(torch.float16)

    class FakeEnc:
        device = torch.device("cpu")

        def embed_frames(self, frames):         # a frame's embedding depends on its first pixel only
            return table[frames[:, 0, 0, 0].long()]

    class HostStager:
        def __init__(self, n, h, w, device): self.shape = (n, h, w, 3)
        def stage(self, fr): return torch.from_numpy(np.stack(fr))
        def get(self, ticket): return ticket
        def done(self, ticket): pass

    values = np.array([0, 0, 1, 1, 1, 2, 0, 3, 3, 4,   4, 4, 0, 5, 5, 6, 7, 7, 2, 8,   8, 8, 8, 8, 8, 8, 8, 8, 8, 8,
                       9, 9, 9, 9, 9], np.uint8)
    frames = np.zeros((35, 8, 8, 3), np.uint8) + values[:, None, None, None]
    p = tmp_path / "clip.npz"
    np.savez(p, frames=frames, fps=np.float64(10.0))
    cfg = SimpleNamespace(video=SimpleNamespace(chunk_size_seconds=1.0, frames_per_chunk=16),
                          encoder=SimpleNamespace(look_ahead_chunks=look_ahead),
                          memory=SimpleNamespace(novelty_threshold=tau))
    mem = _GateMemory(D)
    ex = X.FrameEmbeddingExtractor(cfg, FakeEnc(), mem, top_k=0, stager_factory=HostStager)
    out = asyncio.run(ex.process_video(str(p), str(tmp_path / "out.json")))
    res = json.load(open(out))["results"]
    # the reference, chunk by chunk
    bits = table.view(torch.int16).numpy().view(np.uint16)
    from oracle import cref
    m = cref.cosine_matrix(bits[:10], bits[:10])
    assert (m[~np.eye(10, dtype=bool)] < tau).all()          # distinct pixel values are distinct frames at this tau
    model = N.GatedMemory(D, "f16")
    assert [r["chunk_idx"] for r in res] == [0, 1, 2] and mem.calls == [10, 10, 10]
    run_id = json.load(open(out))["metadata"]["run_id"]
    want_ids = []
    for c, r in enumerate(res):
        batch = bits[values[10 * c:10 * c + 10]]
        keep, row_of = model.append_novel(batch, tau, known=model.known(batch))
        assert r["embedding_rows"] == row_of.tolist() and r["stored_frames"] == int(keep.sum())
        assert r["content"] == "[10 frame embeddings]" and r["similar"] == []
        want_ids += [f"{run_id}_{c}_{i}" for i in np.nonzero(keep)[0]]
    assert [r["stored_frames"] for r in res] == [5, 4, 0]
    assert res[0]["embedding_rows"] == [0, 0, 1, 1, 1, 2, 0, 3, 3, 4]
    assert res[2]["embedding_rows"] == [8] * 10
    assert mem.ids == want_ids and len(mem.ids) == model.total == 9       # ids for the kept rows only


def test_extractor_output_keys_are_unchanged_when_the_gate_is_off(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    import asyncio
    from types import SimpleNamespace
    from vidmem import extractor as X

    class FakeEnc:
        device = torch.device("cpu")
        def embed_frames(self, frames): return torch.zeros((frames.shape[0], 8))

    class FakeMem:          # accepts append(emb, ids, meta) and nothing else
        searchable = 0
        def __init__(self): self.n = 0
        def append(self, emb, ids=None, meta=None):
            first = self.n; self.n += emb.shape[0]; return first
        def id_of(self, r): return None

    class HostStager:
        def __init__(self, n, h, w, device): self.shape = (n, h, w, 3)
        def stage(self, fr): return torch.from_numpy(np.stack(fr))
        def get(self, ticket): return ticket
        def done(self, ticket): pass

    p = tmp_path / "clip.npz"
    np.savez(p, frames=np.zeros((20, 8, 8, 3), np.uint8), fps=np.float64(10.0))
    cfg = SimpleNamespace(video=SimpleNamespace(chunk_size_seconds=1.0, frames_per_chunk=4))
    ex = X.FrameEmbeddingExtractor(cfg, FakeEnc(), FakeMem(), top_k=3, stager_factory=HostStager)
    res = json.load(open(asyncio.run(ex.process_video(str(p), str(tmp_path / "o.json")))))["results"]
    assert set(res[0]) == {"time", "content", "chunk_idx", "processing_time", "group_time", "group_chunks",
                           "embedding_rows", "similar"}
    assert res[1]["embedding_rows"] == [4, 5, 6, 7]
