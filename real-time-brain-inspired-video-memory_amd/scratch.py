"""The device buffers of the memory operations: one base class, one small subclass per kind.

Every operation of ``EmbeddingMemory`` that needs more than its arguments - a workspace, flag or counter arrays, output
buffers of a capturable call - takes them from a scratch.  The rule is the same for all of them:

  * a scratch is either the memory's own (``scratch=None``; ``prepare_*`` returns it) or owned by the caller, who keeps
    ONE instance per stream / captured graph: a hipGraph bakes the addresses in;
  * a scratch is never resized.  One that does not fit is REPLACED by a new object (``fit``), and the old buffers stay
    with whoever still references them - a graph that captured them keeps replaying on valid memory.

A kind states which ``vm_*_workspace_bytes`` entry sizes each of its workspaces and which named buffers it holds.
"""
from __future__ import annotations

import torch


NOVEL_MAX_ROWS = 4096            # rows per vm_memory_append_novel call


class Scratch:
    """The byte workspaces (``ws`` first, each at least 256 bytes) plus the buffers a kind names.  ``shape`` is what the
    kind is sized by, e.g. ``(Q, k)``, as ints."""

    workspaces = ()              # (attribute, the vm_*_workspace_bytes entry that sizes it), ``ws`` first

    @staticmethod
    def _shape(memory, *shape):
        """The shape a request is sized for: a kind clamps it here and adds what its buffers take from the memory."""
        return shape

    @staticmethod
    def _sized_by(*shape):
        """What the sizing entries take after the memory handle."""
        return shape

    @staticmethod
    def _buffers(*shape):
        """-> (name, dtype, dims, fill) per buffer.  ``dims[0]`` is the least length that serves ``shape``; the dims
        after it and the dtype must match exactly."""
        raise NotImplementedError

    def __init__(self, memory, *shape, at_least: "Scratch" = None):
        """``at_least``: a scratch of the same kind; no workspace or buffer comes out shorter than its."""
        self.shape = shape       # as ``_shape`` returned it
        args = self._sized_by(*shape)
        for attr, sizer in self.workspaces:
            need = max(int(getattr(memory.L, sizer)(memory.handle, *args)), 256)
            if at_least is not None:
                need = max(need, getattr(at_least, attr).numel())
            setattr(self, attr, torch.empty(need, dtype=torch.uint8, device=memory.device))
        for name, dtype, dims, fill in self._buffers(*shape):
            if at_least is not None:
                dims = (max(dims[0], getattr(at_least, name).shape[0]),) + dims[1:]
            setattr(self, name, torch.full(dims, fill, dtype=dtype, device=memory.device))

    @classmethod
    def for_(cls, memory, *shape):
        return cls(memory, *cls._shape(memory, *shape))

    def fits(self, memory, *shape) -> bool:
        """Whether a call of ``shape`` on ``memory`` can use these buffers: every buffer long enough (certain for the
        shape it was made for) and every workspace as large as the library asks - one sizing call each, per call."""
        shape = self._shape(memory, *shape)
        if shape != self.shape:
            for name, dtype, dims, _ in self._buffers(*shape):
                t = getattr(self, name)
                if t.shape[0] < dims[0] or t.shape[1:] != dims[1:] or t.dtype != dtype:
                    return False
        args = self._sized_by(*shape)
        for attr, sizer in self.workspaces:
            if getattr(self, attr).numel() < getattr(memory.L, sizer)(memory.handle, *args):
                return False
        return True

    def grown(self, memory, *shape) -> "Scratch":
        """A NEW scratch that fits ``shape``, to take the place of this one: the old buffers are left alone."""
        return self.for_(memory, *shape)

    def fit(self, memory, *shape) -> "Scratch":
        """This object when it fits, else ``grown``."""
        return self if self.fits(memory, *shape) else self.grown(memory, *shape)


def _rows(n: int):
    return (max(n, 1),)


class TopkScratch(Scratch):
    """What one stream of ``topk`` calls of up to (Q, k) needs: the scan workspace, the redo workspace ``redo_ws``, the
    per-query ``flags`` (int32 [Q]) and the uncertified counter ``uncert`` (int32 [1])."""

    workspaces = (("ws", "vm_topk_workspace_bytes"), ("redo_ws", "vm_topk_redo_workspace_bytes"))

    @staticmethod
    def _buffers(Q, k):
        return (("flags", torch.int32, _rows(Q), 0), ("uncert", torch.int32, (1,), 0))

    def grown(self, memory, Q, k) -> "TopkScratch":
        """As ``Scratch.grown``, and every workspace and buffer is at least what this call needs AND at least as long
        as it was (the library's sizes do not grow with Q and k: 0 above k = 58, and the scan's block count falls as Q
        rises); ``uncert`` is carried over."""
        new = TopkScratch(memory, *self._shape(memory, Q, k), at_least=self)
        new.uncert.copy_(self.uncert)
        return new


class _ScanScratch(Scratch):
    """The workspace and the per-query ``flags`` (int32 [Q]) of a grouped, scoped, masked, span, mixed, biased or diverse top-k of up to (Q, k).  The
    uncertified counters of these searches are the memory's, whichever scratch a call used."""

    @staticmethod
    def _buffers(Q, k):
        return (("flags", torch.int32, _rows(Q), 0),)


class GroupedTopkScratch(_ScanScratch):
    workspaces = (("ws", "vm_topk_grouped_workspace_bytes"),)


class ScopedTopkScratch(_ScanScratch):
    workspaces = (("ws", "vm_topk_scoped_workspace_bytes"),)


class MaskedTopkScratch(_ScanScratch):
    workspaces = (("ws", "vm_topk_masked_workspace_bytes"),)


class SpanTopkScratch(_ScanScratch):
    workspaces = (("ws", "vm_topk_span_workspace_bytes"),)


class MixTopkScratch(_ScanScratch):
    """The mixed-query top-k for up to ``C`` mixed queries (of up to 16 terms each) and ``k``."""

    workspaces = (("ws", "vm_topk_mix_workspace_bytes"),)


class FoldTopkScratch(_ScanScratch):
    """The any/all top-k for up to ``C`` fold queries (of up to 16 terms each) and ``k``."""

    workspaces = (("ws", "vm_topk_fold_workspace_bytes"),)


class BiasTopkScratch(_ScanScratch):
    """The biased top-k (cosine plus a per-row prior) for up to ``Q`` queries and ``k``."""

    workspaces = (("ws", "vm_topk_bias_workspace_bytes"),)


class DiverseTopkScratch(_ScanScratch):
    """The diverse (MMR) top-k for up to ``Q`` queries and a pool of ``pool`` rows each; also ``mmr`` (float64
    [Q x pool]): the value at which each row of the last call was picked."""

    workspaces = (("ws", "vm_topk_diverse_workspace_bytes"),)

    @staticmethod
    def _buffers(Q, pool):
        return (("flags", torch.int32, _rows(Q), 0), ("mmr", torch.float64, _rows(Q * pool), 0.0))


class GroupedScopedTopkScratch(_ScanScratch):
    workspaces = (("ws", "vm_topk_grouped_scoped_workspace_bytes"),)


class ClipScratch(Scratch):
    """The clip search for up to ``C`` clips of ``L`` frames with ``k`` hits each: the workspace (query tiles, fp32 score
    columns, window scores and keys, candidates, exact redo scores), ``flags`` (int32 [C]) and the ``scores`` / ``rows``
    outputs (C x k)."""

    workspaces = (("ws", "vm_topk_clip_workspace_bytes"),)

    @staticmethod
    def _buffers(C, L, k):
        return (("flags", torch.int32, _rows(C), 0), ("scores", torch.float64, _rows(C * k), 0.0),
                ("rows", torch.int64, _rows(C * k), -1))


class SeqScratch(Scratch):
    """The sequence search for up to ``C`` sequences of ``J`` steps with ``k`` hits each: the workspace (query tiles, fp32
    score columns, end scores and keys, candidates, the redo's two exact layers), ``flags`` (int32 [C]) and the ``scores``
    / ``rows`` (C x k) and ``step_rows`` / ``step_scores`` (C x k x J) outputs."""

    workspaces = (("ws", "vm_topk_seq_workspace_bytes"),)

    @staticmethod
    def _buffers(C, J, k):
        return (("flags", torch.int32, _rows(C), 0), ("scores", torch.float64, _rows(C * k), 0.0),
                ("rows", torch.int64, _rows(C * k), -1), ("step_rows", torch.int64, _rows(C * k * J), -1),
                ("step_scores", torch.float64, _rows(C * k * J), 0.0))


class NoveltyScratch(Scratch):
    """The gated append for batches of up to ``B`` rows (at most 4,096 reach the library at a time): the workspace
    (norms and pair bits), ``keep`` (int32 [B]), ``row_of`` (int64 [B]) and ``count`` (int32 [1])."""

    workspaces = (("ws", "vm_novelty_workspace_bytes"),)

    @staticmethod
    def _shape(memory, B):
        return (max(1, min(int(B), NOVEL_MAX_ROWS)),)

    @staticmethod
    def _buffers(B):
        return (("keep", torch.int32, (B,), 0), ("row_of", torch.int64, (B,), 0), ("count", torch.int32, (1,), 0))


class RangeScratch(Scratch):
    """The range search for up to ``Q`` queries with ``max_hits`` hits each: the workspace (candidate and hit bits, exact
    scores, chunk counts), ``counts`` and ``rescored`` (int64 [Q]) and the ``rows`` / ``scores`` outputs (Q x max_hits)."""

    workspaces = (("ws", "vm_range_workspace_bytes"),)

    @staticmethod
    def _shape(memory, Q, max_hits):
        return max(1, int(Q)), int(max_hits)

    @staticmethod
    def _sized_by(Q, max_hits):
        return (Q,)

    @staticmethod
    def _buffers(Q, max_hits):
        return (("counts", torch.int64, (Q,), 0), ("rescored", torch.int64, (Q,), 0),
                ("rows", torch.int64, _rows(Q * max_hits), -1), ("scores", torch.float64, _rows(Q * max_hits), 0.0))


class EventsScratch(Scratch):
    """The event segmentation: the workspace (flags and chunk prefixes), ``count`` (int64 [1]), ``first_rows`` (int64
    [max_events]), ``event_of`` (int64 [capacity]) and ``links`` (float64 [capacity])."""

    workspaces = (("ws", "vm_memory_events_workspace_bytes"),)

    @staticmethod
    def _shape(memory, max_events=0):
        return int(max_events), memory.capacity

    @staticmethod
    def _sized_by(max_events, capacity):
        return ()

    @staticmethod
    def _buffers(max_events, capacity):
        return (("count", torch.int64, (1,), 0), ("first_rows", torch.int64, _rows(max_events), -1),
                ("event_of", torch.int64, _rows(capacity), 0), ("links", torch.float64, _rows(capacity), 0.0))


class SummaryScratch(Scratch):
    """The group summaries for windows of up to ``max_groups`` groups: the workspace (group bounds, one score per slot),
    ``count`` (int64 [1]) and the per-group outputs ``first_rows`` / ``n_rows`` / ``keys`` / ``key_rows`` (int64),
    ``key_scores`` (float64) and ``centroids`` ([max_groups, D] of the memory's dtype)."""

    workspaces = (("ws", "vm_memory_summaries_workspace_bytes"),)

    @staticmethod
    def _shape(memory, max_groups):
        return int(max_groups), memory.dim, memory.dtype

    @staticmethod
    def _sized_by(max_groups, dim, dtype):
        return (max_groups,)

    @staticmethod
    def _buffers(max_groups, dim, dtype):
        m = _rows(max_groups)
        return (("count", torch.int64, (1,), 0), ("first_rows", torch.int64, m, -1), ("n_rows", torch.int64, m, -1),
                ("keys", torch.int64, m, -1), ("key_rows", torch.int64, m, -1), ("key_scores", torch.float64, m, 0.0),
                ("centroids", dtype, m + (dim,), 0))


class EraseScratch(Scratch):
    """Erase: the workspace (keep flags, their prefix, one segment of every column), ``new_row_of`` (int64 [capacity])
    and ``erased`` (int64 [1]).  Sized by ``segment_rows``, the rows that move through the workspace at a time (0 = the
    library's default)."""

    workspaces = (("ws", "vm_memory_erase_workspace_bytes"),)

    @staticmethod
    def _shape(memory, segment_rows=0):
        return int(segment_rows), memory.capacity

    @staticmethod
    def _sized_by(segment_rows, capacity):
        return (segment_rows,)

    @staticmethod
    def _buffers(segment_rows, capacity):
        return (("new_row_of", torch.int64, _rows(capacity), -1), ("erased", torch.int64, (1,), 0))

    def fits(self, memory, segment_rows=None) -> bool:
        """A call takes any erase scratch of the memory's capacity (``segment_rows=None``: no sizing call); asked for a
        ``segment_rows``, only the workspace of exactly that size fits - a different segment makes a new scratch."""
        if self.new_row_of.numel() < memory.capacity:
            return False
        return segment_rows is None or self.ws.numel() == max(256, int(
            memory.L.vm_memory_erase_workspace_bytes(memory.handle, int(segment_rows))))

    def grown(self, memory, segment_rows=None) -> "EraseScratch":
        return self.for_(memory, segment_rows or 0)
