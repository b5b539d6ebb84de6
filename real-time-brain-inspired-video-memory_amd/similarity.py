"""Drop-in replacements for the reference's similarity call sites, backed by EmbeddingMemory (HIP).

Same names, argument meaning, return shapes and error convention as the reference:

  * ``HipPreLLMSimilarity._calculate_batch_similarities(chunk_embeddings, neo4j_handler)``
        <- PreLLMInjector._calculate_batch_similarities, src/components/pre_llm_injector.py:346-372
        returns List[Q] of List[<=k] of (chunk_id, score); an Exception entry yields [] (:357-359);
        k = embedder_config.top_k_chunk_with_batch_similarity.
  * ``merge_batch_similarities``          <- the max-merge of src/components/pre_llm_injector.py:238-249
        (host-side dict logic of the CALLER, kept as the reference has it).
  * ``HipVectorSearch._vector_search_chunks(session, query)``
        <- HybridRetriever._vector_search_chunks, src/pipeline/retriever_hybrid.py:284-323
        returns List[{id,time,content,score,source:"vector"}]; any failure -> [] (:321-323).
  * ``HipVectorSearch._post_compress_chunks(query, chunks)``
        <- HybridRetriever._post_compress_chunks, src/pipeline/retriever_hybrid.py:465-514
        keeps segments with cosine >= compression_threshold in encounter order, then [:top_k];
        any failure -> chunks unchanged (:512-514).

Hot-path helpers never raise (they log and degrade), exactly like the reference; programmer errors
(shape / dtype, VidmemError VM_ERR_INVALID) do.
"""
from __future__ import annotations

import logging
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .memory import EmbeddingMemory

logger = logging.getLogger("vidmem.similarity")


def merge_batch_similarities(batch_similarities: Sequence[Sequence[Tuple[str, float]]],
                             top_k_similar_batch: int) -> List[Tuple[str, float]]:
    """src/components/pre_llm_injector.py:238-249: max score per chunk id (first-seen order), stable descending
    sort, first ``top_k_similar_batch``."""
    final_scores: Dict[str, float] = {}
    for chunk_similarities in batch_similarities:
        for chunk_id, score in chunk_similarities:
            if chunk_id not in final_scores or score > final_scores[chunk_id]:
                final_scores[chunk_id] = score
    final_score_list = sorted(final_scores.items(), key=lambda x: x[1], reverse=True)
    return final_score_list[:top_k_similar_batch]


def _length(e) -> int:
    return int(e.shape[-1]) if isinstance(e, torch.Tensor) else len(e)


def _check_distinct(memory: EmbeddingMemory, distinct: bool) -> None:
    if distinct and not getattr(memory, "grouped", False):
        raise ValueError("distinct=True needs a grouped memory (EmbeddingMemory(..., grouped=True), memory.group_by: chunk)")


def _check_scope(memory: EmbeddingMemory, scope, distinct: bool) -> None:
    """``scope`` together with ``distinct=True`` is accepted exactly when the memory object provides
    ``topk_grouped_scoped`` (EmbeddingMemory does; the memory must then be grouped and tagged); any other memory object
    is refused, because ``topk_scoped`` ranks rows and ``topk_grouped`` ranks groups of the whole memory."""
    if scope is None:
        return
    if distinct and not callable(getattr(memory, "topk_grouped_scoped", None)):
        raise ValueError("scope together with distinct=True needs a memory that provides topk_grouped_scoped "
                         "(EmbeddingMemory(..., grouped=True, tagged=True)): the scoped search ranks rows, not groups")
    if not getattr(memory, "tagged", False):
        raise ValueError("scope needs a tagged memory (EmbeddingMemory(..., tagged=True), memory.tag_by: time)")


def _check_mask(mask, scope, distinct: bool) -> None:
    """``mask`` (a row mask of the memory, EmbeddingMemory.topk_masked) stands alone: a scope is a mask already
    (``mask_of_scope``, combined with ``&``), and the masked search ranks rows, not groups."""
    if mask is None:
        return
    if scope is not None:
        raise ValueError("mask and scope are mutually exclusive: combine them as mask & memory.mask_of_scope(scope)")
    if distinct:
        raise ValueError("mask and distinct=True are mutually exclusive: the masked search ranks rows, not groups")


def _check_span(span, scope, mask, distinct: bool) -> None:
    """``span`` (one inclusive row-id range ``(lo, hi)`` for every query, ``None`` = open; EmbeddingMemory.topk_span)
    stands alone: a scope and a mask are other ways to choose rows, and the span search ranks rows, not groups."""
    if span is None:
        return
    if scope is not None:
        raise ValueError("span and scope are mutually exclusive: a span names row ids, a scope tags")
    if mask is not None:
        raise ValueError("span and mask are mutually exclusive: set the span's rows in the mask (memory.mask_of_rows)")
    if distinct:
        raise ValueError("span and distinct=True are mutually exclusive: the span search ranks rows, not groups")
    if isinstance(span, torch.Tensor) or not hasattr(span, "__len__") or len(span) != 2 or \
            any(hasattr(b, "__len__") for b in span):
        raise ValueError("span is one pair (lo, hi) of row ids for every query; None is an open bound")


def _span_rows(memory: EmbeddingMemory, span) -> range:
    """The live row ids one span holds, ascending."""
    last = len(memory) - 1
    first = last - memory.searchable + 1
    return range(first if span[0] is None else max(first, int(span[0])),
                 (last if span[1] is None else min(last, int(span[1]))) + 1)


def batch_similarities(memory: EmbeddingMemory, chunk_embeddings: Sequence, top_k: int, distinct: bool = False,
                       scope=None, mask=None, span=None) -> List[List[Tuple[str, float]]]:
    """One batched top-k launch for every non-failed query; result re-threaded into the reference's list shape.

    A query whose length differs from the stored vectors' scores 0.0 against EVERY row in the reference
    (``_cosine_similarity``: ``if len(vec1) != len(vec2): return 0.0``, src/components/pre_llm_injector.py:378-379), and
    the stable descending sort (:369) then keeps memory order: the answer is the first ``top_k`` stored chunks, each
    with score 0.0.  That is reproduced on the host (no arithmetic involved) instead of raising.

    ``distinct=True`` (grouped memories): at most one hit per group - the best frame of each of the ``top_k`` best
    chunks (EmbeddingMemory.topk_grouped); the wrong-length rule above still lists the first rows.

    ``scope`` (tagged memories): one inclusive tag range ``(lo, hi)`` for every query (memory.scope_of) - the
    reference's ``{graph_uuid: $graph_uuid}`` predicate; only in-scope rows are ranked (EmbeddingMemory.topk_scoped), and
    the wrong-length rule lists the first in-scope rows.  ``None`` = the whole memory, as before.

    ``distinct=True`` together with ``scope``: at most one hit per group among the in-scope rows
    (EmbeddingMemory.topk_grouped_scoped) - accepted when the memory object provides that method, ValueError otherwise.
    The wrong-length rule then lists the first in-scope row of each of the first ``top_k`` in-scope groups.

    ``mask`` (any memory): one row mask for every query (EmbeddingMemory.new_mask / mask_of_rows / mask_where); only the
    selected rows are ranked (EmbeddingMemory.topk_masked), and the wrong-length rule lists the first selected rows.
    Mutually exclusive with ``scope`` and with ``distinct=True`` (ValueError).

    ``span`` (any memory): one inclusive row-id range ``(lo, hi)`` for every query, ``None`` = an open bound - a stretch
    of the memory's time; only the rows in it are ranked (EmbeddingMemory.topk_span), and the wrong-length rule lists the
    first in-span rows.  Mutually exclusive with ``scope``, ``mask`` and ``distinct=True`` (ValueError)."""
    _check_span(span, scope, mask, distinct)
    _check_mask(mask, scope, distinct)
    _check_distinct(memory, distinct)
    _check_scope(memory, scope, distinct)
    ok_idx = [i for i, e in enumerate(chunk_embeddings) if not isinstance(e, Exception) and e is not None]
    out: List[List[Tuple[str, float]]] = [[] for _ in chunk_embeddings]
    if not ok_idx or memory.searchable == 0 or top_k <= 0:
        return out
    wrong = [i for i in ok_idx if _length(chunk_embeddings[i]) != memory.dim]
    if wrong:
        first_row = len(memory) - memory.searchable
        if span is not None:
            zeros = [(memory.id_of(r), 0.0) for r in _span_rows(memory, span)[:top_k]]
        elif mask is not None:
            zeros = [(memory.id_of(r), 0.0) for r in memory.rows_of_mask(mask)[:top_k]]
        elif scope is None:
            zeros = [(memory.id_of(first_row + j), 0.0) for j in range(min(top_k, memory.searchable))]
        else:
            tags = memory.tags_host()
            hit = ((tags >= int(scope[0])) & (tags <= int(scope[1]))).nonzero()[0]
            if distinct:  # every score is 0.0: the ranking keeps memory order, so each group shows its first in-scope row
                keys = memory.group_keys_host()
                starts = (keys[1:] != keys[:-1]).cumsum()            # group index of rows 1 .. n-1; row 0 is in group 0
                gid = [0 if j == 0 else int(starts[j - 1]) for j in hit]
                hit = [j for i, j in enumerate(hit) if i == 0 or gid[i] != gid[i - 1]]
            hit = hit[:top_k]
            zeros = [(memory.id_of(first_row + int(j)), 0.0) for j in hit]
        for i in wrong:
            out[i] = list(zeros)
        ok_idx = [i for i in ok_idx if i not in set(wrong)]
        if not ok_idx:
            return out
    first = chunk_embeddings[ok_idx[0]]
    if isinstance(first, torch.Tensor):
        q = torch.stack([chunk_embeddings[i] for i in ok_idx])
    else:
        q = torch.tensor([list(chunk_embeddings[i]) for i in ok_idx], dtype=torch.float32)
    if span is not None:
        scores, rows = memory.topk_span(q, top_k, span)
    elif mask is not None:
        scores, rows = memory.topk_masked(q, top_k, mask)
    elif scope is not None and distinct:
        scores, rows, _ = memory.topk_grouped_scoped(q, top_k, scope)
    elif scope is not None:
        scores, rows = memory.topk_scoped(q, top_k, scope)
    elif distinct:
        scores, rows, _ = memory.topk_grouped(q, top_k)
    else:
        scores, rows = memory.topk(q, top_k)
    scores, rows = scores.cpu().tolist(), rows.cpu().tolist()
    for slot, i in enumerate(ok_idx):
        out[i] = [(memory.id_of(r), float(s)) for r, s in zip(rows[slot], scores[slot]) if r >= 0]
    return out


def recall_links(memory: EmbeddingMemory, first_row: Optional[int] = None, n_rows: Optional[int] = None, top_k: int = 10,
                 min_gap: int = 1, max_back: Optional[int] = None, exclude_group: bool = False,
                 min_score: Optional[float] = None, score_mode: int = _lib.VM_SCORE_RAW, block: int = 256
                 ) -> List[List[Tuple[str, float]]]:
    """What each stored row resembles in its own past, in the reference's list shape: entry i belongs to the stored row
    ``first_row + i`` (default: every live row) and holds ``[(id, score), ...]`` of its ``top_k`` best matches among the
    rows at least ``min_gap`` and at most ``max_back`` (``None``: any distance) before it - the links a temporal
    consolidation pass would add between disconnected nodes.  Arguments as in ``EmbeddingMemory.recall_links``; ids come
    from ``memory.id_of``; a row with an empty past, or none above ``min_score``, yields ``[]``."""
    scores, rows = memory.recall_links(first_row, n_rows, k=top_k, min_gap=min_gap, max_back=max_back,
                                       exclude_group=exclude_group, min_score=min_score, score_mode=score_mode,
                                       block=block)
    return [[(memory.id_of(r), float(s)) for r, s in zip(rr, ss) if r >= 0]
            for rr, ss in zip(rows.cpu().tolist(), scores.cpu().tolist())]


def clip_similarities(memory: EmbeddingMemory, chunks_of_frame_embeddings: Sequence, top_k: int,
                      min_sep: Optional[int] = None, scope=None, max_gap_ms: Optional[int] = None
                      ) -> List[List[Tuple[str, float]]]:
    """The aligned counterpart of ``batch_similarities`` for a memory that stores one row per frame: each entry of
    ``chunks_of_frame_embeddings`` is a chunk's frames in order (``[L, D]``, 1 <= L <= 16; tensor or lists), and its hits
    are the stored moments it replays frame for frame (EmbeddingMemory.topk_clip: the mean of the L aligned cosines, one
    hit per moment) - where ``batch_similarities`` on the same frames scores L independent queries and ignores order.

    Returns the reference's list shape (src/components/pre_llm_injector.py:346-372): per chunk ``[(id, score), ...]``,
    ``id = memory.id_of(start_row)``; an Exception or ``None`` entry yields ``[]`` (:357-359).
    ``merge_batch_similarities`` consumes it unchanged.  Chunks of one length share one launch.  ``min_sep``, ``scope``
    (one inclusive tag range for every chunk) and ``max_gap_ms`` as in ``topk_clip``."""
    _check_scope(memory, scope, False)
    out: List[List[Tuple[str, float]]] = [[] for _ in chunks_of_frame_embeddings]
    if memory.searchable == 0 or top_k <= 0:
        return out
    by_len: Dict[int, List[int]] = {}
    clips: Dict[int, torch.Tensor] = {}
    for i, e in enumerate(chunks_of_frame_embeddings):
        if isinstance(e, Exception) or e is None:
            continue
        t = e if isinstance(e, torch.Tensor) else torch.tensor([list(f) for f in e], dtype=torch.float32)
        if t.dim() != 2 or t.shape[-1] != memory.dim:
            raise ValueError(f"chunk {i}: frames must be [L, {memory.dim}], got {tuple(t.shape)}")
        clips[i] = t
        by_len.setdefault(int(t.shape[0]), []).append(i)
    for L, idx in by_len.items():
        q = torch.stack([clips[i].to(memory.device) for i in idx])
        scores, rows = memory.topk_clip(q, top_k, min_sep=min_sep, scope=scope, max_gap_ms=max_gap_ms)
        scores, rows = scores.cpu().tolist(), rows.cpu().tolist()
        for slot, i in enumerate(idx):
            out[i] = [(memory.id_of(r), float(s)) for r, s in zip(rows[slot], scores[slot]) if r >= 0]
    return out


def seq_similarities(memory: EmbeddingMemory, sequences_of_step_embeddings: Sequence, top_k: int, max_step: int = 4,
                     min_sep: Optional[int] = None, mask=None, max_gap_ms: Optional[int] = None,
                     min_score: Optional[float] = None
                     ) -> Tuple[List[List[Tuple[str, float]]], List[List[Tuple[str, str]]]]:
    """The ordered counterpart of ``clip_similarities``: each entry of ``sequences_of_step_embeddings`` is the steps of one
    question in order (``[J, D]``, 1 <= J <= 16; tensor or lists - frame embeddings, or one text embedding per sentence),
    and its hits are the stored moments where the steps occur in that order, each at most ``max_step`` rows after the one
    before (EmbeddingMemory.topk_seq: the mean of the J cosines along the best chain, one hit per moment).

    Returns ``(hits, spans)``.  ``hits`` has the reference's list shape (src/components/pre_llm_injector.py:346-372): per
    sequence ``[(id, score), ...]`` with ``id = memory.id_of(end_row)``; an Exception or ``None`` entry yields ``[]``
    (:357-359); ``merge_batch_similarities`` consumes it unchanged.  ``spans`` holds, hit for hit, ``(start_id, end_id)``:
    the ids of the rows of the first and of the last step.  Sequences of one length share one launch.  ``min_sep``,
    ``mask`` (one mask for every sequence), ``max_gap_ms`` and ``min_score`` as in ``topk_seq``."""
    hits: List[List[Tuple[str, float]]] = [[] for _ in sequences_of_step_embeddings]
    spans: List[List[Tuple[str, str]]] = [[] for _ in sequences_of_step_embeddings]
    if memory.searchable == 0 or top_k <= 0:
        return hits, spans
    by_len: Dict[int, List[int]] = {}
    seqs: Dict[int, torch.Tensor] = {}
    for i, e in enumerate(sequences_of_step_embeddings):
        if isinstance(e, Exception) or e is None:
            continue
        t = e if isinstance(e, torch.Tensor) else torch.tensor([list(f) for f in e], dtype=torch.float32)
        if t.dim() != 2 or t.shape[-1] != memory.dim:
            raise ValueError(f"sequence {i}: steps must be [J, {memory.dim}], got {tuple(t.shape)}")
        seqs[i] = t
        by_len.setdefault(int(t.shape[0]), []).append(i)
    for J, idx in by_len.items():
        q = torch.stack([seqs[i].to(memory.device) for i in idx])
        scores, rows, step_rows, _ = memory.topk_seq(q, top_k, max_step=max_step, min_sep=min_sep, mask=mask,
                                                     max_gap_ms=max_gap_ms, min_score=min_score)
        scores, rows, first = scores.cpu().tolist(), rows.cpu().tolist(), step_rows[:, :, 0].cpu().tolist()
        for slot, i in enumerate(idx):
            keep = [h for h, r in enumerate(rows[slot]) if r >= 0]
            hits[i] = [(memory.id_of(rows[slot][h]), float(scores[slot][h])) for h in keep]
            spans[i] = [(memory.id_of(first[slot][h]), memory.id_of(rows[slot][h])) for h in keep]
    return hits, spans


MIX_MAX_TERMS = 16   # terms of one mixed query (EmbeddingMemory.topk_mix)


def feedback_terms(query, positives: Sequence = (), negatives: Sequence = (), alpha: float = 1.0, beta: float = 0.75,
                   gamma: float = 0.15) -> Tuple[torch.Tensor, List[float]]:
    """Rocchio relevance feedback as one mixed query -> ``(terms [J, D], weights [J])`` for ``EmbeddingMemory.topk_mix``
    / ``mix_similarities``: the query with weight ``alpha``, each positive example with ``beta / len(positives)``, each
    negative one with ``-gamma / len(negatives)``, in that order.  Where the textbook form adds the vectors and searches
    with their sum, the mixed search ranks by the weighted sum of the COSINES: every example counts by its direction,
    whatever its length, and the score is a defined fp64 value.  Vectors are ``[D]`` tensors or float sequences (stored
    rows, hits of an earlier search, fresh embeddings).  Pure host code.  ``ValueError`` above 16 terms, for vectors of
    different lengths and for a non-finite coefficient."""
    positives, negatives = list(positives), list(negatives)
    J = 1 + len(positives) + len(negatives)
    if J > MIX_MAX_TERMS:
        raise ValueError(f"feedback_terms: {J} terms, a mixed query holds at most {MIX_MAX_TERMS}")
    for name, v in (("alpha", alpha), ("beta", beta), ("gamma", gamma)):
        if not torch.isfinite(torch.tensor(float(v))):
            raise ValueError(f"feedback_terms: {name} = {v} is not finite")
    vecs = [v.detach().cpu() if isinstance(v, torch.Tensor) else torch.tensor([float(x) for x in v], dtype=torch.float32)
            for v in [query, *positives, *negatives]]
    for i, v in enumerate(vecs):
        if v.dim() != 1 or v.shape != vecs[0].shape:
            raise ValueError(f"feedback_terms: term {i} has shape {tuple(v.shape)}, the query {tuple(vecs[0].shape)}")
    if len({v.dtype for v in vecs}) > 1:
        vecs = [v.to(torch.float32) for v in vecs]
    weights = [float(alpha)] + [float(beta) / len(positives) for _ in positives] \
        + [-float(gamma) / len(negatives) for _ in negatives]
    return torch.stack(vecs), weights


def mix_similarities(memory: EmbeddingMemory, terms, weights, top_k: int, mask=None,
                     min_score: Optional[float] = None) -> List[List[Tuple[str, float]]]:
    """``EmbeddingMemory.topk_mix`` in the reference's list shape (src/components/pre_llm_injector.py:346-372), as
    ``clip_similarities`` returns it: per mixed query ``[(id, score), ...]``, ``id = memory.id_of(row)``, the score the
    weighted sum of cosines; ``merge_batch_similarities`` consumes it unchanged.  ``terms``: ``[C, J, D]`` or ``[J, D]``
    (one query), ``weights``: ``[C, J]`` or one list of J (``feedback_terms`` returns a matching pair); ``mask``: one row
    mask for every query or one per query - ``~memory.mask_of_rows(rows_already_shown)`` keeps earlier hits out."""
    t = terms if isinstance(terms, torch.Tensor) else torch.tensor(terms, dtype=torch.float32)
    n = 1 if t.dim() == 2 else int(t.shape[0])
    if memory.searchable == 0 or top_k <= 0:
        return [[] for _ in range(n)]
    scores, rows = memory.topk_mix(t, weights, top_k, mask=mask, min_score=min_score)
    return [[(memory.id_of(r), float(s)) for r, s in zip(rr, ss) if r >= 0]
            for rr, ss in zip(rows.cpu().tolist(), scores.cpu().tolist())]


def fold_similarities(memory: EmbeddingMemory, terms, top_k: int, op: str = "max", weights=None, mask=None,
                      min_score: Optional[float] = None) -> List[List[Tuple[str, float]]]:
    """``EmbeddingMemory.topk_fold`` in the reference's list shape, as ``mix_similarities`` returns it: per fold query
    ``[(id, score), ...]``, ``id = memory.id_of(row)``, the score the maximum (``op="max"``: any term) or the minimum
    (``op="min"``: all terms) of the weighted cosines; ``weights=None`` = all 1.0, and a zero weight is NOT neutral (its
    product 0.0 takes part).  ``terms``: ``[C, J, D]`` or ``[J, D]`` (one query); ``mask``: one row mask for every query
    or one per query."""
    t = terms if isinstance(terms, torch.Tensor) else torch.tensor(terms, dtype=torch.float32)
    n = 1 if t.dim() == 2 else int(t.shape[0])
    if memory.searchable == 0 or top_k <= 0:
        return [[] for _ in range(n)]
    scores, rows, _ = memory.topk_fold(t, top_k, op=op, weights=weights, mask=mask, min_score=min_score)
    return [[(memory.id_of(r), float(s)) for r, s in zip(rr, ss) if r >= 0]
            for rr, ss in zip(rows.cpu().tolist(), scores.cpu().tolist())]


FOLD_MAX_K = 64      # hits of one fold query (EmbeddingMemory.topk_fold)


def linked_similarities(memory: EmbeddingMemory, chunk_embeddings: Sequence, top_k_each: int, top_k_final: int,
                        mask=None) -> List[Tuple[str, float]]:
    """The graph-node linking of src/components/pre_llm_injector.py:233-249 in one device search: what
    ``merge_batch_similarities(batch_similarities(memory, chunk_embeddings, top_k_each, mask=mask), top_k_final)``
    returns.  The reference gives each of a batch's Q embeddings its own top-``top_k_each`` list and keeps the maximum
    score per stored id; the score that decides is ``max_j cos(embedding_j, row)``, which ``topk_fold(op="max")`` ranks
    by directly: one key column and one list per 16 embeddings on the device, then ONE read-back and a host merge over the
    C x ``top_k_final`` returned entries (C = the groups of 16), where the two-step route reads back and merges Q lists.
    It is not the faster route: measured on one MI355X, a batch of 16 embeddings costs 0.52 ms this way against 0.42 ms for
    the two-step route on 1 M x 768 fp16 rows (0.25 against 0.21 ms on 100 k), because the plain ``topk`` of 16 vectors is
    cheaper than one key-image search.  What it gives is the linking score as one defined, capturable device
    search; a caller who only wants the lists at the highest rate keeps the two-step calls.

    ``Exception`` / ``None`` entries are dropped (they contribute ``[]`` in the reference).  More than 16 usable
    embeddings go as groups of at most 16, all fold queries of ONE call, whose lists are max-merged per row on the host
    (max is associative); the last group is filled with copies of its first embedding, which changes nothing.

    Guarantee, for ``top_k_final <= top_k_each``: the list of SCORES always equals the reference merge's.  The ids
    equal it whenever the fold scores of the returned rows and of the best row left out are pairwise distinct; on exact
    score ties the reference keeps first-seen order and this keeps row-id order.

    The two-step path itself is used, unchanged, when ``top_k_final > top_k_each``, when ``top_k_final`` is above 64,
    when a usable embedding's length differs from ``memory.dim`` (the reference's all-zero rule), and when two of the
    returned rows carry one id (the reference merges per id; a memory with one row per id never gets there)."""
    def two_step():
        return merge_batch_similarities(batch_similarities(memory, chunk_embeddings, top_k_each, mask=mask), top_k_final)

    ok = [e for e in chunk_embeddings if not isinstance(e, Exception) and e is not None]
    if not ok or memory.searchable == 0 or top_k_each <= 0 or top_k_final <= 0:
        return two_step()
    if top_k_final > top_k_each or top_k_final > FOLD_MAX_K or any(_length(e) != memory.dim for e in ok):
        return two_step()
    if isinstance(ok[0], torch.Tensor):
        q = torch.stack(list(ok))
    else:
        q = torch.tensor([list(e) for e in ok], dtype=torch.float32)
    J = min(len(ok), MIX_MAX_TERMS)
    C = -(-len(ok) // J)
    if C * J > len(ok):  # fill the last group with copies of its first term: a repeated term changes nothing
        fill = q[(C - 1) * J].unsqueeze(0).expand(C * J - len(ok), -1)
        q = torch.cat([q, fill.to(q.device)])
    scores, rows, _ = memory.topk_fold(q.reshape(C, J, -1), top_k_final, op="max", mask=mask)
    best: Dict[int, float] = {}
    for rr, ss in zip(rows.cpu().tolist(), scores.cpu().tolist()):
        for r, s in zip(rr, ss):
            if r >= 0 and (r not in best or s > best[r]):
                best[r] = s
    top = sorted(best.items(), key=lambda x: (-x[1], x[0]))[:top_k_final]
    ids = [memory.id_of(r) for r, _ in top]
    if len(set(ids)) != len(ids):
        return two_step()
    return [(i, float(s)) for i, (_, s) in zip(ids, top)]


def biased_similarities(memory: EmbeddingMemory, queries, bias, weight, top_k: int, mask=None,
                        min_score: Optional[float] = None) -> List[List[Tuple[str, float]]]:
    """``EmbeddingMemory.topk_biased`` in the reference's list shape, as ``mix_similarities`` returns it: per query
    ``[(id, score), ...]``, ``id = memory.id_of(row)``, the score the cosine plus ``weight`` times the row's bias.
    ``bias``: one column for every query or one per query (``memory.bias_of_age`` for recency, ``memory.bias_of_rows``
    for a boost of the rows another retrieval leg found); ``weight``: one number, one per query, or ``None`` for 1.0;
    ``mask``: one row mask for every query or one per query."""
    q = queries if isinstance(queries, torch.Tensor) else torch.tensor(queries, dtype=torch.float32)
    n = 1 if q.dim() == 1 else int(q.shape[0])
    if memory.searchable == 0 or top_k <= 0:
        return [[] for _ in range(n)]
    scores, rows = memory.topk_biased(q, top_k, bias, weight=weight, mask=mask, min_score=min_score)
    return [[(memory.id_of(r), float(s)) for r, s in zip(rr, ss) if r >= 0]
            for rr, ss in zip(rows.cpu().tolist(), scores.cpu().tolist())]


def diverse_similarities(memory: EmbeddingMemory, queries, top_k: int, pool: Optional[int] = None, lam=0.5, mask=None,
                         min_score: Optional[float] = None) -> List[List[Tuple[str, float]]]:
    """``EmbeddingMemory.topk_diverse`` in the reference's list shape, as ``mix_similarities`` returns it: per query
    ``[(id, score), ...]`` in PICK order, ``id = memory.id_of(row)``, the score the row's cosine with the query.  What a
    vector store calls ``max_marginal_relevance_search(k, fetch_k, lambda_mult)``: ``top_k`` context slots that are not
    spent on near-identical frames.  ``mask``: one row mask for every query or one per query."""
    q = queries if isinstance(queries, torch.Tensor) else torch.tensor(queries, dtype=torch.float32)
    n = 1 if q.dim() == 1 else int(q.shape[0])
    if memory.searchable == 0 or top_k <= 0:
        return [[] for _ in range(n)]
    scores, rows = memory.topk_diverse(q, top_k, pool=pool, lam=lam, mask=mask, min_score=min_score)
    return [[(memory.id_of(r), float(s)) for r, s in zip(rr, ss) if r >= 0]
            for rr, ss in zip(rows.cpu().tolist(), scores.cpu().tolist())]


class HipPreLLMSimilarity:
    """Mixin / stand-alone object for PreLLMInjector: set ``self.memory`` and ``self.embedder_config``."""

    def __init__(self, memory: EmbeddingMemory, embedder_config: Any, distinct: bool = False, scope=None, mask=None,
                 span=None):
        """``scope``: an inclusive tag range ``(lo, hi)`` (memory.scope_of) every search of this object is restricted to
        - the reference's ``WHERE c.graph_uuid = $graph_uuid`` (src/components/pre_llm_injector.py:395-396); tagged memory
        only.  Together with ``distinct`` it needs a memory that provides ``topk_grouped_scoped`` (a grouped and tagged
        EmbeddingMemory): one hit per group among the in-scope rows; ValueError otherwise.  ``None`` = the whole
        memory.  ``mask``: a row mask every search of this object is restricted to (``batch_similarities``); the object
        keeps the tensor, so rewriting it in place changes the next search.  Not together with ``scope`` or
        ``distinct``.  ``span``: one inclusive row-id range ``(lo, hi)``, ``None`` = open, every search of this object is
        restricted to (EmbeddingMemory.topk_span); not together with ``scope``, ``mask`` or ``distinct``."""
        _check_span(span, scope, mask, distinct)
        _check_mask(mask, scope, distinct)
        _check_distinct(memory, distinct)
        _check_scope(memory, scope, distinct)
        self.memory = memory
        self.embedder_config = embedder_config
        self.distinct = bool(distinct)
        self.scope = scope
        self.mask = mask
        self.span = span

    async def _calculate_batch_similarities(self, chunk_embeddings, neo4j_handler=None
                                            ) -> List[List[Tuple[str, float]]]:
        try:
            return batch_similarities(self.memory, chunk_embeddings,
                                      self.embedder_config.top_k_chunk_with_batch_similarity,
                                      distinct=getattr(self, "distinct", False), scope=getattr(self, "scope", None),
                                      mask=getattr(self, "mask", None), span=getattr(self, "span", None))
        except _lib.VidmemError as e:
            if e.code == _lib.VM_ERR_INVALID:
                raise
            logger.warning("similarity search failed: %s", e)  # reference: log and degrade to empty
            return [[] for _ in chunk_embeddings]


def _zip_truncating_cosine(vec1, vec2) -> float:
    """src/pipeline/retriever_hybrid.py:655-664, for operands of different lengths only (equal lengths go to the device)."""
    import math
    dot_product = sum(a * b for a, b in zip(vec1, vec2))
    mag1 = math.sqrt(sum(a * a for a in vec1))
    mag2 = math.sqrt(sum(b * b for b in vec2))
    if mag1 * mag2 == 0:
        return 0.0
    return dot_product / (mag1 * mag2)


def frames_above(memory: EmbeddingMemory, query_embedding, min_score: float, *, score_mode: int, scope=None,
                 max_hits: Optional[int] = None) -> List[Tuple[str, float]]:
    """Every stored frame whose score against ``query_embedding`` is strictly above ``min_score`` as ``(id, score)``, in
    time order (ascending row id) - the ``min_score`` leg of ``HipVectorSearch`` without the k
    (``vector.similarity.cosine(...) > 0.3``, src/pipeline/retriever_hybrid.py:296-298, with no ``LIMIT``).

    ``score_mode`` is a REQUIRED keyword for the reason ``HipVectorSearch`` gives: the threshold is compared after the
    mapping, and nothing in the reference pins which mapping its server applied.  ``scope``: an inclusive tag range
    (memory.scope_of), tagged memories only; ``max_hits``: keep the first ``max_hits`` frames only (``None`` = all).
    Ids come from ``memory.id_of`` (``None`` for a row stored without one)."""
    if score_mode not in (_lib.VM_SCORE_RAW, _lib.VM_SCORE_UNIT_INTERVAL):
        raise ValueError("score_mode must be VM_SCORE_RAW or VM_SCORE_UNIT_INTERVAL")
    _check_scope(memory, scope, False)
    hit = memory.range_search([query_embedding] if not isinstance(query_embedding, torch.Tensor) else query_embedding,
                              min_score, scope=scope, score_mode=score_mode, max_hits=max_hits)[0]
    return [(memory.id_of(r), float(s)) for r, s in zip(hit.rows.cpu().tolist(), hit.scores.cpu().tolist())]


class HipVectorSearch:
    """Mixin / stand-alone object for HybridRetriever's vector leg."""

    def __init__(self, memory: EmbeddingMemory, embedder: Any, config: Any, *, score_mode: int,
                 min_score: float = 0.3, splitter: Optional[Callable[[str], List[str]]] = None, distinct: bool = False,
                 scope=None, mask=None, span=None):
        """``score_mode`` is REQUIRED (keyword): the reference filters on Neo4j's
        ``vector.similarity.cosine(...) > 0.3`` (src/pipeline/retriever_hybrid.py:296-298), a third-party function of an
        unpinned server image whose value may be the raw cosine or its [0,1] mapping (1+cos)/2 - with the literal 0.3
        meaning cos > 0.3 in one case and cos > -0.4 in the other.  Nothing in the reference pins it (parity unpinned,
        SURVEY.md 8 a10), so the integrator states which one their deployment had: ``_lib.VM_SCORE_RAW`` or
        ``_lib.VM_SCORE_UNIT_INTERVAL``; ``min_score`` (default: the reference's literal) is compared AFTER the mapping.
        ``distinct=True`` (grouped memory only, else ValueError): at most one hit per chunk - ``top_k_chunks`` distinct
        chunks, each represented by its best frame (EmbeddingMemory.topk_grouped).
        ``scope``: an inclusive tag range ``(lo, hi)`` (memory.scope_of) the search is restricted to - the reference's
        ``MATCH (c:Chunk {graph_uuid: $graph_uuid})`` (src/pipeline/retriever_hybrid.py:295); tagged memory only.
        Together with ``distinct`` it needs a memory that provides ``topk_grouped_scoped`` (a grouped and tagged
        EmbeddingMemory; ValueError otherwise): ``top_k_chunks`` distinct chunks of the scope, each represented by its
        best in-scope frame.  ``None`` = the whole memory.
        ``mask``: a row mask the search is restricted to (EmbeddingMemory.topk_masked: a metadata filter, the hits of
        another search, an exclusion); any memory; not together with ``scope`` or ``distinct`` (ValueError).
        ``span``: one inclusive row-id range ``(lo, hi)``, ``None`` = open, the search is restricted to
        (EmbeddingMemory.topk_span: a stretch of the memory's time); any memory; not together with ``scope``, ``mask`` or
        ``distinct`` (ValueError)."""
        if score_mode not in (_lib.VM_SCORE_RAW, _lib.VM_SCORE_UNIT_INTERVAL):
            raise ValueError("score_mode must be VM_SCORE_RAW or VM_SCORE_UNIT_INTERVAL")
        # an embedder that states its width (HipTextEmbedder, FrameEncoder-backed ones) must match the memory's rows: a
        # text tower against a memory built without the joint projection (clip_l14_336: 1024-d) is a wiring error
        out_dim = getattr(embedder, "out_dim", None)
        if out_dim is not None and int(out_dim) != int(memory.dim):
            raise ValueError(f"embedder out_dim {out_dim} != memory.dim {memory.dim}: build the memory with the matching "
                             "image encoder (text questions: encoder.arch clip_l14_336_joint)")
        _check_span(span, scope, mask, distinct)
        _check_mask(mask, scope, distinct)
        _check_distinct(memory, distinct)
        _check_scope(memory, scope, distinct)
        self.memory, self.embedder, self.config = memory, embedder, config
        self.distinct = bool(distinct)
        self.scope = scope
        self.mask = mask
        self.span = span
        self.min_score, self.score_mode, self.splitter = min_score, score_mode, splitter

    async def _vector_search_chunks(self, session, query) -> List[Dict[str, Any]]:
        try:
            query_embedding = await self.embedder.aembed_query(query)
            if getattr(self, "span", None) is not None:
                scores, rows = self.memory.topk_span([query_embedding], self.config.top_k_chunks, self.span,
                                                     min_score=self.min_score, score_mode=self.score_mode)
            elif getattr(self, "mask", None) is not None:
                scores, rows = self.memory.topk_masked([query_embedding], self.config.top_k_chunks, self.mask,
                                                       min_score=self.min_score, score_mode=self.score_mode)
            elif getattr(self, "scope", None) is not None and self.distinct:
                scores, rows, _ = self.memory.topk_grouped_scoped([query_embedding], self.config.top_k_chunks,
                                                                  self.scope, min_score=self.min_score,
                                                                  score_mode=self.score_mode)
            elif getattr(self, "scope", None) is not None:
                scores, rows = self.memory.topk_scoped([query_embedding], self.config.top_k_chunks, self.scope,
                                                       min_score=self.min_score, score_mode=self.score_mode)
            elif self.distinct:
                scores, rows, _ = self.memory.topk_grouped([query_embedding], self.config.top_k_chunks,
                                                           min_score=self.min_score, score_mode=self.score_mode)
            else:
                scores, rows = self.memory.topk([query_embedding], self.config.top_k_chunks, min_score=self.min_score,
                                                score_mode=self.score_mode)
            chunks = []
            for r, s in zip(rows[0].cpu().tolist(), scores[0].cpu().tolist()):
                if r < 0:
                    continue
                meta = self.memory.meta_of(r) or {}
                chunks.append({"id": self.memory.id_of(r), "time": meta.get("time"), "content": meta.get("content"),
                               "score": float(s), "source": "vector"})
            return chunks
        except _lib.VidmemError as e:
            if e.code == _lib.VM_ERR_INVALID:
                raise
            logger.warning("Vector search failed: %s", e)
            return []
        except Exception as e:  # embedder failure etc.: reference returns [] (retriever_hybrid.py:321-323)
            logger.warning("Vector search failed: %s", e)
            return []

    async def _post_compress_chunks(self, query, chunks: List[Dict]) -> List[Dict]:
        if not self.embedder or not chunks:
            return chunks
        try:
            query_embedding = await self.embedder.aembed_query(query)
            segments, owners = [], []
            for chunk in chunks:
                for segment in (self.splitter(chunk["content"]) if self.splitter else [chunk["content"]]):
                    segments.append(segment)
                    owners.append(chunk)
            if not segments:
                return []
            # segment embeds: one failure drops that segment only (retriever_hybrid.py:505-507)
            seg_emb, keep = [], []
            for i, seg in enumerate(segments):
                try:
                    seg_emb.append(await self.embedder.aembed_query(seg))
                    keep.append(i)
                except Exception as e:
                    logger.debug("Failed to embed segment: %s", e)
            if not seg_emb:
                return []
            # ONE [1, D] x [S, D] exact-cosine launch for all segments of all hits (the reference scores them one
            # by one in Python, :497); filter >= threshold in encounter order, then [:top_k] (:499-510).  The operands
            # are scored as fp32 values, not rounded to the memory's 16-bit type: they never enter the memory, and a
            # threshold decision must not flip on a rounding the reference does not make.  A segment whose embedding's
            # length differs from the query's (an embedder that changed its model between calls) is scored on the host
            # by the reference's own zip-truncating expression (:655-664: dot over the common prefix, each magnitude over
            # its whole vector, ``mag1 * mag2 == 0`` -> 0.0) - three Python sums, as there.
            same = [j for j, e in enumerate(seg_emb) if len(e) == len(query_embedding)]
            sims = [0.0] * len(seg_emb)
            if same:
                dev = self.memory.cosine_exact([query_embedding], [seg_emb[j] for j in same], as_f32=True)[0].cpu().tolist()
                for j, v in zip(same, dev):
                    sims[j] = v
            for j, e in enumerate(seg_emb):
                if len(e) != len(query_embedding):
                    sims[j] = _zip_truncating_cosine(query_embedding, e)
            kept = [{**owners[i], "content": segments[i], "compression_score": float(sim)}
                    for i, sim in zip(keep, sims) if sim >= self.config.compression_threshold]
            return kept[: self.config.top_k]
        except Exception as e:
            logger.warning("Post-compression failed: %s", e)
            return chunks
