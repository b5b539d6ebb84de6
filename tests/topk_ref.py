"""Host-side helpers shared by the top-k GPU tests: merging per-chunk answers and the C oracle on a thread pool."""
import numpy as np

from oracle import cref


def merge_topk(parts, k):
    """Merge per-row-chunk oracle answers [(rows + chunk offset, scores)] into one: the oracle's order (returned score
    desc, row asc) over the union, -1 / 0.0 padded.  A row's score does not depend on the other rows, so the k best of
    the union are among the k best of each chunk."""
    rows = np.concatenate([p[0] for p in parts], axis=1)
    scores = np.concatenate([p[1] for p in parts], axis=1)
    Q = rows.shape[0]
    out_r = np.full((Q, k), -1, np.int64)
    out_s = np.zeros((Q, k), np.float64)
    for i in range(Q):
        live = rows[i] >= 0
        r, s = rows[i][live], scores[i][live]
        order = np.lexsort((r, -s))[:k]
        out_r[i, :order.size] = r[order]
        out_s[i, :order.size] = s[order]
    return out_r, out_s


def oracle_rows_parallel(qbits, mbits, k, dtype, picks, threads=8, score_mode=0, min_score=None):
    """cref.cosine_topk for a subset of the queries on a thread pool (ctypes releases the GIL): the memory rows are
    split into one contiguous chunk per thread and the chunks' answers merged (merge_topk), so a handful of queries
    over a large memory also spreads over every thread."""
    from concurrent.futures import ThreadPoolExecutor
    q = np.ascontiguousarray(qbits[np.asarray(picks)])
    M = mbits.shape[0]
    bounds = np.linspace(0, M, min(threads, max(M, 1)) + 1).astype(np.int64)
    chunks = [(int(lo), int(hi)) for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo] or [(0, 0)]

    def run(c):
        lo, hi = c
        r, s = cref.cosine_topk(q, mbits[lo:hi], k, dtype=dtype, score_mode=score_mode, min_score=min_score)
        return np.where(r >= 0, r + lo, -1), s

    with ThreadPoolExecutor(len(chunks)) as ex:
        parts = list(ex.map(run, chunks))
    return merge_topk(parts, k)
