"""Checkers, raw calls and builders of single searches that more than one test file uses: the grouped, the range, the
mixed and the any/all search, the clip search's memory, the events' raw append and regroup, the end-to-end tests' extractor
and clip.  A plain module, as tests/support.py is; everything here needs the GPU when called, nothing when imported.
"""
import ctypes
import functools

import numpy as np
import torch

from tests import fold_ref as FR
from tests import group_ref as G
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests import range_ref as R
from tests import scope_ref as S
from tests.support import bits, check_entries, dev_mask, from_bits, plain_memory, tagged_memory


def ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


# ---- grouped top-k ----------------------------------------------------------------------------------------------------
def grouped_check(mem, q, k, dtype, min_score=None, score_mode=0, exact=False, certified=False):
    """certified=True: also require that the fast path answered every query (no flag, no exhaustive redo)."""
    s, r, kk = mem.topk_grouped(q, k, min_score=min_score, score_mode=score_mode, exact=exact)
    if certified:
        flags = mem.last_group_flags[:q.shape[0]].cpu().numpy()
        assert (flags == 0).all(), f"fast path flagged {int((flags != 0).sum())} of {q.shape[0]} queries: {flags[:8]}"
    base, host_rows = mem.rows_host()
    keys = mem.group_keys_host()
    want_r, want_s, want_k = G.grouped_topk(bits(q), host_rows, keys, k, dtype=dtype, score_mode=score_mode,
                                            min_score=min_score, base=base)
    got_r, got_s, got_k = r.cpu().numpy(), s.cpu().numpy(), kk.cpu().numpy()
    assert np.array_equal(got_r, want_r), (np.argwhere(got_r != want_r)[:5], got_r[:2], want_r[:2])
    assert np.array_equal(got_k, want_k), (np.argwhere(got_k != want_k)[:5], got_k[:2], want_k[:2])
    assert np.array_equal(got_s.view(np.int64), want_s.view(np.int64)), "scores differ (bit-exact bar)"
    return got_r, got_s, got_k


# ---- range search -----------------------------------------------------------------------------------------------------
SENT_ROW, SENT_SCORE, SENT_COUNT = -7, 123.0, -9      # what the output buffers hold before a call
range_memory = functools.partial(plain_memory, step=8192)


def raw_range(mem, q, min_score, scopes=None, score_mode=0, max_hits=0, exact=False, stride=1, offset=0,
              null_out=False, lo_hi=None):
    """One call of the C entry on sentinel-filled buffers -> (rc, rows [Q, max_hits], scores, counts [Q], rescored [Q])
    as numpy arrays.  ``lo_hi``: explicit (lo, hi) pointers (tensors or None) instead of ``scopes``."""
    from vidmem import _lib
    Q = q.shape[0]
    need = int(mem.L.vm_range_workspace_bytes(mem.handle, Q))
    assert 0 < need <= 16 * Q * ((mem.capacity + 63) // 64 * 64) + (1 << 16), need
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    rows = torch.full((Q, max(max_hits, 1)), SENT_ROW, dtype=torch.int64, device="cuda")
    scores = torch.full((Q, max(max_hits, 1)), SENT_SCORE, dtype=torch.float64, device="cuda")
    counts = torch.full((Q,), SENT_COUNT, dtype=torch.int64, device="cuda")
    rescored = torch.full((Q,), SENT_COUNT, dtype=torch.int64, device="cuda")
    if lo_hi is None:
        lo_hi = (None, None)
        if scopes is not None:
            lo, hi = S.scope_arrays(scopes, Q)
            lo_hi = (torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda())
    out_r, out_s = (None, None) if null_out else (rows, scores)
    head = (mem.handle, ptr(q), Q, float(min_score), int(score_mode), ptr(lo_hi[0]), ptr(lo_hi[1]), int(stride),
            int(offset), int(max_hits), ptr(out_r), ptr(out_s), ptr(counts))
    tail = (ptr(ws), ws.numel(), _lib.current_stream_ptr())
    if exact:
        rc = mem.L.vm_range_cosine_exact(*head, *tail)
    else:
        rc = mem.L.vm_range_cosine(*head, ptr(rescored), *tail)
    torch.cuda.synchronize()
    return (rc, rows.cpu().numpy()[:, :max_hits], scores.cpu().numpy()[:, :max_hits], counts.cpu().numpy(),
            rescored.cpu().numpy())


def range_check(mem, q, min_score, want, max_hits=None, scopes=None, score_mode=0, stride=1, offset=0, label=""):
    """Fast and exhaustive entry against ``want`` (range_ref's per-query hits): padded rows, score bits and counts.
    ``max_hits=None``: three more slots than the longest list, so that every hit and some padding is seen.
    -> (counts, rescored) of the fast call."""
    width = max([c for _, _, c in want] + [0]) + 3 if max_hits is None else max_hits
    want_r, want_s, want_c = R.padded(want, width)
    want_r = np.where(want_r >= 0, want_r * stride + offset, -1)
    out = None
    for exact in (False, True):
        rc, r, s, c, resc = raw_range(mem, q, min_score, scopes, score_mode, width, exact, stride, offset,
                                      null_out=width == 0)
        assert rc == 0, (rc, mem.L.vm_last_error(mem.ctx.handle))
        assert np.array_equal(c, want_c), (label, exact, c[:8], want_c[:8])
        assert np.array_equal(r, want_r), (label, exact, np.argwhere(r != want_r)[:5])
        assert np.array_equal(s.view(np.int64), want_s.view(np.int64)), f"{label}: scores differ (bit-exact bar) exact={exact}"
        if not exact:
            assert (resc >= c).all(), (label, resc[:8], c[:8])
            out = (c, resc)
    return out


# ---- the mixed and the any/all search ---------------------------------------------------------------------------------
def per_query(weights, C):
    return [list(weights)] * C if not isinstance(weights[0], (list, tuple)) else [list(w) for w in weights]


def _mask_operand(masks):
    return None if masks is None else (masks if isinstance(masks, torch.Tensor) else dev_mask(masks))


def mix_want(mem, terms, weights, k, dtype, masks=None, index=None, **kw):
    """Statement (A) for the memory as it is: terms [C,J,D] on the device, weights [C][J], masks / index host arrays."""
    base, host_rows = mem.rows_host()
    C = terms.shape[0]
    sel = None if masks is None else MR.selection(masks, index, C, base, host_rows.shape[0], mem.capacity)
    return XR.mix_topk(bits(terms), weights, host_rows, sel, k, dtype=dtype, base=base, **kw)


def mix_check(mem, terms, weights, k, dtype, masks=None, index=None, certified=None, label="", want=None, **kw):
    """Fast and exact entry against (A) (``want``: (A) computed by the caller).  certified: None, or bool per query - the
    fast path must have answered those queries itself (flag 0).  -> (rows, scores, flags) of the fast entry."""
    C = terms.shape[0]
    want = want or mix_want(mem, terms, per_query(weights, C), k, dtype, masks, index, **kw)
    m = _mask_operand(masks)

    def call(exact):
        s, r = mem.topk_mix(terms, weights, k, mask=m, mask_index=index, exact=exact, **kw)
        return r, s
    return check_entries(call, lambda: mem.last_mix_flags[:C], want, certified, label)


def fold_want(mem, terms, weights, k, op, dtype, masks=None, index=None, **kw):
    """Statement (A) for the memory as it is: terms [C,J,D] on the device, weights [C][J], masks / index host arrays."""
    base, host_rows = mem.rows_host()
    C = terms.shape[0]
    sel = None if masks is None else MR.selection(masks, index, C, base, host_rows.shape[0], mem.capacity)
    return FR.fold_topk(bits(terms), weights, host_rows, sel, k, op, dtype=dtype, base=base, **kw)


def fold_check(mem, terms, weights, k, op, dtype, masks=None, index=None, certified=None, label="", want=None, **kw):
    """As ``mix_check``, with the winning term T (int32) as the third output.  -> (rows, scores, flags) of the fast
    entry."""
    C = terms.shape[0]
    want = want or fold_want(mem, terms, per_query(weights, C), k, op, dtype, masks, index, **kw)
    m = _mask_operand(masks)

    def call(exact):
        s, r, t = mem.topk_fold(terms, k, op=op, weights=weights, mask=m, mask_index=index, exact=exact, **kw)
        return r, s, t
    got_r, got_s, _, flags = check_entries(call, lambda: mem.last_fold_flags[:C], want, certified, f"{label} {op}")
    return got_r, got_s, flags


# ---- clip search ------------------------------------------------------------------------------------------------------
def make_memory(bits_, dtype, tags=None, capacity=None, ring=False, grouped=False, step=65536):
    """A memory appended the rows of the uint16 bit patterns ``bits_``, with ``tags`` if given."""
    rows = from_bits(bits_, dtype)
    if tags is None:
        return plain_memory(rows, dtype, capacity, ring, step, grouped=grouped)
    return tagged_memory(rows, tags, dtype, capacity, ring, step, grouped=grouped)


# ---- events -----------------------------------------------------------------------------------------------------------
SENT_LINK, SENT_I = 123.0, -7          # what the output buffers hold before a call
RING_CAP = {"f16_768": 3019, "bf16_1024": 1123, "f16_128": 2203}       # primes below n


def raw_append_memory(bits_, dtype, capacity=None, ring=False, grouped=False, tags=None, step=1000):
    """A memory that was appended ``bits_`` through the C entries with keys NULL (a grouped memory then holds the plain
    append's columns: every row its own group), with ``tags`` if given."""
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory
    n = bits_.shape[0]
    mem = EmbeddingMemory(capacity or max(n, 1), bits_.shape[1], dtype, ring=ring, grouped=grouped, tagged=tags is not None)
    step = min(step, mem.capacity)
    first = ctypes.c_int64(0)
    for c0 in range(0, n, step):
        rows = from_bits(bits_[c0:c0 + step], dtype)
        if tags is None:
            rc = mem.L.vm_memory_append(mem.handle, ptr(rows), rows.shape[0], ctypes.byref(first), _lib.current_stream_ptr())
        else:
            tg = torch.from_numpy(np.ascontiguousarray(tags[c0:c0 + step])).cuda()
            rc = mem.L.vm_memory_append_tagged(mem.handle, ptr(rows), rows.shape[0], ptr(tg), None, ctypes.byref(first),
                                               _lib.current_stream_ptr())
        mem.ctx.check(rc)
        torch.cuda.synchronize()
    mem.sync()
    return mem


def events_ws_need(mem):
    need = int(mem.L.vm_memory_events_workspace_bytes(mem.handle))
    assert 0 < need <= 2 * mem.capacity + (1 << 14), need
    return need


def raw_regroup(mem, threshold, gap=-1, from_row=None, ws_bytes=None):
    """-> (rc, count); ``from_row``: None, an int (copied to the device) or a device tensor."""
    from vidmem import _lib
    need = events_ws_need(mem)
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 256), dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), SENT_I, dtype=torch.int64, device="cuda")
    frm = None
    if from_row is not None:
        frm = from_row if isinstance(from_row, torch.Tensor) else torch.tensor([int(from_row)], dtype=torch.int64).cuda()
    rc = mem.L.vm_memory_regroup_events(mem.handle, float(threshold), int(gap), ptr(frm), ptr(cnt), ptr(ws),
                                        need if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, int(cnt.item())


# ---- end to end -------------------------------------------------------------------------------------------------------
def e2e_extractor(enc, memory_cfg, look_ahead=4):
    """The extractor of the end-to-end tests: one-second chunks of 5 frames, the two-layer ViT-B/16 (``enc``: an encoder
    to share, or None), top 4, a memory of 512 rows with ``memory_cfg``."""
    from vidmem import config
    from vidmem.extractor import FrameEmbeddingExtractor
    cfg = config.from_dict({
        "video": {"chunk_size_seconds": 1.0, "frames_per_chunk": 5},
        "encoder": {"arch": "vit_b16_2l", "dtype": "f16", "seed": 3, "top_k": 4, "look_ahead_chunks": look_ahead},
        "memory": {"capacity": 512, **memory_cfg},
    })
    return FrameEmbeddingExtractor(cfg, encoder=enc)


def scene_clip(seed, lengths, H, W, block=16):
    """-> (frames uint8 [n, H, W, 3], owner int [n]): every scene is one image of random colour blocks shown
    ``lengths[i]`` times in a row, each showing with its own +-1 of pixel noise (tests/novelty_feed.py's frames)."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, size=(len(lengths), H // block, W // block, 3), dtype=np.uint8)
    src = np.kron(blocks, np.ones((1, block, block, 1), np.uint8))
    frames, owner = [], []
    for i, n in enumerate(lengths):
        for _ in range(n):
            noise = rng.integers(-1, 2, size=src[i].shape)
            frames.append(np.clip(src[i].astype(np.int16) + noise, 0, 255).astype(np.uint8))
            owner.append(i)
    return np.stack(frames), np.array(owner)
