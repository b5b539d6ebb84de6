"""CPU: the two statements of the masked top-k oracle (tests/mask_ref.py) against each other, the packing rule of a row
mask, the host-side rules of the masked search (scratch owner rule, refusals, header text, exported symbols) and the data
precondition of the GPU scan test (tests/test_mask_gpu.py), proven here from the oracle alone."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mask_ref as MR
from tests.host_memory import host_memory, owner_rule_holds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed, n=3000, D=768, Q=12):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, D)).astype(np.float16)
    for i in range(0, 200, 7):                       # planted exact duplicates, selected and not
        rows[rng.integers(0, n)] = rows[i]
    q = rows[rng.integers(0, n, Q)].astype(np.float32) + 0.1 * rng.standard_normal((Q, D)).astype(np.float32)
    q = q.astype(np.float16)
    q[3] = rows[0]
    q[4] = 0
    sel = rng.random((Q, n)) < rng.random((Q, 1))    # another selectivity per query
    sel[0] = False                                   # no row
    sel[1] = True                                    # every row
    sel[2] = False
    sel[2, 17] = True                                # one row
    return q.view(np.uint16), rows.view(np.uint16), sel


@pytest.mark.parametrize("score_mode,min_score", [(0, None), (0, 0.3), (1, 0.65)])
@pytest.mark.parametrize("seed", [0, 1])
def test_two_statements_agree(seed, score_mode, min_score):
    q, rows, sel = _case(seed)
    for k in (1, 10, 64):
        ra, sa = MR.masked_topk(q, rows, sel, k, "f16", score_mode, min_score, base=7)
        rb, sb = MR.masked_topk_matrix(q, rows, sel, k, "f16", score_mode, min_score, base=7)
        assert np.array_equal(ra, rb)
        assert np.array_equal(sa.view(np.int64), sb.view(np.int64))
        assert (ra[0] == -1).all() and (sa[0] == 0.0).all() and (ra[2, 1:] == -1).all()
        assert (ra[3:] >= 7).any()
    r, _ = MR.masked_topk(q, rows, sel, 64, "f16", score_mode, min_score)
    for qi in range(q.shape[0]):                     # only selected rows are ever returned
        assert sel[qi][r[qi][r[qi] >= 0]].all()


def test_every_row_selected_equals_the_row_ranking():
    from oracle import cref
    q, rows, sel = _case(5, n=500, D=128, Q=6)
    r0, s0 = cref.cosine_topk(q, rows, 20)
    r1, s1 = MR.masked_topk(q, rows, np.ones_like(sel), 20)
    assert np.array_equal(r0, r1) and np.array_equal(s0.view(np.int64), s1.view(np.int64))


def test_ties_by_row_id_and_zero_query():
    scores = np.array([[0.9, 0.9, 0.5, 0.9, 0.9], [0.0] * 5])
    sel = np.array([[False, True, True, True, False]] * 2)
    r, s = MR.masked_topk_from_scores(scores, sel, 3)
    assert r.tolist() == [[1, 3, 2], [1, 2, 3]] and s[1].tolist() == [0.0] * 3


# ---- packing: bit s & 31 of word s >> 5, s = r mod capacity ----------------------------------------------------------
def _host_ring(capacity, total):
    """A host memory that stands for a ring of ``capacity`` after ``total`` rows: ``len`` is all the host rules read."""
    mem = host_memory(capacity=capacity, library=type("Sized", (), {"vm_memory_size": lambda self, h: total})())
    mem.ring = total > capacity
    mem.ids, mem.meta, mem.table_base = [f"id{r}" for r in range(total)], [{"r": r} for r in range(total)], 0
    return mem


def test_packing_of_a_linear_memory():
    mem = _host_ring(100, 70)
    assert mem.mask_words == MR.mask_words(100) == 4          # 100 rows -> 128 -> 4 words
    assert host_memory(capacity=64).mask_words == 2 and host_memory(capacity=65).mask_words == 4
    want = [0, 31, 32, 63, 64, 69]
    m = mem.mask_where(lambda row, id_, meta: row in want)
    assert m.dtype == torch.int32 and tuple(m.shape) == (4,)
    assert np.array_equal(m.numpy().view(np.uint32), MR.pack_rows(want, 100))
    assert m.numpy().view(np.uint32).tolist() == [0x80000001, 0x80000001, 0x21, 0]
    assert mem.rows_of_mask(m) == want
    assert mem.rows_of_mask(~m) == [r for r in range(70) if r not in want]          # dead bits of ~m are ignored
    assert mem.rows_of_mask(torch.full((4,), -1, dtype=torch.int32)) == list(range(70))
    assert MR.selected(MR.pack_rows(want, 100), 0, 70, 100).nonzero()[0].tolist() == want


def test_packing_of_a_ring_of_40_after_57_rows():
    mem = _host_ring(40, 57)                                     # rows 17 .. 56 live; row r sits in slot r % 40
    assert mem.mask_words == 2
    want = [17, 39, 40, 56]                                      # slots 17, 39, 0, 16
    m = mem.mask_where(lambda row, id_, meta: meta["r"] in want and id_ == f"id{row}")
    words = m.numpy().view(np.uint32)
    assert np.array_equal(words, MR.pack_rows(want, 40))
    assert words.tolist() == [(1 << 17) | (1 << 0) | (1 << 16), 1 << (39 - 32)]
    assert mem.rows_of_mask(m) == want
    assert MR.selected(words, 17, 40, 40).nonzero()[0].tolist() == [0, 22, 23, 39]   # indices among the live rows
    full = torch.full((2,), -1, dtype=torch.int32)
    assert mem.rows_of_mask(full) == list(range(17, 57))         # the padding's bits (slots 40 .. 63) name no row
    sel = MR.selection(np.stack([words, ~words]), [0, 1, 2, -1], 4, 17, 40, 40)
    assert sel[0].sum() == 4 and sel[1].sum() == 36 and not sel[2].any() and not sel[3].any()


# ---- the scratch owner rule for the new kind (tests/host_memory.py's stand-in sizing library) -------------------
def test_masked_scratch_follows_the_owner_rule():
    mem = owner_rule_holds("MaskedTopkScratch", "prepare_topk_masked")
    assert mem.last_mask_flags is None and mem.masked_uncertified_count == 0


# ---- refusals, before the library is called (host_memory's library fails the test when reached) ----------------------
def test_python_refusals():
    mem = host_memory(capacity=100)
    W = mem.mask_words
    q = [[0.0] * mem.dim]
    ok = torch.zeros(W, dtype=torch.int32)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_masked(q, k, ok)
    for bad, what in ((torch.zeros(W, dtype=torch.int64), "int32"), (torch.zeros(W, dtype=torch.uint8), "int32"),
                      ([0] * W, "int32"), (torch.zeros((1, 1, W), dtype=torch.int32), "mask is"),
                      (torch.zeros((0, W), dtype=torch.int32), "mask is"),
                      (torch.zeros(W + 2, dtype=torch.int32), "width"), (torch.zeros((3, W - 1), dtype=torch.int32), "width")):
        with pytest.raises(ValueError, match=what):
            mem.topk_masked(q, 3, bad)
        with pytest.raises(ValueError, match=what):
            mem.rows_of_mask(bad)
    with pytest.raises(ValueError, match="mask_index"):           # 3 masks, 1 query, no index
        mem.topk_masked(q, 3, torch.zeros((3, W), dtype=torch.int32))
    with pytest.raises(ValueError, match="mask ind"):
        mem.topk_masked(q, 3, torch.zeros((3, W), dtype=torch.int32), mask_index=[0, 1])
    with pytest.raises(ValueError, match="mask_index"):
        mem.topk_masked(q, 3, ok, mask_index=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="tagged"):
        mem.mask_of_scope((0, 5))
    with pytest.raises(ValueError, match="int64"):
        mem.mask_of_rows(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        mem.mask_of_rows([1, 2], out=torch.zeros(W + 2, dtype=torch.int32))


class _FakeMemory:
    grouped = False
    tagged = False
    dim = 768
    searchable = 10


class _FakeTaggedGrouped(_FakeMemory):
    grouped = True
    tagged = True


def test_adapters_refuse_mask_with_scope_or_distinct():
    from vidmem import _lib
    from vidmem.similarity import HipPreLLMSimilarity, HipVectorSearch, batch_similarities
    m = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="mask and scope are mutually exclusive"):
        batch_similarities(_FakeTaggedGrouped(), [[0.0] * 768], 3, scope=(0, 10), mask=m)
    with pytest.raises(ValueError, match="mask and distinct=True are mutually exclusive"):
        batch_similarities(_FakeTaggedGrouped(), [[0.0] * 768], 3, distinct=True, mask=m)
    with pytest.raises(ValueError, match="mutually exclusive"):
        HipPreLLMSimilarity(_FakeTaggedGrouped(), object(), scope=(0, 10), mask=m)
    with pytest.raises(ValueError, match="mutually exclusive"):
        HipVectorSearch(_FakeTaggedGrouped(), object(), object(), score_mode=_lib.VM_SCORE_RAW, distinct=True, mask=m)
    assert HipVectorSearch(_FakeMemory(), object(), object(), score_mode=_lib.VM_SCORE_RAW, mask=m).mask is m
    assert HipPreLLMSimilarity(_FakeMemory(), object(), mask=m).mask is m


# ---- the header and the library --------------------------------------------------------------------------------------
def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "vidmem.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("bit s & 31 of word s >> 5 with s = r mod capacity",
                   "A bit whose slot holds no live row",
                   "is ignored by every consumer",
                   "An index outside [0, n_masks) is the EMPTY mask",
                   "mask 0 for every query when n_masks == 1, mask q for query q when n_masks == Q",
                   "equals vm_topk_cosine + vm_topk_redo_flagged",
                   "it equals vm_topk_cosine_scoped",
                   "an erase renumbers rows and a ring overwrites them",
                   "vm_memory_erase_scoped's selector",
                   "Writes every word of the mask"):
        assert phrase in flat, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in (r"int64_t vm_memory_mask_words\(const vm_memory \*mem\);",
                 r"size_t vm_topk_masked_workspace_bytes\(const vm_memory \*mem, int Q, int k\);",
                 r"int vm_topk_cosine_masked\(vm_memory \*mem, const void \*queries, int Q, int k, const uint32_t \*masks, "
                 r"int n_masks,\s+const int32_t \*mask_index, int use_min_score, double min_score, int score_mode,",
                 r"int vm_mask_from_rows\(vm_memory \*mem, const int64_t \*row_ids, int64_t n, int64_t row_stride, "
                 r"int64_t row_offset,\s+int clear_first, uint32_t \*out_mask, void \*stream\);",
                 r"int vm_mask_from_scopes\(vm_memory \*mem, const int64_t \*scope_lo, const int64_t \*scope_hi, "
                 r"int n_ranges,\s+uint32_t \*out_mask, void \*stream\);"):
        assert re.search(decl, code), decl


def test_library_exports_the_mask_symbols_and_abi_4():
    from vidmem import _lib
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_memory_mask_words", "vm_topk_masked_workspace_bytes", "vm_topk_cosine_masked",
                "vm_topk_cosine_masked_exact", "vm_mask_from_rows", "vm_mask_from_scopes"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_memory_mask_words(None) == 0 and L.vm_topk_masked_workspace_bytes(None, 1, 1) == 0
    assert L.vm_topk_cosine_masked(None, None, 1, 1, None, 1, None, 0, 0.0, 0, 1, 0, None, None, None, None, None, 0,
                                   None) == _lib.VM_ERR_INVALID
    assert L.vm_topk_cosine_masked_exact(None, None, 1, 1, None, 1, None, 0, 0.0, 0, 1, 0, None, None, None, 0,
                                         None) == _lib.VM_ERR_INVALID
    assert L.vm_mask_from_rows(None, None, 0, 1, 0, 1, None, None) == _lib.VM_ERR_INVALID
    assert L.vm_mask_from_scopes(None, None, None, 0, None, None) == _lib.VM_ERR_INVALID


# ---- the GPU scan test's precondition --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", [(128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16")])
def test_scan_test_inputs_leave_no_query_to_the_redo(D, dtype, shape):
    """For every data set, Q and mask set of tests/test_mask_gpu.py's scan test: the exact best and 10th selected scores
    lie more than 4 x cert_eps(D) apart, or fewer than 10 rows are selected - the certificate needs 2 x, so a query the
    fast entry flags there is a scan that went wrong, not data that asked for the redo."""
    from tests import range_ref
    assert MR.cert_eps(D) == range_ref.cert_eps(D)
    MR.scan_precondition(D, dtype, shape)
    sets = MR.mask_sets(33, shape)
    total, cap = MR.SHAPES[shape]
    n, capacity, base = min(total, cap or total), cap or total, (total - cap if cap else 0)
    count = {name: MR.selection(m, i, 33, base, n, capacity).sum(axis=1) for name, (m, i) in sets.items()}
    assert (count["full"] == n).all() and (count["empty"] == 0).all() and (count["first_dead"] == 0).all()
    assert (count["last_live"] == 1).all() and (count["first_tile"] == 16).all()
    assert count["one_empty"][16] == 0 and count["one_empty"].sum() == 32 * n
    assert set(count["alternating"].tolist()) <= {n // 2, (n + 1) // 2}
    if cap:
        assert MR.selection(*sets["newest"], 33, base, n, capacity)[0].nonzero()[0].tolist() == [n - 1]
        assert MR.selection(*sets["oldest"], 33, base, n, capacity)[0].nonzero()[0].tolist() == [0]
