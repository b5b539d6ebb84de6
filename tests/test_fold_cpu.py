"""No GPU: the any/all oracle against itself and against the row oracle, the identities of the definition, the +-0.0
rules, the guarantee of ``similarity.linked_similarities`` against the reference's two-step merge (on the real function,
over a memory that answers from the oracle), the Python refusals and the header, the precondition of the GPU scan test
(tests/test_fold_gpu.py) proven from oracle scores alone, and planted defects: each a wrong scorer of the kind a kernel
could be, shown to change a result the GPU cases compare.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import cref
from tests import fold_ref as FR
from tests import mask_ref as MR
from tests.support import same_arrays, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_case = MR.host_case


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", FR.DTS)
def test_loop_and_array_statements_agree_bit_for_bit(D, dtype):
    rows, q, base, live = _case(D, dtype)
    for op in FR.OPS:
        for J in FR.JS:
            for wname in FR.WEIGHT_SETS + ("zeros",):
                w = [0.0, -0.0, 0.0][:J] + [0.0] * max(0, J - 3) if wname == "zeros" else FR.weights_of(wname, J)
                for c in range(3):
                    e = live[FR.term_rows(c, J)]
                    (fa, ta), (fb, tb) = FR.fold_scores_loop(e, w, op), FR.fold_scores(e, w, op)
                    assert same_bits(fa, fb) and np.array_equal(ta, tb), (op, J, wname, c)
                    assert ta.dtype == np.int32 and ta.min() >= 0 and ta.max() < J
        terms = q[[FR.term_rows(c, 5) for c in range(3)]]
        ws = [FR.weights_of("signed", 5)] * 3
        sel = MR.selection(*MR.mask_sets(3, "n47")["alternating"], 3, base, rows.shape[0], 47)
        for k in (1, 5, 64):
            a = FR.fold_topk(terms, ws, rows, sel, k, op, dtype, base=base)
            b = FR.fold_topk(terms, ws, rows, sel, k, op, dtype, base=base, scores=FR.fold_scores)
            assert same_arrays(a, b) and np.array_equal(a[2], b[2])
            assert ((a[2] == -1) == (a[0] == -1)).all()


@pytest.mark.parametrize("D,dtype", FR.DTS)
def test_one_term_of_weight_one_is_the_row_oracle(D, dtype):
    rows, q, base, live = _case(D, dtype)
    terms = q[:4, None, :]
    ws = [[1.0]] * 4
    for op in FR.OPS:
        for k in (1, 5, 20):
            r, s = cref.cosine_topk(q[:4], rows, k, dtype=dtype)
            assert same_arrays(FR.fold_topk(terms, ws, rows, None, k, op, dtype), (r, s))
            for cut in (0.2, -0.1):
                r, s = cref.cosine_topk(q[:4], rows, k, dtype=dtype, min_score=cut)
                assert same_arrays(FR.fold_topk(terms, ws, rows, None, k, op, dtype, min_score=cut), (r, s))
            masks, index = MR.mask_sets(4, "n47")["alternating"]
            sel = MR.selection(masks, index, 4, base, rows.shape[0], 47)
            assert same_arrays(FR.fold_topk(terms, ws, rows, sel, k, op, dtype, base=base),
                         MR.masked_topk(q[:4], rows, sel, k, dtype=dtype, base=base))
    # unit weights: F is the element-wise maximum (minimum) of the J exact score rows
    for J in (2, 5, 16):
        e = live[FR.term_rows(1, J)]
        assert same_bits(FR.fold_scores_loop(e, [1.0] * J, "max")[0], e.max(axis=0))
        assert same_bits(FR.fold_scores_loop(e, [1.0] * J, "min")[0], e.min(axis=0))


def test_permutation_duplicate_and_batch_identities():
    rows, q, base, live = _case(384, "bf16")
    rng = np.random.default_rng(5)
    for op in FR.OPS:
        for wname in FR.WEIGHT_SETS:
            for J in (2, 5, 16):
                e, w = live[FR.term_rows(2, J)], FR.weights_of(wname, J)
                F, T = FR.fold_scores_loop(e, w, op)
                perm = rng.permutation(J)
                Fp, Tp = FR.fold_scores_loop(e[perm], [w[i] for i in perm], op)
                assert same_bits(F, Fp)                                       # no score bit changes, so no row does
                p = np.asarray(w)[:, None] * e
                assert same_bits(p[perm][Tp, np.arange(e.shape[1])], F) and same_bits(p[T, np.arange(e.shape[1])], F)   # only T moves
                if J < 16:                                                      # a copy of a term with its weight: nothing
                    for d in range(J):
                        Fd, Td = FR.fold_scores_loop(np.concatenate([e, e[d:d + 1]]), w + [w[d]], op)
                        assert same_bits(F, Fd) and np.array_equal(T, Td)
        # a query alone equals the same query inside a batch
        terms = q[[FR.term_rows(c, 5) for c in range(3)]]
        ws = [FR.weights_of(n, 5) for n in FR.WEIGHT_SETS]
        sel = MR.selection(*MR.mask_sets(3, "n47")["alternating"], 3, base, rows.shape[0], 47)
        r, s, t = FR.fold_topk(terms, ws, rows, sel, 5, op, "bf16")
        for c in range(3):
            r1, s1, t1 = FR.fold_topk(terms[c:c + 1], ws[c:c + 1], rows, sel[c:c + 1], 5, op, "bf16")
            assert same_arrays((r1, s1), (r[c:c + 1], s[c:c + 1])) and np.array_equal(t1, t[c:c + 1])


def test_signed_zeros_and_zero_weights():
    rows, q, base, live = _case()
    e = live[FR.term_rows(0, 3)]
    assert (e < 0).any() and (e > 0).any()
    n = e.shape[1]
    # a zero weight is not neutral: its product +-0.0 takes part
    F, T = FR.fold_scores_loop(e[:2], [1.0, 0.0], "max")
    assert same_bits(np.abs(F), np.maximum(e[0], 0.0)) and (F >= 0).all() and ((T == 1) == (e[0] < 0)).all()
    F, T = FR.fold_scores_loop(e[:2], [1.0, 0.0], "min")
    assert (F <= 0).all() and ((T == 1) == (e[0] > 0)).all()
    # the one exception to "a permutation changes no score bit": products that tie as zeros of both signs give F the sign
    # of the first in term order, so swapping the two terms flips the sign bit of the zero score - and nothing else
    for op in FR.OPS:
        two = np.stack([e[0], e[0]])
        F, T = FR.fold_scores_loop(two, [0.0, -0.0], op)
        Fp, Tp = FR.fold_scores_loop(two, [-0.0, 0.0], op)
        assert (F == 0.0).all() and (Fp == 0.0).all() and (T == 0).all() and (Tp == 0).all()
        assert np.array_equal(np.signbit(F), ~np.signbit(Fp)) and np.array_equal(np.signbit(F), e[0] < 0)
        keep = np.ones((1, n), dtype=bool)
        assert np.array_equal(MR.masked_topk_from_scores(F[None], keep, 5)[0], MR.masked_topk_from_scores(Fp[None], keep, 5)[0])
    # all-zero weights: every product is +-0.0, the strict compare never replaces the first, so F carries the sign of
    # w_0 * e_0 and T is 0; the ranking is the first k selected rows by id
    for op in FR.OPS:
        for w in ([0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, -0.0, -0.0]):
            F, T = FR.fold_scores_loop(e, w, op)
            assert (F == 0.0).all() and (T == 0).all()
            assert np.array_equal(np.signbit(F), np.signbit(np.float64(w[0]) * e[0]))
            Fb, Tb = FR.fold_scores(e, w, op)
            assert same_bits(F, Fb) and np.array_equal(T, Tb)
        terms = q[[FR.term_rows(c, 3) for c in range(2)]]
        sel = np.zeros((2, n), dtype=bool)
        sel[:, 3::2] = True
        r, s, t = FR.fold_topk(terms, [[0.0, 0.0, 0.0]] * 2, rows, sel, 5, op)
        assert r.tolist() == [[3, 5, 7, 9, 11]] * 2 and (s == 0.0).all() and (t == 0).all()
        e2 = cref.cosine_matrix(terms.reshape(6, -1), rows)[[0, 3]]
        assert np.array_equal(np.signbit(s), np.signbit(e2[:, [3, 5, 7, 9, 11]] * 0.0))


def test_eps_fold_restated():
    for D in (128, 384, 768, 2048):
        for A in (0.0, 1.0, 2.5, 2.0 ** -20, 2.0 ** 20):
            assert FR.eps_fold(D, A) == A * (2.0 * (D + 8) * 2.0 ** -24 + 2.0 ** -21)
    # per column: the coefficient's rounding and the product's, 2^-24 relative each, on a magnitude of at most
    # |w| (1 + cert_eps); max and min are 1-Lipschitz in the sup norm and round nothing
    assert 2 * 2.0 ** -24 * (1 + MR.cert_eps(2048)) * (1 + 2.0 ** -24) < FR.FOLD_C
    assert FR.slack_m(1) == 9 and FR.slack_m(5) == 13 and FR.slack_m(64) == 80
    for name in FR.WEIGHT_SETS:                                     # every scan weight is inside the domain
        for J in FR.JS:
            assert all(FR.W_MIN <= abs(x) <= FR.W_MAX for x in FR.weights_of(name, J))
    assert FR.abs_max([1.0, -2.5, 0.0, 0.25]) == 2.5
    assert FR.weights_of("signed", 5) == [1.0, 1.0, -0.5, 1.0, 1.0] and FR.weights_of("wide", 3) == [0.25, -0.5, 1.0]


# ---- linked_similarities ----------------------------------------------------------------------------------------------------
class OracleMemory:
    """What ``similarity.batch_similarities`` and ``linked_similarities`` use of an EmbeddingMemory, answered by the
    oracle on the host: fp16 rows, one id per row, one optional row mask (a bool vector here)."""

    def __init__(self, rows_f16: torch.Tensor, ids):
        self.rows = rows_f16.contiguous()
        self.bits = self.rows.view(torch.int16).numpy().view(np.uint16)
        self.ids, self.dim, self.device = list(ids), int(rows_f16.shape[1]), torch.device("cpu")
        self.searchable = len(self.ids)
        self.fold_calls = []

    def __len__(self):
        return len(self.ids)

    def id_of(self, r):
        return self.ids[r]

    def rows_of_mask(self, mask):
        return [int(i) for i in np.nonzero(mask)[0]]

    def _q(self, q):
        return q.to(torch.float16).contiguous().view(torch.int16).numpy().view(np.uint16)

    def topk(self, q, k):
        r, s = cref.cosine_topk(self._q(q), self.bits, k, dtype="f16")
        return torch.from_numpy(s), torch.from_numpy(r)

    def topk_masked(self, q, k, mask):
        sel = np.broadcast_to(np.asarray(mask, dtype=bool), (q.shape[0], len(self)))
        r, s = MR.masked_topk(self._q(q), self.bits, sel, k, dtype="f16")
        return torch.from_numpy(s), torch.from_numpy(r)

    def topk_fold(self, terms, k, op="max", weights=None, mask=None, min_score=None):
        t = self._q(terms)
        C, J = t.shape[:2]
        self.fold_calls.append((C, J, k))
        sel = None if mask is None else np.broadcast_to(np.asarray(mask, dtype=bool), (C, len(self)))
        r, s, w = FR.fold_topk(t, [[1.0] * J if weights is None else list(weights)] * C, self.bits, sel, k, op,
                               min_score=min_score)
        return torch.from_numpy(s), torch.from_numpy(r), torch.from_numpy(w)


def _linking_memory(n=90, D=64, seed=3):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randn(n, D, generator=g).to(torch.float16)
    q = (rows[torch.randint(0, n, (40,), generator=g)].float() + 0.7 * torch.randn(40, D, generator=g)).to(torch.float16)
    mem = OracleMemory(rows, [f"chunk-{i:03d}" for i in range(n)])
    return mem, q, cref.cosine_matrix(mem._q(q), mem.bits, dtype="f16")


def test_linked_similarities_equals_the_reference_merge():
    from vidmem.similarity import batch_similarities, linked_similarities, merge_batch_similarities
    mem, q, cos = _linking_memory()
    sel = np.zeros(len(mem), dtype=bool)
    sel[::3] = True
    for Q in (1, 3, 7, 16, 17, 40):
        emb = [q[i] for i in range(Q)]
        for k_each, k_final in ((10, 10), (10, 4), (5, 1), (64, 64), (70, 64)):
            for mask, sl in ((None, None), (sel, sel)):
                want = FR.reference_linking(list(cos[:Q]), mem.ids, k_each, k_final, sl)
                # the model of the reference is the adapter's own two-step path, and (restated) the reference's lines
                assert want == merge_batch_similarities(batch_similarities(mem, emb, k_each, mask=mask), k_final)
                n_calls = len(mem.fold_calls)
                got = linked_similarities(mem, emb, k_each, k_final, mask=mask)
                assert len(mem.fold_calls) == n_calls + 1                       # ONE call, whatever Q
                assert mem.fold_calls[-1] == (-(-Q // min(Q, 16)), min(Q, 16), k_final)
                assert [s for _, s in got] == [s for _, s in want], (Q, k_each, k_final)
                scores = [s for _, s in FR.reference_linking(list(cos[:Q]), mem.ids, k_each + 1, k_final + 1, sl)]
                assert len(set(scores)) == len(scores)                          # tie-free, the best row left out included
                assert got == want, (Q, k_each, k_final)
                assert got == FR.fold_linking(list(cos[:Q]), mem.ids, k_final, sl)
    # failed / None entries contribute [] in the reference
    emb = [q[0], ValueError("embedder failed"), q[1], None, q[2]]
    assert linked_similarities(mem, emb, 6, 6) == FR.reference_linking([cos[0], None, cos[1], None, cos[2]], mem.ids, 6, 6)
    assert linked_similarities(mem, [None, RuntimeError("x")], 6, 6) == []
    assert linked_similarities(mem, [], 6, 6) == []
    # list embeddings, as the reference's embedder returns them
    emb = [q[i].float().tolist() for i in range(3)]
    assert linked_similarities(mem, emb, 6, 5) == FR.reference_linking(list(cos[:3]), mem.ids, 6, 5)
    # the fallbacks are the two-step path itself and call no fold
    n_calls = len(mem.fold_calls)
    emb = [q[i] for i in range(4)]
    assert linked_similarities(mem, emb, 3, 6) == FR.reference_linking(list(cos[:4]), mem.ids, 3, 6)
    assert linked_similarities(mem, emb, 80, 70) == FR.reference_linking(list(cos[:4]), mem.ids, 80, 70)
    short = [q[0], q[1][:32]]
    assert linked_similarities(mem, short, 5, 5) == merge_batch_similarities(batch_similarities(mem, short, 5), 5)
    assert linked_similarities(mem, emb, 0, 0) == [] and len(mem.fold_calls) == n_calls
    # two returned rows under one id: the reference merges per id, so the two-step path answers
    twin = OracleMemory(mem.rows, ["same" if i in (4, 5) else x for i, x in enumerate(mem.ids)])
    emb = [mem.rows[4], mem.rows[5]]
    got = linked_similarities(twin, emb, 5, 5)
    assert got == merge_batch_similarities(batch_similarities(twin, emb, 5), 5) and [i for i, _ in got].count("same") == 1


def test_linked_similarities_on_an_exact_tie_orders_by_row_id_where_the_reference_orders_by_first_seen():
    from vidmem.similarity import linked_similarities
    rows = torch.zeros(8, 64, dtype=torch.float16)
    for i in range(8):
        rows[i, i] = 1.0
        rows[i, 63] = 0.25 * (i + 1)                                            # no two rows alike
    rows[2], rows[5] = 0.0, 0.0
    rows[2, 10], rows[5, 11] = 2.0, 3.0                                         # two one-hot rows
    mem = OracleMemory(rows, [f"chunk-{i}" for i in range(8)])
    emb = [rows[5], rows[2]]                                                    # row 5 is seen first, in embedding 0's list
    cos = cref.cosine_matrix(mem._q(torch.stack(emb)), mem.bits, dtype="f16")
    assert cos[0, 5] == 1.0 and cos[1, 2] == 1.0 and cos[0, 2] == 0.0 and cos[1, 5] == 0.0
    want = FR.reference_linking(list(cos), mem.ids, 3, 2)
    got = linked_similarities(mem, emb, 3, 2)
    assert want == [("chunk-5", 1.0), ("chunk-2", 1.0)]                         # first-seen
    assert got == [("chunk-2", 1.0), ("chunk-5", 1.0)]                          # row id
    assert [s for _, s in got] == [s for _, s in want] and sorted(got) == sorted(want)


# ---- the Python layer, before the library is called ------------------------------------------------------------------------
def test_python_refusals_and_scratch():
    from tests.host_memory import host_memory
    from tests.host_memory import SizingLibrary
    from vidmem import memory as M
    mem = host_memory(capacity=100)
    t = torch.zeros((2, 3, mem.dim))
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_fold(t, k)
    with pytest.raises(ValueError, match="op must be"):
        mem.topk_fold(t, 3, op="sum")
    with pytest.raises(ValueError, match="J"):
        mem.topk_fold(torch.zeros((1, 17, mem.dim)), 3)
    with pytest.raises(ValueError, match="J"):
        mem.topk_any(torch.zeros((1, 0, mem.dim)), 3)
    with pytest.raises(ValueError, match="terms must be"):
        mem.topk_all(torch.zeros((2, 3, mem.dim + 1)), 3)
    with pytest.raises(ValueError, match="weights must be"):
        mem.topk_fold(t, 3, weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="width"):
        mem.topk_fold(t, 3, mask=torch.zeros(mem.mask_words + 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="mask_index"):
        mem.topk_fold(t, 3, mask=torch.zeros((3, mem.mask_words), dtype=torch.int32))
    with pytest.raises(ValueError, match="needs a mask"):
        mem.topk_fold(t, 3, mask_index=[0, 0])
    with pytest.raises(ValueError, match="NaN"):
        mem.topk_fold(t, 3, min_score=float("nan"))
    with pytest.raises(ValueError, match="J"):
        mem.prepare_topk_fold(1, 17, 3)
    sized = host_memory(capacity=16, library=SizingLibrary())
    first = sized.prepare_topk_fold(4, 5, 10)                       # the stand-in sizes any vm_*_workspace_bytes entry
    assert isinstance(first, M.FoldTopkScratch) and first.fits(sized, 4, 10)
    assert first.flags.dtype == torch.int32
    assert sized.prepare_topk_fold(2, 16, 5) is first               # J does not size the workspace
    assert sized.prepare_topk_fold(64, 3, 32) is not first
    assert mem.last_fold_flags is None and mem.fold_uncertified_count == 0


def test_header_and_library():
    from vidmem import _lib
    text = open(os.path.join(ROOT, "include", "vidmem.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", text))
    for phrase in ("if p_j > acc (max) / p_j < acc (min): acc = p_j, arg = j",
                   "the first term wins a tie, and +0.0 is never replaced by -0.0",
                   "A ZERO WEIGHT IS NOT NEUTRAL here, unlike in vm_topk_cosine_mix",
                   "The padding columns J .. 15 of the query tile never take part",
                   "ranked by (F DESCENDING, row id ascending) for BOTH ops",
                   "F > min_score",
                   "-1 where the row is -1",
                   "Non-finite weights are undefined, as stored NaN is",
                   "eps_fold = A (2 (D + 8) 2^-24 + 2^-21), A = max_j |w_j|",
                   "every nonzero |w_j| lies in [2^-20, 2^20]"):
        assert phrase in flat, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in (r"enum vm_fold_op \{ VM_FOLD_MAX = 0, VM_FOLD_MIN = 1 \};",
                 r"size_t vm_topk_fold_workspace_bytes\(const vm_memory \*mem, int C, int k\);",
                 r"int vm_topk_cosine_fold\(vm_memory \*mem, const void \*terms, const double \*weights, int C, int J, int k, "
                 r"int op,",
                 r"int vm_topk_cosine_fold_exact\(vm_memory \*mem, const void \*terms, const double \*weights, int C, int J, "
                 r"int k, int op,"):
        assert re.search(decl, code), decl
    assert (_lib.VM_FOLD_MAX, _lib.VM_FOLD_MIN) == (0, 1)
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_topk_fold_workspace_bytes", "vm_topk_cosine_fold", "vm_topk_cosine_fold_exact"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_topk_fold_workspace_bytes(None, 1, 1) == 0
    assert L.vm_topk_cosine_fold(None, None, None, 1, 1, 1, 0, None, 0, None, 0, 0.0, 1, 0, None, None, None, None, None,
                                 None, 0, None) == _lib.VM_ERR_INVALID
    assert L.vm_topk_cosine_fold_exact(None, None, None, 1, 1, 1, 1, None, 0, None, 0, 0.0, 1, 0, None, None, None, None,
                                       0, None) == _lib.VM_ERR_INVALID


# ---- the GPU scan test's precondition --------------------------------------------------------------------------------------
def test_scan_precondition_holds_for_every_case():
    """The GPU scan test demands flag 0 where rank k and rank M + 1 of the oracle's F are more than 4 x eps_fold apart (or
    fewer than M + 1 rows are selected).  That holds for all 39,168 (dataset, op, C, J, weight set, mask set, k, query)
    cases, the unmasked ones included."""
    kept = total = 0
    smallest = (np.inf, None)
    for D, dtype in FR.DTS:
        for shape in MR.SHAPES:
            _, _, base, live = MR.host_dataset(D, dtype, shape)
            n = live.shape[1]
            sels = {C: FR.scan_selections(C, shape, base, n) for C in FR.CS}
            for op in FR.OPS:
                for J in FR.JS:
                    for wname in FR.WEIGHT_SETS:
                        F, _, w = FR.scan_scores(D, dtype, shape, J, wname, op)
                        A = FR.abs_max(w)
                        for C in FR.CS:
                            for name, sel in sels[C].items():
                                for c in range(C):
                                    best = np.sort(F[c][sel[c]])[::-1]
                                    for k in FR.KS:
                                        ok = FR.flag0_ok(best, k, D, A)
                                        total += 1
                                        kept += ok
                                        assert ok, (D, dtype, shape, op, J, wname, name, c, k, FR.margin(best, k, D, A))
                                        m = FR.margin(best, k, D, A)
                                        if m < smallest[0]:
                                            smallest = (m, (D, dtype, shape, op, J, wname, name, c, k))
    print(f"smallest margin {smallest[0]:.1f} x eps_fold at {smallest[1]}; {kept} of {total} cases keep flag 0")
    assert total == 39168 and kept == total
    assert smallest[0] > 4


# ---- planted defects --------------------------------------------------------------------------------------------------------
# Each is a scorer (e [J, n], w [J], op) -> (F, T) that is wrong the way a kernel could be.  ``_changes`` runs it through
# the ranking the GPU tests compare - rows, score bits, T - on cases those tests run, and reports whether anything differs.
def _changes(scorer, cases):
    for e, w, op, sel, k in cases:
        F, T = FR.fold_scores_loop(e, w, op)
        G, U = scorer(e, w, op)
        keep = np.ones((1, e.shape[1]), dtype=bool) if sel is None else sel[None]
        a = MR.masked_topk_from_scores(F[None], keep, k)
        b = MR.masked_topk_from_scores(np.asarray(G, dtype=np.float64)[None], keep, k)
        if not same_arrays(a, b) or not np.array_equal(FR.terms_of_rows(T[None], a[0]), FR.terms_of_rows(np.asarray(U)[None], b[0])):
            return True
    return False


def _scan_cases(ops=FR.OPS, wnames=FR.WEIGHT_SETS, Js=FR.JS):
    _, _, _, live = MR.host_dataset(128, "f16", "n47")
    return [(live[FR.term_rows(c, J)], FR.weights_of(wn, J), op, None, k)
            for op in ops for J in Js for wn in wnames for c in range(3) for k in FR.KS]


def _sum_instead(e, w, op):
    acc = np.zeros(e.shape[1])
    for j in range(e.shape[0]):
        acc = acc + np.float64(w[j]) * e[j]
    return acc, FR.fold_scores_loop(e, w, op)[1]


def _padding_votes(e, w, op):
    J = e.shape[0]
    return FR.fold_scores_loop(np.concatenate([e, np.zeros((16 - J, e.shape[1]))]), list(w) + [0.0] * (16 - J), op)


def _not_strict(e, w, op):
    F = np.empty(e.shape[1])
    T = np.empty(e.shape[1], dtype=np.int32)
    for r in range(e.shape[1]):
        acc, arg = float(w[0]) * float(e[0, r]), 0
        for j in range(1, e.shape[0]):
            p = float(w[j]) * float(e[j, r])
            if (p >= acc) if op == "max" else (p <= acc):
                acc, arg = p, j
        F[r], T[r] = acc, arg
    return F, T


def _last_tied_term(e, w, op):
    F, _ = FR.fold_scores_loop(e, w, op)
    p = np.asarray(w, dtype=np.float64)[:, None] * e
    return F, (e.shape[0] - 1 - np.argmax((p == F[None])[::-1], axis=0)).astype(np.int32)


def _min_ascending(e, w, op):
    F, T = FR.fold_scores_loop(e, w, op)
    return (-F, T) if op == "min" else (F, T)


def _weight_after_fold(e, w, op):
    F, T = FR.fold_scores_loop(e, [1.0] * e.shape[0], op)
    return np.asarray([w[t] for t in T]) * F, T


def test_planted_defects_change_results_the_gpu_cases_compare():
    scan = _scan_cases()
    assert not _changes(FR.fold_scores_loop, scan) and not _changes(FR.fold_scores, scan)      # the harness itself
    # 1. the sum in place of the fold
    assert _changes(_sum_instead, scan)
    # 2. the padding columns J .. 15 voting with their zero score: a minimum over positive cosines becomes 0.0
    assert _changes(_padding_votes, _scan_cases(ops=("min",), wnames=("ones",), Js=(1, 2, 5)))
    assert not _changes(_padding_votes, _scan_cases(Js=(16,)))                                  # nothing to pad
    # 3. >= instead of >: a later tied term replaces the first - T on identical terms, the sign of a zero
    _, _, _, live = MR.host_dataset(128, "f16", "n47")
    e = live[FR.term_rows(0, 3)]
    twice = [(np.stack([e[0], e[0]]), [1.0, 1.0], op, None, 5) for op in FR.OPS]               # "identical terms"
    zeros = [(e, [0.0, 0.0, 0.0], op, None, 5) for op in FR.OPS]                               # "all zero"
    assert _changes(_not_strict, twice) and _changes(_not_strict, zeros)
    F, _ = _not_strict(e, [0.0, 0.0, 0.0], "max")
    assert not same_bits(F, FR.fold_scores_loop(e, [0.0, 0.0, 0.0], "max")[0])                # the sign bit alone
    # 4. T of the last instead of the first tied term (the scores are right)
    assert _changes(_last_tied_term, twice) and not _changes(_last_tied_term, scan)
    # 5. the minimum ranked ascending: the worst rows first
    assert _changes(_min_ascending, _scan_cases(ops=("min",)))
    # 6. the weight applied after the fold: the unweighted winner, then scaled
    assert _changes(_weight_after_fold, _scan_cases(wnames=("signed", "wide"), Js=(2, 5, 16)))
    assert not _changes(_weight_after_fold, _scan_cases(wnames=("ones",)))
    # 7. the mask of query 0 used for every query: the alternating set gives query 1 the other half of the rows
    n = live.shape[1]
    sels = FR.scan_selections(2, "n47", 0, n)["alternating"]
    F, T = FR.fold_scores_loop(live[FR.term_rows(1, 5)], FR.weights_of("signed", 5), "max")
    right = MR.masked_topk_from_scores(F[None], sels[1:2], 5)
    wrong = MR.masked_topk_from_scores(F[None], sels[0:1], 5)
    assert not same_arrays(right, wrong) and not set(right[0][0]) & set(wrong[0][0])
    # 8. A = the SUM of the |w_j| where the bound states their maximum: the certificate asks for sixteen times the gap
    # with sixteen unit weights, and a query the test demands flag 0 for (more than 4 eps_fold(max) between rank k and
    # rank M + 1) can no longer be certified once the gap is at most eps(sum) - eps(max): the scanned rank M + 1 may sit
    # eps(max) below the exact one.  tests/test_fold_gpu.py test_certificate_uses_the_largest_weight builds that gap.
    D, J = 128, 16
    gap = FR.certificate_gap_case()[2]
    assert 4 * FR.eps_fold(D, 1.0) < gap <= FR.eps_fold(D, float(J)) - FR.eps_fold(D, 1.0)
    best = np.concatenate([[1.0], np.full(15, 1.0 - gap)])
    assert FR.flag0_ok(best, 1, D, FR.abs_max([1.0] * J)) and not FR.flag0_ok(best, 1, D, float(J))
    # 9. A smaller than the largest |w_j| (A = |w_0|): a certificate that does not hold - with weights (2^-20, 1) the
    # bound would shrink by 2^20 while one column still errs by cert_eps
    assert FR.eps_fold(D, 2.0 ** -20) * 2 ** 19 < MR.cert_eps(D) < FR.eps_fold(D, FR.abs_max([2.0 ** -20, 1.0]))

