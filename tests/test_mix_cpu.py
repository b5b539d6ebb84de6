"""No GPU: the mixed-query oracle against itself and against the row oracle, the host half of the feature
(``similarity.feedback_terms``, the Python refusals, the header), and the precondition of the GPU scan test
(tests/test_mix_gpu.py) proven from oracle scores alone.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import cref
from tests import mask_ref as MR
from tests import mix_ref as XR
from tests.support import same_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_case = MR.host_case


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", XR.DTS)
def test_loop_and_array_statements_agree_bit_for_bit(D, dtype):
    rows, q, base, live = _case(D, dtype)
    for J in XR.JS:
        for wname in XR.WEIGHT_SETS:
            w = XR.weights_of(wname, J)
            for c in range(3):
                e = live[XR.term_rows(c, J)]
                a, b = XR.mix_scores_loop(e, w), XR.mix_scores(e, w)
                assert np.array_equal(a.view(np.int64), b.view(np.int64)), (J, wname, c)
    terms = q[[XR.term_rows(c, 5) for c in range(3)]]
    ws = [XR.weights_of("feedback", 5)] * 3
    sel = MR.selection(*MR.mask_sets(3, "n47")["alternating"], 3, base, rows.shape[0], 47)
    for k in (1, 5, 64):
        assert same_arrays(XR.mix_topk(terms, ws, rows, sel, k, dtype, base=base),
                     XR.mix_topk(terms, ws, rows, sel, k, dtype, base=base, scores=XR.mix_scores))


@pytest.mark.parametrize("D,dtype", XR.DTS)
def test_one_term_of_weight_one_is_the_row_oracle(D, dtype):
    rows, q, base, live = _case(D, dtype)
    terms = q[:4, None, :]
    ws = [[1.0]] * 4
    for k in (1, 5, 20):
        r, s = cref.cosine_topk(q[:4], rows, k, dtype=dtype)
        assert same_arrays(XR.mix_topk(terms, ws, rows, None, k, dtype), (r, s))
        for cut in (0.2, -0.1):
            r, s = cref.cosine_topk(q[:4], rows, k, dtype=dtype, min_score=cut)
            assert same_arrays(XR.mix_topk(terms, ws, rows, None, k, dtype, min_score=cut), (r, s))
        masks, index = MR.mask_sets(4, "n47")["alternating"]
        sel = MR.selection(masks, index, 4, base, rows.shape[0], 47)
        assert same_arrays(XR.mix_topk(terms, ws, rows, sel, k, dtype, base=base),
                     MR.masked_topk(q[:4], rows, sel, k, dtype=dtype, base=base))


def test_zero_weight_padding_is_bit_neutral():
    rows, q, base, live = _case(384, "bf16")
    for wname in ("mean", "feedback", "wide"):
        w3 = XR.weights_of(wname, 3)
        t3 = q[[XR.term_rows(c, 3) for c in range(3)]]
        t16 = np.concatenate([t3, q[None, 10:23].repeat(3, axis=0)], axis=1)
        assert t16.shape[1] == 16
        for k in (1, 5):
            assert same_arrays(XR.mix_topk(t3, [w3] * 3, rows, None, k, "bf16"),
                         XR.mix_topk(t16, [w3 + [0.0] * 13] * 3, rows, None, k, "bf16"))
    e = live[XR.term_rows(0, 16)]
    w = XR.weights_of("wide", 5)
    a, b = XR.mix_scores_loop(e[:5], w), XR.mix_scores_loop(e, w + [0.0] * 11)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.array_equal(XR.mix_scores_loop(e, [0.0] * 16).view(np.int64), np.zeros(e.shape[1], np.int64))    # +0.0


def test_permuting_the_queries_permutes_the_results():
    rows, q, base, live = _case()
    terms = q[[XR.term_rows(c, 5) for c in range(3)]]
    ws = [XR.weights_of(n, 5) for n in ("mean", "feedback", "wide")]
    sel = MR.selection(*MR.mask_sets(3, "n47")["alternating"], 3, base, rows.shape[0], 47)
    r, s = XR.mix_topk(terms, ws, rows, sel, 5)
    perm = [2, 0, 1]
    rp, sp = XR.mix_topk(terms[perm], [ws[i] for i in perm], rows, sel[perm], 5)
    assert same_arrays((rp, sp), (r[perm], s[perm]))


def test_eps_mix_restated():
    for D in (128, 384, 768, 2048):
        for A in (0.0, 1.0, 2.5, 2.0 ** -20, 2.0 ** 24):
            assert XR.eps_mix(D, A) == A * (2.0 * (D + 8) * 2.0 ** -24 + 2.0 ** -21)
    assert XR.eps_mix(768, 1.0) == MR.cert_eps(768) + 2.0 ** -21
    # 6 roundings of at most 2^-24 relative each, with slack
    assert 6 * 2.0 ** -24 < 2.0 ** -21
    assert XR.slack_m(1) == 9 and XR.slack_m(5) == 13 and XR.slack_m(64) == 80
    for name in XR.WEIGHT_SETS:                                     # every scan weight is inside the domain, or zero
        for J in XR.JS:
            assert all(x == 0.0 or XR.W_MIN <= abs(x) <= XR.W_MAX for x in XR.weights_of(name, J))
    assert XR.abs_sum([1.0, -0.5, 0.0, 0.25]) == 1.75


# ---- feedback_terms -------------------------------------------------------------------------------------------------------
def test_feedback_terms_weights_and_errors():
    from vidmem.similarity import feedback_terms
    q = torch.arange(8, dtype=torch.float16)
    pos = [torch.ones(8, dtype=torch.float16) * i for i in (1, 2, 3)]
    neg = [torch.full((8,), -1.0, dtype=torch.float16), torch.zeros(8, dtype=torch.float16)]
    terms, w = feedback_terms(q, pos, neg)
    assert terms.shape == (6, 8) and terms.dtype == torch.float16
    assert torch.equal(terms, torch.stack([q, *pos, *neg]))         # the query, the positives, the negatives
    assert w == [1.0, 0.75 / 3, 0.75 / 3, 0.75 / 3, -0.15 / 2, -0.15 / 2]
    terms, w = feedback_terms(q, pos[:1], (), alpha=2.0, beta=0.5, gamma=9.0)
    assert terms.shape == (2, 8) and w == [2.0, 0.5]
    terms, w = feedback_terms([0.5] * 8)                            # lists, no examples: the query alone
    assert terms.shape == (1, 8) and terms.dtype == torch.float32 and w == [1.0]
    terms, w = feedback_terms([0.5] * 8, negatives=[q])             # mixed kinds become float32
    assert terms.dtype == torch.float32 and w == [1.0, -0.15]
    terms, w = feedback_terms(q, [q] * 8, [q] * 7)                  # 16 terms: the most a mixed query holds
    assert terms.shape == (16, 8) and len(w) == 16
    with pytest.raises(ValueError, match="at most 16"):
        feedback_terms(q, [q] * 8, [q] * 8)
    with pytest.raises(ValueError, match="shape"):
        feedback_terms(q, [torch.ones(7)])
    with pytest.raises(ValueError, match="not finite"):
        feedback_terms(q, [q], beta=float("inf"))


# ---- the Python layer, before the library is called ------------------------------------------------------------------------
def test_python_refusals_and_scratch():
    from tests.host_memory import host_memory
    from tests.host_memory import SizingLibrary
    from vidmem import memory as M
    mem = host_memory(capacity=100)
    t = torch.zeros((2, 3, mem.dim))
    for k in (0, 65):
        with pytest.raises(ValueError, match="k"):
            mem.topk_mix(t, [1.0, 0.0, 0.0], k)
    with pytest.raises(ValueError, match="J"):
        mem.topk_mix(torch.zeros((1, 17, mem.dim)), [1.0] * 17, 3)
    with pytest.raises(ValueError, match="J"):
        mem.topk_mix(torch.zeros((1, 0, mem.dim)), [], 3)
    with pytest.raises(ValueError, match="terms must be"):
        mem.topk_mix(torch.zeros((2, 3, mem.dim + 1)), [1.0] * 3, 3)
    with pytest.raises(ValueError, match="terms must be"):
        mem.topk_mix(torch.zeros(mem.dim), [1.0], 3)
    with pytest.raises(ValueError, match="weights must be"):
        mem.topk_mix(t, [1.0, 2.0], 3)
    with pytest.raises(ValueError, match="weights must be"):
        mem.topk_mix(t, [[1.0, 2.0, 3.0]] * 3, 3)
    with pytest.raises(ValueError, match="width"):
        mem.topk_mix(t, [1.0] * 3, 3, mask=torch.zeros(mem.mask_words + 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="mask_index"):
        mem.topk_mix(t, [1.0] * 3, 3, mask=torch.zeros((3, mem.mask_words), dtype=torch.int32))
    with pytest.raises(ValueError, match="needs a mask"):
        mem.topk_mix(t, [1.0] * 3, 3, mask_index=[0, 0])
    with pytest.raises(ValueError, match="NaN"):
        mem.topk_mix(t, [1.0] * 3, 3, min_score=float("nan"))
    with pytest.raises(ValueError, match="J"):
        mem.prepare_topk_mix(1, 17, 3)
    sized = host_memory(capacity=16, library=SizingLibrary())
    first = sized.prepare_topk_mix(4, 5, 10)                        # the stand-in sizes any vm_*_workspace_bytes entry
    assert isinstance(first, M.MixTopkScratch) and first.fits(sized, 4, 10)
    assert first.ws.numel() == 1000 + 64 * 14 and first.flags.dtype == torch.int32
    assert sized.prepare_topk_mix(2, 16, 5) is first                # J does not size the workspace
    assert sized.prepare_topk_mix(64, 3, 32) is not first
    assert mem.last_mix_flags is None and mem.mix_uncertified_count == 0


def test_header_and_library():
    from vidmem import _lib
    text = open(os.path.join(ROOT, "include", "vidmem.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("W(c, r) = sum_j w[c][j] * e_j(r)",
                   "left to right, one rounding per product and one per addition, never fused",
                   "appended terms of weight 0.0 change no bit",
                   "W > min_score",
                   "A (2 (D + 8) 2^-24 + 2^-21), A = sum_j |w_j|",
                   "every nonzero |w_j| lies in [2^-20, 2^20]",
                   "not on the other queries of the call"):
        assert phrase in flat, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for decl in (r"size_t vm_topk_mix_workspace_bytes\(const vm_memory \*mem, int C, int k\);",
                 r"int vm_topk_cosine_mix\(vm_memory \*mem, const void \*terms, const double \*weights, int C, int J, int k,",
                 r"int vm_topk_cosine_mix_exact\(vm_memory \*mem, const void \*terms, const double \*weights, int C, int J, "
                 r"int k,"):
        assert re.search(decl, code), decl
    L = _lib.lib()
    assert L.vm_abi_version() == 4
    for sym in ("vm_topk_mix_workspace_bytes", "vm_topk_cosine_mix", "vm_topk_cosine_mix_exact"):
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    assert L.vm_topk_mix_workspace_bytes(None, 1, 1) == 0
    assert L.vm_topk_cosine_mix(None, None, None, 1, 1, 1, None, 0, None, 0, 0.0, 1, 0, None, None, None, None, None, 0,
                                None) == _lib.VM_ERR_INVALID
    assert L.vm_topk_cosine_mix_exact(None, None, None, 1, 1, 1, None, 0, None, 0, 0.0, 1, 0, None, None, None, 0,
                                      None) == _lib.VM_ERR_INVALID


# ---- the GPU scan test's precondition --------------------------------------------------------------------------------------
def test_scan_precondition_unmasked_holds_everywhere_and_masked_nearly_everywhere():
    """The GPU scan test demands flag 0 where rank k and rank M + 1 of the oracle's W are more than 4 x eps_mix apart (or
    fewer than M + 1 rows are selected).  Unmasked, that holds for every case; over all (shape, mask set, J, weights, c, k)
    cases at least 90 % keep the demand."""
    kept = total = 0
    smallest = (np.inf, None)
    for D, dtype in XR.DTS:
        for shape in MR.SHAPES:
            _, _, base, live = MR.host_dataset(D, dtype, shape)
            n = live.shape[1]
            sels = {C: XR.scan_selections(C, shape, base, n) for C in XR.CS}
            for J in XR.JS:
                for wname in XR.WEIGHT_SETS:
                    W, w = XR.scan_scores(D, dtype, shape, J, wname)
                    A = XR.abs_sum(w)
                    for C in XR.CS:
                        for name, sel in sels[C].items():
                            for c in range(C):
                                best = np.sort(W[c][sel[c]])[::-1]
                                for k in XR.KS:
                                    ok = XR.flag0_ok(best, k, D, A)
                                    total += 1
                                    kept += ok
                                    if name == "none":
                                        assert ok, (D, dtype, shape, J, wname, c, k, XR.margin(best, k, D, A))
                                        m = XR.margin(best, k, D, A)
                                        if m < smallest[0]:
                                            smallest = (m, (D, dtype, shape, J, wname, c, k))
    print(f"smallest unmasked margin {smallest[0]:.1f} x eps_mix at {smallest[1]}; {kept} of {total} cases keep flag 0")
    assert smallest[0] > 4
    assert kept >= 0.9 * total, (kept, total)
