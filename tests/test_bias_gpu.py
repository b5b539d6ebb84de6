"""GPU: the biased top-k (vm_topk_cosine_biased, csrc/topk_bias.hip) and its two builders against tests/bias_ref.py.

Bar: rows, fp64 score bits and padding identical to statement (A) of the oracle, for the fast and the ``exact=True``
entry.  The scan test runs the shapes at which the shared tile scan can go wrong (tests/tile_scan_data.py) for
every (Q, bias set, weight, mask set, k) of tests/bias_ref.py and demands flag 0 wherever the oracle's scores allow it: the
redo would hide a broken scan.  That they allow it is asserted from the oracle's scores before any search, and proven
without a GPU in tests/test_bias_cpu.py.
"""
import numpy as np
import pytest
import torch

from tests import bias_ref as BR
from tests import mask_ref as MR
from tests.support import (bits, check_entries, clustered, dev_bias, dev_mask, plain_memory, queries_near, redone, same_result,
                           scan_memory)
from tests.tile_scan_data import dataset

pytestmark = pytest.mark.gpu


def want_of(mem, q, cols, bindex, betas, k, dtype, masks=None, index=None, **kw):
    """Statement (A) for the memory as it is: q on the device, cols / bindex / betas / masks / index host values."""
    base, host_rows = mem.rows_host()
    Q = q.shape[0]
    sel = None if masks is None else MR.selection(masks, index, Q, base, host_rows.shape[0], mem.capacity)
    return BR.bias_topk(bits(q), host_rows, cols, bindex, betas, sel, k, dtype=dtype, base=base, capacity=mem.capacity,
                        **kw)


def check(mem, q, cols, bindex, betas, k, dtype, masks=None, index=None, certified=None, label="", want=None,
          dcols=None, dmask=None, **kw):
    """Fast and exact entry against (A) (``want``: (A) computed by the caller).  certified: None, or bool per query - the
    fast path must have answered those queries itself (flag 0)."""
    want = want or want_of(mem, q, cols, bindex, betas, k, dtype, masks, index, **kw)
    b = dcols if dcols is not None else dev_bias(cols)
    m = dmask if dmask is not None else (None if masks is None else dev_mask(masks))

    def call(exact):
        s, r = mem.topk_biased(q, k, b, weight=betas, bias_index=bindex, mask=m, mask_index=index, exact=exact, **kw)
        return r, s
    return check_entries(call, lambda: mem.last_bias_flags[:q.shape[0]], want, certified, label)


# ---- 1. the scan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MR.SHAPES))
@pytest.mark.parametrize("D,dtype", BR.DTS)
def test_scan(D, dtype, shape):
    mem, q_all, base, live, total, cap = scan_memory(D, dtype, shape)
    assert mem.bias_stride == BR.bias_stride(mem.capacity)
    n = live.shape[1]
    cols = BR.set_columns(base, n, mem.capacity)            # NaN in the slots without a live row: ignored
    dcols = dev_bias(cols)
    S = BR.scan_scores(D, dtype, shape)                     # (A), from the shared matrix
    demanded = cases = 0
    for Q in BR.QS:
        q = q_all[:Q].contiguous()
        bindex = [BR.query_case(i)[0] for i in range(Q)]
        betas = [BR.query_case(i)[1] for i in range(Q)]
        exact_S = np.stack([S[bindex[i], betas[i]][i] for i in range(Q)])
        sels = BR.scan_selections(Q, shape, base, n)
        sets = {"none": (None, None, None)}
        sets.update({name: (masks, index, dev_mask(masks)) for name, (masks, index) in MR.mask_sets(Q, shape).items()})
        for name, (masks, index, dmask) in sets.items():
            sel = sels[name]
            for k in BR.KS:
                # the condition of the flag-0 demand, from oracle scores, before any search
                ok = [BR.flag0_ok(np.sort(exact_S[i][sel[i]])[::-1], k, D) for i in range(Q)]
                if name == "none":
                    assert all(ok), f"precondition: {shape} D={D} {dtype} Q={Q} k={k}"
                want = MR.masked_topk_from_scores(exact_S, sel, k, base=base)
                got_r, got_s, _ = check(mem, q, cols, bindex, betas, k, dtype, masks, index, certified=ok, want=want,
                                        dcols=dcols, dmask=dmask, label=f"{shape} Q={Q} {name} k={k}")
                demanded += sum(ok)
                cases += Q
                if name in ("empty", "first_dead"):
                    assert (got_r == -1).all() and (got_s == 0.0).all()
                if name == "newest":
                    assert (got_r[:, 0] == total - 1).all() and (got_r[:, 1:] == -1).all()
        # a NULL index: one column for every query, and one column per query
        for k in BR.KS:
            check(mem, q, cols[1:2], None, betas, k, dtype, label=f"{shape} Q={Q} n_bias=1 k={k}")
            check(mem, q, cols[bindex], None, betas, k, dtype, want=MR.masked_topk_from_scores(exact_S, sels["none"], k, base=base),
                  certified=[True] * Q, label=f"{shape} Q={Q} n_bias=Q k={k}")
        check(mem, q, cols[3:4], None, None, 5, dtype, label=f"{shape} Q={Q} no weights")       # NULL weights: 1.0
    assert demanded >= 0.9 * cases
    mem.close()


# ---- 2. identities on the device --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_identities(dtype):
    rows, _ = clustered([5] * 200, 384, dtype, seed=21)
    mem = plain_memory(rows, dtype)
    q = queries_near(rows, 16, 9, dtype)
    mask = dev_mask(MR.pack_rows(range(100, 900, 3), mem.capacity)[None])
    g = torch.Generator(device="cuda").manual_seed(2)
    noise = torch.randn((1, mem.bias_stride), device="cuda", generator=g)
    zero = mem.new_bias()
    for k in (1, 10, 64):
        for exact in (False, True):
            plain, masked = mem.topk(q, k), mem.topk_masked(q, k, mask)
            # beta = 0 whatever the column holds, and a column of zeros whatever the weight: the reference cosine
            assert same_result(mem.topk_biased(q, k, noise, weight=0.0, exact=exact), plain), (k, exact)
            assert same_result(mem.topk_biased(q, k, zero, weight=-0.5, exact=exact), plain), (k, exact)
            assert same_result(mem.topk_biased(q, k, noise, bias_index=[-1] * 16, exact=exact), plain), (k, exact)
            assert same_result(mem.topk_biased(q, k, noise, weight=0.0, mask=mask, exact=exact), masked), (k, exact)
            assert same_result(mem.topk_biased(q, k, zero, mask=mask, exact=exact), masked), (k, exact)
    # a query's result is the same alone and inside a batch
    cols = torch.cat([noise, 0.1 * noise.flip(1), zero])
    betas = [(1.0, -0.5, 0.3)[i % 3] for i in range(16)]
    bindex = [i % 3 for i in range(16)]
    masks = torch.cat([mask, ~mask])
    mindex = [i % 2 for i in range(16)]
    for exact in (False, True):
        s16, r16 = mem.topk_biased(q, 10, cols, weight=betas, bias_index=bindex, mask=masks, mask_index=mindex, exact=exact)
        for i in (0, 1, 5, 15):
            one = mem.topk_biased(q[i:i + 1], 10, cols[bindex[i]], weight=betas[i], mask=masks[mindex[i]], exact=exact)
            assert same_result(one, (s16[i:i + 1], r16[i:i + 1])), (i, exact)
    check(mem, q, cols.cpu().numpy(), bindex, betas, 10, dtype, masks.cpu().numpy().view(np.uint32), mindex, label="batch")
    mem.close()


# ---- 3. what must go to the redo and still be exact -------------------------------------------------------------------
def _redone(mem, q, cols, bindex, betas, k, dtype, label, flag=None, **kw):
    return redone(lambda: check(mem, q, cols, bindex, betas, k, dtype, label=label, **kw), lambda: mem.bias_uncertified_count,
                  q.shape[0], label, flag)


def test_redo_cases():
    from vidmem import _lib
    rows, _ = clustered([5] * 8, 128, "f16", seed=31)
    q = queries_near(rows, 2, 4, "f16")
    # a static scene: 40 identical rows with equal bias - every S is the same, the first k rows by id come back
    still = rows[7:8].expand(40, -1).contiguous()
    mem = plain_memory(still, "f16")
    S = mem.bias_stride
    got_r, got_s = _redone(mem, q, np.full((1, S), 0.25, np.float32), None, [1.0, -0.5], 5, "f16", "static scene",
                           flag=_lib.VM_FLAG_GAP)
    assert got_r.tolist() == [[0, 1, 2, 3, 4]] * 2 and (got_s[:, :1] == got_s).all()
    mem.close()
    mem = plain_memory(rows, "f16")
    age = np.zeros((1, S), np.float32)
    age[0, :40] = -np.arange(40)[::-1] / 64.0
    # a weight outside the bound's domain
    got_r, _ = _redone(mem, q, age, None, [2.0 ** 30, -2.0 ** 30], 5, "f16", "weight 2^30", flag=_lib.VM_FLAG_GAP)
    assert got_r[0].tolist() == [39, 38, 37, 36, 35] and got_r[1].tolist() == [0, 1, 2, 3, 4]
    _redone(mem, q, age, None, [2.0 ** -30, -2.0 ** -30], 5, "f16", "weight 2^-30", flag=_lib.VM_FLAG_GAP)
    # |b| = 2^50 on a selected row: the scan itself finds it ...
    wide = age.copy()
    wide[0, 11] = 2.0 ** 50
    got_r, _ = _redone(mem, q, wide, None, [1.0, -1.0], 5, "f16", "bias 2^50", flag=_lib.VM_FLAG_GAP)
    assert got_r[0, 0] == 11 and 11 not in got_r[1]
    wide[0, 11] = -2.0 ** 50
    _redone(mem, q, wide, None, [0.3, 0.3], 5, "f16", "bias -2^50", flag=_lib.VM_FLAG_GAP)
    # ... in the queries that use the column and select the row only
    # (flag 0 is demanded where the oracle's own scores leave the margin for it: rank 5 against rank M + 1 = 14)
    only = MR.pack_rows([r for r in range(40) if r != 11], 40)[None]

    def clear(cols, bindex, masks=None):
        s14 = want_of(mem, q, cols, bindex, [1.0, 1.0], 14, "f16", masks)[1]
        return [BR.flag0_ok(s14[i], 5, 128) for i in range(2)]
    both = np.concatenate([wide, age])
    assert clear(both, [1, 0])[0] and all(clear(wide, None, only))
    _, _, flags = check(mem, q, both, [1, 0], [1.0, 1.0], 5, "f16", label="one query of two")
    assert flags[0] == 0 and flags[1] == _lib.VM_FLAG_GAP
    _, _, flags = check(mem, q, wide, None, [1.0, 1.0], 5, "f16", masks=only, label="the wide row masked out")
    assert (flags == 0).all()
    mem.close()
    # a bf16 query whose norm is outside [2^-40, 2^40]
    rows, _ = clustered([5] * 8, 128, "bf16", seed=32)
    mem = plain_memory(rows, "bf16")
    qb = queries_near(rows, 2, 4, "bf16")
    tiny = (qb.float() * 2.0 ** -50).to(torch.bfloat16)
    assert float(tiny.double().norm(dim=1).max()) < 2.0 ** -40 and (tiny.float() != 0).any()
    _redone(mem, tiny, age, None, [1.0, 0.5], 5, "bf16", "tiny bf16 query", flag=_lib.VM_FLAG_GAP)
    mem.close()


def test_redo_when_more_rows_share_the_cut_than_the_buffer_holds():
    from vidmem import _lib
    rows, _ = clustered([5] * 2, 128, "f16", seed=33)
    n = 8192 + 300
    still = rows[3:4].expand(n, -1).contiguous()
    mem = plain_memory(still, "f16")
    q = queries_near(rows, 1, 4, "f16")
    cols = np.full((1, mem.bias_stride), -0.375, np.float32)
    got_r, got_s = _redone(mem, q, cols, None, [1.0], 5, "f16", "8,492 equal rows", flag=_lib.VM_FLAG_OVERFLOW)
    assert got_r.tolist() == [[0, 1, 2, 3, 4]]
    # twenty graded boosts lift the best M + 1 = 14 keys clear of the crowd: the cut is above it and, every cosine being
    # the same, rank 5 and rank 14 are 9/16 apart - certified again
    pos = [100 + 419 * i for i in range(20)]
    cols[0, pos] = 0.5 + np.arange(20, dtype=np.float32) / 16
    got_r, _, flags = check(mem, q, cols, None, [1.0], 5, "f16", label="twenty boosted rows")
    assert got_r.tolist() == [pos[:14:-1]] and flags[0] == 0
    mem.close()


# ---- 4. the builders --------------------------------------------------------------------------------------------------
def _bits32(t):
    return t.detach().cpu().numpy().view(np.int32)


def test_bias_of_rows_bit_for_bit():
    D, dtype = 128, "f16"
    rows, q_all, base, _ = dataset(D, dtype, "ring40")
    mem = plain_memory(rows, dtype, capacity=40, ring=True, step=19)           # live rows 17 .. 56
    n, cap = 40, 40
    ids = [-1, 17, 56, 57, 16, 30, 30, -5, 10 ** 12, 41, 0]                     # -1, dead on both sides, a duplicate
    vals = [9.0, 1.5, -2.25, 3.0, 4.0, 0.125, 0.125, 5.0, 6.0, 2.0 ** -130, 7.0]
    want = BR.bias_from_rows_ref(ids, vals, base, n, cap)
    got = mem.bias_of_rows(ids, vals)
    assert got.shape == (mem.bias_stride,) and np.array_equal(_bits32(got), want.view(np.int32))
    assert np.count_nonzero(want) == 4
    # a device tensor as a search wrote it, -1 padding included; one value for all; clear=False keeps the other entries
    _, found = mem.topk_masked(q_all[:3], 5, dev_mask(MR.pack_rows([20, 21, 50], cap)[None]))
    assert (found == -1).any()
    start = torch.arange(mem.bias_stride, dtype=torch.float32, device="cuda") * -0.5
    want2 = BR.bias_from_rows_ref(found.cpu().numpy().ravel(), [0.75] * found.numel(), base, n, cap, start=start.cpu().numpy())
    out = start.clone()
    assert mem.bias_of_rows(found, 0.75, out=out, clear=False) is out
    assert np.array_equal(_bits32(out), want2.view(np.int32)) and (out[[20, 21, 10]] == 0.75).all() and out[5] == -2.5
    out2 = mem.bias_of_rows(found, torch.full((found.numel(),), 0.75, device="cuda"), out=out)     # clear=True
    assert out2 is out and np.array_equal(_bits32(out), BR.bias_from_rows_ref(found.cpu().numpy().ravel(), [0.75] * 15,
                                                                             base, n, cap).view(np.int32))
    assert mem.bias_of_rows([], []).abs().sum() == 0
    # the C entry: ids of the form row * 3 + 1 only
    gids = torch.tensor([17 * 3 + 1, 18 * 3 + 2, 19 * 3, 56 * 3 + 1, 57 * 3 + 1, -1], dtype=torch.int64, device="cuda")
    gv = torch.arange(1, 7, dtype=torch.float32, device="cuda")
    col = mem.new_bias()[0]
    from vidmem import _lib
    assert mem.L.vm_bias_from_rows(mem.handle, gids.data_ptr(), gv.data_ptr(), 6, 3, 1, 1, col.data_ptr(),
                                   _lib.current_stream_ptr()) == _lib.VM_OK
    want3 = BR.bias_from_rows_ref(gids.cpu().numpy(), gv.cpu().numpy(), base, n, cap, stride=(3, 1))
    assert np.array_equal(_bits32(col), want3.view(np.int32)) and np.count_nonzero(want3) == 2
    for bad in (dict(out=col.data_ptr() + 4), dict(out=None), dict(n=-1), dict(stride=0)):
        rc = mem.L.vm_bias_from_rows(mem.handle, gids.data_ptr(), gv.data_ptr(), bad.get("n", 6), bad.get("stride", 3), 1, 1,
                                     bad.get("out", col.data_ptr()), _lib.current_stream_ptr())
        assert rc == _lib.VM_ERR_INVALID and "vm_bias_from_rows" in mem.L.vm_last_error(mem.ctx.handle).decode()
    torch.cuda.synchronize()
    mem.close()


def test_bias_of_age_bit_for_bit():
    from vidmem import _lib
    from vidmem.memory import EmbeddingMemory, make_tag
    D, dtype = 128, "f16"
    rows, _, _, _ = dataset(D, dtype, "ring40")                                # 57 rows
    for cap, ring in ((40, True), (100, False)):
        mem = EmbeddingMemory(cap, D, dtype, ring=ring, tagged=True)
        mem.append(rows[:20], tag=[make_tag(3, 1000 * i + 7) for i in range(20)])
        mem.append(rows[20:31])                                                # untagged
        mem.append(rows[31:57], tag=[make_tag(5, (1 << 40) - 1 - 333 * i) for i in range(26)])
        base = mem.rows_host()[0]
        tags = mem.tags_host()
        assert (tags == BR.INT64_MIN).sum() == (11 if not ring else 11 - max(0, base - 20))
        for now, per_ms, fill in ((60_000, 1e-6, 0.0), (0, -0.3, -7.5), ((1 << 40) - 1, 1e-6, 2.0 ** -140),
                                  (12_345, 1.0 / 3, 1.0)):
            want = BR.bias_from_tags_ref(tags, base, cap, now, per_ms, fill)
            got = mem.bias_of_age(now, per_ms, fill)
            assert np.array_equal(_bits32(got), want.view(np.int32)), (cap, now, per_ms, fill)
            out = torch.full((1, mem.bias_stride), 99.0, device="cuda")
            assert mem.bias_of_age(now, per_ms, fill, out=out) is out          # writes all S entries
            assert np.array_equal(_bits32(out[0]), want.view(np.int32))
        mem.close()
    plain = EmbeddingMemory(16, D, dtype)
    col = plain.new_bias()
    assert plain.L.vm_bias_from_tags(plain.handle, 0, 1e-6, 0.0, col.data_ptr(), _lib.current_stream_ptr()) == _lib.VM_ERR_INVALID
    assert "not tagged" in plain.L.vm_last_error(plain.ctx.handle).decode()
    plain.close()


# ---- 5. ring and lifecycle ----------------------------------------------------------------------------------------------
def test_ring_after_appends_and_a_linear_memory_after_an_erase():
    D, dtype = 128, "f16"
    rows, q_all, base, _ = dataset(D, dtype, "ring40")
    more, _ = clustered([4] * 6, D, dtype, seed=41)
    mem = plain_memory(rows, dtype, capacity=40, ring=True, step=19)
    q = q_all[:17].contiguous()
    bindex = [BR.query_case(i)[0] for i in range(17)]
    betas = [BR.query_case(i)[1] for i in range(17)]
    check(mem, q, BR.set_columns(base, 40, 40), bindex, betas, 5, dtype, label="ring")
    mem.append(more[:13])                                           # overwrites 13 more rows: the seam moves
    assert mem.rows_host()[0] == base + 13
    cols = BR.set_columns(base + 13, 40, 40)
    got_r, _, _ = check(mem, q, cols, bindex, betas, 5, dtype, label="ring after appends")
    assert (got_r >= base + 13).all()
    check(mem, q, cols, bindex, betas, 5, dtype, MR.pack_rows(range(base + 13, base + 53, 2), 40)[None], label="ring, masked")
    mem.close()
    # a linear memory after an erase, the column rebuilt on the device from a previous search
    rows, _ = clustered([5] * 12, D, dtype, seed=42)
    mem = plain_memory(rows, dtype, capacity=64)
    q = queries_near(rows, 3, 6, dtype)
    check(mem, q, BR.set_columns(0, 60, 64), [1, 3, 4], [1.0, 0.3, -0.5], 5, dtype, label="before erase")
    mem.erase(rows=[0, 7, 8, 9, 30, 59])
    assert len(mem) == 54
    check(mem, q, BR.set_columns(0, 54, 64), [1, 3, 4], [1.0, 0.3, -0.5], 5, dtype, label="after erase")
    s1, r1 = mem.topk(q, 5)                                         # the hits of round one, boosted in round two
    boost = mem.bias_of_rows(r1, s1.float().reshape(-1))            # not read on the host
    want_col = BR.bias_from_rows_ref(r1.cpu().numpy().ravel(), s1.float().cpu().numpy().ravel(), 0, 54, 64)
    # (a row found by two queries carries two different values: the column is compared where it is unambiguous)
    flat = r1.cpu().numpy().ravel()
    once = [r for r in set(flat.tolist()) if (flat == r).sum() == 1]
    assert np.array_equal(_bits32(boost)[once], want_col.view(np.int32)[once])
    host_col = boost.cpu().numpy()[None]
    got_r, _, _ = check(mem, q, host_col, None, [-2.0, -2.0, -2.0], 5, dtype, label="earlier hits pushed down")
    assert not set(got_r[0].tolist()) & set(r1[0].tolist())
    mem.close()


# ---- 6. arguments -------------------------------------------------------------------------------------------------------
def test_arguments():
    from vidmem import _lib
    rows, _ = clustered([5] * 60, 384, "bf16", seed=51)
    mem = plain_memory(rows, "bf16", grouped=True)                  # any memory: here a grouped one
    S = mem.bias_stride
    q = queries_near(rows, 3, 5, "bf16")
    rng = np.random.default_rng(1)
    cols = (rng.standard_normal((2, S)) * 0.25).astype(np.float32)
    betas = [1.0, -0.5, 0.3]
    masks = np.stack([MR.pack_rows(np.nonzero(rng.random(300) < p)[0], 300) for p in (0.5, 0.1, 0.03)])
    for cut in (0.3, 0.0, -0.2, None):                              # a strict filter on the raw sum, negative included
        got_r, got_s, _ = check(mem, q, cols, [0, 1, 0], betas, 64, "bf16", masks, [2, 0, 1], min_score=cut,
                                label=f"min_score {cut}")
        if cut is not None:
            assert (got_s[got_r >= 0] > cut).all() and (got_r == -1).any()
        if cut is not None and cut < 0:
            assert (got_s[got_r >= 0] < 0).any()                    # scores below zero pass a negative threshold
    check(mem, q, cols, [0, 1, 0], betas, 64, "bf16", min_score=-0.2, label="negative threshold, unmasked")
    got_r, _, _ = check(mem, q, cols, [0, 1, 0], betas, 5, "bf16", masks, [0, 3, -1], label="mask index out of range")
    assert (got_r[1:] == -1).all() and (got_r[0] >= 0).all()
    check(mem, q, cols, [2, -1, 1], betas, 5, "bf16", label="bias index out of range")
    plain = check(mem, q, cols, [0, 1, 0], betas, 7, "bf16", label="stride 1")
    wr, wscore = want_of(mem, q, cols, [0, 1, 0], betas, 7, "bf16")
    dcols = dev_bias(cols)
    for exact in (False, True):
        s, r = mem.topk_biased(q, 7, dcols, weight=betas, bias_index=[0, 1, 0], stride=(3, 1), exact=exact)
        assert np.array_equal(r.cpu().numpy(), wr * 3 + 1) and np.array_equal(s.cpu().numpy().view(np.int64), wscore.view(np.int64))
    assert np.array_equal(plain[0], wr)
    # device tensors of the final dtype are passed through untouched
    w_dev = torch.tensor(betas, dtype=torch.float64, device="cuda")
    i_dev = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    assert mem._biases(dcols).data_ptr() == dcols.data_ptr() and mem._bias_weight(w_dev, 3) is w_dev
    assert mem._bias_index(i_dev, 2, 3) is i_dev and mem._as_rows(q).data_ptr() == q.data_ptr()
    with pytest.raises(ValueError, match="is on"):
        mem.topk_biased(q, 5, torch.zeros(S))
    # the C entry point refuses, with a text
    sc = mem.prepare_topk_biased(3, 5)
    need = mem.L.vm_topk_bias_workspace_bytes(mem.handle, 3, 5)
    assert sc.ws.numel() >= need > mem.L.vm_topk_masked_workspace_bytes(mem.handle, 3, 5) > 4 * 3 * 300
    assert mem.L.vm_memory_bias_stride(mem.handle) == S == 32 * mem.L.vm_memory_mask_words(mem.handle)
    out_s = torch.full((3, 64), 7.0, dtype=torch.float64, device="cuda")
    out_r = torch.full((3, 64), 7, dtype=torch.int64, device="cuda")
    m = dev_mask(masks)

    def call(Q=3, k=5, qp=q.data_ptr(), bias=dcols.data_ptr(), n_bias=1, bidx=None, w=w_dev.data_ptr(), outs=(out_s, out_r),
             ws_ptr=sc.ws.data_ptr(), ws_bytes=None, mask_ptr=None, n_masks=0, stride=1, exact=False):
        head = (mem.handle, qp, Q, k, bias, n_bias, bidx, w, mask_ptr, n_masks, None, 0, 0.0, stride, 0,
                outs[0].data_ptr() if outs[0] is not None else None, outs[1].data_ptr() if outs[1] is not None else None)
        tail = (ws_ptr, sc.ws.numel() if ws_bytes is None else ws_bytes, _lib.current_stream_ptr())
        if exact:
            return mem.L.vm_topk_cosine_biased_exact(*head, *tail)
        return mem.L.vm_topk_cosine_biased(*head, None, None, *tail)

    for exact in (False, True):
        out_s.fill_(7.0)
        out_r.fill_(7)
        for kw, text in ((dict(k=0), "k=0"), (dict(k=65), "k=65"), (dict(Q=0), "Q=0"),
                         (dict(qp=None), "null queries or bias"), (dict(bias=None), "null queries or bias"),
                         (dict(outs=(None, out_r)), "null outputs"), (dict(outs=(out_s, None)), "null outputs"),
                         (dict(stride=0), "row_stride=0"),
                         (dict(bias=dcols.data_ptr() + 4), "bias must be 16-byte aligned"),
                         (dict(n_bias=2), "need a bias_index"), (dict(n_bias=0), "need a bias_index"),
                         (dict(ws_bytes=need - 1), "workspace"), (dict(ws_ptr=None), "workspace"),
                         (dict(ws_ptr=sc.ws.data_ptr() + 16), "aligned"), (dict(qp=q.data_ptr() + 2), "aligned"),
                         (dict(w=w_dev.data_ptr() + 4), "aligned"),
                         (dict(mask_ptr=m.data_ptr() + 2, n_masks=3), "aligned"),
                         (dict(mask_ptr=m.data_ptr(), n_masks=2), "mask_index"),
                         (dict(mask_ptr=m.data_ptr(), n_masks=0), "mask_index")):
            assert call(exact=exact, **kw) == _lib.VM_ERR_INVALID, (kw, exact)
            assert text in mem.L.vm_last_error(mem.ctx.handle).decode(), (kw, mem.L.vm_last_error(mem.ctx.handle))
        assert call(exact=exact, n_bias=(1 << 30) // S + 1, bidx=i_dev.data_ptr()) == _lib.VM_ERR_UNSUPPORTED
        assert "2^30 bias values" in mem.L.vm_last_error(mem.ctx.handle).decode()
        torch.cuda.synchronize()
        assert (out_s == 7.0).all() and (out_r == 7).all()          # refused before any launch
        assert call(exact=exact, n_bias=2, bidx=i_dev.data_ptr()) == _lib.VM_OK
    torch.cuda.synchronize()
    want_r, want_s = want_of(mem, q, cols, [0, 1, 0], betas, 5, "bf16")
    assert np.array_equal(out_r.reshape(-1)[:15].cpu().numpy().reshape(3, 5), want_r)      # [3, k] as the library wrote it
    mem.close()


def test_an_empty_memory():
    from vidmem.memory import EmbeddingMemory
    mem = EmbeddingMemory(64, 128, "f16", tagged=True)
    q = torch.randn(2, 128, device="cuda", generator=torch.Generator("cuda").manual_seed(3)).to(torch.float16)
    col = mem.bias_of_age(1000, 1e-6, fill=3.0)
    assert (col == 3.0).all()
    for exact in (False, True):
        for mask in (None, ~mem.new_mask()):
            s, r = mem.topk_biased(q, 4, col, weight=[1.0, 2.0 ** 30], mask=mask, exact=exact)
            assert (r == -1).all() and (s == 0.0).all()
    assert (mem.last_bias_flags[:2] == 0).all() and mem.bias_uncertified_count == 0
    mem.close()


# ---- 7. capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_replayed_after_an_append_and_rewritten_operands():
    from vidmem.memory import BiasTopkScratch, EmbeddingMemory
    rows, _ = clustered([4] * 128, 384, "f16", seed=61)
    mem = EmbeddingMemory(1024, 384, "f16")
    mem.append(rows[:256])
    Q, k = 3, 10
    mem.prepare_topk_biased(Q, k)                     # the memory's counter exists before the capture
    scratch = BiasTopkScratch.for_(mem, Q, k)         # and the capture runs on a scratch the caller owns
    q = queries_near(rows, Q, 6, "f16").contiguous()
    bias = mem.new_bias(2)
    weights = torch.ones(Q, dtype=torch.float64, device="cuda")
    bindex = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    mask = mem.new_mask(2)
    mindex = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):       # one linear graph, at the default queue setting
            out_s, out_r = mem.topk_biased(q, k, bias, weight=weights, bias_index=bindex, mask=mask, mask_index=mindex,
                                           scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    assert mem._own[BiasTopkScratch] is not scratch and mem._last[BiasTopkScratch] is scratch
    rng = np.random.default_rng(9)

    def replay_and_check(cols, ws, bi, words, mi, label):
        bias.copy_(dev_bias(cols))                    # all rewritten in place
        weights.copy_(torch.tensor(ws, dtype=torch.float64))
        bindex.copy_(torch.tensor(bi, dtype=torch.int32))
        mask.copy_(dev_mask(words))
        mindex.copy_(torch.tensor(mi, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want_r, want_s = want_of(mem, q, cols, bi, ws, k, "f16", words, mi)
        assert np.array_equal(out_r.cpu().numpy(), want_r), label
        assert np.array_equal(out_s.cpu().numpy().view(np.int64), want_s.view(np.int64)), label
        return want_r

    S = mem.bias_stride
    cols = (rng.standard_normal((2, S)) * 0.5).astype(np.float32)
    r = replay_and_check(cols, [1.0, 0.5, -0.25], [0, 1, 0],
                         np.stack([MR.pack_rows(range(0, 128), 1024), MR.pack_rows(range(100, 256), 1024)]), [0, 1, 0], "first")
    assert (r[0] < 128).all() and (r[1] >= 100).all()
    cols2 = np.zeros((2, S), np.float32)
    cols2[1, 7] = 5.0
    r = replay_and_check(cols2, [0.3, 1.0, 1.0], [1, 1, 5],
                         np.stack([MR.pack_rows(range(200, 400), 1024), MR.pack_rows(range(0, 256), 1024)]), [1, 1, 0], "rewritten")
    assert r[0, 0] == 7 and r[1, 0] == 7 and ((r[2] >= 200) & (r[2] < 256)).all()   # rows 256 .. 399 are not live yet
    mem.append(rows[256:512])
    q.copy_(rows[300:303])
    cols3 = cols.copy()
    cols3[0, 256:512] += 0.125
    r = replay_and_check(cols3, [1.0, 0.5, -0.25], [0, 1, 0],
                         np.stack([MR.pack_rows(range(200, 400), 1024), MR.pack_rows(range(0, 512, 2), 1024)]), [0, 1, 0], "appended")
    assert (r[0] >= 256).any() and (r[1] % 2 == 0).all()                              # the rows appended since
    mem.close()
