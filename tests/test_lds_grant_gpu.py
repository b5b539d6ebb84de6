"""GPU: the host launch code.  1. The dynamic-LDS grant of a context (csrc/vm_common.h vm_lds_opt_in): one kernel
instantiation driven through growing sizes in one process.  2. The create functions of the two towers on bad weight
lists (csrc/encoder.hip WeightBlob).

1. Every search launches one kernel instantiation per (dtype, operation) whatever the memory's D, and sizes its dynamic
   LDS from D at run time.  A memory of D = 128 is searched, then one of the smallest D at which the site's dynamic LDS
   passes the 64 KiB a launch gets without hipFuncAttributeMaxDynamicSharedMemorySize, then the first again:

     site (kernel)                                   dynamic LDS            D = 128    the large memory
     tile scan, Q <= 16 (topk_masked, mix, diverse)  16 rows x D x 2        4,096      D = 2,176: 69,632
     mixed / any-all finalize, redo scan, fold terms J x D x 2, J = 16      4,096      D = 2,176: 69,632 (J = 15: 65,280)
     diverse pair kernel                             16 rows x D x 2        4,096      D = 2,176: 69,632
     plain list scan (k = 5: KL = 8, one tile)       16 x D x 2             8,192 (*)  D = 2,176: 69,632; 3,712: 118,784
     bf16 finalize with the KL = 8 rows staged       D x 2 + 8 (D + 8) x 2  2,432      D = 2,176: 39,296; 3,712: 66,944
     group sums (summaries)                          (D + 1) x 16           2,064      D = 4,096: 65,552
     (*) the lanes' merge lists, 8 waves x 16 x 8 x 8, where they exceed the query tile
   The event links and the summaries' key scores stream rows through two buffers of a fixed size: their size does not
   grow, they run at the same three memories.  D = 2,176 and 3,712 lie above the 2,048 for which the certificate's bound is stated
   (include/vidmem.h): a query may go to the exhaustive redo there, the answer is the oracle's all the same, and nothing
   here demands a flag.

   The memory: 333 rows in a ring of 200 slots (the live rows wrap, the last tile is ragged), Q = 3, k = 5.  Bar: rows,
   fp64 score bits and padding equal to the oracle for the fast and the ``exact=True`` entry (tests/support.py
   check_entries, the searches' own checkers).  The tests hold before and after the grant table: a library that sets
   the attribute on every call passes them too.

2. A wrong ``n_weights`` and a null layer weight, for both towers, on a spec of hidden 256 and 2 layers: the code and
   the message, then a correct create and encode in the same process against its reference.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import cref
from oracle import vit_ref as V
from tests import diverse_ref as DR
from tests import events_ref as E
from tests import fold_ref as FR
from tests import mask_ref as MR
from tests import summary_ref as S
from tests import text_ref as TR
from tests import topk_plan as TP
from tests.search_checks import fold_check, mix_check
from tests.support import TD, bits, check_entries, dev_mask, from_bits, grouped_memory, plain_memory, same_bits

pytestmark = pytest.mark.gpu

CAP, TOTAL, Q, K, J = 200, 333, 3, 5, 16
BASE = TOTAL - CAP                                       # live rows 133 .. 332; row 200 lies in slot 0
SMALL, BIG = 128, 2176
GRADES = (0.9, 0.8, 0.7, 0.6, 0.5, 0.4)                  # cosine of a planted row with its query's centre
PLANTED = ((133, 199, 200, 260, 332, 140), (134, 201, 299, 331, 150, 175), (135, 198, 202, 270, 330, 160))
MIX_W = (1.0, -0.5, 0.25)                                # cycled over the J terms
FOLD_W = (1.0, 1.25, 1.5, 1.75)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def case(D, dtype):
    """Host data, made once per (D, dtype): random unit rows with six live rows per query planted at graded cosines with
    the query (the seam of the ring included), so the five best are far apart and far above the rest; J terms scattered
    around each query for the mixed and the any/all search; one mask per query.  -> (rows, queries, terms, masks)."""
    rng = np.random.default_rng(1000 + D)
    centre = _unit(rng.standard_normal((Q, D)))
    rows = _unit(rng.standard_normal((TOTAL, D)))
    for c in range(Q):
        for g, r in zip(GRADES, PLANTED[c]):
            rows[r] = g * centre[c] + np.sqrt(1.0 - g * g) * rows[r]
    terms = centre[:, None, :] + 0.5 * _unit(rng.standard_normal((Q, J, D)))
    live = np.arange(BASE, TOTAL)
    masks = np.stack([MR.pack_rows(sorted(set(live[live % 3 != c]) | set(PLANTED[c][:3])), CAP) for c in range(Q)])
    to = lambda x: torch.from_numpy(x.astype(np.float32)).to(TD[dtype]).contiguous()
    return to(rows), to(centre), to(terms), masks


def memory_of(D, dtype):
    rows = case(D, dtype)[0]
    mem = plain_memory(rows.cuda(), dtype, capacity=CAP, ring=True, step=19)
    assert mem.rows_host()[0] == BASE and np.array_equal(mem.rows_host()[1], bits(rows[BASE:]))
    return mem


def small_large_small(dtype, search, sizes=(SMALL, BIG)):
    """search(mem, D, label) on a memory of sizes[0], then on one of each larger size, then on the first again."""
    first = memory_of(sizes[0], dtype)
    search(first, sizes[0], f"{dtype} D={sizes[0]}")
    for D in sizes[1:]:
        mem = memory_of(D, dtype)
        search(mem, D, f"{dtype} D={D}")
        mem.close()
    search(first, sizes[0], f"{dtype} D={sizes[0]} again")
    first.close()


# ---- 1. one instantiation, growing sizes ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_tile_scan_through_topk_masked(dtype):
    def search(mem, D, label):
        _, q, _, masks = case(D, dtype)
        q, m = q.cuda(), dev_mask(masks)
        base, host_rows = mem.rows_host()
        want = MR.masked_topk(bits(q), host_rows, MR.selection(masks, None, Q, base, CAP, CAP), K, dtype=dtype, base=base)
        check_entries(lambda exact: mem.topk_masked(q, K, m, exact=exact)[::-1], lambda: mem.last_mask_flags[:Q], want,
                      label=label)
    assert 16 * SMALL * 2 <= 65536 < 16 * BIG * 2 and 16 * (BIG - 128) * 2 <= 65536
    small_large_small(dtype, search)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_mixed_and_any_all_finalize_and_redo(dtype):
    def search(mem, D, label):
        _, _, terms, masks = case(D, dtype)
        t = terms.cuda()
        for m in (None, masks):
            mix_check(mem, t, [MIX_W[j % 3] for j in range(J)], K, dtype, m, label=f"mix {label}")
            for op in FR.OPS:
                fold_check(mem, t, [FOLD_W[j % 4] for j in range(J)], K, op, dtype, m, label=f"fold {label}")
    assert J * SMALL * 2 <= 65536 < J * BIG * 2 and (J - 1) * BIG * 2 <= 65536
    small_large_small(dtype, search)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_diverse_pair_kernel(dtype):
    def search(mem, D, label):
        q = case(D, dtype)[1].cuda()
        base, host_rows = mem.rows_host()
        want = DR.diverse_topk(bits(q), host_rows, None, K, 16, 0.5, dtype=dtype, base=base)

        def call(exact):
            s, r = mem.topk_diverse(q, K, pool=16, lam=0.5, exact=exact)
            return r, s, mem.last_diverse_mmr
        check_entries(call, lambda: mem.last_diverse_flags[:Q], want, label=label)
    small_large_small(dtype, search)


FIN_D = 3712                        # where the bf16 finalize's dynamic LDS passes 64 KiB at k = 5


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_plain_scan_and_bf16_finalize(dtype):
    """Two steps up.  The sizes come from the plan the library picks (tests/topk_plan.py, the mirror of csrc/topk.hip): k = 5
    gives lists of KL = 8 and one query tile, so the scan asks for max(16 x D x 2, 8 waves x 16 x 8 x 8) bytes and the
    bf16 finalize, which stages its KL candidate rows beside the query row, for D x 2 + KL (D + 8) x 2.  The scan passes
    64 KiB at D = 2,176; the finalize only at D = 3,712 (66,944 bytes, still staged: at most 96 KiB), where the scan grows
    again (118,784)."""
    def search(mem, D, label):
        q = case(D, dtype)[1].cuda()
        r, s = cref.cosine_topk(bits(q), mem.rows_host()[1], K, dtype=dtype)
        check_entries(lambda exact: mem.topk(q, K, exact=exact)[::-1], lambda: mem.last_flags[:Q], (r + BASE, s),
                      label=label)
    plans = {D: TP.plan(Q, K, D, dtype, CAP) for D in (SMALL, BIG - 128, BIG, FIN_D - 128, FIN_D)}
    assert all(p.family == "list" and p.QT == 1 and p.KL == 8 for p in plans.values())
    scan = {D: max(p.QT * 16 * D * 2, 8 * p.QT * 16 * p.KL * 8) for D, p in plans.items()}
    fin = {D: D * 2 + p.KL * (D + 8) * 2 for D, p in plans.items()}
    assert scan[SMALL] == 8192 and scan[BIG - 128] <= 65536 < scan[BIG] < scan[FIN_D] == 118784
    assert fin[SMALL] < fin[BIG] <= fin[FIN_D - 128] <= 65536 < fin[FIN_D] == 66944
    assert dtype == "f16" or all(p.staged for p in plans.values())
    small_large_small(dtype, search, sizes=(SMALL, BIG, FIN_D))


@functools.lru_cache(maxsize=None)
def scenes(D, dtype):
    """333 rows in scenes of 1 .. 23 rows, one group key per scene -> (bits, sizes, keys per scene, links of all rows)."""
    rng = np.random.default_rng(77 + D)
    sizes = []
    while sum(sizes) < TOTAL:
        sizes.append(min(int(rng.integers(1, 24)), TOTAL - sum(sizes)))
    centres = _unit(rng.standard_normal((len(sizes), D)))
    rows = _unit(np.repeat(centres, sizes, axis=0) + 0.3 * _unit(rng.standard_normal((TOTAL, D))))
    b = bits(torch.from_numpy(rows.astype(np.float32)).to(TD[dtype]))
    return b, sizes, [1000 + i for i in range(len(sizes))], E.links(b, dtype)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_events_and_summaries(dtype):
    """A small D, a large one (the group sums' LDS passes 64 KiB at D = 4,096), the small one again on a second memory;
    the Python entries against tests/events_ref.py and tests/summary_ref.py, as their own tests hold them."""
    assert (4096 + 1) * 16 > 65536 >= (4096 - 128 + 1) * 16
    for D in (SMALL, 4096, SMALL):
        b, sizes, keys, link_all = scenes(D, dtype)
        mem = grouped_memory(from_bits(b, dtype), sizes, dtype, capacity=CAP, ring=True, keys=keys)
        mem.sync()
        assert mem.rows_host()[0] == BASE and np.array_equal(mem.rows_host()[1], b[BASE:])
        link = link_all[BASE:].copy()
        link[0] = 0.0
        seg = E.segment(E.opens(link, 0.5), BASE)
        got = mem.events(0.5, with_links=True)
        assert 1 < seg.count < CAP and got.count == seg.count, (D, got.count, seg.count)
        assert np.array_equal(got.first_rows.cpu().numpy(), seg.first_rows), D
        assert np.array_equal(got.event_of.cpu().numpy(), seg.event_of) and same_bits(got.links.cpu().numpy(), link), D
        want = S.summarize(b[BASE:], np.repeat(np.asarray(keys, dtype=np.int64), sizes)[BASE:], dtype, base=BASE)
        got = mem.summaries()
        assert got.count == want.first_rows.size, (D, got.count)
        for name in ("first_rows", "n_rows", "keys", "key_rows"):
            assert np.array_equal(getattr(got, name).cpu().numpy(), getattr(want, name)), (D, name)
        assert np.array_equal(bits(got.centroids), want.centroids), (D, "centroid bits")
        assert same_bits(got.key_scores.cpu().numpy(), want.key_scores), (D, "key scores (bit-exact bar)")
        mem.close()


# ---- 2. the create functions on bad weight lists ----------------------------------------------------------------------
VISION = dict(arch="t", image=64, patch=16, hidden=256, layers=2, heads=4, mlp=512, act="quick_gelu", ln_eps=1e-5,
              pre_ln=True, patch_bias=False, proj_dim=0, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))


def test_vision_create_refuses_a_bad_weight_list_and_the_next_create_works(monkeypatch):
    from vidmem import _lib, encoder, synthetic as syn
    w = syn.encoder_weights(VISION, seed=3, std=0.05)
    order = encoder._weight_order
    with monkeypatch.context() as mp:                    # one pointer short
        mp.setattr(encoder, "_weight_order", lambda spec: order(spec)[:-1])
        with pytest.raises(_lib.VidmemError) as e:
            encoder.FrameEncoder(VISION, w, dtype="f16")
    assert e.value.code == _lib.VM_ERR_INVALID and "expected 33 weight pointers, got 32" in str(e.value)
    with pytest.raises(_lib.VidmemError) as e:           # a layer weight that has bytes and no pointer
        encoder.FrameEncoder(VISION, {n: a for n, a in w.items() if n != "l1.fc1_w"}, dtype="f16")
    assert e.value.code == _lib.VM_ERR_HIP
    assert "encoder weight copy failed: " in str(e.value) and "(null or short weight pointer?)" in str(e.value)
    enc = encoder.FrameEncoder(VISION, w, dtype="f16")
    px = syn.normal(77, "px", (3, 3, 64, 64))
    got = enc.encode_patches(enc.patches_from_pixels(torch.from_numpy(px))).float().cpu().numpy()
    want_32 = V.vit_forward_ref(VISION, w, px, quant=None)
    rel = lambda a, b: float(np.linalg.norm(np.float64(a) - b) / np.linalg.norm(b))
    # the bar of tests/test_encoder_gpu.py: the contract, or 1.5 x the floor of this stack with f16 matrix operands
    bar = max(1e-3, 1.5 * rel(V.vit_forward_ref(VISION, w, px, quant={p: "f16" for p in V.OPERAND_POINTS}), want_32))
    assert rel(got, V.vit_forward_ref(VISION, w, px, quant="f16")) < bar and rel(got, want_32) < bar
    enc.close()


def test_text_create_refuses_a_bad_weight_list_and_the_next_create_works(monkeypatch):
    from vidmem import _lib, synthetic as syn, text
    spec = TR.tiny_text_spec(hidden=256, layers=2, vocab=1000, context=77, proj_dim=128)
    w = syn.text_encoder_weights(spec, seed=5, std=0.02)
    order = text._text_weight_order
    with monkeypatch.context() as mp:
        mp.setattr(text, "_text_weight_order", lambda s: order(s)[:-1])
        with pytest.raises(_lib.VidmemError) as e:
            text.TextEncoder(spec, w, dtype="f16", device=0)
    assert e.value.code == _lib.VM_ERR_INVALID and "expected 29 weight pointers, got 28" in str(e.value)
    with pytest.raises(_lib.VidmemError) as e:
        text.TextEncoder(spec, {n: a for n, a in w.items() if n != "l1.fc1_w"}, dtype="f16", device=0)
    assert e.value.code == _lib.VM_ERR_HIP
    assert "text encoder weight copy failed: " in str(e.value) and "(null or short weight pointer?)" in str(e.value)
    enc = text.TextEncoder(spec, w, dtype="f16", device=0)
    eots = [0, 1, 15, 16, 17, 76]
    ids = np.random.default_rng(12).integers(0, spec["vocab"] - 1, size=(len(eots), 77))
    ids[ids == spec["eot_id"]] = 3
    ids[np.arange(len(eots)), eots] = spec["eot_id"]
    want32 = TR.hf_text_embeds(spec, w, ids)
    # the bar of tests/test_text_gpu.py, per embedding: 1.5 x the distance of the restatement that rounds where the device does
    floor = TR.rel(TR.text_forward_ref(spec, w, ids, quant="f16"), want32)
    err = TR.rel(enc.encode_ids(ids).float().cpu().numpy(), want32)
    assert np.all(err <= 1.5 * floor), (err.tolist(), floor.tolist())
    enc.close()
