"""GPU: a memory carried through a whole life against ONE host model (tests/lifecycle_ref.py).

Two scripts - a linear memory of 1,600 rows and a ring of 600, grouped and tagged - apply every mutator in turn: keyed,
tagged and gated appends, erases by scope and by rows, whole and tail regroups, the ring overwrite, reset, snapshot /
restore.  After every step ``lifecycle_ref.checkpoint`` compares the accessors, the raw columns and all seventeen readers
- ``topk``, ``topk_grouped``, ``topk_scoped``, ``topk_grouped_scoped``, ``topk_clip``, ``range_search``, ``events``,
``summaries``, ``topk_masked``, ``topk_span``, ``topk_mix``, ``topk_diverse`` with ``last_diverse_mmr``,
``recall_links``, ``topk_biased``, ``topk_fold`` (max and min, with its term indices) and ``topk_seq`` (with its step
rows and step scores), the mask builders ``mask_of_rows`` / ``mask_of_scope`` / ``mask_where`` through ``rows_of_mask``
and the column builders ``bias_of_rows`` / ``bias_of_age`` read back at the slots of the live rows; each top-k reader in
its default and its exact form - with the model: rows, keys and fp64 score bits equal.  The masks are
all ones, a scope mask, the exclusion of the rows just shown, a metadata filter and the previous checkpoint's exclusion
mask searched again, stale, after the mutation; the spans include one carried over in the same way, and so do the bias
columns (zeros, a boost of the rows just shown, age with a fill that would win every ranking, and the previous
checkpoint's boost).  The six sequences lie across an erase join, at the newest and the oldest row (in the wrapped ring:
across slots capacity - 1 and 0), across a change of source, over a row their mask leaves out, and under the carried mask.
Where a feature's own oracle condition says that the fast path of the masked, span, mixed, diverse, biased, any/all or
sequence search must certify a query, its flag must be 0.  tests/test_lifecycle_cpu.py proves the scripts' conditions and
that the checkpoint fails on planted defects.

Measured on one MI355X (profiles/lifecycle.json): 1.6 - 4.3 s per script and dtype (1.0 - 2.3 s with the
fourteen readers of the parent commit, same session), 4.4 s for the slowest case under pytest; most of the added time is
the host oracles', the fold oracle's first.  Flag 0 is demanded of the biased, the any/all and the sequence search for
nearly every query of every fp16 checkpoint and was met; it is not demanded on the empty memory, of a query without a
selected row, of the `min` queries under WEIGHTS for which fold_ref.flag0_ok does not hold, and in bf16 once the sticky
word is set.
"""
import time

import numpy as np
import pytest
import torch

from tests import lifecycle_ref as LC
from tests.support import TD, bits

pytestmark = pytest.mark.gpu

SEG = 256                                  # erase segments of 256 rows: three and more per erase


class IO:
    """What ``checkpoint`` and the driver need beside the memory's public surface."""

    def __init__(self, dtype, tmp_path):
        self.dtype, self.tmp_path, self.n = dtype, tmp_path, 0

    def t(self, bits):
        """uint16 bit patterns -> device tensor of the memory dtype."""
        return torch.from_numpy(np.array(bits, copy=True).view(np.int16)).view(TD[self.dtype]).cuda()

    @staticmethod
    def i64(x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64))

    bits = staticmethod(bits)

    @staticmethod
    def stack(masks):
        """Masks ``[W]`` -> one device tensor ``[n_masks, W]``."""
        return torch.stack(list(masks))

    @staticmethod
    def f64(x):
        return torch.tensor(list(x), dtype=torch.float64).cuda()

    @staticmethod
    def i64d(x):
        """-> device int64 tensor (the spans as ``[Q, 2]``)."""
        return torch.tensor(x, dtype=torch.int64).cuda()

    @staticmethod
    def col_at(col, slots):
        """A device fp32 bias column read back at the given slots -> numpy."""
        return col[torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int64)).to(col.device)].cpu().numpy()

    @staticmethod
    def keep(col):
        """A copy of a column that outlives the stack it was built in: the next checkpoint searches it again."""
        return col.clone()

    @staticmethod
    def _col(mem, fn, n, width=None):
        from vidmem.memory import _tensor_from_ptr
        shape = (n,) if width is None else (n, width)
        dt = torch.int64 if width is None else torch.int16
        return _tensor_from_ptr(fn(mem.handle), shape, dt, mem.device).cpu().numpy().copy()

    def ordinals(self, mem):
        """The ordinal column of the live rows in row-id order."""
        total, n = len(mem), mem.searchable
        if n == 0:
            return np.zeros(0, np.int64)
        o = self._col(mem, mem.L.vm_memory_group_ordinals, n)
        return np.roll(o, -(total % mem.capacity)) if mem.ring and total > mem.capacity else o

    def raw(self, mem, n):
        """Rows, tags, keys and ordinals over slots [0, n), slot order: vacated slots included."""
        if n == 0:
            return [np.zeros((0, mem.dim), np.uint16)] + [np.zeros(0, np.int64)] * 3
        return [self._col(mem, mem.L.vm_memory_rows, n, mem.dim).view(np.uint16),
                self._col(mem, mem.L.vm_memory_tags, n), self._col(mem, mem.L.vm_memory_group_keys, n),
                self._col(mem, mem.L.vm_memory_group_ordinals, n)]

    def restore(self, mem, capacity):
        from vidmem.memory import EmbeddingMemory
        self.n += 1
        path = str(self.tmp_path / f"life_{self.n}.npz")
        mem.snapshot(path)
        back = EmbeddingMemory.restore(path, capacity=capacity)
        assert back.grouped and back.tagged and not back.ring
        back.prepare_erase(SEG)
        return back


def run_life(script, dtype, capacity, ring, tmp_path):
    """One script on a fresh memory -> (the driver it began with, the driver it ended with, what
    tools/lifecycle_probe.py records: seconds, checkpoints, the uncertified counts of every checkpoint)."""
    from vidmem.memory import EmbeddingMemory
    t0 = time.perf_counter()
    mem = EmbeddingMemory(capacity, LC.DIMS[dtype], dtype, ring=ring, grouped=True, tagged=True)
    mem.prepare_erase(SEG)
    d = LC.Driver(mem, LC.Model(LC.DIMS[dtype], dtype, capacity, ring), IO(dtype, tmp_path))
    end = script(d)
    torch.cuda.synchronize()
    for x in [mem] + [r.mem for r in d.restored]:          # every memory of the life, the restored ones included
        x.close()
    seconds = time.perf_counter() - t0                      # set-up to tear-down
    record = {"seconds": round(seconds, 2), "checkpoints": len(d.log),
              "uncertified": [{"checkpoint": label, **counts} for label, counts in d.log]}
    print(f"{script.__name__} {dtype}: {len(d.log)} checkpoints in {seconds:.1f} s")
    worst = {name: max(counts[name] for _, counts in d.log) for name in LC.UNCERT}
    print(f"{script.__name__} {dtype}: most queries sent to the redo by one memory: "
          + ", ".join(f"{name[:-len('_count')]}={n}" for name, n in worst.items()))
    return d, end, record


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_linear_life(dtype, tmp_path):
    d, end, _ = run_life(LC.linear_script, dtype, 1600, False, tmp_path)
    assert len(d.log) == 13 and d.stored + end.stored < 1600


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_ring_life(dtype, tmp_path):
    d, _, _ = run_life(LC.ring_script, dtype, 600, True, tmp_path)
    assert len(d.log) == 9 and d.model.total < 600 and d.stored < 1600


def test_tail_regroup_after_erase_can_repeat_a_key():
    """DESIGN.md 16 beside 14's wart: a tail regroup keys an event by its first row's id, and an erase renumbers the
    rows but keeps the keys' values.  Ten rows regrouped as events [0..4] and [5..9] (keys 0 and 5), rows 0..4 erased
    (the survivors are rows 0..4 now, still keyed 5), five rows of another scene appended (rows 5..9) and regrouped from
    row 5: the new event is keyed 5 and sits next to the surviving event keyed 5 - two groups by their ordinals, one
    run of equal keys.  What the header's rules say today, pinned:
      * ``topk_grouped`` goes by the ordinals: two groups, both keyed 5;
      * a following erase of any row re-derives the groups from the keys: one group;
      * a whole regroup instead keeps them two and gives them distinct keys."""
    from vidmem.memory import EmbeddingMemory
    dtype, D = "f16", 128
    bits, scene = LC.pool(dtype)
    starts = np.nonzero(np.concatenate([[True], scene[1:] != scene[:-1]]))[0]
    sizes = np.diff(starts)
    a, b, c = [int(starts[i]) for i in np.nonzero(sizes >= 5)[0][:3]]
    rows = np.concatenate([bits[a:a + 5], bits[b:b + 5]])
    new = bits[c:c + 5]
    io = IO(dtype, None)
    q = io.t(np.stack([rows[7], new[2]]))

    def life():
        mem = EmbeddingMemory(64, D, dtype, grouped=True, tagged=True)
        tags = [LC.make_tag(0, i * LC.MS) for i in range(15)]
        mem.append(io.t(rows), group=list(range(100, 110)), tag=tags[:10])
        assert mem.regroup_events(0.5) == 2 and mem.group_keys_host().tolist() == [0] * 5 + [5] * 5
        assert mem.erase(rows=list(range(5))).count == 5
        assert mem.group_keys_host().tolist() == [5] * 5
        assert mem.append(io.t(new), group=list(range(200, 205)), tag=tags[10:]) == 5
        assert mem.regroup_events(0.5, from_row=5) == 1
        assert mem.group_keys_host().tolist() == [5] * 10                     # the stale key and the new event's key
        o = io.ordinals(mem)
        assert (o - o[0]).tolist() == [0] * 5 + [1] * 5                      # two groups all the same
        return mem

    mem = life()
    for exact in (False, True):
        s, r, k = mem.topk_grouped(q, 3, exact=exact)
        assert k.tolist() == [[5, 5, -1], [5, 5, -1]]                         # two groups, one key
        assert r[:, 0].tolist() == [2, 7] and (r[:, 1] >= 0).all() and (r[:, 2] == -1).all()
    assert mem.summaries().count == 2
    assert mem.erase(rows=[9]).count == 1                                     # any erase re-derives groups from keys
    o = io.ordinals(mem)
    assert (o - o[0]).tolist() == [0] * 9 and mem.summaries().count == 1
    s, r, k = mem.topk_grouped(q, 3)
    assert k.tolist() == [[5, -1, -1], [5, -1, -1]] and r[:, 0].tolist() == [2, 7]
    mem.close()
    mem = life()
    assert mem.regroup_events(0.5) == 2                                       # a whole regroup repairs it
    assert mem.group_keys_host().tolist() == [0] * 5 + [5] * 5
    s, r, k = mem.topk_grouped(q, 3)
    assert k[0].tolist()[:2] == [0, 5] and k[1].tolist()[:2] == [5, 0] and r[:, 0].tolist() == [2, 7]
    mem.close()
