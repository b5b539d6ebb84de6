"""CPU: the erase model (tests/erase_ref.py) against itself, the selector check of EmbeddingMemory.erase, and the binding
table (include/vidmem.h vm_memory_erase_*).  No GPU call is made here."""
import numpy as np
import pytest

from tests import erase_ref as E


def _columns(n=600, D=8, seed=0):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 1 << 16, size=(n, D), dtype=np.uint16)
    src = np.arange(n) // 75                                  # 8 sources of 75 rows
    tags = (src.astype(np.int64) << 40) | ((np.arange(n) % 75) * 33)
    keys = (np.arange(n) // 7).astype(np.int64)
    return E.Columns(rows, tags, keys)


def _same(a: E.ErasedModel, b: E.ErasedModel):
    for x, y in zip(a.cols, b.cols):
        assert np.array_equal(x, y)
    assert np.array_equal(a.new_row_of, b.new_row_of) and a.count == b.count
    assert np.array_equal(a.ordinals, b.ordinals) and a.state == b.state


def test_scopes_equal_the_ids_of_the_same_rows():
    c = _columns()
    scopes = [(2 << 40, (3 << 40) - 1), ((5 << 40) | 330, (5 << 40) | 660), (7, 3)]     # the last one is empty
    drop = E.mask_of_scopes(c.tags, scopes)
    assert drop.sum() == 75 + 11
    ids = np.nonzero(drop)[0]
    padded = np.concatenate([ids, ids[:5], [-1, -7, 600, 10 ** 9, -1]]).reshape(2, -1)     # duplicates, padding, past the end
    _same(E.erase(c, drop), E.erase(c, E.mask_of_rows(600, padded)))


def test_two_erases_equal_one_erase_of_the_union():
    c = _columns()
    rng = np.random.default_rng(1)
    d1 = rng.random(600) < 0.3
    first = E.erase(c, d1)
    d2 = rng.random(first.cols.rows.shape[0]) < 0.4
    second = E.erase(first.cols, d2)
    union = d1.copy()
    union[np.nonzero(~d1)[0][d2]] = True
    both = E.erase(c, union)
    for x, y in zip(second.cols, both.cols):
        assert np.array_equal(x, y)
    assert np.array_equal(E.compose(first.new_row_of, second.new_row_of), both.new_row_of)
    assert first.count + second.count == both.count
    assert np.array_equal(second.ordinals, both.ordinals) and second.state == both.state


def test_erasing_nothing_is_the_identity():
    c = _columns()
    out = E.erase(c, np.zeros(600, bool))
    assert out.count == 0 and np.array_equal(out.new_row_of, np.arange(600))
    for x, y in zip(out.cols, c):
        assert np.array_equal(x, y)
    assert np.array_equal(out.ordinals, np.arange(600) // 7) and out.state == (86, 85, 1)
    everything = E.erase(c, np.ones(600, bool))
    assert everything.count == 600 and everything.cols.rows.shape == (0, 8) and everything.state == (0, 0, 0)
    assert (everything.new_row_of == -1).all()


def test_equal_key_groups_that_become_adjacent_merge():
    keys = np.array([4, 4, 9, 9, 9, 4, 4, 4, 2], np.int64)          # A B A C
    c = E.Columns(np.arange(9 * 4, dtype=np.uint16).reshape(9, 4), None, keys)
    assert E.ordinals_of(keys).tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 3]
    out = E.erase(c, E.mask_of_rows(9, [2, 3, 4]))
    assert out.cols.keys.tolist() == [4, 4, 4, 4, 4, 2]
    assert out.ordinals.tolist() == [0, 0, 0, 0, 0, 1] and out.state == (2, 2, 1)
    # a group that loses rows keeps the rest, and the last survivor's key is the state's
    out = E.erase(c, E.mask_of_rows(9, [0, 3, 8]))
    assert out.cols.keys.tolist() == [4, 9, 9, 4, 4, 4] and out.ordinals.tolist() == [0, 1, 1, 2, 2, 2]
    assert out.state == (3, 4, 1)


def test_the_selector_check_needs_exactly_one():
    from vidmem.memory import _check_erase_selectors
    with pytest.raises(ValueError):
        _check_erase_selectors(None, None)
    with pytest.raises(ValueError):
        _check_erase_selectors([1, 2], (0, 5))
    _check_erase_selectors([1, 2], None)
    _check_erase_selectors(None, (0, 5))


def test_binding_table_holds_the_new_symbols():
    from vidmem import _lib
    for name in ("vm_memory_erase_workspace_bytes", "vm_memory_erase_scoped", "vm_memory_erase_rows"):
        assert name in _lib.SYMBOLS
