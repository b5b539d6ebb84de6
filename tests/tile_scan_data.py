"""The data of the tile-scan tests (tests/test_tile_scan_gpu.py and every search's ``test_scan``): the shapes at which the
shared fp32 tile scan (csrc/topk_tile_scan.h) can go wrong, one oracle score matrix per data set.

Shapes: D = 128 and 384 are 4 and 12 k-steps (less than one load batch of 8, and one and a half); 17, 33 and 47 live rows
are one, two and three 16-row tiles with a ragged last one; a ring of capacity 40 after 57 rows has its head in slot 17;
Q = 1, 16, 17, 33 are one 16-query tile, the switch to two, and a second query group with one live query.  k = 1, so the
searches re-score M = 9 candidates and the certificate bounds the 10th against the rest.  The data itself, its constants
and ``gap_ok`` are made in tests/mask_ref.py, which the CPU tests use too; here it is uploaded, once.
"""
import functools

import numpy as np

from tests.mask_ref import CLUSTERS, K, M1, QS, SHAPES, gap_ok, host_dataset  # noqa: F401
from tests.support import ALL, make_tag


@functools.lru_cache(maxsize=None)
def dataset(D, dtype, shape):
    """mask_ref.host_dataset with the rows and the queries on the device: (rows, queries, base, oracle score matrix
    [33, live rows])."""
    rows, q, base, live = host_dataset(D, dtype, shape)
    return rows.cuda(), q.cuda(), base, live


def tags_of(total):
    """Two sources interleaved row by row: tag = (row id % 2) << 40 | row id."""
    r = np.arange(total, dtype=np.int64)
    return ((r % 2) << 40) | r


def scope_sets(Q, base, cap):
    """name -> Q scopes.  `first_tile`: source 0's rows of physical slots 0 .. 15 - every other tile has no in-scope
    row and takes the skip path."""
    r0 = cap if cap else 0          # the row id in physical slot 0 (a ring of capacity cap after cap + 17 rows: cap)
    return {"all": [ALL] * Q,
            "half_per_query": [(make_tag(i % 2, 0), make_tag(i % 2, (1 << 40) - 1)) for i in range(Q)],
            "one_empty": [(10, 5) if i == Q // 2 else ALL for i in range(Q)],
            "first_tile": [(make_tag(0, r0), make_tag(0, r0 + 15))] * Q}
