"""What the oracles of the searches that rank by a score of their own share word for word: tests/mix_ref.py,
tests/fold_ref.py, tests/bias_ref.py and tests/diverse_ref.py.  Their scores, their bounds (``eps_*``) and the comparison
that decides a flag-0 demand stay with each of them: those differ.
"""
from __future__ import annotations

import numpy as np

from tests import mask_ref as MR

DTS = ((128, "f16"), (128, "bf16"), (384, "f16"), (384, "bf16"))
NQ = 33                             # queries of the tile-scan dataset: term j of query c is dataset query (c J + j) % 33
# the cases the mixed and the any/all scan test share
CS = (1, 2, 3)                      # QT = 1, QT = 2, and a second query group with one live tile
JS = (1, 2, 5, 16)
KS = (1, 5)
W_MIN, W_MAX = 2.0 ** -20, 2.0 ** 20     # the weight domain of the bound


def term_rows(c: int, J: int):
    return [(c * J + j) % NQ for j in range(J)]


def slack_m(k: int) -> int:
    """M: the candidates re-scored exactly (vm_topk_geom); rank M + 1 bounds the rest."""
    return k + max(k // 4, 8)


def rank_pair(best_first, k: int):
    """best_first: one query's exact selected scores, descending -> (the value at rank k, the value at rank M + 1), or
    None when fewer than M + 1 rows are selected (everything is re-scored exactly)."""
    M1 = slack_m(k) + 1
    return None if best_first.size < M1 else (best_first[k - 1], best_first[M1 - 1])


def scan_selections(Q, shape, base, n):
    """name -> bool [Q, n]: 'none' (no mask) and every set of mask_ref.mask_sets(Q, shape)."""
    total, cap = MR.SHAPES[shape]
    out = {"none": np.ones((Q, n), dtype=bool)}
    for name, (masks, index) in MR.mask_sets(Q, shape).items():
        out[name] = MR.selection(masks, index, Q, base, n, cap or total)
    return out
