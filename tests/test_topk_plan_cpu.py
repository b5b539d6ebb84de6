"""CPU: the top-k dispatch mirror (tests/topk_plan.py) and the coverage of tests/test_topk_paths_gpu.py's case table.

The GPU module pins each case to the mirror's launch counts; here the mirror's rules are checked at their boundaries
and the case table is checked to reach every kernel instantiation the dispatch can pick, so a case that drifts off its
path, or a path no case reaches, fails without a GPU.
"""
import numpy as np
import pytest

from oracle import cref
from tests import topk_plan as TP
from tests import test_topk_paths_gpu as PATHS
from tests.topk_ref import merge_topk, oracle_rows_parallel

NUM_CUS = 256   # MI355X


@pytest.mark.parametrize("k,KL", [(1, 8), (6, 8), (7, 16), (12, 16), (13, 32), (26, 32), (27, 64), (58, 64)])
def test_list_length_boundaries(k, KL):
    assert TP.pick_kl(k) == KL


def test_k_above_58_is_the_exhaustive_kernel():
    p = TP.plan(16, 59, 768, "f16", 100_000)
    assert p.family == "exact" and p.launches == {"topk_scan": 0, "topk_finalize": 0}
    assert TP.plan(16, 58, 768, "f16", 100_000).family == "cascade"


@pytest.mark.parametrize("Q,KL,D,QT", [(64, 16, 1152, 4), (64, 16, 1280, 2), (64, 8, 2048, 2), (200, 16, 2048, 2),
                                       (40, 32, 2048, 2), (40, 16, 1280, 2), (16, 8, 2048, 1), (17, 64, 256, 1),
                                       (100, 32, 256, 2), (49, 8, 128, 4), (48, 8, 128, 2)])
def test_query_tiles_and_the_lds_limit(Q, KL, D, QT):
    assert TP.pick_qt(Q, KL, D) == QT


@pytest.mark.parametrize("cap,few,many", [
    (65_536, [(0, None)], [(0, 32_768), (32_768, None)]),
    (100_000, [(0, None)], [(0, 32_768), (32_768, None)]),
    (300_000, [(0, 131_072), (131_072, None)], [(0, 32_768), (32_768, 262_144), (262_144, None)]),
    (1_000_000, [(0, 131_072), (131_072, None)], [(0, 32_768), (32_768, 262_144), (262_144, None)]),
])
def test_pass_limits(cap, few, many):
    assert TP.pass_limits(128, cap) == few      # Q <= 128: growth 32
    assert TP.pass_limits(129, cap) == many     # Q > 128: growth 8
    for Q, want in ((1, few), (300, many)):
        p = TP.plan(Q, 20, 256, "f16", cap)
        assert p.family == "cascade"
        assert [(x.begin, x.limit) for x in p.passes[1:]] == want
        assert p.launches == {"topk_scan": len(want) + 1, "topk_finalize": len(want) + 2}


@pytest.mark.parametrize("Q,cap,kinds", [(300, 300_000, "dense emit gscan emit"),
                                         (600, 300_000, "dense emit gscan emit"),
                                         (1024, 100_000, "dense emit gscan"),
                                         (256, 100_000, "dense emit emit"),       # table B: no pass has the tiles
                                         (128, 1_000_000, "dense emit emit")])    # <= 128 queries: never gscan
def test_gscan_choice_per_pass(Q, cap, kinds):
    for D in (256, 1024):
        p = TP.plan(Q, 10, D, "bf16", cap, NUM_CUS)
        assert " ".join(x.kind for x in p.passes) == kinds


def test_gscan_counts_rows_from_the_capacity_not_the_rows_stored():
    # the pass over [32,768, 262,144) of a 300k memory has 896 row panels x 2 query tiles >= 4 x 256 tiles whatever
    # the memory holds; one CU fewer than a multiple of 8 turns it off
    assert TP.gscan_supported(300, 262_144 - 32_768, 256, NUM_CUS)
    assert not TP.gscan_supported(300, 262_144 - 32_768, 256, 255)
    assert not TP.gscan_supported(128, 10 ** 6, 256, NUM_CUS)
    assert not TP.gscan_supported(7040, 16_383, 256, NUM_CUS)


def test_families_and_launch_counts():
    assert TP.plan(16, 10, 768, "f16", 100_000).launches == {"topk_scan": 1, "topk_finalize": 1}     # QT 1
    p = TP.plan(40, 10, 768, "f16", 100_000)
    assert p.family == "list+prepass" and p.launches == {"topk_scan": 2, "topk_finalize": 2}
    assert TP.plan(40, 10, 768, "f16", 65_535).family == "list"                                    # no pre-pass
    assert TP.plan(64, 10, 1280, "f16", 100_000).family == "list+prepass"                          # D outside emit
    assert TP.plan(64, 10, 768, "f16", 65_535).family == "list"
    assert TP.plan(49, 10, 768, "f16", 65_536).family == "cascade"
    assert TP.plan(48, 12, 768, "f16", 65_536).family == "list+prepass"
    assert TP.plan(1, 13, 768, "f16", 65_536).family == "cascade"                                  # KL 32
    p = TP.plan(129, 10, 768, "f16", 100_000)
    assert (p.KS, p.NG) == (6, 2)
    assert (TP.plan(129, 10, 1024, "f16", 100_000).NG, TP.plan(128, 10, 768, "f16", 100_000).NG) == (1, 1)


def test_bf16_finalize_staging():
    assert TP.plan(20, 40, 512, "bf16", 60_000).staged is True
    assert TP.plan(20, 40, 1024, "bf16", 60_000).staged is False
    assert TP.plan(20, 40, 768, "bf16", 60_000).staged is False
    assert TP.plan(20, 20, 1024, "bf16", 60_000).staged is True        # KL 32
    assert TP.plan(20, 40, 512, "f16", 60_000).staged is None


@pytest.mark.parametrize("n,head,want", [(0, 0, (0, 0)), (1, 0, (0, 1)), (4_095, 0, (0, 4_095)),
                                         (4_096, 0, (256, 4_096)), (4_097, 0, (256, 4_097)),
                                         (32_800, 0, (28_928, 32_800)), (131_100, 0, (127_232, 131_100)),
                                         (100_000, 1, (0, 4_095)), (100_000, 3_839, (0, 4_095)),
                                         (100_000, 3_840, (0, 3_840)), (100_000, 4_095, (0, 4_095)),
                                         (100_000, 4_096, (256, 4_096))])
def test_dense_range(n, head, want):
    assert TP.dense_range(n, head) == want


def test_fill_levels_straddle_the_pass_limits():
    """The two fill levels the issue names put the dense range across a pass limit of the Q > 128 and Q <= 128
    cascades."""
    d0, d1 = TP.dense_range(32_800, 0)
    assert d0 < 32_768 < d1 and 32_768 in TP.plan(300, 10, 256, "bf16", 300_000).limits
    d0, d1 = TP.dense_range(131_100, 0)
    assert d0 < 131_072 < d1 and 131_072 in TP.plan(16, 20, 256, "f16", 300_000).limits


def _expected_instantiations():
    want = set()
    for dt in ("f16", "bf16"):
        want |= {f"scan/{dt}/KL{kl}/QT{qt}" for kl, qt in PATHS.LIST_PAIRS}
        want |= {f"prepass/{dt}", f"gscan/{dt}", f"mixed/{dt}"}
        want |= {f"emit/{dt}/KS{ks}/NG1" for ks in (1, 2, 4, 6, 8)}
        want |= {f"emit/{dt}/KS{ks}/NG2" for ks in (1, 2, 4, 6)}
    want |= {"finalize/bf16/staged", "finalize/bf16/unstaged"}
    return want


def test_case_table_reaches_every_instantiation():
    reached = set()
    for case in PATHS.CASES:
        reached |= case.plan(NUM_CUS).instantiations
    want = _expected_instantiations()
    assert len([w for w in want if w.startswith("scan/")]) == 18      # 2 dtypes x 9 (KL, QT) pairs
    assert len([w for w in want if w.startswith("emit/")]) == 18      # 2 dtypes x (5 KS at NG 1 + 4 at NG 2)
    missing = sorted(want - reached)
    assert not missing, f"no case reaches {missing}"
    print(f"\n[topk paths] {len(PATHS.CASES)} cases reach all {len(want)} instantiations: " + " ".join(sorted(want)))


def test_case_tables_take_their_paths():
    """Each table's cases are on the path its name promises (the ids carry it: a failure says which path broke)."""
    fam = lambda cases: {c.plan(NUM_CUS).family for c in cases}
    assert fam(PATHS.CASES_B) == {"cascade"} and fam(PATHS.CASES_C) == {"cascade"}
    assert all("gscan" in {p.kind for p in c.plan(NUM_CUS).passes} for c in PATHS.CASES_C)
    assert all("gscan" not in {p.kind for p in c.plan(NUM_CUS).passes} for c in PATHS.CASES_B)
    assert fam(PATHS.CASES_D) == {"list", "list+prepass"} and fam(PATHS.CASES_H) == {"exact"}
    assert fam([c for c in PATHS.CASES_A if c.k >= 13]) == {"cascade"}
    assert fam([c for c in PATHS.CASES_A if c.k < 13]) == {"list"}
    for cap in (100_000, 300_000):
        fams = fam([c for c in PATHS.CASES_E if c.mem.cap == cap])
        assert fams == {"list", "list+prepass", "cascade"}
    assert len({c.id for c in PATHS.CASES}) == len(PATHS.CASES)
    for c in PATHS.CASES:
        assert c.mem.ring or c.mem.total <= c.mem.cap


def test_planted_slots_map_to_row_ids():
    m = PATHS.MemSpec("f16", 256, 100_000, 100_000 + 3_839, ring=True)
    assert (m.n, m.head, m.base) == (100_000, 3_839, 3_839)
    assert m.row_of_slot(3_839) == 3_839 + 0 and m.row_of_slot(0) == 100_000
    w = PATHS.MemSpec("f16", 256, 100_000, 200_000, ring=True)
    assert (w.head, w.row_of_slot(0), w.row_of_slot(99_999)) == (0, 100_000, 199_999)
    g = PATHS.MemSpec("f16", 256, 100_000, 5_000)
    assert (g.n, g.head, g.base, g.row_of_slot(4_999)) == (5_000, 0, 0, 4_999)


def test_row_chunked_oracle_equals_one_call():
    """The shared oracle helper splits the memory rows over threads and merges: same rows, same score bits, for
    ties (duplicates in different chunks), zero rows / queries, k > rows, min_score and score_mode."""
    rng = np.random.default_rng(3)
    D = 128
    m = rng.standard_normal((301, D)).astype(np.float16)
    m[200] = m[10]
    m[250:260] = m[3]
    m[77] = 0
    q = rng.standard_normal((6, D)).astype(np.float16)
    q[0] = m[3]
    q[1] = 0
    qb, mb = q.view(np.uint16), m.view(np.uint16)
    for k, kw in ((5, {}), (400, {}), (12, dict(score_mode=1, min_score=0.55)), (7, dict(min_score=0.1))):
        for threads in (1, 4, 7):
            got = oracle_rows_parallel(qb, mb, k, "f16", np.arange(6), threads=threads, **kw)
            want = cref.cosine_topk(qb, mb, k, dtype="f16", **kw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    got = merge_topk([(np.full((2, 3), -1), np.zeros((2, 3)))], 3)
    assert (got[0] == -1).all() and (got[1] == 0).all()
