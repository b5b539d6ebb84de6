"""CPU: the preconditions of tests/domain_ref.py's classes, against the C oracle and the fp32 stand-in.

  * every class marked exact: the scaling is exact, and the oracle's cosine matrix of the scaled vectors is
    bit-identical to that of the unscaled ones (64 x 512) - the metamorphic expectation the GPU tests lean on;
  * every class marked inside: the stand-in stays within cert_eps(D) x ||q|| of the exact cosine x ||q|| on 64 x 4,099
    pairs, and every norm lies in the certificate's interval;
  * every class marked outside: on its own planted pair the stand-in is not finite or misses by more than the bound, and
    some norm does leave the interval - the class leaves the domain in fact, and the library's guard is stated on the
    right quantity.
"""
import numpy as np
import pytest

from oracle import cref
from tests import domain_ref as DR


def _within(cls_name, ds, qs, D):
    qb, rb = DR.bits(qs), DR.bits(ds.rows)
    dt = ds.cls.dtype
    exact = cref.cosine_matrix(qb, rb, dtype=dt)
    qn = DR.norms(qb, dt)
    with np.errstate(all="ignore"):
        err = np.abs(DR.standin(qb, rb, dt).astype(np.float64) - exact * qn[:, None])
    return err, DR.cert_eps(D) * qn[:, None]


@pytest.mark.parametrize("name", DR.EXACT)
def test_exact_scaling_leaves_the_reference_cosine_bit_identical(name):
    ds = DR.domain_set(name, 64, 512, seed=3)
    qb, qs, q_exact, _, zero = ds.queries(64, seed=4)
    assert ds.rows_exact and q_exact, "the class is marked exact but its scaling lost bits"
    dt = ds.cls.dtype
    want = cref.cosine_matrix(DR.bits(qb), DR.bits(ds.base), dtype=dt)
    got = cref.cosine_matrix(DR.bits(qs), DR.bits(ds.rows), dtype=dt)
    assert np.array_equal(want.view(np.int64), got.view(np.int64))
    assert (want[zero] == 0.0).all() and (want[:, ds.zero_row] == 0.0).all()
    assert want[0, ds.dup[0]] == want[0, ds.dup[1]] > 0.999           # query 0 probes the exact duplicate pair
    a, b = ds.pairs[0]
    assert want[1, a] > 0.9 and want[1, b] > 0.9                      # query 1 the near-duplicate pair


def test_inexact_class_is_reported_inexact():
    ds = DR.domain_set("f16_subnormal", 64, 512, seed=3)
    assert not ds.rows_exact
    v = DR.as_f64(DR.bits(ds.rows), "f16")
    assert (np.abs(v[v != 0]) < 2.0 ** -14).mean() > 0.9, "most elements are meant to be fp16 subnormals"


@pytest.mark.parametrize("name", DR.INSIDE)
def test_inside_classes_stay_within_the_bound(name):
    D = 256
    ds = DR.domain_set(name, 4099, D, seed=5, pair_at=[4096])
    _, qs, _, _, _ = ds.queries(64, seed=6)
    err, bound = _within(name, ds, qs, D)
    assert np.isfinite(err).all()
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{name}: worst stand-in error {worst:.3f} x cert_eps ||q||")
    assert (err <= bound).all(), worst
    for nrm in (DR.norms(DR.bits(ds.rows), ds.cls.dtype), DR.norms(DR.bits(qs), ds.cls.dtype)):
        nz = nrm[nrm > 0]
        if ds.cls.dtype == "bf16":
            assert ((nz >= DR.NORM_MIN) & (nz <= DR.NORM_MAX)).all()
        else:       # fp16 cannot leave the interval: the guard is not even compiled for it
            assert ((nz >= 2.0 ** -24) & (nz <= 2.0 ** 22)).all()


@pytest.mark.parametrize("name", DR.OUTSIDE)
def test_outside_classes_leave_the_domain_on_their_planted_pair(name):
    D = 256
    ds = DR.domain_set(name, 4099, D, seed=5, pair_at=[4096])
    _, qs, _, picks, _ = ds.queries(64, seed=6)
    err, bound = _within(name, ds, qs, D)
    if ds.cls.rnorm_plants:
        pairs = [(2, r) for r in ds.rnorm_rows] + [(1, r) for r in ds.big_rows]   # query 1: the 2^10 query
    else:
        a, b = ds.pairs[0]
        pairs = [(1, a), (1, b)]                                                  # query 1 probes the pair
    for q, r in pairs:
        assert not np.isfinite(err[q, r]) or err[q, r] > bound[q, 0], (name, q, r, err[q, r], bound[q, 0])
    nrm = np.concatenate([DR.norms(DR.bits(ds.rows), "bf16"), DR.norms(DR.bits(qs), "bf16")])
    nz = nrm[nrm > 0]
    assert ((nz < DR.NORM_MIN) | (nz > DR.NORM_MAX)).any(), "the guard's interval would not catch this class"
