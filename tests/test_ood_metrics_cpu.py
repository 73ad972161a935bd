"""`cmhar.ood.fpr_at_tpr` and `cmhar.ood.aupr` against sklearn (in-distribution = positive, higher score), on the
tie-heavy and lopsided score sets of tests/test_ood.py."""
import numpy as np
import pytest


def _sk_fpr_at_tpr(a, b, t):
    from sklearn.metrics import roc_curve
    fpr, tpr, _ = roc_curve(np.r_[np.ones(a.size), np.zeros(b.size)], np.r_[a, b], drop_intermediate=False)
    return fpr[np.argmax(tpr >= t)]


def _sk_aupr(a, b):
    from sklearn.metrics import average_precision_score
    return average_precision_score(np.r_[np.ones(a.size), np.zeros(b.size)], np.r_[a, b])


def _check(a, b):
    from cmhar.ood import aupr, fpr_at_tpr
    for t in (0.95, 0.8, 0.5, 1.0):
        assert abs(fpr_at_tpr(a, b, t) - _sk_fpr_at_tpr(a, b, t)) < 1e-12, t
    assert abs(fpr_at_tpr(a, b) - _sk_fpr_at_tpr(a, b, 0.95)) < 1e-12
    assert abs(aupr(a, b) - _sk_aupr(a, b)) < 1e-12


def test_metrics_match_sklearn_with_ties():
    rng = np.random.default_rng(0)
    _check(np.round(rng.normal(1.0, 1.0, 300), 1), np.round(rng.normal(0.0, 1.0, 200), 1))


@pytest.mark.parametrize('n_in,n_out,decimals', [(1, 5000, 2), (20000, 30000, 1), (50000, 7, 3), (4096, 4096, 0)])
def test_metrics_large_and_lopsided_vs_sklearn(n_in, n_out, decimals):
    rng = np.random.default_rng(n_in + n_out)
    _check(np.round(rng.normal(0.5, 1.0, n_in), decimals), np.round(rng.normal(0.0, 1.0, n_out), decimals))


def test_metrics_edge_cases():
    from cmhar.ood import aupr, fpr_at_tpr
    hi, lo = np.arange(10.0) + 10, np.arange(10.0)
    assert fpr_at_tpr(hi, lo) == 0.0 and aupr(hi, lo) == 1.0              # perfect separation
    assert fpr_at_tpr(lo, hi) == 1.0                                      # perfectly wrong: every OOD sample first
    _check(lo, hi)
    a, b = np.full(7, 3.0), np.full(9, 3.0)                               # one tied run across both sets
    assert fpr_at_tpr(a, b) == 1.0 and abs(aupr(a, b) - 7 / 16) < 1e-15
    _check(a, b)
    assert aupr(np.ones((2, 3)), np.zeros((3, 1))) == 1.0                 # any shape, flattened
    for f in (fpr_at_tpr, aupr):
        with pytest.raises(ValueError):
            f([], [1.0])
        with pytest.raises(ValueError):
            f([1.0], np.zeros(0))
