"""Cross-validation on the CPU: tests/cv_checker.py (the literal restatement of src/crossvalidation.jl) against finite differences
and refits, the one-contraction form of DESIGN.md §7b against the checker, and the fold validation of gpmi355x.crossvalidation."""
import math

import numpy as np
import pytest

import cv_checker as CV
from oracle import gp_oracle as G
from gpmi355x import ArgumentError
from gpmi355x.crossvalidation import MAX_FOLD, _check_folds

SE = ("se_iso", math.log(0.5), math.log(0.8))
COMP = ("sum", ("se_ard", [0.1, -0.3], 0.0), ("mat52_iso", math.log(0.7), math.log(0.5)))


def _data(n, d=1, seed=1):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-2, 2, (d, n)), axis=1)
    y = np.abs(x[0] - 5) * np.cos(2 * x[0]) + 0.8 * rng.standard_normal(n)
    return x, y


FOLD_CASES = {
    "loo": None,
    "folds": [range(0, 5), range(5, 14), range(14, 20)],
    "partial": [[0, 3, 7], [10, 11], [15, 19, 2]],
    "singletons": [[i] for i in range(20)],
}


def _criterion(spec, x, y, ln, folds):
    f = CV.fit(spec, x, y, ln)
    return CV.logp_LOO(f) if folds is None else CV.logp_CVfold(f, folds)


@pytest.mark.parametrize("spec", [SE, COMP], ids=["se_iso", "composite"])
@pytest.mark.parametrize("case", list(FOLD_CASES))
def test_checker_matches_finite_differences(spec, case):
    import periodic_checker as P

    d = 1 if spec is SE else 2
    x, y = _data(20, d)
    folds = FOLD_CASES[case]
    ln = math.log(0.8)
    f = CV.fit(spec, x, y, ln)
    g = CV.dlogpdθ_LOO(f, True, True) if folds is None else CV.dlogpdθ_CVfold(f, folds, True, True)
    hyp = np.asarray(P.get_params(spec), dtype=np.float64)
    h = 1e-5
    num = [(_criterion(spec, x, y, ln + h, folds) - _criterion(spec, x, y, ln - h, folds)) / (2 * h)]
    for p in range(len(hyp)):
        e = np.zeros_like(hyp)
        e[p] = h
        num.append((_criterion(P.with_params(spec, hyp + e), x, y, ln, folds) - _criterion(P.with_params(spec, hyp - e), x, y, ln, folds)) / (2 * h))
    np.testing.assert_allclose(g, num, atol=1e-6, rtol=0)


def test_checker_predict_CVfold_is_a_refit():
    x, y = _data(20)
    ln = math.log(0.8)
    mspec = ("lin", [1.0])
    f = CV.fit(SE, x, y, ln, mspec)
    folds = [list(range(0, 5)), list(range(5, 14)), list(range(14, 20)), ]
    mus, covs = CV.predict_CVfold(f, folds)
    for V, mu, S in zip(folds, mus, covs):
        T = [j for j in range(20) if j not in V]
        ref = G.update_mll(SE, x[:, T], y[T], ln, mspec)
        m, c = G.predict_y(SE, x[:, T], ref, x[:, V], ln, mspec, full_cov=True)
        np.testing.assert_allclose(mu, m, rtol=0, atol=1e-10)
        np.testing.assert_allclose(S, c, rtol=0, atol=1e-10)


def g_form(f, folds):
    """dlogp/dθj = tr(∂K/∂θj G), dlogp/dlogσ = 2σ² tr(G), G = ½(α b' + b α') − ½ W B W, b = W u"""
    W, a = f["invS"], f["alpha"]
    n = len(a)
    folds = [[i] for i in range(n)] if folds is None else [list(V) for V in folds]
    u = np.zeros(n)
    B = np.zeros((n, n))
    for V in folds:
        SV = np.linalg.inv(W[np.ix_(V, V)])
        uV = SV @ a[V]
        u[V] = uV
        B[np.ix_(V, V)] = SV + np.outer(uV, uV)
    b = W @ u
    Gm = 0.5 * (np.outer(a, b) + np.outer(b, a)) - 0.5 * W @ B @ W
    return np.asarray([2 * math.exp(2 * float(f["log_noise"])) * np.trace(Gm)] + [float(np.sum(dK * Gm)) for dK in f["dKs"]])


@pytest.mark.parametrize("case", list(FOLD_CASES))
def test_g_form_matches_the_reference_form(case):
    x, y = _data(30, 2, seed=3)
    folds = FOLD_CASES[case]
    if folds is not None:
        folds = [[i for i in V if i < 30] for V in folds]
    f = CV.fit(COMP, x, y, math.log(0.4))
    lit = CV.dlogpdθ_LOO(f, True, True) if folds is None else CV.dlogpdθ_CVfold(f, folds, True, True)
    np.testing.assert_allclose(g_form(f, folds), lit, rtol=0, atol=1e-12 * max(1.0, np.abs(lit).max()))


def test_check_folds_builds_csr():
    ptr, idx = _check_folds([range(0, 3), [7, 5], np.array([9])], 10)
    assert ptr.tolist() == [0, 3, 5, 6] and idx.tolist() == [0, 1, 2, 7, 5, 9]
    assert ptr.dtype == np.int64 and idx.dtype == np.int64


@pytest.mark.parametrize("folds", [
    [],                       # no folds
    [[0, 1], []],             # empty fold
    [[0, 1], [1, 2]],         # overlap
    [[0, 10]],                # out of range
    [[-1]],                   # negative
    [[0.5]],                  # not an integer
    [[True]],                 # bool is not an index
    [["a"]],                  # not a number
    "abc",                    # not a sequence of sequences
    [3],                      # a fold that is not a sequence
], ids=["none", "empty", "overlap", "range", "negative", "float", "bool", "str", "string", "scalar"])
def test_check_folds_rejects(folds):
    with pytest.raises(ArgumentError):
        _check_folds(folds, 10)


def test_check_folds_limit():
    _check_folds([range(MAX_FOLD)], MAX_FOLD + 1)
    with pytest.raises(ArgumentError, match="2048"):
        _check_folds([range(MAX_FOLD + 1)], MAX_FOLD + 1)
