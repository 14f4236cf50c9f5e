"""A literal NumPy fp64 restatement of src/crossvalidation.jl: the reference's own algorithm, not the device's.

Every function follows the Julia source line by line: inv(Σ) explicitly, one Zj = inv(Σ) ∂K/∂θj and one Zj inv(Σ) per
hyper-parameter (grad_cov of the oracle, or of periodic_checker for specs with a Periodic leaf), the per-observation and
per-fold loops, and logp_CVfold's make_posdef!(Σ_V; nugget = 1e-10).  Folds are 0-based index sequences.
Nothing here uses the one-contraction form the device runs; tests/test_cv_host.py checks that form
against this file."""
import math

import numpy as np

import periodic_checker as P
from oracle import gp_oracle as G

LOG2PI = math.log(2.0 * math.pi)


def fit(spec, x, y, log_noise, mspec=("zero",)):
    """update_mll!: Σ = K + σ²I (or diag(exp(2 logNoise))), alpha = Σ \\ (y - m), and the stack of ∂K/∂θ"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    K, dKs = P.grad_cov(spec, x)
    n = x.shape[1]
    S = K + np.diag(np.broadcast_to(np.exp(2.0 * np.asarray(log_noise, dtype=np.float64)), (n,)))
    ym = y - G.mean(mspec, x)
    alpha = np.linalg.solve(S, ym)
    return {"Sigma": S, "invS": np.linalg.inv(S), "alpha": alpha, "y": y, "dKs": dKs, "log_noise": log_noise}


# ---- leave-one-out (crossvalidation.jl:8-175) --------------------------------------------------------------------------------
def predict_LOO(f):
    s2 = 1.0 / np.diag(f["invS"])
    return -f["alpha"] * s2 + f["y"], s2


def logp_LOO(f):
    mu, s2 = predict_LOO(f)
    return float(sum(-0.5 * LOG2PI - 0.5 * math.log(v) - 0.5 * (yi - m) ** 2 / v for m, v, yi in zip(mu, s2, f["y"])))


def _loo_term(invS, Zj, y, alpha):
    """the body of dlogpdθ_LOO_kern! / dlogpdσ2_LOO for one Zj (before the factor -1/2)"""
    s2 = 1.0 / np.diag(invS)
    mu = -alpha * s2 + y
    ZjSinv = np.diag(Zj @ invS)
    ds2 = ZjSinv * s2 ** 2
    dmu = (Zj @ alpha) * s2 - alpha * ds2
    g = 0.0
    for i in range(len(y)):
        g -= 2 * (y[i] - mu[i]) / s2[i] * dmu[i]
        g -= (y[i] - mu[i]) ** 2 * ZjSinv[i]
        g += ZjSinv[i] * s2[i]
    return g


def dlogpdθ_LOO(f, noise, kern):
    out = []
    invS, y, alpha = f["invS"], f["y"], f["alpha"]
    if noise:
        out.append(-_loo_term(invS, invS, y, alpha) / 2 * 2 * math.exp(2 * float(f["log_noise"])))
    if kern:
        out.extend(-0.5 * _loo_term(invS, invS @ dK, y, alpha) for dK in f["dKs"])
    return np.asarray(out, dtype=np.float64)


# ---- arbitrary folds (crossvalidation.jl:180-341) ---------------------------------------------------------------------------
def predict_CVfold(f, folds):
    invS = f["invS"]
    mus, covs = [], []
    for V in folds:
        V = list(V)
        SV = np.linalg.inv(invS[np.ix_(V, V)])
        mus.append(f["y"][V] - SV @ f["alpha"][V])
        covs.append(SV)
    return mus, covs


def logp_CVfold(f, folds, nugget=1e-10):
    """nugget: the reference's make_posdef! nugget (0 gives the exact criterion the device computes)"""
    mus, covs = predict_CVfold(f, folds)
    cv = 0.0
    for mu, SV, V in zip(mus, covs, folds):
        SV = SV.copy()
        SV[np.diag_indices_from(SV)] += nugget  # make_posdef!(ΣVT, chol; nugget=1e-10)
        L = np.linalg.cholesky(SV)
        r = np.linalg.solve(L, f["y"][list(V)] - mu)
        cv += -0.5 * len(V) * LOG2PI - float(np.sum(np.log(np.diag(L)))) - 0.5 * float(r @ r)  # logpdf(MvNormal(μ, Σ), y_V)
    return cv


def _gradient_fold(invS, alpha, ZjSinv, Zja, V):
    V = list(V)
    SVinv = invS[np.ix_(V, V)]
    SVa = np.linalg.solve(SVinv, alpha[V])
    Zs = ZjSinv[np.ix_(V, V)]
    g = 0.0
    g -= 2 * float(SVa @ Zja[V])
    g += float(SVa @ (Zs @ SVa))
    g += float(np.trace(np.linalg.solve(SVinv, Zs)))
    return g


def _fold_term(invS, Zj, alpha, folds):
    Zja = Zj @ alpha
    ZjSinv = Zj @ invS
    return sum(_gradient_fold(invS, alpha, ZjSinv, Zja, V) for V in folds)


def dlogpdθ_CVfold(f, folds, noise, kern):
    out = []
    invS, alpha = f["invS"], f["alpha"]
    if noise:
        out.append(-_fold_term(invS, invS, alpha, folds) / 2 * 2 * math.exp(2 * float(f["log_noise"])))
    if kern:
        out.extend(-0.5 * _fold_term(invS, invS @ dK, alpha, folds) for dK in f["dKs"])
    return np.asarray(out, dtype=np.float64)
