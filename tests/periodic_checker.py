"""Checker for the Periodic kernel (src/kernels/periodic.jl), which the oracle (oracle/gp_oracle.py) does not have.

A NumPy restatement of the Periodic leaf, composed with the oracle's own leaves for everything else in a tree (Sum, Prod,
Masked and Fixed are restated here because the oracle's recursion cannot see a Periodic leaf), and the few GPE / FITC
statements the Periodic tests need, written against that covariance:
    periodic.jl:33-52            Periodic(ll, lσ, lp): ℓ2 = e^{2 ll}, σ2 = e^{2 lσ}, p = e^{lp};  k = σ2 exp(−2/ℓ2 sin²(π r/p))
                                 dk/dll = 2 σ2 s e^{−s}, s = 2 sin²(π r/p)/ℓ2;  dk/dlσ = 2k;  dk/dlp = σ2 (π r/p)(2/ℓ2) sin(2π r/p) e^{−s}
    GPE.jl:169-212               update_mll! (dense): cov + nugget, Cholesky, α, logdet, mll
    GP.jl:25-84                  predict_f (pointwise variance clamped at 0, or the full covariance)
    GPE.jl:219-241, 273-275      update_dmll!: ½ tr((ααᵀ − K⁻¹) ∂K/∂θ) and the noise term
    fully_indep_train_conditional.jl:134-156, :38-41, :80   FITC update_cK!, `\\`, logdet
Specs are the oracle's nested tuples with one more leaf: ("periodic", ll, lσ, lp)."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as G

LOG2PI = math.log(2.0 * math.pi)


def has_periodic(spec):
    if spec[0] == "periodic":
        return True
    if spec[0] in ("sum", "prod"):
        return has_periodic(spec[1]) or has_periodic(spec[2])
    if spec[0] in ("masked", "fixed"):
        return has_periodic(spec[1])
    return False


def periodic_leaf(ll, lsig, lp, X1, X2):
    """cov(pe::Periodic, r) on every pair (periodic.jl:45), r the Euclidean distance (distance.jl:64-71)."""
    l2, s2, p = math.exp(2.0 * ll), math.exp(2.0 * lsig), math.exp(lp)
    r = np.sqrt(G._sqdist(np.asarray(X1, dtype=np.float64), np.asarray(X2, dtype=np.float64)))
    return s2 * np.exp(-2.0 / l2 * np.sin(np.pi * r / p) ** 2)


def cov(spec, X1, X2=None):
    X1 = np.asarray(X1, dtype=np.float64)
    X2 = X1 if X2 is None else np.asarray(X2, dtype=np.float64)
    if not has_periodic(spec):
        return G.cov(spec, X1, X2)
    name = spec[0]
    if name == "periodic":
        return periodic_leaf(spec[1], spec[2], spec[3], X1, X2)
    if name == "sum":
        return cov(spec[1], X1, X2) + cov(spec[2], X1, X2)
    if name == "prod":
        return cov(spec[1], X1, X2) * cov(spec[2], X1, X2)
    if name == "masked":
        dims = list(spec[2])
        return cov(spec[1], X1[dims, :], X2[dims, :])
    return cov(spec[1], X1, X2)  # fixed


def num_params(spec):
    name = spec[0]
    if name == "periodic":
        return 3
    if name in ("sum", "prod"):
        return num_params(spec[1]) + num_params(spec[2])
    if name == "masked":
        return num_params(spec[1])
    return G.num_params(spec)


def grad_cov(spec, X):
    """(K, [∂K/∂θ_p]) in get_params order (composites: sum_kernel.jl:18-51, prod_kernel.jl:17-68, masked_kernel.jl:51-56)."""
    X = np.asarray(X, dtype=np.float64)
    if not has_periodic(spec):
        return G.grad_cov(spec, X)
    name = spec[0]
    if name == "periodic":
        ll, lsig, lp = spec[1], spec[2], spec[3]
        l2, s2, p = math.exp(2.0 * ll), math.exp(2.0 * lsig), math.exp(lp)
        r = np.sqrt(G._sqdist(X, X))
        u = np.pi * r / p
        s = 2.0 * np.sin(u) ** 2 / l2
        K = s2 * np.exp(-s)
        return K, [2.0 * s2 * s * np.exp(-s), 2.0 * K, s2 * u * (2.0 / l2) * np.sin(2.0 * u) * np.exp(-s)]
    if name == "sum":
        K1, d1 = grad_cov(spec[1], X)
        K2, d2 = grad_cov(spec[2], X)
        return K1 + K2, d1 + d2
    if name == "prod":
        K1, d1 = grad_cov(spec[1], X)
        K2, d2 = grad_cov(spec[2], X)
        return K1 * K2, [d * K2 for d in d1] + [K1 * d for d in d2]
    if name == "masked":
        return grad_cov(spec[1], X[list(spec[2]), :])
    K, d = grad_cov(spec[1], X)  # fixed
    return K, [d[i] for i in spec[2]]


def with_params(spec, hyp):
    """The spec with its log-scale parameters replaced by hyp (get_params order; no Fixed wrappers)."""
    hyp = list(map(float, hyp))

    def walk(s):
        name = s[0]
        if name in ("sum", "prod"):
            return (name, walk(s[1]), walk(s[2]))
        if name == "masked":
            return (name, walk(s[1]), s[2])
        out = [name]
        for v in s[1:]:
            if np.ndim(v):
                out.append([hyp.pop(0) for _ in v])
            else:
                out.append(hyp.pop(0))
        return tuple(out)

    out = walk(spec)
    assert not hyp, "too many parameters"
    return out


def get_params(spec):
    name = spec[0]
    if name in ("sum", "prod"):
        return get_params(spec[1]) + get_params(spec[2])
    if name == "masked":
        return get_params(spec[1])
    out = []
    for v in spec[1:]:
        out.extend(float(t) for t in np.atleast_1d(v))
    return out


def kdiag(spec):
    """k(x, x): every leaf here is stationary, so one point at the origin of a 1-dimensional copy suffices per leaf."""
    name = spec[0]
    if name == "sum":
        return kdiag(spec[1]) + kdiag(spec[2])
    if name == "prod":
        return kdiag(spec[1]) * kdiag(spec[2])
    if name in ("masked", "fixed"):
        return kdiag(spec[1])
    return math.exp(2.0 * float(spec[2] if name not in ("noise", "const") else spec[1]))


def update_mll(spec, x, y, log_noise):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    K = cov(spec, x)
    K[np.diag_indices_from(K)] += math.exp(2.0 * log_noise)
    U = sla.cholesky(K, lower=False)
    alpha = sla.cho_solve((U, False), y)
    logdet = 2.0 * float(np.sum(np.log(np.diag(U))))
    mll = -(float(y @ alpha) + logdet + LOG2PI * x.shape[1]) / 2.0
    return {"mll": mll, "alpha": alpha, "U": U, "K": K}


def predict_f(spec, x, fit, xs, full_cov=False):
    Kc = cov(spec, x, xs)
    mu = Kc.T @ fit["alpha"]
    V = sla.solve_triangular(fit["U"], Kc, trans="T", lower=False)
    if full_cov:
        S = cov(spec, xs) - V.T @ V
        return mu, np.triu(S) + np.triu(S, 1).T
    return mu, np.maximum(kdiag(spec) - np.sum(V * V, axis=0), 0.0)


def update_dmll(spec, x, y, log_noise, fit=None):
    """[d mll / d logNoise, d mll / d θ_kernel…] (mean zero)."""
    x = np.asarray(x, dtype=np.float64)
    fit = fit or update_mll(spec, x, y, log_noise)
    Kinv = sla.cho_solve((fit["U"], False), np.eye(x.shape[1]))
    W = np.outer(fit["alpha"], fit["alpha"]) - Kinv
    _, dKs = grad_cov(spec, x)
    return np.array([math.exp(2.0 * log_noise) * np.trace(W)] + [0.5 * float(np.sum(W * dK)) for dK in dKs])


def fitc_mll(spec, x, xu, y, log_noise):
    """update_mll! on FITC: update_cK! (fully_indep_train_conditional.jl:134-156, both make_posdef! nuggets of 1e-10),
    `\\` (:38-41) and logdet (:80) as the reference states them."""
    x = np.asarray(x, dtype=np.float64)
    xu = np.asarray(xu, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    Kuu = cov(spec, xu)
    Kuu[np.diag_indices_from(Kuu)] += 1e-10
    Uuu = sla.cholesky(Kuu, lower=False)
    Kuf = cov(spec, xu, x)
    Luf = sla.solve_triangular(Uuu, Kuf, trans="T", lower=False)
    lam = math.exp(2.0 * log_noise) + kdiag(spec) - np.sum(Luf * Luf, axis=0)
    SQR = Kuf @ (Kuf / lam).T + Kuu
    SQR = np.triu(SQR) + np.triu(SQR, 1).T
    SQR[np.diag_indices_from(SQR)] += 1e-10
    Usqr = sla.cholesky(SQR, lower=False)
    Lk = sla.solve_triangular(Usqr, Kuf, trans="T", lower=False)
    yl = y / lam
    alpha = (y - Lk.T @ (Lk @ yl)) / lam
    logdet = 2.0 * float(np.sum(np.log(np.diag(Usqr)))) - 2.0 * float(np.sum(np.log(np.diag(Uuu)))) + float(np.sum(np.log(lam)))
    return -(float(y @ alpha) + logdet + LOG2PI * x.shape[1]) / 2.0
