"""Cross-validation criteria on the device — src/crossvalidation.jl.

predict_LOO / logp_LOO live in gpe.py (diag of the inverse, gpmi_inv_diag).  This module adds the rest of the reference's
model-selection surface: dlogpdθ_LOO, predict_CVfold, logp_CVfold and dlogpdθ_CVfold, through gpmi_loo_grad /
gpmi_cvfold_predict / gpmi_cvfold_grad (csrc/cv.hip; the derivation is DESIGN.md §7b).  Dense exact handles only.

Folds are sequences of 0-based integer indices (the reference's are 1-based Julia ranges).  They must be non-empty and
disjoint, with at most MAX_FOLD indices each; indices in no fold are training data of every fold, as in the reference.
Gradients come in the reference's order [logNoise; kernel…]; the keywords are required, as they are there.
"""
import ctypes as C
import numbers

import numpy as np

from . import _lib

MAX_FOLD = 2048  # GPMI_CV_MAX_FOLD: the super-panel width the fold blocks are factored in


def _check_folds(folds, n):
    """folds -> (fold_ptr, fold_idx) int64 CSR arrays; ArgumentError on empty, overlapping, out-of-range or non-integer
    entries and on folds over MAX_FOLD.  Pure host code: nothing reaches the device before it passes."""
    if isinstance(folds, (str, bytes)) or not hasattr(folds, "__len__") or len(folds) == 0:
        raise _lib.ArgumentError("folds must be a non-empty sequence of index sequences")
    ptr = [0]
    idx = []
    seen = set()
    for f, V in enumerate(folds):
        if isinstance(V, (str, bytes)) or not hasattr(V, "__len__"):
            raise _lib.ArgumentError(f"fold {f} is not a sequence of indices")
        if len(V) == 0:
            raise _lib.ArgumentError(f"fold {f} is empty")
        if len(V) > MAX_FOLD:
            raise _lib.ArgumentError(f"fold {f} has {len(V)} indices; at most {MAX_FOLD} (the super-panel width) are supported")
        for i in V:
            if isinstance(i, (bool, np.bool_)) or not isinstance(i, (numbers.Integral, np.integer)):
                raise _lib.ArgumentError(f"fold {f}: index {i!r} is not an integer")
            i = int(i)
            if i < 0 or i >= n:
                raise _lib.ArgumentError(f"fold {f}: index {i} is out of range 0 .. {n - 1}")
            if i in seen:
                raise _lib.ArgumentError(f"folds overlap at index {i}")
            seen.add(i)
            idx.append(i)
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)


def _dense(gp, who):
    from .gpe import HIPPDMat

    if getattr(gp, "covstrat", None) is not None or type(getattr(gp, "cK", None)) is not HIPPDMat:
        raise _lib.ArgumentError(f"{who}: dense exact handle only")
    if gp.alpha is None:
        raise _lib.ArgumentError(f"{who} needs a fitted model (call update_mll first)")


def _grad(gp, who, folds, noise, domean, kern):
    _dense(gp, who)
    if domean and gp.mean.num_params() > 0:
        raise _lib.ArgumentError(f"{who}: mean-parameter gradients are not defined (the reference throws "
                                 "\"I don't know how to do means yet\")")
    if noise and np.ndim(gp.logNoise) != 0:
        raise _lib.ArgumentError(f"{who}: the noise gradient needs a scalar logNoise (GPE.jl:313)")
    ptr_idx = _check_folds(folds, gp.nobs) if folds is not None else None
    ln = np.atleast_1d(np.asarray(gp.logNoise, dtype=np.float64))
    nfull = gp.kernel._full_num_params()
    kd, keep = gp.kernel.descriptor(gp.dim)
    dk = np.empty(max(nfull, 1), dtype=np.float64)
    dn = C.c_double()
    lp = C.c_double()
    dbl = C.POINTER(C.c_double)
    lib = _lib.load()
    if ptr_idx is None:
        rc = lib.gpmi_loo_grad(gp.cK.h, C.byref(kd), ln.ctypes.data_as(dbl), ln.shape[0], C.byref(lp), dk.ctypes.data_as(dbl), nfull,
                               C.byref(dn) if noise else None)
    else:
        ptr, idx = ptr_idx
        rc = lib.gpmi_cvfold_grad(gp.cK.h, C.byref(kd), ln.ctypes.data_as(dbl), ln.shape[0], len(ptr) - 1, ptr.ctypes.data, idx.ctypes.data,
                                  C.byref(lp), dk.ctypes.data_as(dbl), nfull, C.byref(dn) if noise else None)
    del keep
    gp.ctx.check(rc)
    parts = []
    if noise:
        parts.append(dn.value)
    if kern:
        parts.extend(dk[i] for i in gp.kernel.grad_slots())
    return lp.value, np.asarray(parts, dtype=np.float64)


def dlogpdθ_LOO(gp, *, noise, domean, kern):
    """dlogpdθ_LOO (crossvalidation.jl:146-175): the gradient of logp_LOO, [logNoise; kernel…]."""
    return _grad(gp, "dlogpdθ_LOO", None, noise, domean, kern)[1]


def loo_logp_and_grad(gp, *, noise, domean, kern):
    """(logp_LOO, dlogpdθ_LOO) from one device call"""
    return _grad(gp, "dlogpdθ_LOO", None, noise, domean, kern)


def predict_CVfold(gp, folds):
    """predict_CVfold (crossvalidation.jl:180-215): lists of μ_V and Σ_V, the predictions of y_V from every other observation."""
    _dense(gp, "predict_CVfold")
    ptr, idx = _check_folds(folds, gp.nobs)
    dt = _lib.np_dtype(gp.cK.bits)
    sizes = np.diff(ptr)
    resid = np.empty(int(ptr[-1]), dtype=dt)
    cov = np.empty(int(np.sum(sizes * sizes)), dtype=dt)
    lp = C.c_double()
    gp.ctx.check(_lib.load().gpmi_cvfold_predict(gp.cK.h, len(sizes), ptr.ctypes.data, idx.ctypes.data, resid.ctypes.data, cov.ctypes.data,
                                                 C.byref(lp)))
    mus, covs = [], []
    q = 0
    for f, s in enumerate(sizes):
        s = int(s)
        V = idx[ptr[f]:ptr[f + 1]]
        mus.append(gp.y[V] - resid[ptr[f]:ptr[f + 1]].astype(np.float64))
        covs.append(cov[q:q + s * s].astype(np.float64).reshape(s, s, order="F"))
        q += s * s
    return mus, covs


def logp_CVfold(gp, folds):
    """logp_CVfold (crossvalidation.jl:217-248): Σ_V log N(y_V; μ_V, Σ_V), reduced on the device."""
    _dense(gp, "logp_CVfold")
    ptr, idx = _check_folds(folds, gp.nobs)
    lp = C.c_double()
    gp.ctx.check(_lib.load().gpmi_cvfold_predict(gp.cK.h, len(ptr) - 1, ptr.ctypes.data, idx.ctypes.data, None, None, C.byref(lp)))
    return lp.value


def dlogpdθ_CVfold(gp, folds, *, noise, domean, kern):
    """dlogpdθ_CVfold (crossvalidation.jl:313-341): the gradient of logp_CVfold, [logNoise; kernel…]."""
    return _grad(gp, "dlogpdθ_CVfold", folds, noise, domean, kern)[1]


def cvfold_logp_and_grad(gp, folds, *, noise, domean, kern):
    """(logp_CVfold, dlogpdθ_CVfold) from one device call"""
    return _grad(gp, "dlogpdθ_CVfold", folds, noise, domean, kern)


# ASCII spellings
dlogpdtheta_LOO = dlogpdθ_LOO
dlogpdtheta_CVfold = dlogpdθ_CVfold
