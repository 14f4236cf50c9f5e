"""Cross-validation on the device (gpmi_loo_grad / gpmi_cvfold_predict / gpmi_cvfold_grad, csrc/cv.hip) against tests/cv_checker.py,
the literal NumPy restatement of src/crossvalidation.jl, and against refits and finite differences of the device's own criteria.

Which path runs what: LOO reads W_ii off the diagonal; folds of s <= 64 go through cv_small_kernel (potf2_wg, one workgroup per
fold), folds of 65 .. 2048 through the super-block factor + inverse; N >= 8192 takes the chunked form of W (G2 holds -W)."""
import math

import numpy as np
import pytest

import cv_checker as CV
import gpmi355x as g
import kernel_cases as KC
from gpmi355x.crossvalidation import cvfold_logp_and_grad, loo_logp_and_grad

pytestmark = pytest.mark.gpu

PER = ("prod", ("periodic", math.log(0.8), 0.3, math.log(0.37)), ("se_iso", math.log(2.0), 0.1))
SPECS = KC.ALL + [PER]


def _ref_data(n):
    rng = np.random.default_rng(1)
    x = np.sort(rng.uniform(-2, 2, n))[None, :]
    y = np.abs(x[0] - 5) * np.cos(2 * x[0]) + 0.8 * rng.standard_normal(n)
    return x, y


def _gp(x, y, spec, ln, dtype=np.float64, mean=None):
    return g.GPE(x, y, mean if mean is not None else g.MeanZero(), g.from_spec(spec), ln, dtype=dtype, ctx=g.Context.default(0))


def _rel(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want).max()
    assert err <= tol * max(1.0, np.abs(want).max()), f"{what}: max |diff| {err:.3e} > {tol:g} max(1, |ref|) ({np.abs(want).max():.3e})"


@pytest.mark.parametrize("case", ["loo", "folds"])
def test_reference_scenarios(case):
    """test/test_crossvalidation.jl: n = 10 LOO and n = 20 folds [1:5, 6:14, 15:20], SEIso(0.5, 0.8), MeanLin([1.0]), after optimize"""
    n = 10 if case == "loo" else 20
    folds = None if case == "loo" else [range(0, 5), range(5, 14), range(14, 20)]
    x, y = _ref_data(n)
    gp = g.GPE(x, y, g.MeanLin([1.0]), g.SEIso(math.log(0.5), math.log(0.8)), math.log(0.8), ctx=g.Context.default(0))
    g.optimize(gp, domean=False)
    spec = ("se_iso", *map(float, gp.kernel.get_params()))
    ln = float(gp.logNoise)
    f = CV.fit(spec, x, y, ln, ("lin", [1.0]))
    if folds is None:
        lp, gr = loo_logp_and_grad(gp, noise=True, domean=False, kern=True)
        _rel(lp, CV.logp_LOO(f), 1e-9, "logp_LOO")
        _rel(gr, CV.dlogpdθ_LOO(f, True, True), 1e-9, "dlogpdθ_LOO")
        mu, s2 = gp.predict_LOO()
        for i in range(n):  # a refit without observation i on the device
            T = [j for j in range(n) if j != i]
            gt = g.GPE(x[:, T], y[T], g.MeanLin([1.0]), g.from_spec(spec), ln, ctx=g.Context.default(0))
            m, v = gt.predict_y(x[:, [i]])
            assert abs(m[0] - mu[i]) <= 1e-9 and abs(v[0] - s2[i]) <= 1e-9
    else:
        mus, covs = gp.predict_CVfold(folds)
        for V, m0, c0 in zip(folds, mus, covs):
            V = list(V)
            T = [j for j in range(n) if j not in V]
            gt = g.GPE(x[:, T], y[T], g.MeanLin([1.0]), g.from_spec(spec), ln, ctx=g.Context.default(0))
            m, c = gt.predict_y(x[:, V], full_cov=True)
            np.testing.assert_allclose(m0, m, rtol=0, atol=1e-9)
            np.testing.assert_allclose(c0, c, rtol=0, atol=1e-9)
        lp, gr = cvfold_logp_and_grad(gp, folds, noise=True, domean=False, kern=True)
        assert abs(lp - gp.logp_CVfold(folds)) <= 1e-12 * abs(lp)
        _rel(lp, CV.logp_CVfold(f, folds), 1e-9, "logp_CVfold")
        _rel(gr, CV.dlogpdθ_CVfold(f, folds, True, True), 1e-9, "dlogpdθ_CVfold")
    # finite differences of the device's own criterion (refit at every point)
    hyp = np.concatenate([[ln], gp.kernel.get_params()])

    def crit(h):
        gq = g.GPE(x, y, g.MeanLin([1.0]), g.SEIso(h[1], h[2]), h[0], ctx=g.Context.default(0))
        return gq.logp_LOO() if folds is None else gq.logp_CVfold(folds)

    num = []
    for p in range(3):
        e = np.zeros(3)
        e[p] = 1e-5
        num.append((crit(hyp + e) - crit(hyp - e)) / 2e-5)
    np.testing.assert_allclose(gr, num, rtol=0, atol=1e-6)


def _check_case(spec, n, d, folds, ln=math.log(0.3), dtype=np.float64, tol=1e-8, ltol=1e-10, seed=7):
    from oracle import gp_oracle as G

    x, y, _ = G.synthetic_inputs(n, d, p=1, seed=seed)
    gp = _gp(x, y, spec, ln, dtype=dtype)
    f = CV.fit(spec, x, y, ln)
    if folds is None:
        lp, gr = loo_logp_and_grad(gp, noise=True, domean=False, kern=True)
        lr, grr = CV.logp_LOO(f), CV.dlogpdθ_LOO(f, True, True)
    else:
        lp, gr = cvfold_logp_and_grad(gp, folds, noise=True, domean=False, kern=True)
        # the reference's logp_CVfold adds a 1e-10 nugget to every Σ_V (make_posdef!): ½ 1e-10 tr(W_VV) + ..., 2e-9 relative at
        # N = 3072 with σ² = 0.09 — above 1e-10.  The bound holds against the criterion without it; the nugget's share is checked apart
        lr, grr = CV.logp_CVfold(f, folds, nugget=0.0), CV.dlogpdθ_CVfold(f, folds, True, True)
        lnug = CV.logp_CVfold(f, folds)
        Fi = [i for V in folds for i in V]
        u = np.asarray(y)[Fi] - np.concatenate(CV.predict_CVfold(f, folds)[0])
        eps_share = 1e-10 * (float(np.sum(np.diag(f["invS"])[Fi])) + float(u @ u))  # first order in the nugget, with room
        assert dtype != np.float64 or abs(lp - lnug) <= eps_share, (lp, lnug, eps_share)
    _rel(gr, grr, tol, "gradient")
    assert abs(lp - lr) <= ltol * abs(lr), (lp, lr)
    return gp


def _partial_cover(n, k, seed=5):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)[: n - n // 10]  # a tenth of the points in no fold
    return [sorted(v.tolist()) for v in np.array_split(perm, k)]


@pytest.mark.parametrize("spec", SPECS, ids=KC.ids(KC.ALL) + ["periodic_x_se"])
def test_every_kernel_loo_and_folds(spec):
    d = 1 if spec is PER else KC.D  # (Periodic on the Euclidean distance is positive definite in one dimension only)
    _check_case(spec, 700, d, None)
    _check_case(spec, 700, d, _partial_cover(700, 7))


def _g_form_reference(spec, x, y, ln, folds):
    """the one-contraction form of DESIGN.md §7b in NumPy (checked against the literal checker in tests/test_cv_host.py):
    the literal form's per-parameter N^3 products are out of reach at N = 9000 on the host"""
    from oracle import gp_oracle as G
    import scipy.linalg as sla

    K, dKs = G.grad_cov(spec, x)
    n = len(y)
    K[np.diag_indices(n)] += math.exp(2 * ln)
    c, low = sla.cho_factor(K)
    W = sla.cho_solve((c, low), np.eye(n))
    a = W @ y
    folds = [[i] for i in range(n)] if folds is None else folds
    u = np.zeros(n)
    S = np.zeros((n, sum(len(V) for V in folds)))
    lp, o = 0.0, 0
    for V in folds:
        WV = W[np.ix_(V, V)]
        L = np.linalg.cholesky(WV)
        SV = np.linalg.inv(WV)
        uV = SV @ a[V]
        u[V] = uV
        BL = np.linalg.cholesky(SV + np.outer(uV, uV))
        S[:, o:o + len(V)] = W[:, V] @ BL
        o += len(V)
        lp += -0.5 * len(V) * CV.LOG2PI + np.sum(np.log(np.diag(L))) - 0.5 * float(a[V] @ uV)
    b = W @ u
    Gm = 0.5 * (np.outer(a, b) + np.outer(b, a)) - 0.5 * S @ S.T
    return lp, np.asarray([2 * math.exp(2 * ln) * np.trace(Gm)] + [float(np.sum(dK * Gm)) for dK in dKs])


@pytest.mark.parametrize("case", ["loo", "folds"])
def test_chunked_w(case):
    """N = 9000: npad >= 4 x grad_chunk, the tiles hold -W"""
    from oracle import gp_oracle as G

    spec = ("se_iso", math.log(0.3), 0.0)
    x, y, _ = G.synthetic_inputs(9000, 2, p=1, seed=11)
    ln = math.log(0.3)
    folds = None if case == "loo" else [list(range(k, 9000, 9)) for k in range(0, 8)]  # 8 folds of 1000, a ninth in none
    gp = _gp(x, y, spec, ln)
    if folds is None:
        lp, gr = loo_logp_and_grad(gp, noise=True, domean=False, kern=True)
    else:
        lp, gr = cvfold_logp_and_grad(gp, folds, noise=True, domean=False, kern=True)
    lr, grr = _g_form_reference(spec, x, y, ln, folds)
    assert abs(lp - lr) <= 1e-9 * abs(lr), (lp, lr)
    _rel(gr, grr, 1e-8, "gradient (chunked W)")


def test_fold_sizes_across_kernel_boundaries():
    sizes = [1, 15, 16, 63, 64, 65, 700, 2048]
    n = sum(sizes) + 100
    perm = np.random.default_rng(3).permutation(n)
    folds, o = [], 0
    for s in sizes:
        folds.append(sorted(perm[o:o + s].tolist()))
        o += s
    _check_case(("se_iso", math.log(0.3), 0.0), n, 2, folds)


def test_singleton_folds_equal_loo():
    from oracle import gp_oracle as G

    x, y, _ = G.synthetic_inputs(500, 3, p=1)
    gp = _gp(x, y, KC.COMPOSITES[2], math.log(0.3))
    a = loo_logp_and_grad(gp, noise=True, domean=False, kern=True)
    b = cvfold_logp_and_grad(gp, [[i] for i in range(500)], noise=True, domean=False, kern=True)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
    _rel(b[1], a[1], 1e-12, "singletons vs LOO")


def test_vector_lognoise_kern_only():
    from oracle import gp_oracle as G

    x, y, _ = G.synthetic_inputs(600, 2, p=1)
    ln = np.log(0.2 + 0.2 * np.random.default_rng(2).uniform(size=600))
    spec = ("se_iso", math.log(0.4), 0.0)
    gp = _gp(x, y, spec, ln)
    f = CV.fit(spec, x, y, ln)
    folds = _partial_cover(600, 5)
    _rel(gp.dlogpdθ_LOO(noise=False, domean=False, kern=True), CV.dlogpdθ_LOO(f, False, True), 1e-8, "LOO, vector logNoise")
    _rel(gp.dlogpdθ_CVfold(folds, noise=False, domean=False, kern=True), CV.dlogpdθ_CVfold(f, folds, False, True), 1e-8, "folds, vector logNoise")
    with pytest.raises(g.ArgumentError):
        gp.dlogpdθ_LOO(noise=True, domean=False, kern=True)


def test_fp32():
    spec = ("sum", ("se_ard", [0.1, -0.2], 0.0), ("mat52_iso", math.log(0.7), math.log(0.5)))
    for folds in (None, _partial_cover(2000, 10)):
        _check_case(spec, 2000, 2, folds, ln=math.log(0.3), dtype=np.float32, tol=2e-2, ltol=2e-2)


def test_bits_repeat_and_model_state_unchanged():
    from oracle import gp_oracle as G

    x, y, xs = G.synthetic_inputs(900, 3, p=64)
    gp = _gp(x, y, KC.COMPOSITES[3], math.log(0.3))
    mu0, v0 = gp.predict_f(xs)
    gp.update_dmll()
    d0 = gp.dmll.copy()
    folds = _partial_cover(900, 6)
    r1 = loo_logp_and_grad(gp, noise=True, domean=False, kern=True), cvfold_logp_and_grad(gp, folds, noise=True, domean=False, kern=True)
    r2 = loo_logp_and_grad(gp, noise=True, domean=False, kern=True), cvfold_logp_and_grad(gp, folds, noise=True, domean=False, kern=True)
    for a, b in zip(r1, r2):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    m1, c1 = gp.predict_CVfold(folds)
    m2, c2 = gp.predict_CVfold(folds)
    assert all(np.array_equal(p, q) for p, q in zip(m1 + c1, m2 + c2))
    mu1, v1 = gp.predict_f(xs)
    gp.update_dmll()
    assert np.array_equal(mu0, mu1) and np.array_equal(v0, v1) and np.array_equal(d0, gp.dmll)


def test_error_contract():
    from oracle import gp_oracle as G

    x, y, _ = G.synthetic_inputs(300, 2, p=1)
    k = g.SEIso(0.0, 0.0)
    fitc = g.FITC(x, x[:, ::10], y, g.MeanZero(), k, -1.0, ctx=g.Context.default(0))
    packed = g.GP(x, y, g.MeanZero(), g.SEIso(0.0, 0.0), -1.0, packed=True, block=256, stripe_blocks=2, ctx=g.Context.default(0))
    for m in (fitc, packed):
        with pytest.raises(g.ArgumentError, match="dense exact handle only"):
            g.dlogpdθ_LOO(m, noise=True, domean=False, kern=True)
        with pytest.raises(g.ArgumentError, match="dense exact handle only"):
            g.predict_CVfold(m, [[0, 1]])
    gm = g.GPE(x, y, g.MeanLin([1.0, 0.5]), g.SEIso(0.0, 0.0), -1.0, ctx=g.Context.default(0))
    with pytest.raises(g.ArgumentError, match="mean"):
        g.dlogpdθ_LOO(gm, noise=True, domean=True, kern=True)
    with pytest.raises(TypeError):
        g.dlogpdθ_LOO(gm)  # the keywords are required, as in the reference
    for bad in ([[0, 1], [1]], [[]], [[300]], [[0.5]]):
        with pytest.raises(g.ArgumentError):
            g.logp_CVfold(gm, bad)
    # the C ABI refuses the same on its own: before a fit, bad folds, s = 2049, n_kern mismatch
    import ctypes as C
    from gpmi355x import _lib

    lib = _lib.load()
    big = g.GPE(*G.synthetic_inputs(2100, 2, p=1)[:2], g.MeanZero(), g.SEIso(0.0, 0.0), -1.0, ctx=g.Context.default(0))
    ptr = np.asarray([0, 2049], dtype=np.int64)
    idx = np.arange(2049, dtype=np.int64)
    lp = C.c_double()
    rc = lib.gpmi_cvfold_predict(big.cK.h, 1, ptr.ctypes.data, idx.ctypes.data, None, None, C.byref(lp))
    assert rc == _lib.GPMI_EARG and b"2048" in lib.gpmi_last_error(big.ctx.h)
    ptr = np.asarray([0, 2, 3], dtype=np.int64)
    idx = np.asarray([0, 1, 1], dtype=np.int64)
    assert lib.gpmi_cvfold_predict(big.cK.h, 2, ptr.ctypes.data, idx.ctypes.data, None, None, C.byref(lp)) == _lib.GPMI_EARG
    kd, keep = big.kernel.descriptor(big.dim)
    ln = np.asarray([-1.0])
    dk = np.empty(3)
    dbl = C.POINTER(C.c_double)
    assert lib.gpmi_loo_grad(big.cK.h, C.byref(kd), ln.ctypes.data_as(dbl), 1, C.byref(lp), dk.ctypes.data_as(dbl), 3, None) == _lib.GPMI_EARG
    h = C.c_void_p()
    ctx = g.Context.default(0)
    ctx.check(lib.gpmi_gp_create(ctx.h, 64, 2, 100, big.x.ctypes.data, C.byref(h)))
    try:
        assert lib.gpmi_loo_grad(h, C.byref(kd), ln.ctypes.data_as(dbl), 1, C.byref(lp), dk.ctypes.data_as(dbl), 2, None) == _lib.GPMI_EARG
        assert b"gpmi_fit" in lib.gpmi_last_error(ctx.h)
    finally:
        lib.gpmi_gp_destroy(h)
    del keep
