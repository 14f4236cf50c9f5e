"""Periodic kernel, host side (no GPU): the Python type (src/kernels/periodic.jl), its descriptor in the C ABI
(include/gpmi.h GPMI_K_PERIODIC), the Julia shim's dispatch, and the NumPy checker the GPU tests compare with
(tests/periodic_checker.py) — against scikit-learn's ExpSineSquared and against finite differences of itself."""
import math
import os
import re

import numpy as np
import pytest

import gpmi355x as g
from gpmi355x import kernels as gk
import periodic_checker as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_periodic_fields_and_param_round_trip():
    k = g.Periodic(0.3, -0.2, 0.7)
    assert k.l2 == pytest.approx(math.exp(0.6), rel=1e-15)
    assert k.s2 == pytest.approx(math.exp(-0.4), rel=1e-15)
    assert k.p == pytest.approx(math.exp(0.7), rel=1e-15)
    np.testing.assert_allclose(k.get_params(), [0.3, -0.2, 0.7], rtol=0, atol=1e-15)
    assert k.num_params() == 3
    k.set_params([-1.0, 0.5, 2.0])
    np.testing.assert_allclose(k.get_params(), [-1.0, 0.5, 2.0], rtol=0, atol=1e-15)
    assert type(g.from_spec(("periodic", 0.1, 0.2, 0.3))) is g.Periodic


@pytest.mark.parametrize("n", [2, 4])
def test_periodic_argument_error(n):
    with pytest.raises(g.ArgumentError, match=f"Periodic function has three parameters, received {n}."):
        g.Periodic(0.0, 0.0, 0.0).set_params([0.0] * n)


def test_periodic_descriptor_in_tree_order():
    """op 13, stored fields [ℓ2, σ2, p], in postfix order inside Sum / Prod / Masked (the Mauna Loa tree of
    docs/src/mauna_loa.md plus a Masked leaf)."""
    k = g.SEIso(4.0, 4.0) + g.Periodic(0.0, 1.0, 0.0) * g.SEIso(4.0, 0.0) + g.RQIso(0.0, 0.0, -1.0) \
        + g.Masked(g.Periodic(0.2, -0.1, math.log(0.5)), [1])
    ops, dims_off, dims, params = k.flat(2)
    assert ops == [1, 13, 1, 101, 100, 9, 100, 13, 100]
    assert dims == [1] and dims_off == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    e = math.exp
    want = [e(8.0), e(8.0), 1.0, e(2.0), 1.0, e(8.0), 1.0, 1.0, 1.0, e(-1.0), e(0.4), e(-0.2), 0.5]
    np.testing.assert_allclose(params, want, rtol=1e-15)
    assert k.num_params() == 13
    np.testing.assert_allclose(k.get_params()[-3:], [0.2, -0.1, math.log(0.5)], rtol=1e-15)
    # Fixed exposes a subset; the descriptor still carries the whole leaf
    f = g.fix(g.Periodic(0.1, 0.2, 0.3), 2)
    assert f.get_params() == pytest.approx([0.1, 0.2]) and f.flat(1)[0] == [13]


def test_op_table_matches_the_c_enum():
    src = open(os.path.join(ROOT, "include", "gpmi.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"GPMI_K_(\w+)\s*=\s*(\d+)", src)}
    c_name = {"SEIso": "SE_ISO", "SEArd": "SE_ARD", "Mat12Iso": "MAT12_ISO", "Mat12Ard": "MAT12_ARD", "Mat32Iso": "MAT32_ISO",
              "Mat32Ard": "MAT32_ARD", "Mat52Iso": "MAT52_ISO", "Mat52Ard": "MAT52_ARD", "RQIso": "RQ_ISO", "RQArd": "RQ_ARD",
              "Noise": "NOISE", "Const": "CONST", "Periodic": "PERIODIC"}
    assert set(gk.OP) == set(c_name)
    for py, c in c_name.items():
        assert gk.OP[py] == enum[c], py
    assert gk.OP_SUM == enum["SUM"] and gk.OP_PROD == enum["PROD"]


def test_julia_shim_flattens_periodic_to_op_13():
    src = open(os.path.join(ROOT, "gaussianprocesses.jl_amd", "julia", "GPMI355X.jl")).read()
    assert re.search(r"flatten!\(kd, k::Periodic, a\)\s*=\s*leaf!\(kd, 13, a, \[k\.ℓ2, k\.σ2, k\.p\]\)", src)


def test_checker_matches_scikit_learn():
    """σ2 · ExpSineSquared(ℓ, p) is the same function: exp(−2 sin²(π d/p) / ℓ²)."""
    kernels = pytest.importorskip("sklearn.gaussian_process.kernels")
    rng = np.random.default_rng(5)
    for d, ell, per, s2 in [(1, 0.7, 1.3, 2.0), (3, 1.9, 0.4, 0.5)]:
        X, X2 = rng.uniform(-4, 4, (d, 60)), rng.uniform(-4, 4, (d, 45))
        ref = s2 * kernels.ExpSineSquared(length_scale=ell, periodicity=per)(X.T, X2.T)
        K = P.periodic_leaf(math.log(ell), 0.5 * math.log(s2), math.log(per), X, X2)
        np.testing.assert_allclose(K, ref, rtol=0, atol=1e-13 * s2)  # (the two distances round differently: π r/p up to ~60)


def test_checker_composes_with_the_oracle():
    """Trees without a Periodic leaf go to the oracle unchanged; Sum / Prod / Masked around one compose as the oracle's do."""
    from oracle import gp_oracle as G

    rng = np.random.default_rng(6)
    X = rng.uniform(0, 3, (2, 30))
    se = ("se_iso", 0.2, 0.1)
    np.testing.assert_array_equal(P.cov(("sum", se, ("rq_iso", 0.0, 0.0, -1.0)), X), G.cov(("sum", se, ("rq_iso", 0.0, 0.0, -1.0)), X))
    per = ("periodic", 0.1, -0.3, 0.4)
    Kp = P.periodic_leaf(0.1, -0.3, 0.4, X[[1], :], X[[1], :])
    np.testing.assert_allclose(P.cov(("prod", ("masked", per, [1]), se), X), Kp * G.cov(se, X), rtol=1e-15)
    assert P.kdiag(("sum", ("prod", per, se), ("const", 0.3))) == pytest.approx(math.exp(-0.6) * math.exp(0.2) + math.exp(0.6))


def test_checker_gradient_against_finite_differences():
    """The analytic ∂K/∂θ the GPU gradient tests compare with (periodic.jl:48-64 and the oracle's leaves) against central
    differences of the checker's own covariance, over the Mauna Loa tree with a Masked Periodic."""
    rng = np.random.default_rng(7)
    X = rng.uniform(0, 6, (2, 25))
    spec = ("sum", ("sum", ("se_iso", 0.4, 0.3), ("prod", ("periodic", 0.1, 0.2, -0.3), ("se_iso", 0.9, 0.0))),
            ("masked", ("periodic", -0.2, 0.1, 0.5), [1]))
    h0 = np.array(P.get_params(spec))
    _, dK = P.grad_cov(spec, X)
    assert len(dK) == P.num_params(spec) == len(h0) == 10
    eps = 1e-6
    for i in range(len(h0)):
        hp, hm = h0.copy(), h0.copy()
        hp[i] += eps
        hm[i] -= eps
        fd = (P.cov(P.with_params(spec, hp), X) - P.cov(P.with_params(spec, hm), X)) / (2 * eps)
        np.testing.assert_allclose(dK[i], fd, rtol=0, atol=1e-7 * max(1.0, np.abs(fd).max()), err_msg=f"parameter {i}")


def test_mauna_loa_fixture_and_checker_anchor():
    """tests/golden/mauna_loa_co2.csv (the reference's notebooks/data/CO2_data.csv): 682 monthly rows, 550 before 2004; the
    checker's mll at the notebook's initial parameters is −228.566186683 (computed with NumPy; cond(K + σn²I) ≈ 8.5e7,
    so the anchor is rel 1e-9)."""
    data = np.loadtxt(os.path.join(ROOT, "tests", "golden", "mauna_loa_co2.csv"), delimiter=",")
    assert data.shape == (682, 2)
    yr, co2 = data[:, 0], data[:, 1]
    assert (yr < 2004).sum() == 550 and (yr >= 2004).sum() == 132
    spec = ("sum", ("sum", ("sum", ("se_iso", 4.0, 4.0), ("prod", ("periodic", 0.0, 1.0, 0.0), ("se_iso", 4.0, 0.0))),
                    ("rq_iso", 0.0, 0.0, -1.0)), ("se_iso", -2.0, -2.0))
    fit = P.update_mll(spec, yr[yr < 2004][None, :], co2[yr < 2004], -2.0)
    assert abs(fit["mll"] - (-228.56618668265037)) <= 1e-9 * 228.57
