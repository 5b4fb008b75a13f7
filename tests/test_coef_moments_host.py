"""diagnostics.coef_moments / reconstruct (the host restatement of gs_coef_moments_*) and the
b_moments keyword's validation: CPU only."""
import numpy as np
import pytest

from pulsar_timing_gibbsspec_amd.diagnostics import coef_moments, reconstruct


def test_coef_moments_is_the_pooled_covariance():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((5, 40, 7)) @ rng.standard_normal((7, 7)) + rng.standard_normal(7)
    r = coef_moments(B)
    flat = B.reshape(-1, 7)
    assert r["n"] == 200 and r["n"].dtype == np.int64
    assert np.array_equal(r["shift"], B[0, 0])                         # the device's rule
    assert np.allclose(r["mean"], flat.mean(axis=0), rtol=1e-13, atol=0)
    ref = np.cov(flat, rowvar=False, ddof=0)
    assert np.allclose(r["cov"], ref, rtol=0, atol=1e-13 * np.abs(ref).max())
    assert np.array_equal(r["cov"], r["cov"].T)
    other = coef_moments(B, shift=np.full(7, 0.25))                    # any shift: the same moments
    assert np.allclose(other["cov"], r["cov"], rtol=0, atol=1e-13 * np.abs(ref).max())
    assert np.allclose(other["mean"], r["mean"], rtol=1e-14, atol=0)


def test_coef_moments_reproduces_planted_moments_far_from_zero():
    """Columns many standard deviations from zero: the shift keeps the covariance."""
    rng = np.random.default_rng(1)
    m, N = 6, 4096
    sd = 10.0 ** rng.uniform(-9, -3, m)
    mean = sd * 10.0 ** rng.uniform(6, 10, m)
    z = rng.standard_normal((N, m))
    z -= z.mean(axis=0)
    q, _ = np.linalg.qr(z)                                             # exactly orthogonal columns
    L = np.linalg.cholesky(0.5 * np.eye(m) + 0.5)                      # correlation 0.5
    B = mean + (q * np.sqrt(N)) @ L.T * sd
    r = coef_moments(B.reshape(4, N // 4, m))
    planted = np.outer(sd, sd) * (0.5 * np.eye(m) + 0.5)
    # the data are doubles near `mean`: each sample carries up to half an ulp of it
    ulp = np.spacing(mean)
    assert (np.abs(r["mean"] - mean) <= ulp).all()
    assert (np.abs(r["cov"] - planted) <= 1e-12 * np.abs(planted) + 4 * np.outer(ulp, sd) + 4 * np.outer(sd, ulp)).all()
    empty = coef_moments(np.zeros((3, 0, m)))
    assert empty["n"] == 0 and np.isnan(empty["mean"]).all() and np.isnan(empty["cov"]).all()


def test_reconstruct_is_the_diagonal_of_t_c_tt():
    rng = np.random.default_rng(2)
    T = rng.standard_normal((23, 9))
    A = rng.standard_normal((9, 9))
    cov, mean = A @ A.T, rng.standard_normal(9)
    mu, sd = reconstruct(T, mean, cov)
    assert np.allclose(mu, T @ mean, rtol=1e-14) and np.allclose(sd, np.sqrt(np.diag(T @ cov @ T.T)), rtol=1e-13)
    cols = [7, 2, 3]
    mu, sd = reconstruct(T, mean, cov, cols)
    Tc = T[:, cols]
    assert mu.shape == sd.shape == (23,)
    assert np.allclose(mu, Tc @ mean[cols], rtol=1e-14)
    assert np.allclose(sd, np.sqrt(np.diag(Tc @ cov[np.ix_(cols, cols)] @ Tc.T)), rtol=1e-13)


def test_b_moments_needs_the_summary_mode():
    from pulsar_timing_gibbsspec_amd.pulsar_gibbs import summary_arguments
    args = dict(bins=None, burn=None, record_chains=None, niter=100, nchains=4, resume=False)
    assert summary_arguments("memory", **args) is None
    assert summary_arguments("memory", **args, b_moments=False) is None
    with pytest.raises(ValueError):
        summary_arguments("memory", **args, b_moments=True)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            summary_arguments("summary", **args, b_moments=bad)
    assert summary_arguments("summary", **args) == (64, 0, 1, 0, False)
    assert summary_arguments("summary", **args, b_moments=True) == (64, 0, 1, 0, True)
    with pytest.raises(NotImplementedError):
        summary_arguments("summary", **{**args, "resume": True}, b_moments=True)
