"""gs_chain_acf_*, the acf_lags keyword of the single-pulsar samplers and the host side of the
estimator (diagnostics.acov_chains, iat_from_acov), as far as they go without a device (CPU only)."""
import numpy as np
import pytest


def ar1(phi, C, n, seed, offset=0.0):
    """(C, n) stationary AR(1) chains of unit innovation, each with its own offset."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((C, n))
    x = np.empty((C, n))
    x[:, 0] = e[:, 0] / np.sqrt(1 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x + offset * rng.standard_normal((C, 1))


def test_entries_reject_a_null_context():
    from pulsar_timing_gibbsspec_amd import _lib
    L = _lib.load()
    assert L.gs_chain_acf_block(None, 1, 1, 1, None, 1, 1, 0, 0, 1, None, None) == 1
    assert b"ctx" in L.gs_last_error()
    assert L.gs_chain_acf_reduce(None, 1, 1, 1, 1, None, None, None) == 1
    assert b"ctx" in L.gs_last_error()


def test_state_size_counts_the_kept_values_and_rejects_bad_shapes():
    from pulsar_timing_gibbsspec_amd import _lib
    L = _lib.load()
    G, C, npar, lags = 3, 5, 30, 8
    T = G * C * npar
    size = L.gs_chain_acf_state_size(G, C, npar, lags)
    assert size >= T * (1 + 2 * lags) + (lags + 1) * G * npar      # s1, head, tail and one partial at least
    assert L.gs_chain_acf_state_size(G, C, npar, lags) == size     # the shapes alone fix it
    assert L.gs_chain_acf_state_size(0, C, npar, lags) >= 0 and L.gs_chain_acf_state_size(G, 0, npar, lags) >= 0
    for bad in ((-1, C, npar, lags), (G, -1, npar, lags), (G, C, 0, lags), (G, C, npar, 0), (G, C, npar, 4097)):
        assert L.gs_chain_acf_state_size(*bad) < 0


def test_acf_lags_is_rejected_before_anything_is_touched(tmp_path):
    from pulsar_timing_gibbsspec_amd import PulsarBlockGibbs, synthetic
    gb = PulsarBlockGibbs(synthetic.single_pulsar_pta("J1713+0747", seed=0), nchains=2, seed=5)
    d = tmp_path / "never"
    x0 = np.full(30, -6.0)
    for kw in (dict(acf_lags=4), dict(history="memory", acf_lags=4),           # without history="summary"
               dict(history="summary", acf_lags=0), dict(history="summary", acf_lags=-1),
               dict(history="summary", acf_lags=10),                           # niter - burn - 1 = 9
               dict(history="summary", burn=5, acf_lags=5),                    # niter - burn - 1 = 4
               dict(history="summary", acf_lags=4.0), dict(history="summary", acf_lags=True),
               dict(history="summary", acf_lags="4")):
        with pytest.raises(ValueError):
            gb.sample(x0, outdir=str(d), niter=10, **kw)
    with pytest.raises(ValueError):
        gb.sample(x0, outdir=str(d), niter=5000, history="summary", acf_lags=4097)
    assert not d.exists() and gb._ctx is None      # no directory, no device context


def test_acf_lags_is_rejected_by_the_array_sampler(tmp_path):
    from pulsar_timing_gibbsspec_amd import synthetic
    from pulsar_timing_gibbsspec_amd.array_gibbs import PulsarArrayGibbs
    arr = PulsarArrayGibbs(synthetic.pulsar_ptas(synthetic.array_pta(kind="indep", seed=0))[:2], nchains=2, seed=5)
    d = tmp_path / "never"
    x0 = [np.full(30, -6.0)] * 2
    for kw in (dict(acf_lags=4), dict(history="summary", acf_lags=10), dict(history="summary", acf_lags=2.0)):
        with pytest.raises(ValueError):
            arr.sample(x0, outdir=str(d), niter=10, **kw)
    assert not d.exists()


@pytest.mark.parametrize("phi", [0.5, 0.9])
def test_iat_from_acov_is_pooled_iat(phi):
    from pulsar_timing_gibbsspec_amd.diagnostics import acov_chains, iat_from_acov, pooled_iat
    C, n = 8, 4000
    X = np.stack([ar1(phi, C, n, seed=3), 0.05 * ar1(phi, C, n, seed=4, offset=2.2)], axis=2)
    tau, win = iat_from_acov(acov_chains(X, n - 1))
    assert tau.shape == (2,) and win.shape == (2,) and win.dtype == np.int64
    for j in range(2):
        t_ref, m_ref = pooled_iat(X[:, :, j])
        assert 0 < m_ref < n - 1                   # the reference found its window
        assert win[j] == m_ref
        assert abs(tau[j] - t_ref) <= 1e-9 * t_ref
        # the same window from any L that reaches it, none from a shorter one
        t2, w2 = iat_from_acov(acov_chains(X[:, :, j:j + 1], m_ref))
        assert w2[0] == m_ref and abs(t2[0] - t_ref) <= 1e-9 * t_ref
        short = acov_chains(X[:, :, j:j + 1], m_ref - 1)
        t3, w3 = iat_from_acov(short)
        tau_L = 2.0 * np.sum(short[0] / short[0, 0]) - 1.0
        assert w3[0] == -1 and abs(t3[0] - max(tau_L, 1.0)) <= 1e-12 * tau_L


def test_acov_chains_is_the_fft_autocovariance_of_pooled_iat():
    from pulsar_timing_gibbsspec_amd.diagnostics import acov_chains
    C, n = 5, 257
    X = np.stack([ar1(0.9, C, n, seed=1, offset=1.0), ar1(0.5, C, n, seed=2)], axis=2)
    got = acov_chains(X, n + 3)
    assert got.shape == (2, n + 4) and got.dtype == np.float64
    for j in range(2):
        x = X[:, :, j] - X[:, :, j].mean(axis=1, keepdims=True)            # pooled_iat's lines
        f = np.fft.rfft(x, 2 * n, axis=1)
        ref = np.fft.irfft(f.real ** 2 + f.imag ** 2, axis=1)[:, :n].mean(axis=0) / n
        assert np.max(np.abs(got[j, :n] - ref)) <= 1e-12 * ref[0]
        assert (got[j, n:] == 0).all()             # lags >= n are exactly 0


def test_iat_from_acov_edge_cases():
    from pulsar_timing_gibbsspec_amd.diagnostics import acf_summary, iat_from_acov
    acov = np.array([[1.0, 0.0, 0.0, 0.0],         # white: tau = 1 at every M, and M >= 5 lies beyond L = 3
                     [0.0, 0.0, 0.0, 0.0],         # no variance
                     [np.nan, 0.0, 0.0, 0.0],
                     [2.0, -1.0, 0.0, 0.0]])       # anticorrelated: tau(1) = 0, window 1, clamped to 1
    tau, win = iat_from_acov(acov)
    assert win.tolist() == [-1, -1, -1, 1]
    assert tau[0] == 1.0 and np.isnan(tau[1]) and np.isnan(tau[2]) and tau[3] == 1.0
    s = acf_summary(acov, n=100, nchains=4)
    assert sorted(s) == ["acf_lags", "acov", "ess", "ess_per_sweep", "ess_se", "iat", "iat_window"]
    assert int(s["acf_lags"]) == 3 and s["iat_window"].dtype == np.int64
    assert s["ess"][0] == 400.0 and s["ess_per_sweep"][3] == 1.0
    assert np.isnan(s["ess_se"][:3]).all() and s["ess_se"][3] == np.sqrt(2.0 * 3 / 400)
