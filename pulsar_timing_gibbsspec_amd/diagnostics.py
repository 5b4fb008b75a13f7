"""Chain diagnostics (host-side metric; the reference used the absent ``acor``,
pulsar_gibbs.py:370 and singlepulsar…ipynb:257).

``iat``: integrated autocorrelation time with Sokal's adaptive window
(smallest M with M >= c * tau(M), c = 5); ESS = n / iat.
"""
import numpy as np


def iat(x, c=5.0):
    x = np.asarray(x, float) - np.mean(x)
    n = x.size
    if n < 4:
        return 1.0
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n]
    if acf[0] <= 0:
        return 1.0
    acf /= acf[0]
    tau = 2.0 * np.cumsum(acf) - 1.0
    M = np.arange(n)
    ok = M >= c * tau
    if ok.any():
        return float(tau[np.argmax(ok)])
    return float(tau[-1])


# bench.py's ESS runs: (burn-in, recorded sweeps) per chain for each line, the same on the GPU leg and
# the CPU port's (oracle/cpu_baseline.py); recorded >= 50 x the slowest bin's IAT
# (round-6 measurement, profiles/r06a: slowest-bin IAT 29 / 65 / 72 / 261 / 159 / 41 / 42 / 57 sweeps in the
# order below)
ESS_RUN = {"single": (1000, 6000), "indep": (500, 3500), "curn": (500, 5000), "curn_red": (500, 13000),
           "curn_plred": (1000, 8000), "ecorr": (500, 3000), "ecorr_white": (500, 3000), "config5": (500, 3000)}


def pooled_iat(x, c=5.0):
    """(tau, M) of independent chains of one quantity, x: (chains, n).  Each chain's mean is
    removed, the chains' autocovariances (biased, / n) are averaged lag by lag, and tau is read
    off the pooled autocorrelation with Sokal's adaptive window (smallest M with M >= c tau(M)).
    One estimator for every leg of the bench (GPU chains and the CPU port's processes alike)."""
    x = np.atleast_2d(np.asarray(x, float))
    x = x - x.mean(axis=1, keepdims=True)
    C, n = x.shape
    if n < 4:
        return 1.0, 0
    f = np.fft.rfft(x, 2 * n, axis=1)
    acov = np.fft.irfft(f.real ** 2 + f.imag ** 2, axis=1)[:, :n].mean(axis=0)
    if acov[0] <= 0:
        return 1.0, 0
    tau = 2.0 * np.cumsum(acov / acov[0]) - 1.0
    ok = np.arange(n) >= c * tau
    M = int(np.argmax(ok)) if ok.any() else n - 1
    return float(max(tau[M], 1.0)), M


def ess_table(X, c=5.0, groups=16):
    """Per column of X (chains, n, k): the ESS per chain-sweep 1/tau of the pooled chains and its
    standard error -- the larger of (a) Sokal's asymptotic one, var(tau) = 2 (2M + 1) tau^2 / N with
    N = chains x n pooled samples (se(1/tau) = (1/tau) sqrt(2 (2M + 1) / N)), and (b) the spread over
    G = min(chains, groups) disjoint groups of chains, each group's pooled 1/tau (se = std / sqrt(G)),
    which also covers chains that visit a slowly mixing tail only now and then (for which (a), an
    asymptotic formula, reads low with few chains)."""
    X = np.asarray(X)
    C, n, k = X.shape
    out = np.empty(k)
    se = np.empty(k)
    G = min(C, groups)
    parts = np.array_split(np.arange(C), G) if G >= 3 else None
    for j in range(k):
        tau, M = pooled_iat(X[:, :, j], c)
        out[j] = 1.0 / tau
        se[j] = out[j] * np.sqrt(2.0 * (2 * M + 1) / (C * n))
        if parts is not None:
            f = np.array([1.0 / pooled_iat(X[g, :, j], c)[0] for g in parts])
            se[j] = max(se[j], float(np.std(f, ddof=1)) / np.sqrt(G))
    return out, se


def ess_summary(X, burn_in, c=5.0):
    """The bench's ESS record of X (chains, n, k) recorded after ``burn_in`` dropped sweeps: the
    worst column's ESS per chain-sweep with its standard error, and every column's."""
    e, se = ess_table(X, c)
    j = int(np.argmin(e))
    return {"per_chain_sweep_min_bin": float(e[j]), "se": float(se[j]), "bin": j, "chains": int(X.shape[0]),
            "sweeps": int(X.shape[1]), "burn_in": int(burn_in), "per_bin": [float(v) for v in e],
            "se_bin": [float(v) for v in se], "estimator": "pooled ACF over chains, Sokal window c=5"}


def ess_compare(gpu, cpu):
    """z-score of the GPU and CPU ESS per sweep at the GPU's worst column (both from ess_summary),
    and the share of columns that agree within 2 standard errors."""
    g, gs = np.array(gpu["per_bin"]), np.array(gpu["se_bin"])
    h, hs = np.array(cpu["per_bin"]), np.array(cpu["se_bin"])
    if g.shape != h.shape:
        return None
    z = (g - h) / np.sqrt(gs ** 2 + hs ** 2)
    j = int(gpu["bin"])
    return {"bin": j, "gpu": float(g[j]), "gpu_se": float(gs[j]), "cpu": float(h[j]), "cpu_se": float(hs[j]),
            "z": float(z[j]), "frac_bins_within_2se": float(np.mean(np.abs(z) < 2.0))}


def ess(chain, c=5.0):
    """Effective sample size of each column of a (n, k) chain."""
    chain = np.atleast_2d(np.asarray(chain, float))
    if chain.shape[0] == 1:
        chain = chain.T
    return np.array([chain.shape[0] / max(iat(chain[:, k], c), 1.0) for k in range(chain.shape[1])])


def summarize_chains(X, lo, hi, n_bins):
    """Host restatement of the on-device summary (engine.ChainSummary, sample(history="summary"))
    for X (chains, n, k) -- e.g. a chains.npy -- with per-column ranges lo, hi (k,).  Sums are
    accumulated in numpy long double about mid = (lo + hi) / 2:
      s1_c = sum_i (X_ci - mid), s2_c = sum_i (X_ci - mid)^2,
      m_c = mid + s1_c / n, v_c = (s2_c - s1_c^2 / n) / (n - 1),
      mean = mean_c(m_c), W = mean_c(v_c), Bn = var_c(m_c, ddof=1),
      var = sum_c s2_c / (C n) - (sum_c s1_c / (C n))^2  (pooled, ddof=0),
      rhat = sqrt(((n - 1) / n W + Bn) / W), NaN where n < 2, C < 2 or W = 0.
    counts (k, n_bins): a value v with lo <= v <= hi falls in bin min(floor((v - lo) * scale),
    n_bins - 1), scale = n_bins / (hi - lo), all in double; anything else (NaN, +-inf) counts in
    ``outside`` (k,) and still enters the sums.  Returns a dict of double / int64 arrays."""
    X = np.asarray(X, float)
    C, n, k = X.shape
    n_bins = int(n_bins)
    lo, hi = np.asarray(lo, float).reshape(k), np.asarray(hi, float).reshape(k)
    scale = n_bins / (hi - lo)
    L = np.longdouble
    mid = (lo + hi) / 2
    d = X.astype(L) - mid.astype(L)
    s1, s2 = d.sum(axis=1), (d * d).sum(axis=1)                            # (C, k)
    nan = np.full(k, np.nan)
    with np.errstate(all="ignore"):
        m_c = mid.astype(L) + s1 / L(n) if n else np.full((C, k), np.nan, L)
        v_c = (s2 - s1 * s1 / L(n)) / L(n - 1) if n > 1 else np.full((C, k), np.nan, L)
        mean, W = m_c.mean(axis=0), v_c.mean(axis=0)
        Bn = m_c.var(axis=0, ddof=1) if C > 1 else nan.astype(L)
        var = s2.sum(axis=0) / L(C * n) - (s1.sum(axis=0) / L(C * n)) ** 2 if n else nan.astype(L)
        rhat = np.sqrt((L(n - 1) / L(n) * W + Bn) / W) if n > 1 else nan.astype(L)
        rhat = np.where(W > 0, rhat, np.nan)
    counts = np.zeros((k, n_bins), np.int64)
    outside = np.zeros(k, np.int64)
    for j in range(k):
        v = X[:, :, j].ravel()
        with np.errstate(invalid="ignore"):
            inside = (v >= lo[j]) & (v <= hi[j])
        b = np.minimum(np.floor((v[inside] - lo[j]) * scale[j]).astype(np.int64), n_bins - 1)
        counts[j] = np.bincount(b, minlength=n_bins)
        outside[j] = v.size - int(inside.sum())
    f = lambda a: np.asarray(a, float)  # noqa: E731
    return dict(counts=counts, outside=outside, n=np.int64(n), mean=f(mean), var=f(var), W=f(W), Bn=f(Bn),
                rhat=f(rhat))


def acov_chains(X, max_lag):
    """Host restatement of the on-device pooled autocovariance (gs_chain_acf_block /
    gs_chain_acf_reduce, sample(history="summary", acf_lags=L)) for X (chains, n, k), in numpy long
    double: pooled_iat's estimator truncated at max_lag,
      acov[j, lag] = 1 / (C n) sum_c sum_{t=0}^{n-1-lag} (X_ctj - m_cj) (X_c,t+lag,j - m_cj),
    m_cj chain c's own mean of column j (biased, / n, averaged over the chains), and 0 for
    lag >= n.  Returns (k, max_lag + 1) doubles."""
    X = np.asarray(X, float)
    C, n, k = X.shape
    Lg = int(max_lag)
    d = X.astype(np.longdouble)
    if n:
        d = d - d.mean(axis=1, keepdims=True)
    out = np.zeros((k, Lg + 1), np.longdouble)
    for lag in range(min(Lg + 1, n)):
        out[:, lag] = (d[:, :n - lag] * d[:, lag:]).sum(axis=(0, 1)) / np.longdouble(C * n)
    return np.asarray(out, float)


def iat_from_acov(acov, c=5.0):
    """(iat, window) per parameter from acov (..., L + 1), a pooled autocovariance up to lag L
    (acov_chains, a summary.npz's ``acov``): tau(M) = 2 sum_{k <= M} acov[k] / acov[0] - 1 at the
    smallest M <= L with M >= c tau(M) (Sokal's window, as pooled_iat), clamped below at 1.  Where no
    such M exists within L the window is -1 and iat = max(tau(L), 1): a lower bound, the sum was cut
    short.  NaN (window -1) where acov[0] is not positive and finite."""
    a = np.asarray(acov, float)
    flat = a.reshape(-1, a.shape[-1])
    tau_out = np.full(flat.shape[0], np.nan)
    win = np.full(flat.shape[0], -1, np.int64)
    lags = np.arange(flat.shape[1])
    for i, row in enumerate(flat):
        if not (np.isfinite(row[0]) and row[0] > 0):
            continue
        tau = 2.0 * np.cumsum(row / row[0]) - 1.0
        ok = lags >= c * tau                   # False for a NaN tau
        if ok.any():
            win[i] = int(np.argmax(ok))
            tau_out[i] = max(tau[win[i]], 1.0)
        else:
            tau_out[i] = max(tau[-1], 1.0) if np.isfinite(tau[-1]) else np.nan
    return tau_out.reshape(a.shape[:-1]), win.reshape(a.shape[:-1])


def acf_summary(acov, n, nchains, c=5.0):
    """The keys a summary.npz gains with acf_lags, from acov (k, L + 1) over n rows of nchains
    chains: iat and iat_window (iat_from_acov), ess_per_sweep = 1 / iat, ess = nchains n / iat and
    ess_se = ess_per_sweep sqrt(2 (2 M + 1) / (nchains n)) -- Sokal's asymptotic term, (a) of
    ess_table; NaN where the window was not reached within L.  The spread over groups of chains,
    ess_table's term (b), needs the chains themselves and is not estimated."""
    tau, M = iat_from_acov(acov, c)
    N = float(nchains) * float(n)
    with np.errstate(all="ignore"):
        per = 1.0 / tau
        se = np.where(M >= 0, per * np.sqrt(2.0 * (2.0 * M + 1.0) / N), np.nan) if N > 0 else np.full_like(per, np.nan)
    return dict(acf_lags=np.int64(np.shape(acov)[-1] - 1), acov=np.asarray(acov, float), iat=tau, iat_window=M,
                ess_per_sweep=per, ess=N * per, ess_se=se)


def coef_moments(B, shift=None):
    """Host restatement of the on-device pooled coefficient moments (gs_coef_moments_block /
    gs_coef_moments_reduce, sample(history="summary", b_moments=True)) for B (chains, n, m), in numpy
    long double: with d = B - shift over the N = chains x n samples,
      mean = shift + sum d / N,   cov = sum d d^T / N - (sum d)(sum d)^T / N^2   (pooled, ddof 0).
    shift (m,): the device's rule when none is given -- chain 0's first row.  Returns a dict of n
    (int64), shift, mean (m,) and cov (m, m) as doubles; NaN mean and cov for N = 0."""
    B = np.asarray(B, float)
    C, n, m = B.shape
    N = C * n
    if shift is None:
        shift = B[0, 0] if N else np.zeros(m)
    shift = np.asarray(shift, float).reshape(m)
    if N == 0:
        return dict(n=np.int64(0), shift=shift, mean=np.full(m, np.nan), cov=np.full((m, m), np.nan))
    d = B.reshape(N, m).astype(np.longdouble) - shift.astype(np.longdouble)
    s1 = d.sum(axis=0)
    s2 = d.T @ d
    Nl = np.longdouble(N)
    mean = shift.astype(np.longdouble) + s1 / Nl
    cov = s2 / Nl - np.outer(s1, s1) / (Nl * Nl)
    return dict(n=np.int64(N), shift=shift, mean=np.asarray(mean, float), cov=np.asarray(cov, float))


def reconstruct(T, mean, cov, cols=None):
    """Posterior mean and sd, at every TOA, of the delay carried by the columns ``cols`` of the
    basis T (n_toa, m) -- e.g. a pulsar's Fourier columns -- from the pooled moments of b (a
    summary.npz's b_mean, b_cov; coef_moments): (T_c mean_c, sqrt(diag(T_c cov_cc T_c^T))), the
    diagonal taken row by row without forming the n_toa x n_toa matrix.  cols=None: every column."""
    T = np.asarray(T, float)
    mean, cov = np.asarray(mean, float), np.asarray(cov, float)
    cols = np.arange(T.shape[1]) if cols is None else np.asarray(cols, dtype=np.int64).ravel()
    Tc = T[:, cols]
    var = np.einsum("ti,ti->t", Tc @ cov[np.ix_(cols, cols)], Tc)
    return Tc @ mean[cols], np.sqrt(np.maximum(var, 0.0))


def hist_quantiles(counts, lo, hi, q):
    """Quantile(s) q of histograms counts (k, n_bins) over [lo, hi] (k,), e.g. a summary.npz's: linear
    interpolation inside the bin where the cumulative count crosses q x total (the first non-empty
    bin whose cumulative count reaches it).  Returns (k,) for a scalar q, (k, len(q)) otherwise; NaN
    for an empty histogram."""
    counts = np.atleast_2d(np.asarray(counts, float))
    k, nb = counts.shape
    lo, hi = np.broadcast_to(np.asarray(lo, float), (k,)), np.broadcast_to(np.asarray(hi, float), (k,))
    qs = np.atleast_1d(np.asarray(q, float))
    out = np.full((k, qs.size), np.nan)
    for j in range(k):
        cum = np.cumsum(counts[j])
        if cum[-1] <= 0:
            continue
        for i, qq in enumerate(qs):
            target = qq * cum[-1]
            b = int(np.searchsorted(cum, target, side="left"))
            b = min(b, nb - 1)
            while counts[j, b] == 0:           # an empty bin holds no quantile: the next filled one
                b += 1
            below = cum[b] - counts[j, b]
            out[j, i] = lo[j] + (b + (target - below) / counts[j, b]) * (hi[j] - lo[j]) / nb
    return out[:, 0] if np.ndim(q) == 0 else out


def acor(x, maxlag=10):
    """(tau, mean, sigma) of a 1-d chain: restatement of J. Goodman's ``acor``
    algorithm (PyPI ``acor`` 1.1.x, the module pulsar_gibbs.py:370-371 calls; absent
    here and unpinned by the reference): autocovariances C[0..maxlag] over the
    first L - maxlag points, D = C0 + 2 sum C[s], tau = D / C0; while
    tau * 5 >= maxlag the chain is pair-summed (length halves) and the estimate
    recomputed from the coarse chain (D = sigma^2 L / 4 with sigma from the
    recursion).  Chains shorter than 5 * maxlag return the estimate so far."""
    x = np.asarray(x, float).copy()
    return _acor(x, int(maxlag))


def _acor(x, maxlag):
    L = x.size
    mean = float(np.mean(x)) if L else 0.0
    x = x - mean
    if L < 5 * maxlag:
        return 1.0, mean, 0.0
    i_max = L - maxlag
    C = np.array([np.dot(x[:i_max], x[s:s + i_max]) for s in range(maxlag + 1)]) / i_max
    D = C[0] + 2.0 * np.sum(C[1:])
    if C[0] <= 0 or D < 0:
        return 1.0, mean, 0.0
    sigma = np.sqrt(D / L)
    tau = D / C[0]
    if tau * 5 < maxlag:
        return float(tau), mean, float(sigma)
    Lh = L // 2
    xx = x[0:2 * Lh:2] + x[1:2 * Lh:2]
    if Lh < 5 * maxlag:
        return float(tau), mean, float(sigma)
    _, _, sigma = _acor(xx, maxlag)
    D = 0.25 * sigma * sigma * L
    return float(D / C[0]), mean, float(np.sqrt(D / L))


def white_aclength(short_chain, burn=100):
    """aclength_white = max_j int(acor(short_chain[burn:, j])[0])  (pulsar_gibbs.py:370-371)."""
    sc = np.asarray(short_chain, float)[burn:]
    return int(np.max([int(acor(sc[:, j])[0]) for j in range(sc.shape[1])]))
