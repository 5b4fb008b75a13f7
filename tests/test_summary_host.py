"""Host side of sample(history="summary"): diagnostics.summarize_chains (the yardstick of the
device summary), diagnostics.hist_quantiles and plumbing.flat_bounds (CPU only)."""
import numpy as np

from pulsar_timing_gibbsspec_amd import plumbing
from pulsar_timing_gibbsspec_amd.diagnostics import hist_quantiles, summarize_chains


def test_summarize_chains_against_numpy():
    rng = np.random.default_rng(3)
    C, n, k, nb = 5, 40, 3, 8
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([1.0, 3.0, 2.5])
    X = lo + (hi - lo) * rng.uniform(-0.1, 1.1, (C, n, k))
    X[0, 0, 0], X[1, 1, 0], X[2, 2, 1] = lo[0], hi[0], lo[1] + 3 * (hi[1] - lo[1]) / nb    # edges
    s = summarize_chains(X, lo, hi, nb)
    assert int(s["n"]) == n and s["counts"].shape == (k, nb) and s["counts"].dtype == np.int64
    m_c, v_c = X.mean(axis=1), X.var(axis=1, ddof=1)
    w = hi - lo
    assert np.allclose(s["mean"], m_c.mean(axis=0), rtol=0, atol=1e-14 * w.max())
    assert np.allclose(s["W"], v_c.mean(axis=0), rtol=1e-12)
    assert np.allclose(s["Bn"], m_c.var(axis=0, ddof=1), rtol=1e-11)
    assert np.allclose(s["var"], X.reshape(C * n, k).var(axis=0), rtol=1e-12)
    assert np.allclose(s["rhat"], np.sqrt(((n - 1) / n * s["W"] + s["Bn"]) / s["W"]), rtol=1e-13)
    for j in range(k):
        v = X[:, :, j].ravel()
        inside = (v >= lo[j]) & (v <= hi[j])
        h, _ = np.histogram(v[inside], bins=nb, range=(lo[j], hi[j]))
        # numpy's own binning may differ from floor((v - lo) * scale) by one bin at an inner edge
        # only; none of the random values sits on one, and the planted ones are checked below
        planted = j < 2
        if not planted:
            assert np.array_equal(s["counts"][j], h)
        assert s["counts"][j].sum() == inside.sum() and s["outside"][j] == (~inside).sum()
    assert np.array_equal(s["counts"].sum(axis=1), C * n - s["outside"])
    assert (s["outside"] > 0).all()
    # the planted edges: lo in bin 0, hi in the last bin, an inner edge in the bin it opens
    one = summarize_chains(np.array([[[lo[0], hi[1], lo[2] + 3 * (hi[2] - lo[2]) / nb]]]), lo, hi, nb)
    assert one["counts"][0, 0] == 1 and one["counts"][1, nb - 1] == 1 and one["counts"][2, 3] == 1
    # non-finite values count as outside
    bad = summarize_chains(np.array([[[np.nan, np.inf, -np.inf]]]), lo, hi, nb)
    assert np.array_equal(bad["outside"], [1, 1, 1]) and not bad["counts"].any()
    assert np.isnan(bad["rhat"]).all()            # n < 2


def test_rhat_of_iid_and_shifted_chains():
    """R-hat is about 1 for 12 i.i.d. chains and above 1.5 with one chain shifted by 3 sigma.
    The shift of one chain out of C adds 9 / C to Bn (W = 1), so R-hat -> sqrt(1 + 9 / C): 1.32 for
    all 12 chains -- the definition itself keeps it below 1.5 there -- and 1.80 for 4 of them, the
    case the 1.5 bound is asserted on."""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((12, 2000, 2))
    lo, hi = np.full(2, -8.0), np.full(2, 8.0)
    r = summarize_chains(X, lo, hi, 32)["rhat"]
    assert np.all(np.abs(r - 1) < 0.01), r
    X[3, :, 1] += 3.0
    r = summarize_chains(X[:4], lo, hi, 32)["rhat"]
    assert abs(r[0] - 1) < 0.01 and r[1] > 1.5, r
    r = summarize_chains(X, lo, hi, 32)["rhat"]
    assert abs(r[0] - 1) < 0.01 and abs(r[1] - np.sqrt(1 + 9 / 12)) < 0.02, r
    assert np.isnan(summarize_chains(X[:1], lo, hi, 32)["rhat"]).all()        # one chain: no R-hat
    assert np.isnan(summarize_chains(np.zeros((3, 10, 2)), lo, hi, 32)["rhat"]).all()   # W = 0


def test_hist_quantiles_known_histogram():
    counts = np.array([[1, 1, 1, 1], [0, 4, 0, 4], [0, 0, 0, 0]])
    lo, hi = np.array([0.0, 10.0, 0.0]), np.array([4.0, 18.0, 1.0])
    q = hist_quantiles(counts, lo, hi, 0.5)
    assert q.shape == (3,)
    assert q[0] == 2.0 and q[1] == 14.0 and np.isnan(q[2])
    q = hist_quantiles(counts, lo, hi, [0.0, 0.125, 0.75, 1.0])
    assert q.shape == (3, 4)
    assert np.allclose(q[0], [0.0, 0.5, 3.0, 4.0], rtol=0, atol=1e-15)
    # bins of width 2 over [10, 18]; the mass sits in [12, 14] and [16, 18]
    assert np.allclose(q[1], [12.0, 12.5, 17.0, 18.0], rtol=0, atol=1e-14)
    # a 95 % upper limit of a flat histogram
    assert np.isclose(hist_quantiles(np.ones((1, 20)), [0.0], [1.0], 0.95)[0], 0.95)


def test_flat_bounds_of_a_facade_pta():
    from pulsar_timing_gibbsspec_amd import synthetic
    pta = synthetic.array_pta(kind="curn_plred", n_psr=4, seed=2)
    names = plumbing.expand_names(pta.params)
    lo, hi = plumbing.flat_bounds(pta.params)
    assert lo.shape == hi.shape == (len(names),) and (hi > lo).all()
    gw = [i for i, n in enumerate(names) if "gw" in n]
    assert len(gw) == 30
    assert len({(lo[i], hi[i]) for i in gw}) == 1            # the vector parameter repeats one pair
    for p in pta.params:
        i = names.index(p.name) if not p.size else names.index(p.name + "_0")
        assert (lo[i], hi[i]) == plumbing.uniform_bounds(p)
    amp = [i for i, n in enumerate(names) if n.endswith("log10_A")]
    gam = [i for i, n in enumerate(names) if n.endswith("gamma")]
    assert len(amp) == 4 and len(gam) == 4
    assert {(lo[i], hi[i]) for i in amp}.isdisjoint({(lo[i], hi[i]) for i in gam})
    assert (lo[gw[0]], hi[gw[0]]) not in {(lo[i], hi[i]) for i in gam}
