"""PulsarBlockGibbs.sample / PulsarArrayGibbs.sample(history="summary", acf_lags=L) against
diagnostics.acov_chains and pooled_iat of a default-mode run of the same seed.  Pattern and sizes:
tests/test_gpu_pulsar_summary.py."""
import numpy as np
import pytest

from tests.test_gpu_pulsar_summary import BINS, BURN, KEYS, NCH, NITER, SAVE, Runs

pytestmark = pytest.mark.gpu

LAGS = NITER - BURN - 1                            # 192 = n - 1: every lag the rows have
ACF_KEYS = ["acf_lags", "acov", "ess", "ess_per_sweep", "ess_se", "iat", "iat_window"]
TOL = 1e-9


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("j1713_acf"))


def _b(runs):                                      # run B
    return runs.run("B", history="summary", burn=BURN, bins=BINS, acf_lags=LAGS)


def _c(runs):                                      # run C
    return runs.run("C", history="summary", burn=BURN, bins=BINS, acf_lags=48)


def _check_acov(s, chains, lags, nch=NCH):
    from pulsar_timing_gibbsspec_amd.diagnostics import acov_chains
    ref = acov_chains(chains, lags)
    assert (ref[:, 0] > 0).all()
    assert int(s["acf_lags"]) == lags and s["acf_lags"].dtype == np.int64
    assert s["acov"].shape == (chains.shape[2], lags + 1) and s["acov"].dtype == np.float64
    print(f"max |acov - ref| / ref[0] = {np.max(np.abs(s['acov'] - ref) / ref[:, :1]):.3e}")
    assert (np.abs(s["acov"] - ref) <= TOL * ref[:, :1]).all()
    n = chains.shape[1]
    assert np.array_equal(s["ess_per_sweep"], 1.0 / s["iat"])
    assert np.allclose(s["ess"], nch * n / s["iat"], rtol=1e-15)
    assert s["iat_window"].dtype == np.int64 and (s["iat"] >= 1).all()
    return ref


def test_summary_holds_the_pooled_autocovariance_and_the_iat(runs):
    from pulsar_timing_gibbsspec_amd.diagnostics import pooled_iat
    a, b = runs.all_chains(), _b(runs)
    s = dict(np.load(b["dir"] / "summary.npz"))
    assert sorted(s) == sorted(KEYS + ACF_KEYS)
    chains = a["gb"].chains[:, BURN:NITER]
    _check_acov(s, chains, LAGS)
    ref = [pooled_iat(chains[:, :, j]) for j in range(30)]
    same = np.array([int(s["iat_window"][j]) == M for j, (_, M) in enumerate(ref)])
    print(f"windows: device {s['iat_window'].tolist()}, pooled_iat {[M for _, M in ref]}")
    assert same.sum() >= 29                        # a window decision can tie within rounding
    for j in np.nonzero(same)[0]:
        tau, M = ref[j]
        assert abs(s["iat"][j] - tau) <= 1e-8 * tau, j
        assert s["ess_se"][j] == s["ess_per_sweep"][j] * np.sqrt(2.0 * (2 * M + 1) / (NCH * (NITER - BURN)))
    assert sorted(b["gb"].summary) == sorted(s)
    for k in s:
        assert np.array_equal(b["gb"].summary[k], s[k], equal_nan=s[k].dtype.kind == "f"), k


def test_save_point_copy_covers_the_rows_so_far(runs):
    a, b = runs.all_chains(), _b(runs)
    assert sorted(b["copies"]) == [101, 201, NITER]
    s = dict(np.load(b["copies"][201]))
    assert int(s["rows"]) == 201 and int(s["n"]) == 201 - BURN
    ref = _check_acov(s, a["gb"].chains[:, BURN:201], LAGS)
    assert (ref[:, 201 - BURN:] == 0).all() and (s["acov"][:, 201 - BURN:] == 0).all()    # lags >= n


def test_chain_files_are_those_of_the_default_mode(runs):
    a, b = runs.all_chains(), _b(runs)
    for f in ("chain.npy", "bchain.npy"):
        assert (b["dir"] / f).read_bytes() == (a["dir"] / f).read_bytes(), f
    assert np.array_equal(b["chain"], a["chain"]) and b["gb"].chains is None


def test_the_other_summary_keys_do_not_move(runs):
    """What acf_lags adds is added beside the summary: every other key is the plain mode's."""
    b = _b(runs)
    plain = runs.run("plain", history="summary", burn=BURN, bins=BINS)
    assert sorted(plain["gb"].summary) == KEYS
    for k in KEYS:
        v = np.asarray(plain["gb"].summary[k])
        assert np.array_equal(b["gb"].summary[k], v, equal_nan=v.dtype.kind == "f"), k


def test_a_shorter_lag_range_is_the_same_estimate_cut_short(runs):
    b, c = _b(runs), _c(runs)
    sb, sc = b["gb"].summary, c["gb"].summary
    assert int(sc["acf_lags"]) == 48 and sc["acov"].shape == (30, 49)
    assert (np.abs(sc["acov"] - sb["acov"][:, :49]) <= TOL * sb["acov"][:, :1]).all()
    beyond = sb["iat_window"] > 48
    print(f"windows of B: {sb['iat_window'].tolist()}")
    assert (sc["iat_window"][beyond] == -1).all() and np.isnan(sc["ess_se"][beyond]).all()
    within = (sb["iat_window"] >= 0) & (sb["iat_window"] <= 48)
    assert np.array_equal(sc["iat_window"][within], sb["iat_window"][within])
    assert np.isfinite(sc["iat"]).all() and (sc["iat"] >= 1).all()


def test_pulsar_array_keeps_an_autocovariance_per_pulsar(tmp_path):
    from pulsar_timing_gibbsspec_amd import synthetic
    from pulsar_timing_gibbsspec_amd.array_gibbs import PulsarArrayGibbs
    ptas = synthetic.pulsar_ptas(synthetic.array_pta(kind="indep", seed=0))[:3]
    x0 = [np.random.default_rng(p).uniform(-8.5, -4.5, 30) for p in range(3)]
    a = PulsarArrayGibbs(ptas, nchains=5, seed=5)
    a.sample(x0, outdir=str(tmp_path / "a"), niter=NITER, save_every=SAVE)
    b = PulsarArrayGibbs(ptas, nchains=5, seed=5)
    b.sample(x0, outdir=str(tmp_path / "b"), niter=NITER, save_every=SAVE, history="summary", burn=BURN, bins=BINS,
             acf_lags=64)
    refs = []
    for sa, sb in zip(a.samplers, b.samplers):
        assert np.array_equal(sb.chain, sa.chain) and np.array_equal(sb.bchain, sa.bchain)
        s = dict(np.load(tmp_path / "b" / sb.pulsar_name / "summary.npz"))
        assert sorted(s) == sorted(KEYS + ACF_KEYS)
        refs.append(_check_acov(s, sa.chains[:, BURN:NITER], 64, nch=5))
        for k in s:
            assert np.array_equal(sb.summary[k], s[k], equal_nan=s[k].dtype.kind == "f"), k
    # a pulsar's autocovariance is its own
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
