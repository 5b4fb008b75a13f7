"""PulsarBlockGibbs.sample / PulsarArrayGibbs.sample(history="summary") against
diagnostics.summarize_chains of a default-mode run of the same seed."""
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NITER, SAVE, NCH, BURN, BINS = 230, 100, 6, 37, 16
KEYS = ["Bn", "W", "burn", "counts", "hi", "lo", "mean", "n", "n_bins", "names", "nchains", "outside", "rhat",
        "rows", "var"]


def _keep_copies(sampler, copies):
    """Wrap a sampler's write helper: keep every summary.npz it writes, by its rows."""
    write = sampler._write_summary

    def hook(outdir, summary):
        write(outdir, summary)
        copy = f"{outdir}/summary_{int(summary['rows'])}.npz"
        shutil.copy(f"{outdir}/summary.npz", copy)
        copies[int(summary["rows"])] = copy
    sampler._write_summary = hook


class Runs:
    """The runs of the J1713-style single pulsar, each made once and shared by the tests."""

    def __init__(self, root):
        from pulsar_timing_gibbsspec_amd import plumbing, synthetic
        self.root = root
        self.pta = synthetic.single_pulsar_pta("J1713+0747", seed=0)
        self.x0 = np.random.default_rng(17).uniform(-8.5, -4.5, 30)
        self.lo, self.hi = plumbing.flat_bounds(self.pta.params)
        self.done = {}

    def new(self):
        from pulsar_timing_gibbsspec_amd import PulsarBlockGibbs
        return PulsarBlockGibbs(self.pta, nchains=NCH, seed=5)

    def run(self, name, **kw):
        if name not in self.done:
            gb = self.new()
            d = self.root / name
            copies = {}
            if kw.get("history") == "summary":
                _keep_copies(gb, copies)
            chain = gb.sample(self.x0, outdir=str(d), niter=NITER, save_every=SAVE, **kw)
            self.done[name] = dict(dir=d, chain=np.array(chain), gb=gb, copies=copies)
        return self.done[name]

    def all_chains(self):                          # run A
        return self.run("A")

    def summary(self):                             # run B
        return self.run("B", history="summary", burn=BURN, bins=BINS)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("j1713"))


def _check_summary(s, ref, lo, hi, names, rows, n, nch=NCH):
    """tests/test_gpu_summary.py's _check_summary: the same tolerances."""
    w = hi - lo
    assert (ref["W"] > 0).all()                    # so R-hat is compared in every column (seed 5)
    assert int(s["rows"]) == rows and int(s["n"]) == n == int(ref["n"])
    assert int(s["burn"]) == BURN and int(s["n_bins"]) == BINS and int(s["nchains"]) == nch
    assert list(s["names"]) == list(names)
    assert np.array_equal(s["lo"], lo) and np.array_equal(s["hi"], hi)
    assert s["counts"].dtype == np.int64 and s["outside"].dtype == np.int64
    assert s["counts"].shape == (len(lo), BINS) and s["outside"].shape == (len(lo),)
    assert np.array_equal(s["counts"], ref["counts"]) and np.array_equal(s["outside"], ref["outside"])
    fig = {k: float(np.max(np.abs(s[k] - ref[k]) / w ** (1 if k == "mean" else 2))) for k in ("mean", "var", "W", "Bn")}
    fig["rhat"] = float(np.max(np.abs(s["rhat"] / ref["rhat"] - 1)))
    print(f"rows {rows}: max scaled error {fig}")
    assert (np.abs(s["mean"] - ref["mean"]) <= 1e-13 * w).all()
    for k in ("var", "W", "Bn"):
        assert (np.abs(s[k] - ref[k]) <= 1e-11 * w ** 2).all(), k
    assert (np.abs(s["rhat"] - ref["rhat"]) <= 1e-8 * np.abs(ref["rhat"])).all()


def test_files_are_those_of_the_default_mode(runs):
    a, b = runs.all_chains(), runs.summary()
    assert a["gb"].chains.shape == (NCH, NITER, 30)
    for f in ("chain.npy", "bchain.npy"):
        assert (b["dir"] / f).read_bytes() == (a["dir"] / f).read_bytes(), f
    assert np.array_equal(b["chain"], a["chain"]) and np.array_equal(b["gb"].bchain, a["gb"].bchain)
    assert b["gb"].chains is None and not (b["dir"] / "chains.npy").exists()
    assert (a["dir"] / "chains.npy").exists()


def test_final_summary_matches_the_recorded_chains(runs):
    from pulsar_timing_gibbsspec_amd.diagnostics import summarize_chains
    a, b = runs.all_chains(), runs.summary()
    ref = summarize_chains(a["gb"].chains[:, BURN:NITER], runs.lo, runs.hi, BINS)
    s = dict(np.load(b["dir"] / "summary.npz"))
    assert sorted(s) == KEYS
    _check_summary(s, ref, runs.lo, runs.hi, b["gb"].param_names, rows=NITER, n=NITER - BURN)
    assert int(s["rows"]) == 230 and int(s["n"]) == 193
    assert sorted(b["gb"].summary) == sorted(s)
    for k in s:
        assert np.array_equal(b["gb"].summary[k], s[k], equal_nan=s[k].dtype.kind == "f"), k
    assert not (b["dir"] / "summary.npz.tmp").exists()


def test_save_point_summary_matches_the_recorded_chains(runs):
    """summary.npz as it stood at the save point of row 200 covers rows [burn, 200]."""
    from pulsar_timing_gibbsspec_amd.diagnostics import summarize_chains
    a, b = runs.all_chains(), runs.summary()
    assert sorted(b["copies"]) == [101, 201, NITER]
    ref = summarize_chains(a["gb"].chains[:, BURN:201], runs.lo, runs.hi, BINS)
    _check_summary(dict(np.load(b["copies"][201])), ref, runs.lo, runs.hi, b["gb"].param_names, rows=201,
                   n=201 - BURN)


def test_record_chains_keeps_the_first_chains(runs):
    a = runs.all_chains()
    c = runs.run("C", history="summary", burn=BURN, bins=BINS, record_chains=3, flush_final=True)
    assert c["gb"].chains.shape == (3, NITER, 30) and np.array_equal(c["gb"].chains, a["gb"].chains[:3])
    saved = np.load(c["dir"] / "chains.npy")
    assert saved.shape == (3, NITER, 30) and np.array_equal(saved, a["gb"].chains[:3])
    assert np.array_equal(c["chain"], a["chain"])
    b = runs.summary()                             # what reaches the host does not touch the summary
    for k in ("counts", "outside", "mean", "var", "W", "Bn", "rhat"):
        assert np.array_equal(c["gb"].summary[k], b["gb"].summary[k]), k


def test_pulsar_array_keeps_a_summary_per_pulsar(tmp_path):
    from pulsar_timing_gibbsspec_amd import plumbing, synthetic
    from pulsar_timing_gibbsspec_amd.array_gibbs import PulsarArrayGibbs
    from pulsar_timing_gibbsspec_amd.diagnostics import summarize_chains
    ptas = synthetic.pulsar_ptas(synthetic.array_pta(kind="indep", seed=0))[:3]
    x0 = [np.random.default_rng(p).uniform(-8.5, -4.5, 30) for p in range(3)]
    a = PulsarArrayGibbs(ptas, nchains=5, seed=5)
    a.sample(x0, outdir=str(tmp_path / "a"), niter=NITER, save_every=SAVE)
    b = PulsarArrayGibbs(ptas, nchains=5, seed=5)
    b.sample(x0, outdir=str(tmp_path / "b"), niter=NITER, save_every=SAVE, history="summary", burn=BURN, bins=BINS)
    refs = []
    for sa, sb in zip(a.samplers, b.samplers):
        lo, hi = plumbing.flat_bounds(sb.params)
        assert sa.chains.shape == (5, NITER, 30) and sb.chains is None
        assert np.array_equal(sb.chain, sa.chain) and np.array_equal(sb.bchain, sa.bchain)
        da, db = tmp_path / "a" / sa.pulsar_name, tmp_path / "b" / sb.pulsar_name
        for f in ("chain.npy", "bchain.npy"):
            assert (db / f).read_bytes() == (da / f).read_bytes(), f
        assert not (db / "chains.npy").exists() and not (db / "summary.npz.tmp").exists()
        ref = summarize_chains(sa.chains[:, BURN:NITER], lo, hi, BINS)
        s = dict(np.load(db / "summary.npz"))
        _check_summary(s, ref, lo, hi, sb.param_names, rows=NITER, n=NITER - BURN, nch=5)
        for k in s:
            assert np.array_equal(sb.summary[k], s[k], equal_nan=s[k].dtype.kind == "f"), k
        refs.append(ref)
    # a pulsar's counts are its own: the references differ from one another
    assert not np.array_equal(refs[0]["counts"], refs[1]["counts"])
    assert not np.array_equal(refs[1]["counts"], refs[2]["counts"])


def _raises_and_leaves(exc, call, d):
    with pytest.raises(exc):
        call()
    assert not d.exists()                          # nothing was touched


def test_rejected_sample_arguments(runs, tmp_path):
    from pulsar_timing_gibbsspec_amd import PulsarBlockGibbs, synthetic
    from pulsar_timing_gibbsspec_amd.array_gibbs import PulsarArrayGibbs
    d = tmp_path / "never"
    gb = runs.new()
    arr = PulsarArrayGibbs(synthetic.pulsar_ptas(synthetic.array_pta(kind="indep", seed=0))[:2], nchains=NCH, seed=5)
    samplers = ((gb, runs.x0), (arr, [runs.x0, runs.x0]))
    for s, x0 in samplers:
        go = lambda **kw: s.sample(x0, outdir=str(d), niter=NITER, save_every=SAVE, **kw)   # noqa: E731
        for kw in (dict(history="nope"), dict(history="disk"),
                   dict(bins=8), dict(burn=3), dict(history="memory", bins=8), dict(history="memory", burn=3),
                   dict(bins=64), dict(burn=0), dict(record_chains=1),     # given at all, even at the defaults
                   dict(history="summary", bins=0), dict(history="summary", bins=257),
                   dict(history="summary", bins=8.0), dict(history="summary", bins=True),
                   dict(history="summary", burn=NITER), dict(history="summary", burn=-1),
                   dict(history="summary", record_chains=0), dict(history="summary", record_chains=NCH + 1)):
            _raises_and_leaves(ValueError, lambda: go(**kw), d)
        _raises_and_leaves(NotImplementedError, lambda: go(history="summary", resume=True), d)
    # the models that take the red, ECORR and white sample loops
    others = (synthetic.single_pulsar_pta("J1713+0747", seed=0, powerlaw_red=True),
              synthetic.ecorr_pulsar_pta(seed=0),
              synthetic.single_pulsar_pta("J1713+0747", seed=0, efac_vary=True))
    for pta, loop in zip(others, ("_red_loop", "_ecorr_loop", "_white_loop")):
        other = PulsarBlockGibbs(pta, nchains=2, seed=5)
        assert getattr(other, loop)()
        x0 = np.concatenate([np.atleast_1d(p.sample()).ravel() for p in other.params])
        _raises_and_leaves(NotImplementedError,
                           lambda: other.sample(x0, outdir=str(d), niter=NITER, save_every=SAVE, history="summary"), d)
