"""gs_chain_summary through the C-ABI against numpy, and PTABlockGibbs.sample(history="summary")
against diagnostics.summarize_chains of a history="disk" run of the same seed."""
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ the kernel, through the C-ABI
# (n_chain, n_param, n_rows, n_bins, padding of a row): parameter counts on both sides of a 64-lane
# tile, chain counts that are no multiple of a strip, the largest table; the last shape has more
# chains than workgroups the launcher aims at (256), so a thread owns several chains (strips of 20:
# two batches of its four chains in flight, the second partial, and a last strip of 3 chains)
SHAPES = [(1, 1, 1, 1, 0), (6, 38, 1, 64, 0), (5, 65, 3, 7, 3), (130, 150, 2, 256, 0), (5003, 3, 2, 5, 1)]
EDGES = (1, 2, 3, 5, 6, 17, 63, 128, 255)


def _tables(npar, nb, seed):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-10.0, -4.0, npar) + np.arange(npar) * 1e-3          # distinct per parameter
    hi = lo + rng.uniform(0.5, 6.0, npar)
    return lo, hi, nb / (hi - lo), (lo + hi) / 2


def _data(C, npar, n_rows, nb, pad, lo, hi, seed):
    """Rows uniform in [lo - 0.1 w, hi + 0.1 w] with lo, hi, bin edges, NaN and +-inf planted where
    the shape has room; returns the padded (n_rows, stride) block (padding: NaN)."""
    rng = np.random.default_rng(seed)
    w = hi - lo
    x = lo - 0.1 * w + 1.2 * w * rng.random((n_rows, C, npar))
    cols = x.reshape(n_rows * C, npar)     # a view: column j holds parameter j's n_rows x C values
    room = n_rows * C - 1                  # one value per column stays random
    bad = dict(zip(rng.permutation(npar)[:3].tolist(), (np.nan, np.inf, -np.inf))) if npar >= 3 else {}
    for j in range(npar):
        vals = [lo[j], hi[j]] + [lo[j] + k * (hi[j] - lo[j]) / nb for k in EDGES if k < nb]
        slots = rng.permutation(n_rows * C)
        m = min(len(vals), room)
        cols[slots[:m], j] = vals[:m]
        if j in bad:
            cols[slots[m], j] = bad[j]
    block = np.full((n_rows, C * npar + pad), np.nan)
    block[:, :C * npar] = x.reshape(n_rows, -1)
    return x, block


class Host:
    """The definitions of include/pulsar_gibbs.h evaluated by numpy on the same rows."""

    def __init__(self, C, npar, nb, lo, hi, scale, mid):
        self.nb, self.lo, self.hi, self.scale, self.mid = nb, lo, hi, scale, mid
        self.s1 = np.zeros((C, npar))
        self.s2 = np.zeros((C, npar), np.longdouble)
        self.sq = np.zeros((C, npar), np.longdouble)          # sum of d^2 (the bound's scale)
        self.counts = np.zeros((npar, nb), np.int64)
        self.outside = np.zeros(npar, np.int64)
        self.n = 0
        self.finite = np.ones((C, npar), bool)

    def add(self, row):
        with np.errstate(invalid="ignore", over="ignore"):
            d = row - self.mid
            self.s1 = self.s1 + d                              # sequential, in double
            dl = d.astype(np.longdouble)
            self.s2 += dl * dl
            self.sq += dl * dl
            self.finite &= np.isfinite(row)
            inside = (row >= self.lo) & (row <= self.hi)
            k = np.minimum(np.floor((row - self.lo) * self.scale), self.nb - 1)
        jj = np.broadcast_to(np.arange(row.shape[1]), row.shape)
        np.add.at(self.counts, (jj[inside], k[inside].astype(np.int64)), 1)
        self.outside += (~inside).sum(axis=0)
        self.n += 1


class Dev:
    def __init__(self, ctx, C, npar, nb, lo, hi, scale, mid):
        dev = ctx.device
        self.ctx, self.C, self.npar, self.nb = ctx, C, npar, nb
        t = lambda a: torch.as_tensor(a, dtype=torch.float64).to(dev)   # noqa: E731
        self.tab = [t(lo), t(hi), t(scale), t(mid)]
        self.s1 = torch.zeros(C, npar, dtype=torch.float64, device=dev)
        self.s2 = torch.zeros_like(self.s1)
        self.counts = torch.zeros(npar, nb, dtype=torch.int64, device=dev)
        self.outside = torch.zeros(npar, dtype=torch.int64, device=dev)
        self.n_acc = torch.zeros(1, dtype=torch.int64, device=dev)

    def call(self, block, sweep=0, burn=0, **over):
        from pulsar_timing_gibbsspec_amd._lib import ptr
        x = torch.as_tensor(block, dtype=torch.float64).to(self.ctx.device)
        a = dict(ctx=self.ctx.handle, n_chain=self.C, n_param=self.npar, n_rows=block.shape[0],
                 stride=block.shape[1], n_bins=self.nb)
        a.update(over)
        rc = self.ctx.lib.gs_chain_summary(
            a["ctx"], a["n_chain"], a["n_param"], ptr(x), a["n_rows"], a["stride"], sweep, burn, a["n_bins"],
            *[ptr(v) for v in self.tab], ptr(self.s1), ptr(self.s2), ptr(self.counts), ptr(self.outside),
            ptr(self.n_acc))
        self.ctx.stream.synchronize()
        return rc

    def compare(self, host):
        assert int(self.n_acc.item()) == host.n
        assert np.array_equal(self.counts.cpu().numpy(), host.counts)
        assert np.array_equal(self.outside.cpu().numpy(), host.outside)
        assert host.counts.sum() + host.outside.sum() == host.n * self.C * self.npar
        f = host.finite
        s1, s2 = self.s1.cpu().numpy(), self.s2.cpu().numpy()
        assert np.array_equal(s1[f], host.s1[f])                           # bit for bit
        with np.errstate(invalid="ignore"):                                # inf - inf outside f
            err = np.abs(s2.astype(np.longdouble) - host.s2)[f]
        bound = (4 * host.n * 2.0 ** -53 * host.sq)[f]                     # n fused or unfused additions
        print(f"s2: max err / bound = {float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0:.3f}")
        assert (err <= bound).all()
        assert not np.isfinite(s1[~f]).any()                               # a non-finite value enters the sums


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=1)


@pytest.mark.parametrize("C,npar,n_rows,nb,pad", SHAPES)
def test_kernel_matches_numpy(ctx, C, npar, n_rows, nb, pad):
    """Two calls on the same accumulators with different data."""
    tabs = _tables(npar, nb, seed=npar)
    dev, host = Dev(ctx, C, npar, nb, *tabs), Host(C, npar, nb, *tabs)
    for call in (0, 1):
        x, block = _data(C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=100 * C + call)
        assert dev.call(block, sweep=call * n_rows) == 0
        for r in range(n_rows):
            host.add(x[r])
        dev.compare(host)
    if npar >= 3:
        assert host.outside.sum() >= 3 and not host.finite.all()           # the planted values were there


def test_burn_skips_the_rows_below_it(ctx):
    C, npar, n_rows, nb, pad = SHAPES[2]
    tabs = _tables(npar, nb, seed=1)
    dev, host = Dev(ctx, C, npar, nb, *tabs), Host(C, npar, nb, *tabs)
    x, block = _data(C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=7)
    assert dev.call(block, sweep=10, burn=12) == 0                         # sweeps 10, 11, 12
    host.add(x[2])
    dev.compare(host)
    assert dev.call(block, sweep=3, burn=12) == 0                          # all below: nothing moves
    dev.compare(host)


def test_sweep_counter_shifts_the_rows(ctx):
    from pulsar_timing_gibbsspec_amd import _lib
    C, npar, n_rows, nb, pad = SHAPES[2]
    tabs = _tables(npar, nb, seed=2)
    dev, host = Dev(ctx, C, npar, nb, *tabs), Host(C, npar, nb, *tabs)
    x, block = _data(C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=8)
    counter = torch.full((1,), 2, dtype=torch.int64, device=ctx.device)
    _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, _lib.ptr(counter)), "gs_ctx_set_sweep_counter")
    try:
        assert dev.call(block, sweep=9, burn=12) == 0                      # sweeps 11, 12, 13
    finally:
        _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, None), "gs_ctx_set_sweep_counter")
    host.add(x[1])
    host.add(x[2])
    dev.compare(host)


def test_rejected_arguments(ctx):
    C, npar, n_rows, nb, pad = SHAPES[2]
    tabs = _tables(npar, nb, seed=3)
    dev, host = Dev(ctx, C, npar, nb, *tabs), Host(C, npar, nb, *tabs)
    _, block = _data(C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=9)
    err = lambda: ctx.lib.gs_last_error().decode()                        # noqa: E731
    assert dev.call(block, ctx=None) == 1 and "ctx" in err()
    assert dev.call(block, n_bins=0) != 0 and "n_bins" in err()
    assert dev.call(block, n_bins=257) != 0 and "n_bins" in err()
    assert dev.call(block, stride=C * npar - 1) != 0 and "row_stride" in err()
    assert dev.call(block, n_rows=-1) != 0 and "n_rows" in err()
    assert dev.call(block, n_param=0) != 0 and "n_param" in err()
    dev.compare(host)                                                      # nothing was accumulated


# ------------------------------------------------------------------ sample(history="summary")
NITER, SAVE, NCH, BURN, BINS = 230, 100, 6, 37, 16
KINDS = {"curn": "conditional", "curn_red": "conditional", "curn_plred": "mh"}


class Runs:
    """The runs of one model kind, each made once and shared by the tests."""

    def __init__(self, kind, root):
        from pulsar_timing_gibbsspec_amd import plumbing, synthetic
        self.kind, self.root = kind, root
        self.pta = synthetic.array_pta(kind=kind, n_psr=4, seed=2)
        keep = np.random.get_state()           # the priors draw from numpy's global generator
        np.random.seed(17)
        self.x0 = np.concatenate([np.atleast_1d(p.sample()).ravel() for p in self.new().params])
        np.random.set_state(keep)
        self.lo, self.hi = plumbing.flat_bounds(self.pta.params)
        self.done = {}

    def new(self):
        from pulsar_timing_gibbsspec_amd import PTABlockGibbs
        return PTABlockGibbs(self.pta, hypersample="conditional", redsample=KINDS[self.kind], nchains=NCH, seed=5)

    def run(self, name, niter=NITER, **kw):
        if name not in self.done:
            gb = self.new()
            d = self.root / name
            copies = {}
            if kw.get("history") == "summary":
                write = gb._write_summary

                def hook(outdir, summary):     # keep every summary.npz the run writes, by its rows
                    write(outdir, summary)
                    shutil.copy(f"{outdir}/summary.npz", f"{outdir}/summary_{int(summary['rows'])}.npz")
                    copies[int(summary["rows"])] = f"{outdir}/summary_{int(summary['rows'])}.npz"
                gb._write_summary = hook
            chain = gb.sample(self.x0, outdir=str(d), niter=niter, save_every=SAVE, **kw)
            self.done[name] = dict(dir=d, chain=np.array(chain), chains=np.array(gb.chains), gb=gb, copies=copies)
        return self.done[name]

    def all_chains(self):                      # run A
        return self.run("A", history="disk", flush_final=True)

    def summary(self):                         # run B
        return self.run("B", history="summary", burn=BURN, bins=BINS)

    def one_chain(self):
        return self.run("D", history="disk", record_chains=1)


@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Runs(kind, tmp_path_factory.mktemp(kind))
        return made[kind]
    return get


@pytest.fixture(scope="module", params=list(KINDS))
def runs(request, pool):
    return pool(request.param)


def _check_summary(s, ref, runs, rows, n):
    w = runs.hi - runs.lo
    assert (ref["W"] > 0).all()                # so R-hat is compared in every column (seed 5)
    assert int(s["rows"]) == rows and int(s["n"]) == n == int(ref["n"])
    assert int(s["burn"]) == BURN and int(s["n_bins"]) == BINS and int(s["nchains"]) == NCH
    assert list(s["names"]) == list(runs.new().param_names)
    assert np.array_equal(s["lo"], runs.lo) and np.array_equal(s["hi"], runs.hi)
    assert s["counts"].dtype == np.int64 and s["outside"].dtype == np.int64
    assert np.array_equal(s["counts"], ref["counts"]) and np.array_equal(s["outside"], ref["outside"])
    fig = {k: float(np.max(np.abs(s[k] - ref[k]) / w ** (1 if k == "mean" else 2))) for k in ("mean", "var", "W", "Bn")}
    fig["rhat"] = float(np.max(np.abs(s["rhat"] / ref["rhat"] - 1)))
    print(f"{runs.kind} rows {rows}: max scaled error {fig}")
    assert (np.abs(s["mean"] - ref["mean"]) <= 1e-13 * w).all()
    for k in ("var", "W", "Bn"):
        assert (np.abs(s[k] - ref[k]) <= 1e-11 * w ** 2).all(), k
    assert (np.abs(s["rhat"] - ref["rhat"]) <= 1e-8 * np.abs(ref["rhat"])).all()


def test_files_are_those_of_the_disk_mode(runs):
    a, b, d = runs.all_chains(), runs.summary(), runs.one_chain()
    assert (b["dir"] / "chain.txt").read_bytes() == (d["dir"] / "chain.txt").read_bytes()
    assert (b["dir"] / "chains.npy").read_bytes() == (d["dir"] / "chains.npy").read_bytes()
    assert np.array_equal(b["chain"], d["chain"]) and np.array_equal(b["chain"], a["chain"])
    assert b["chains"].shape == (1, NITER, len(runs.x0))
    # the state of the last save point: the summary kernel does not touch the chain
    sb, sd = np.load(b["dir"] / "gibbs_state.npz"), np.load(d["dir"] / "gibbs_state.npz")
    assert sorted(sb.files) == sorted(sd.files) and int(sb["rows"]) == 201
    for k in sd.files:
        assert np.array_equal(sb[k], sd[k]), k
    assert np.array_equal(sb["x"], a["chains"][:, 201])
    # the whole blocks were replays of one captured graph
    assert b["gb"]._engine.graph is not None and b["gb"]._engine.graph_rec is None


def test_final_summary_matches_the_recorded_chains(runs):
    from pulsar_timing_gibbsspec_amd.diagnostics import summarize_chains
    a = runs.all_chains()
    ref = summarize_chains(a["chains"][:, BURN:NITER], runs.lo, runs.hi, BINS)
    b = runs.summary()
    s = dict(np.load(b["dir"] / "summary.npz"))
    _check_summary(s, ref, runs, rows=NITER, n=NITER - BURN)
    assert int(s["n"]) == 193
    assert sorted(b["gb"].summary) == sorted(s)
    for k in s:
        assert np.array_equal(b["gb"].summary[k], s[k], equal_nan=s[k].dtype.kind == "f"), k
    assert not (b["dir"] / "summary.npz.tmp").exists()


def test_save_point_summary_matches_the_recorded_chains(runs):
    """summary.npz as it stood at the save point of row 200 covers rows [burn, 200]."""
    from pulsar_timing_gibbsspec_amd.diagnostics import summarize_chains
    a, b = runs.all_chains(), runs.summary()
    assert sorted(b["copies"]) == [101, 201, NITER]
    ref = summarize_chains(a["chains"][:, BURN:201], runs.lo, runs.hi, BINS)
    _check_summary(dict(np.load(b["copies"][201])), ref, runs, rows=201, n=201 - BURN)


def test_without_burn_every_row_is_counted(pool):
    runs = pool("curn")
    s = runs.run("burn0", history="summary")["gb"].summary
    assert int(s["n"]) == NITER and int(s["n_bins"]) == 64 and s["counts"].shape == (len(runs.x0), 64)
    assert np.array_equal(s["counts"].sum(axis=1) + s["outside"], np.full(len(runs.x0), NCH * NITER))


def test_rejected_sample_arguments(pool, tmp_path):
    runs = pool("curn")
    gb = runs.new()
    d = tmp_path / "never"
    for kw in (dict(history="summary", bins=0), dict(history="summary", bins=257), dict(history="summary", bins=8.0),
               dict(history="summary", burn=NITER), dict(history="summary", burn=-1),
               dict(history="disk", bins=8), dict(history="memory", burn=3)):
        with pytest.raises(ValueError):
            gb.sample(runs.x0, outdir=str(d), niter=NITER, save_every=SAVE, **kw)
    with pytest.raises(NotImplementedError):
        gb.sample(runs.x0, outdir=str(d), niter=NITER, save_every=SAVE, history="summary", resume=True)
    assert not d.exists()                      # nothing was touched
    # ... nor in a directory that holds a run
    b = runs.run("B", history="summary", burn=BURN, bins=BINS)
    before = {p.name: p.stat().st_mtime_ns for p in b["dir"].iterdir()}
    with pytest.raises(NotImplementedError):
        gb.sample(runs.x0, outdir=str(b["dir"]), niter=NITER, save_every=SAVE, history="summary", resume=True)
    assert before == {p.name: p.stat().st_mtime_ns for p in b["dir"].iterdir()}


def test_sharded_engine_refuses_a_summary(pool):
    runs = pool("curn")
    b = runs.run("B", history="summary", burn=BURN, bins=BINS)
    eng = b["gb"]._engine
    from pulsar_timing_gibbsspec_amd.engine import ChainSummary
    summ = ChainSummary(eng.ctx, eng.C, eng.n_param, runs.lo, runs.hi)
    eng.sharded = True
    try:
        with pytest.raises(NotImplementedError):
            eng.sweep(summary=summ)
        with pytest.raises(NotImplementedError):
            eng.capture(2, summary=summ)
    finally:
        eng.sharded = False
    assert int(summ.n_acc.item()) == 0
