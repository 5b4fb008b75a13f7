"""gs_chain_acf_block / gs_chain_acf_reduce through the C-ABI against diagnostics.acov_chains (numpy
long double): |acov - ref| <= 1e-9 ref[:, 0], the project's parity standard."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-9

# (n_group, n_chain, n_param, rows per call, max_lag, padding of a row)
SHAPES = [
    (1, 1, 1, [1], 1, 0),              # the smallest valid call
    (3, 5, 30, [7, 7, 7, 2], 8, 2),    # L above the block length, groups ending mid-wave
    (2, 130, 65, [3, 40], 16, 3),      # more than 64 parameters, the head filled across two calls
    (1, 5003, 3, [20], 4, 1),          # many chains, a partial last strip
    (2, 4, 30, [101, 101], 128, 0),    # a real block, L above it
    (1, 6, 2, [300], 256, 0),          # a window beyond one LDS tile
    (2, 3, 4, [2, 3], 8, 0),           # n <= L: lags >= n are exactly 0
]
GROUPED = SHAPES[1]


def _chains(G, C, npar, n, seed):
    """x (n, G, C, npar) and mid (npar,): per chain an AR(1) series of sd 0.05 .. 0.3 (phi 0 .. 0.95
    by parameter) about its own level, the levels up to 2.2 from mid."""
    rng = np.random.default_rng(seed)
    mid = rng.uniform(-7.0, -6.0, npar)
    phi = np.linspace(0.0, 0.95, npar)[::-1] if npar > 1 else np.array([0.8])
    sd = rng.uniform(0.05, 0.3, (G, C, npar))
    level = mid + rng.uniform(-2.2, 2.2, (G, C, npar))
    e = rng.standard_normal((n, G, C, npar))
    z = np.empty_like(e)
    z[0] = e[0]
    for t in range(1, n):
        z[t] = phi * z[t - 1] + np.sqrt(1 - phi * phi) * e[t]
    return level + sd * z, mid


def _reference(x, L):
    """acov_chains per group of x (n, G, C, npar): (G, npar, L + 1)."""
    from pulsar_timing_gibbsspec_amd.diagnostics import acov_chains
    return np.stack([acov_chains(np.moveaxis(x[:, g], 0, 1), L) for g in range(x.shape[1])])


class DevAcf:
    """One opaque state on the device and the entries on it."""

    def __init__(self, ctx, G, C, npar, L, mid):
        self.ctx, self.G, self.C, self.npar, self.L = ctx, G, C, npar, L
        size = ctx.lib.gs_chain_acf_state_size(G, C, npar, L)
        assert size > 0
        self.state = torch.zeros(size, dtype=torch.float64, device=ctx.device)
        self.mid = torch.as_tensor(mid, dtype=torch.float64).to(ctx.device)

    def block(self, rows, pad=0, sweep=0, burn=0, **over):
        """rows (n_rows, G, C, npar) as one padded block (padding: NaN)."""
        from pulsar_timing_gibbsspec_amd._lib import ptr
        T = self.G * self.C * self.npar
        blk = np.full((rows.shape[0], T + pad), np.nan)
        blk[:, :T] = rows.reshape(rows.shape[0], -1)
        x = torch.as_tensor(blk, dtype=torch.float64).to(self.ctx.device)
        a = dict(ctx=self.ctx.handle, n_group=self.G, n_chain=self.C, n_param=self.npar, n_rows=rows.shape[0],
                 stride=T + pad, max_lag=self.L, mid=ptr(self.mid), state=ptr(self.state))
        a.update(over)
        rc = self.ctx.lib.gs_chain_acf_block(a["ctx"], a["n_group"], a["n_chain"], a["n_param"], ptr(x), a["n_rows"],
                                             a["stride"], sweep, burn, a["max_lag"], a["mid"], a["state"])
        self.ctx.stream.synchronize()
        return rc

    def feed(self, x, calls, pad=0, sweep=0, burn=0):
        at = 0
        for n in calls:
            assert self.block(x[at:at + n], pad, sweep=sweep + at, burn=burn) == 0
            at += n
        assert at == x.shape[0]

    def reduce(self, **over):
        from pulsar_timing_gibbsspec_amd._lib import ptr
        acov = torch.full((self.G, self.npar, self.L + 1), -7.0, dtype=torch.float64, device=self.ctx.device)
        n = torch.full((1,), -7, dtype=torch.int64, device=self.ctx.device)
        a = dict(ctx=self.ctx.handle, n_group=self.G, n_chain=self.C, n_param=self.npar, max_lag=self.L,
                 state=ptr(self.state))
        a.update(over)
        rc = self.ctx.lib.gs_chain_acf_reduce(a["ctx"], a["n_group"], a["n_chain"], a["n_param"], a["max_lag"],
                                              a["state"], ptr(acov), ptr(n))
        self.ctx.stream.synchronize()
        return rc, acov, n


def _close(acov, ref, what=""):
    got = acov.cpu().numpy()
    err = np.abs(got - ref) / ref[..., :1]
    print(f"{what}: max |acov - ref| / ref[0] = {np.nanmax(err):.3e}")
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= TOL * ref[..., :1]).all()


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=1)


@pytest.fixture(scope="module")
def grouped():
    """The data and reference the smaller tests share: GROUPED's shape, 23 rows."""
    G, C, npar, calls, L, pad = GROUPED
    x, mid = _chains(G, C, npar, sum(calls), seed=11)
    return x, mid, _reference(x, L)


@pytest.mark.parametrize("G,C,npar,calls,L,pad", SHAPES)
def test_kernel_matches_numpy(ctx, G, C, npar, calls, L, pad):
    n = sum(calls)
    x, mid = _chains(G, C, npar, n, seed=100 * C + L)
    ref = _reference(x, L)
    dev = DevAcf(ctx, G, C, npar, L, mid)
    dev.feed(x, calls, pad)
    rc, acov, n_dev = dev.reduce()
    assert rc == 0 and int(n_dev.item()) == n
    if n > 1:
        _close(acov, ref, f"{G}x{C}x{npar} rows {calls} L {L}")
    else:                                          # one row: the chain's mean is the value, acov = 0
        assert (acov.cpu().numpy()[..., 0] == 0).all() and (ref == 0).all()
    if L >= n:                                     # lags >= n are exactly 0
        assert (acov.cpu().numpy()[..., n:] == 0).all()
    if G > 1:                                      # the groups saw different data
        assert not np.array_equal(ref[0], ref[1])


def test_burn_skips_the_rows_below_it(ctx, grouped):
    G, C, npar, calls, L, pad = GROUPED
    x, mid, _ = grouped
    ref = _reference(x[9:], L)
    dev = DevAcf(ctx, G, C, npar, L, mid)
    assert dev.block(x[:7], pad, sweep=3, burn=12) == 0                    # sweeps 3 .. 9: all below, nothing moves
    assert not dev.state.any()
    assert dev.block(x[7:14], pad, sweep=10, burn=12) == 0                 # sweeps 10 .. 16: rows 2 .. 6 of the call
    assert dev.block(x[14:], pad, sweep=17, burn=12) == 0
    rc, acov, n = dev.reduce()
    assert rc == 0 and int(n.item()) == x.shape[0] - 9
    _close(acov, ref, "burn inside a block")


def test_sweep_counter_shifts_the_rows(ctx, grouped):
    from pulsar_timing_gibbsspec_amd import _lib
    G, C, npar, calls, L, pad = GROUPED
    x, mid, _ = grouped
    ref = _reference(x[1:], L)
    dev = DevAcf(ctx, G, C, npar, L, mid)
    counter = torch.full((1,), 2, dtype=torch.int64, device=ctx.device)
    _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, _lib.ptr(counter)), "gs_ctx_set_sweep_counter")
    try:
        assert dev.block(x[:7], pad, sweep=9, burn=12) == 0                # sweeps 11 .. 17: rows 1 .. 6
        assert dev.block(x[7:], pad, sweep=16, burn=12) == 0
    finally:
        _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, None), "gs_ctx_set_sweep_counter")
    rc, acov, n = dev.reduce()
    assert rc == 0 and int(n.item()) == x.shape[0] - 1
    _close(acov, ref, "attached sweep counter")


def test_one_call_and_many_calls_agree(ctx, grouped):
    G, C, npar, calls, L, pad = GROUPED
    x, mid, ref = grouped
    n = x.shape[0]
    for split in ([n], [1] * n, [5, 1, 9, 8]):
        dev = DevAcf(ctx, G, C, npar, L, mid)
        dev.feed(x, split, pad)
        rc, acov, n_dev = dev.reduce()
        assert rc == 0 and int(n_dev.item()) == n
        _close(acov, ref, f"calls {split}")


def test_results_are_reproducible_and_reduce_leaves_the_state(ctx, grouped):
    G, C, npar, calls, L, pad = GROUPED
    x, mid, _ = grouped
    a, b = DevAcf(ctx, G, C, npar, L, mid), DevAcf(ctx, G, C, npar, L, mid)
    a.feed(x, calls, pad)
    b.feed(x, calls, pad)
    assert torch.equal(a.state, b.state)           # two fresh states, the same calls: the same bits
    before = a.state.clone()
    _, acov1, n1 = a.reduce()
    _, acov2, n2 = a.reduce()
    _, acov3, _ = b.reduce()
    assert torch.equal(acov1, acov2) and torch.equal(acov1, acov3) and torch.equal(n1, n2)
    assert torch.equal(a.state, before)
    # and a reduction in the middle changes nothing of what follows
    c = DevAcf(ctx, G, C, npar, L, mid)
    c.feed(x[:14], [7, 7], pad)
    c.reduce()
    c.feed(x[14:], [7, 2], pad, sweep=14)
    assert torch.equal(c.state, a.state)


def test_a_nan_poisons_its_own_parameter_only(ctx, grouped):
    G, C, npar, calls, L, pad = GROUPED
    x, mid, ref = grouped
    bad = x.copy()
    bad[10, 1, 3, 17] = np.nan                     # row 10, group 1, chain 3, parameter 17
    dev = DevAcf(ctx, G, C, npar, L, mid)
    dev.feed(bad, calls, pad)
    rc, acov, _ = dev.reduce()
    got = acov.cpu().numpy()
    assert rc == 0 and np.isnan(got[1, 17]).all()
    keep = np.ones((G, npar), bool)
    keep[1, 17] = False
    assert np.isfinite(got[keep]).all()
    assert (np.abs(got[keep] - ref[keep]) <= TOL * ref[keep][:, :1]).all()


def test_rejected_arguments_leave_the_state(ctx, grouped):
    G, C, npar, calls, L, pad = GROUPED
    x, mid, _ = grouped
    dev = DevAcf(ctx, G, C, npar, L, mid)
    dev.feed(x[:7], [7], pad)
    before = dev.state.clone()
    err = lambda: ctx.lib.gs_last_error().decode()                        # noqa: E731
    rows = x[7:14]
    assert dev.block(rows, pad, ctx=None) == 1 and "ctx" in err()
    assert dev.block(rows, pad, max_lag=0) != 0 and "max_lag" in err()
    assert dev.block(rows, pad, max_lag=4097) != 0 and "max_lag" in err()
    assert dev.block(rows, pad, stride=G * C * npar - 1) != 0 and "row_stride" in err()
    assert dev.block(rows, pad, n_rows=-1) != 0 and "n_rows" in err()
    assert dev.block(rows, pad, n_group=-1) != 0 and "n_group" in err()
    assert dev.block(rows, pad, n_chain=-1) != 0 and "n_chain" in err()
    assert dev.block(rows, pad, n_param=0) != 0 and "n_param" in err()
    assert dev.block(rows, pad, mid=None) != 0 and "mid" in err()
    assert dev.block(rows, pad, state=None) != 0 and "state" in err()
    assert dev.reduce(ctx=None)[0] == 1 and "ctx" in err()
    assert dev.reduce(max_lag=0)[0] != 0 and "max_lag" in err()
    assert dev.reduce(n_param=0)[0] != 0 and "n_param" in err()
    assert dev.reduce(state=None)[0] != 0 and "state" in err()
    assert torch.equal(dev.state, before)
    assert dev.block(rows, pad, n_rows=0) == 0     # no rows: accepted, nothing moves
    assert torch.equal(dev.state, before)


def test_chain_summary_carries_acov(ctx, grouped):
    """engine.ChainSummary(acf_lags=L): accumulate_block, finalize and pack / unpack."""
    from pulsar_timing_gibbsspec_amd.engine import ChainSummary
    G, C, npar, calls, L, pad = GROUPED
    x, mid, ref = grouped
    lo, hi = mid - 4.0, mid + 4.0                  # mid = (lo + hi) / 2 up to rounding: the tolerance covers it
    plain = ChainSummary(ctx, C, npar, lo, hi, n_bins=8, n_group=G)
    assert len(plain.extra_shapes) == 2 and plain.acf_state is None
    summ = ChainSummary(ctx, C, npar, lo, hi, n_bins=8, n_group=G, acf_lags=L)
    assert summ.extra_shapes[2] == (G * npar * (L + 1),) and len(summ.extra_shapes) == 3
    at = 0
    for n in calls:
        blk = torch.as_tensor(x[at:at + n].reshape(n, G * C, npar)).to(ctx.device)
        summ.accumulate_block(blk, at, n)
        at += n
    f = summ.finalize()
    ctx.stream.synchronize()
    assert f["acov"].shape == (G, npar, L + 1)
    _close(f["acov"], ref, "ChainSummary.finalize")
    bufs = [torch.zeros(s, dtype=torch.float64, device=ctx.device) for s in summ.extra_shapes]
    side = torch.cuda.Stream(device=ctx.device)
    summ.pack_behind(side, *bufs)
    torch.cuda.synchronize()
    out = summ.unpack(*[b.cpu() for b in bufs])
    assert np.array_equal(out["acov"], f["acov"].cpu().numpy()) and int(out["n"]) == at
    with pytest.raises(ValueError):
        summ.pack(bufs[0], bufs[1])                # the third buffer is missing
    with pytest.raises(NotImplementedError):
        summ.accumulate(None)
    with pytest.raises(ValueError):
        ChainSummary(ctx, C, npar, lo, hi, acf_lags=4097)
