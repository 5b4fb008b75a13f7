"""gs_chain_summary_block through the C-ABI: against numpy (tests/test_gpu_summary.py's Host, one
per group) and against a loop of gs_chain_summary over the groups."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_summary import Dev, Host, _data, _tables

pytestmark = pytest.mark.gpu

# (n_group, n_chain, n_param, n_rows, n_bins, padding of a row)
SHAPES = [
    (1, 1, 1, 1, 1, 0),          # the smallest valid call
    (3, 5, 30, 7, 64, 2),        # 30 does not divide 64: waves straddle chains, a group ends mid-wave
    (2, 130, 65, 3, 7, 3),       # more than 64 parameters
    (2, 3, 150, 2, 256, 0),      # a table beyond 64 KB: one gs_chain_summary launch per group
    (1, 5003, 3, 2, 5, 1),       # many chains, a partial last strip
    (45, 4, 30, 101, 16, 0),     # the array's group count and one real block of rows
]
GROUPED = SHAPES[1]


def _block(G, C, npar, n_rows, nb, pad, lo, hi, seed):
    """x (G, n_rows, C, npar), each group planted as _data plants, and the padded block
    (n_rows, G * C * npar + pad) that holds them (padding: NaN)."""
    xs = np.stack([_data(C, npar, n_rows, nb, 0, lo, hi, seed=seed + 7919 * g)[0] for g in range(G)])
    block = np.full((n_rows, G * C * npar + pad), np.nan)
    block[:, :G * C * npar] = np.moveaxis(xs, 0, 1).reshape(n_rows, -1)
    return xs, block


class DevBlock:
    """The accumulators of n_group groups on the device and the new entry on them."""

    def __init__(self, ctx, G, C, npar, nb, lo, hi, scale, mid):
        dev = ctx.device
        self.ctx, self.G, self.C, self.npar, self.nb = ctx, G, C, npar, nb
        t = lambda a: torch.as_tensor(a, dtype=torch.float64).to(dev)   # noqa: E731
        self.tab = [t(lo), t(hi), t(scale), t(mid)]
        self.s1 = torch.zeros(G * C, npar, dtype=torch.float64, device=dev)
        self.s2 = torch.zeros_like(self.s1)
        self.counts = torch.zeros(G, npar, nb, dtype=torch.int64, device=dev)
        self.outside = torch.zeros(G, npar, dtype=torch.int64, device=dev)
        self.n_acc = torch.zeros(1, dtype=torch.int64, device=dev)

    def call(self, block, sweep=0, burn=0, **over):
        from pulsar_timing_gibbsspec_amd._lib import ptr
        x = torch.as_tensor(block, dtype=torch.float64).to(self.ctx.device)
        a = dict(ctx=self.ctx.handle, n_group=self.G, n_chain=self.C, n_param=self.npar, n_rows=block.shape[0],
                 stride=block.shape[1], n_bins=self.nb)
        a.update(over)
        rc = self.ctx.lib.gs_chain_summary_block(
            a["ctx"], a["n_group"], a["n_chain"], a["n_param"], ptr(x), a["n_rows"], a["stride"], sweep, burn,
            a["n_bins"], *[ptr(v) for v in self.tab], ptr(self.s1), ptr(self.s2), ptr(self.counts),
            ptr(self.outside), ptr(self.n_acc))
        self.ctx.stream.synchronize()
        return rc

    def group(self, g):
        """Group g's accumulators, shaped as tests/test_gpu_summary.py's Dev holds them."""
        rows = slice(g * self.C, (g + 1) * self.C)
        return SimpleNamespace(C=self.C, npar=self.npar, n_acc=self.n_acc, counts=self.counts[g],
                               outside=self.outside[g], s1=self.s1[rows], s2=self.s2[rows])

    def compare(self, hosts):
        for g, host in enumerate(hosts):
            Dev.compare(self.group(g), host)       # the old test's compare, per group


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=1)


@pytest.mark.parametrize("G,C,npar,n_rows,nb,pad", SHAPES)
def test_kernel_matches_numpy(ctx, G, C, npar, n_rows, nb, pad):
    """Two calls on the same accumulators with different data."""
    tabs = _tables(npar, nb, seed=npar)
    dev, hosts = DevBlock(ctx, G, C, npar, nb, *tabs), [Host(C, npar, nb, *tabs) for _ in range(G)]
    for call in (0, 1):
        xs, block = _block(G, C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=100 * C + call)
        assert dev.call(block, sweep=call * n_rows) == 0
        for g in range(G):
            for r in range(n_rows):
                hosts[g].add(xs[g, r])
        dev.compare(hosts)
    if npar >= 3:
        for host in hosts:
            assert host.outside.sum() >= 3 and not host.finite.all()       # the planted values were there
    if G > 1:                                      # the groups saw different data: no histogram is another's
        assert not np.array_equal(hosts[0].counts, hosts[1].counts)


@pytest.mark.parametrize("G,C,npar,n_rows,nb,pad", [SHAPES[1], SHAPES[2]])
def test_block_entry_equals_a_loop_of_the_old_entry(ctx, G, C, npar, n_rows, nb, pad):
    from pulsar_timing_gibbsspec_amd._lib import ptr
    tabs = _tables(npar, nb, seed=npar + 1)
    new, old = DevBlock(ctx, G, C, npar, nb, *tabs), DevBlock(ctx, G, C, npar, nb, *tabs)
    hosts = [Host(C, npar, nb, *tabs) for _ in range(G)]
    n_old = torch.zeros(G, dtype=torch.int64, device=ctx.device)
    for call in (0, 1):
        xs, block = _block(G, C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=31 * C + call)
        assert new.call(block, sweep=call * n_rows) == 0
        x = torch.as_tensor(block, dtype=torch.float64).to(ctx.device)
        for g in range(G):
            v = old.group(g)
            rc = ctx.lib.gs_chain_summary(
                ctx.handle, C, npar, ptr(x.view(-1)[g * C * npar:]), n_rows, block.shape[1], call * n_rows, 0, nb,
                *[ptr(t) for t in old.tab], ptr(v.s1), ptr(v.s2), ptr(v.counts), ptr(v.outside),
                ptr(n_old[g:g + 1]))
            assert rc == 0
            for r in range(n_rows):
                hosts[g].add(xs[g, r])
        ctx.stream.synchronize()
    assert n_old.tolist() == [2 * n_rows] * G and int(new.n_acc.item()) == 2 * n_rows
    assert torch.equal(new.counts, old.counts) and torch.equal(new.outside, old.outside)
    a, b = new.s1.cpu().numpy(), old.s1.cpu().numpy()
    finite = np.isfinite(b)
    assert np.array_equal(a[finite].view(np.int64), b[finite].view(np.int64))      # bit for bit
    assert not finite.all() and np.array_equal(a, b, equal_nan=True)               # NaN and +-inf alike
    new.compare(hosts)                             # s2 within the bound of the long-double sum ...
    old.n_acc.copy_(new.n_acc)
    old.compare(hosts)                             # ... for both entries


def test_burn_skips_the_rows_below_it(ctx):
    G, C, npar, n_rows, nb, pad = GROUPED
    tabs = _tables(npar, nb, seed=1)
    dev, hosts = DevBlock(ctx, G, C, npar, nb, *tabs), [Host(C, npar, nb, *tabs) for _ in range(G)]
    xs, block = _block(G, C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=7)
    assert dev.call(block, sweep=10, burn=12) == 0                         # sweeps 10 .. 16: rows 2 .. 6
    for g in range(G):
        for r in range(2, n_rows):
            hosts[g].add(xs[g, r])
    dev.compare(hosts)
    assert int(dev.n_acc.item()) == n_rows - 2
    assert dev.call(block, sweep=3, burn=12) == 0                          # all below: nothing moves
    dev.compare(hosts)


def test_sweep_counter_shifts_the_rows(ctx):
    from pulsar_timing_gibbsspec_amd import _lib
    G, C, npar, n_rows, nb, pad = GROUPED
    tabs = _tables(npar, nb, seed=2)
    dev, hosts = DevBlock(ctx, G, C, npar, nb, *tabs), [Host(C, npar, nb, *tabs) for _ in range(G)]
    xs, block = _block(G, C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=8)
    counter = torch.full((1,), 2, dtype=torch.int64, device=ctx.device)
    _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, _lib.ptr(counter)), "gs_ctx_set_sweep_counter")
    try:
        assert dev.call(block, sweep=9, burn=12) == 0                      # sweeps 11 .. 17: rows 1 .. 6
    finally:
        _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, None), "gs_ctx_set_sweep_counter")
    for g in range(G):
        for r in range(1, n_rows):
            hosts[g].add(xs[g, r])
    dev.compare(hosts)


def test_rejected_arguments(ctx):
    G, C, npar, n_rows, nb, pad = GROUPED
    tabs = _tables(npar, nb, seed=3)
    dev, hosts = DevBlock(ctx, G, C, npar, nb, *tabs), [Host(C, npar, nb, *tabs) for _ in range(G)]
    _, block = _block(G, C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=9)
    err = lambda: ctx.lib.gs_last_error().decode()                        # noqa: E731
    assert dev.call(block, ctx=None) == 1 and "ctx" in err()
    assert dev.call(block, n_bins=0) != 0 and "n_bins" in err()
    assert dev.call(block, n_bins=257) != 0 and "n_bins" in err()
    assert dev.call(block, stride=G * C * npar - 1) != 0 and "row_stride" in err()
    assert dev.call(block, n_rows=-1) != 0 and "n_rows" in err()
    assert dev.call(block, n_group=-1) != 0 and "n_group" in err()
    assert dev.call(block, n_param=0) != 0 and "n_param" in err()
    dev.compare(hosts)                                                     # nothing was accumulated


def test_accumulate_block_takes_padded_rows_and_rejects_other_layouts(ctx):
    from pulsar_timing_gibbsspec_amd.engine import ChainSummary
    G, C, npar, n_rows, nb, pad = GROUPED
    tabs = _tables(npar, nb, seed=4)
    _, block = _block(G, C, npar, n_rows, nb, pad, tabs[0], tabs[1], seed=10)
    x = torch.as_tensor(block, dtype=torch.float64).to(ctx.device)
    padded = x[:, :G * C * npar].view(n_rows, G * C, npar)                 # row stride G C npar + pad
    assert padded.stride(0) == G * C * npar + pad and not padded.is_contiguous()
    a = ChainSummary(ctx, C, npar, tabs[0], tabs[1], n_bins=nb, n_group=G)
    b = ChainSummary(ctx, C, npar, tabs[0], tabs[1], n_bins=nb, n_group=G)
    a.accumulate_block(padded, 0, n_rows)
    b.accumulate_block(padded.contiguous(), 0, n_rows)
    ctx.stream.synchronize()
    assert torch.equal(a.counts, b.counts) and torch.equal(a.outside, b.outside)
    assert a.counts.shape == (G, npar, nb) and int(a.n_acc.item()) == n_rows
    assert torch.equal(a.s1.nan_to_num(1.0, 2.0, 3.0), b.s1.nan_to_num(1.0, 2.0, 3.0))
    for bad in (padded.transpose(1, 2).contiguous().transpose(1, 2),       # inner axes not contiguous
                padded.to(torch.float32), padded.cpu(), padded[:, :-1]):
        with pytest.raises(ValueError):
            a.accumulate_block(bad, 0, n_rows)
    assert int(a.n_acc.item()) == n_rows
