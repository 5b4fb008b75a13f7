"""gs_coef_moments_block / gs_coef_moments_reduce through the C-ABI against diagnostics.coef_moments
(numpy long double) about the device's reported shift.  Pattern: tests/test_gpu_summary_block.py.

The tolerance is derived, not measured.  With u = 2^-53, N samples of a group and ref_ii = sum d_i^2
(d = v - shift, long double), the device's second-moment sums obey
  |S2_ik - ref| <= 4 (N + 2) u sqrt(ref_ii ref_kk)
(Cauchy-Schwarz on sum |d_i d_k|; the factor 4 covers the subtraction's rounding and any summation
order), and the same bound carried through cov = S2 / N - S1 S1^T / N^2 is that over N.  mean - shift
= S1 / N is held to 4 (N + 2) u sqrt(ref_ii / N); the double that holds mean = shift + S1 / N is
rounded once on the device and once in the reference, u |mean| each, which no fp64 output escapes
(|mean| / sd goes up to 1e10 here)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# (n_group, n_chain, m, ldb, n_rows, padding of a row)
SHAPES = [
    (1, 1, [1], 2, 1, 0),                                      # the smallest call
    (1, 6, [76], 76, 7, 0),                                    # J1713: a partial last tile, 42 samples
    (3, 5, [68, 77, 17], 77, 9, 3),                            # ragged m, NaN beyond m[g] and in the padding
    (2, 3, [216, 130], 216, 2, 0),                             # 14 column blocks: tile pairs over workgroups
    (1, 5003, [16], 17, 2, 1),                                 # exactly one tile, many chain strips and a tail
    (45, 4, [61 + g % 17 for g in range(45)], 77, 101, 0),     # the array's group count, one real block
]
IDS = ["smallest", "j1713", "ragged", "wide", "strips", "array"]
GROUPED = SHAPES[2]


def _block(G, C, m, ldb, n_rows, pad, seed):
    """vs[g] (n_rows, C, m[g]): columns with sd from 1e-9 to 1e-3 and |mean| / sd up to 1e10,
    correlated through a common factor; and the padded block (n_rows, G * C * ldb + pad) that holds
    them, NaN beyond m[g] and in the padding.  Column scales depend on (g, column) only, so the
    calls on one state see the same distribution."""
    rng = np.random.default_rng(seed)
    block = np.full((n_rows, G * C * ldb + pad), np.nan)
    body = block[:, :G * C * ldb].reshape(n_rows, G, C, ldb)
    vs = []
    for g in range(G):
        col = np.random.default_rng(1000 + g)
        sd = 10.0 ** col.uniform(-9, -3, m[g])
        far = col.uniform(0, 10, m[g])
        far[0] = 10.0                              # the case the shift exists for, in every group
        mean = sd * 10.0 ** far * col.choice([-1.0, 1.0], m[g])
        z = rng.standard_normal((n_rows, C, m[g])) + 0.5 * rng.standard_normal((n_rows, C, 1))
        v = mean + sd * z
        body[:, g, :, :m[g]] = v
        vs.append(v)
    return vs, block


class Dev:
    """One state on the device, the reduce outputs, and the entries on them."""

    def __init__(self, ctx, G, C, m, ldb):
        dev = ctx.device
        self.ctx, self.G, self.C, self.m_host, self.ldb = ctx, G, C, list(m), ldb
        size = int(ctx.lib.gs_coef_moments_state_size(G, C, ldb))
        assert size >= 0
        self.state = torch.zeros(size, dtype=torch.float64, device=dev)
        self.m = torch.tensor(self.m_host, dtype=torch.int32, device=dev)
        self.n = torch.full((G,), -7, dtype=torch.int64, device=dev)
        self.shift = torch.full((G, ldb), 7.0, dtype=torch.float64, device=dev)
        self.mean = torch.full((G, ldb), 7.0, dtype=torch.float64, device=dev)
        self.cov = torch.full((G, ldb, ldb), 7.0, dtype=torch.float64, device=dev)

    def call(self, block, sweep=0, burn=0, **over):
        from pulsar_timing_gibbsspec_amd._lib import ptr
        b = torch.as_tensor(block, dtype=torch.float64).to(self.ctx.device)
        a = dict(ctx=self.ctx.handle, n_group=self.G, n_chain=self.C, ldb=self.ldb, m=ptr(self.m), b=ptr(b),
                 n_rows=block.shape[0], stride=block.shape[1], state=ptr(self.state))
        a.update(over)
        rc = self.ctx.lib.gs_coef_moments_block(a["ctx"], a["n_group"], a["n_chain"], a["ldb"], a["m"], a["b"],
                                                a["n_rows"], a["stride"], sweep, burn, a["state"])
        self.ctx.stream.synchronize()
        return rc

    def reduce(self, **over):
        from pulsar_timing_gibbsspec_amd._lib import ptr
        a = dict(ctx=self.ctx.handle, n_group=self.G, n_chain=self.C, ldb=self.ldb, m=ptr(self.m),
                 state=ptr(self.state), n=ptr(self.n), shift=ptr(self.shift), mean=ptr(self.mean), cov=ptr(self.cov))
        a.update(over)
        rc = self.ctx.lib.gs_coef_moments_reduce(a["ctx"], a["n_group"], a["n_chain"], a["ldb"], a["m"], a["state"],
                                                 a["n"], a["shift"], a["mean"], a["cov"])
        self.ctx.stream.synchronize()
        return rc

    def out(self):
        assert self.reduce() == 0
        return dict(n=self.n.cpu().numpy(), shift=self.shift.cpu().numpy(), mean=self.mean.cpu().numpy(),
                    cov=self.cov.cpu().numpy())


def check_group(o, g, m, V, label="", first=None):
    """Group g of the reduce output o against the long-double reference for its samples V (N, m)."""
    from pulsar_timing_gibbsspec_amd.diagnostics import coef_moments
    N = V.shape[0]
    sh, mean, cov = o["shift"][g], o["mean"][g], o["cov"][g]
    assert int(o["n"][g]) == N
    assert (sh[m:] == 0).all() and (mean[m:] == 0).all()               # exactly 0 beyond m[g]
    assert (cov[m:] == 0).all() and (cov[:, m:] == 0).all()
    assert np.array_equal(cov, cov.T)                                  # exactly symmetric
    if first is not None:
        assert np.array_equal(sh[:m], first)                           # chain 0 of the first post-burn row
    ref = coef_moments(V[None], shift=sh[:m])
    d = V.astype(np.longdouble) - sh[:m].astype(np.longdouble)
    rii = np.asarray((d * d).sum(axis=0), float)
    tol_cov = 4 * (N + 2) * U * np.sqrt(np.outer(rii, rii)) / N
    tol_mean = 4 * (N + 2) * U * np.sqrt(rii / N) + 2 * U * np.abs(ref["mean"])
    e_cov, e_mean = np.abs(cov[:m, :m] - ref["cov"]), np.abs(mean[:m] - ref["mean"])
    worst = lambda e, t: float(np.max(e[t > 0] / t[t > 0], initial=0.0))   # noqa: E731
    print(f"{label} group {g}: N = {N}, cov error / bound <= {worst(e_cov, tol_cov):.3g}, "
          f"mean error / bound <= {worst(e_mean, tol_mean):.3g}")
    assert (e_cov <= tol_cov).all()
    assert (e_mean <= tol_mean).all()
    return ref


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=1)


@pytest.mark.parametrize("G,C,m,ldb,n_rows,pad", SHAPES, ids=IDS)
def test_kernel_matches_long_double(ctx, G, C, m, ldb, n_rows, pad):
    """Two calls on one state with different data; checked after each."""
    dev = Dev(ctx, G, C, m, ldb)
    seen = [[] for _ in range(G)]
    first = None
    for call in (0, 1):
        vs, block = _block(G, C, m, ldb, n_rows, pad, seed=100 * C + call)
        first = first or [v[0, 0].copy() for v in vs]
        assert dev.call(block, sweep=call * n_rows) == 0
        o = dev.out()
        refs = []
        for g in range(G):
            seen[g].append(vs[g].reshape(-1, m[g]))
            refs.append(check_group(o, g, m[g], np.concatenate(seen[g]), f"call {call}", first[g]))
    if G > 1:                                      # the groups saw different data: no result is another's
        k = min(m[0], m[1])
        assert not np.array_equal(refs[0]["cov"][:k, :k], refs[1]["cov"][:k, :k])
    r = refs[0]                                    # the planted case was there: |mean| / sd near 1e10
    assert np.abs(r["mean"][0]) / np.sqrt(r["cov"][0, 0]) > 1e9


def test_burn_skips_the_rows_below_it(ctx):
    G, C, m, ldb, n_rows, pad = GROUPED
    dev = Dev(ctx, G, C, m, ldb)
    vs, block = _block(G, C, m, ldb, n_rows, pad, seed=7)
    assert dev.call(block, sweep=3, burn=12) == 0                          # sweeps 3 .. 11: all below
    assert not dev.state.any()                                             # the state stays all zero
    o = dev.out()
    assert (o["n"] == 0).all() and (o["shift"] == 0).all()
    for g in range(G):                                                     # an empty group: NaN, 0 beyond m[g]
        assert np.isnan(o["mean"][g, :m[g]]).all() and np.isnan(o["cov"][g, :m[g], :m[g]]).all()
        assert (o["mean"][g, m[g]:] == 0).all() and (o["cov"][g, m[g]:] == 0).all()
        assert (o["cov"][g, :, m[g]:] == 0).all()
    assert dev.call(block, sweep=10, burn=12) == 0                         # sweeps 10 .. 18: rows 2 .. 8
    o = dev.out()
    for g in range(G):                                                     # the shift from its own first row
        check_group(o, g, m[g], vs[g][2:].reshape(-1, m[g]), "straddle", first=vs[g][2, 0])


def test_sweep_counter_shifts_the_rows(ctx):
    from pulsar_timing_gibbsspec_amd import _lib
    G, C, m, ldb, n_rows, pad = GROUPED
    dev = Dev(ctx, G, C, m, ldb)
    vs, block = _block(G, C, m, ldb, n_rows, pad, seed=8)
    counter = torch.full((1,), 2, dtype=torch.int64, device=ctx.device)
    _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, _lib.ptr(counter)), "gs_ctx_set_sweep_counter")
    try:
        assert dev.call(block, sweep=9, burn=12) == 0                      # sweeps 11 .. 19: rows 1 .. 8
    finally:
        _lib.check(ctx.lib.gs_ctx_set_sweep_counter(ctx.handle, None), "gs_ctx_set_sweep_counter")
    o = dev.out()
    for g in range(G):
        check_group(o, g, m[g], vs[g][1:].reshape(-1, m[g]), "counter", first=vs[g][1, 0])


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=["ragged", "wide"])
def test_results_are_reproducible_and_reduce_reads_only(ctx, shape):
    G, C, m, ldb, n_rows, pad = shape
    a, b = Dev(ctx, G, C, m, ldb), Dev(ctx, G, C, m, ldb)
    for call in (0, 1):
        _, block = _block(G, C, m, ldb, n_rows, pad, seed=40 + call)
        assert a.call(block, sweep=call * n_rows) == 0 and b.call(block, sweep=call * n_rows) == 0
    assert torch.equal(a.state.view(torch.int64), b.state.view(torch.int64))       # bit for bit
    before = a.state.clone()
    o1 = a.out()
    o2 = a.out()                                                           # reduce twice: the same output
    ob = b.out()
    assert torch.equal(a.state.view(torch.int64), before.view(torch.int64))        # and the state untouched
    for k in o1:
        assert np.array_equal(o1[k], o2[k]) and np.array_equal(o1[k], ob[k]), k


def test_a_nan_stays_in_its_group(ctx):
    G, C, m, ldb, n_rows, pad = GROUPED
    dev = Dev(ctx, G, C, m, ldb)
    vs, block = _block(G, C, m, ldb, n_rows, pad, seed=9)
    block[4, (1 * C + 2) * ldb + 33] = np.nan                              # group 1, chain 2, column 33
    assert dev.call(block) == 0
    o = dev.out()
    assert np.isnan(o["mean"][1, :m[1]]).all() and np.isnan(o["cov"][1, :m[1], :m[1]]).all()
    assert (o["mean"][1, m[1]:] == 0).all() and (o["cov"][1, m[1]:] == 0).all()
    assert int(o["n"][1]) == n_rows * C
    for g in (0, 2):
        check_group(o, g, m[g], vs[g].reshape(-1, m[g]), "nan", first=vs[g][0, 0])
    block[4, (1 * C + 2) * ldb + 33] = np.inf                              # +inf does the same
    dev = Dev(ctx, G, C, m, ldb)
    assert dev.call(block) == 0
    o = dev.out()
    assert np.isnan(o["mean"][1, :m[1]]).all() and np.isnan(o["cov"][1, :m[1], :m[1]]).all()
    check_group(o, 0, m[0], vs[0].reshape(-1, m[0]), "inf")


def test_calls_with_no_work(ctx):
    G, C, m, ldb, n_rows, pad = GROUPED
    dev = Dev(ctx, G, C, m, ldb)
    _, block = _block(G, C, m, ldb, n_rows, pad, seed=10)
    assert dev.call(block, n_rows=0) == 0 and dev.call(block, n_group=0) == 0
    assert dev.call(block, n_chain=0, stride=0) == 0
    assert not dev.state.any()
    assert dev.reduce(n_group=0) == 0
    assert int(dev.n[0].item()) == -7                                      # nothing was written
    lib = ctx.lib
    assert lib.gs_coef_moments_state_size(0, 0, 1) >= 0 and lib.gs_coef_moments_state_size(3, 0, 76) >= 0
    for bad in ((-1, 4, 76), (1, -1, 76), (1, 4, 0), (1, 4, 513)):
        assert lib.gs_coef_moments_state_size(*bad) == -1


def test_rejected_arguments(ctx):
    G, C, m, ldb, n_rows, pad = GROUPED
    dev = Dev(ctx, G, C, m, ldb)
    _, block = _block(G, C, m, ldb, n_rows, pad, seed=11)
    err = lambda: ctx.lib.gs_last_error().decode()                        # noqa: E731
    for over, idx, word in ((dict(ctx=None), 1, "ctx"), (dict(n_group=-1), 2, "n_group"),
                            (dict(n_chain=-1), 3, "n_chain"), (dict(ldb=0), 4, "ldb"), (dict(ldb=513), 4, "ldb"),
                            (dict(m=None), 5, "m "), (dict(b=None), 6, "b "), (dict(n_rows=-1), 7, "n_rows"),
                            (dict(n_rows=2 ** 31 // (G * C) + 1, stride=G * C * ldb), 7, "n_rows"),
                            (dict(stride=G * C * ldb - 1), 8, "row_stride"), (dict(state=None), 11, "state")):
        assert dev.call(block, **over) == idx and word in err(), over
    assert not dev.state.any()                                             # nothing was accumulated
    for over, idx, word in ((dict(ctx=None), 1, "ctx"), (dict(n_group=-1), 2, "n_group"),
                            (dict(n_chain=-1), 3, "n_chain"), (dict(ldb=0), 4, "ldb"), (dict(ldb=513), 4, "ldb"),
                            (dict(m=None), 5, "m "), (dict(state=None), 6, "state"), (dict(n=None), 7, "n "),
                            (dict(shift=None), 8, "shift"), (dict(mean=None), 9, "mean"), (dict(cov=None), 10, "cov")):
        assert dev.reduce(**over) == idx and word in err(), over
    assert int(dev.n[0].item()) == -7


def test_engine_class_takes_padded_rows_and_rejects_other_layouts(ctx):
    from pulsar_timing_gibbsspec_amd.engine import CoefMoments
    G, C, m, ldb, n_rows, pad = GROUPED
    vs, block = _block(G, C, m, ldb, n_rows, pad, seed=12)
    x = torch.as_tensor(block, dtype=torch.float64).to(ctx.device)
    padded = x[:, :G * C * ldb].view(n_rows, G * C, ldb)                   # row stride G C ldb + pad
    assert padded.stride(0) == G * C * ldb + pad and not padded.is_contiguous()
    a, b = CoefMoments(ctx, C, m, ldb, burn=2), CoefMoments(ctx, C, m, ldb, burn=2)
    a.accumulate_block(padded, 0, n_rows)
    b.accumulate_block(padded.contiguous(), 0, n_rows)
    fa, fb = a.finalize(), b.finalize()
    ctx.stream.synchronize()
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k
    assert fa["cov"].shape == (G, ldb, ldb) and fa["n"].tolist() == [(n_rows - 2) * C] * G
    # pack into a streamer slot's buffers and unpack from the host
    bufs = [torch.zeros(s, dtype=torch.float64, device=ctx.device) for s in a.extra_shapes]
    a.pack(*bufs)
    ctx.stream.synchronize()
    host = a.unpack(*[t.cpu() for t in bufs])
    assert host["n"].dtype == np.int64
    for g in range(G):
        check_group(host, g, m[g], vs[g][2:].reshape(-1, m[g]), "engine", first=vs[g][2, 0])
    for bad in (padded.transpose(1, 2).contiguous().transpose(1, 2),       # inner axes not contiguous
                padded.to(torch.float32), padded.cpu(), padded[:, :-1]):
        with pytest.raises(ValueError):
            a.accumulate_block(bad, 0, n_rows)
    with pytest.raises(ValueError):
        CoefMoments(ctx, C, [0, 5], ldb)
    with pytest.raises(ValueError):
        CoefMoments(ctx, C, [ldb + 1], ldb)
