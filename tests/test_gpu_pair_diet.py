"""k_sweep_pair with the paired elimination's dead updates removed (gibbs_tile2.h tile_elim_pair: at an
odd pivot step the register of rows k - 1, k of A is skipped, in the last tile the register of the
padding rows 14, 15 as well) and its sweep loop's arguments loaded where they are used, against
the one-chain kernel: GS_OPT_SWEEP_SCHED = 3 equals = 2 bit for bit in x_rec, b_rec, the final x and b,
info and the failure counts.

Besides the launch shapes (part-filled workgroups, a first draw from x0, continued launches, compact b
records, three pulsars with a global pulsar index) two things are aimed at the skipped updates:

* failed factorisations.  A skipped register still holds a diagonal element the pivot read-out takes,
  so the first bad pivot must be reported at the same index: the model's S[j][j] is made hugely
  negative mid-run for j = 0 and for odd local columns of a full tile (21) and of the last tile (57);
  and one chain of a pair is made to fail alone (its prior precision on S[0][0] pinned to the lower
  bound 1e8 through its b, its partner's near the upper bound 1e18, S[0][0] = -1e15).
* a prior at both bounds in one chain: x0 alternates -9 / -4 over the frequencies, so the first draw's
  diagonal carries 1e18 and 1e8 on neighbouring entries of every tile, the last one included.
"""
import numpy as np
import pytest

from tests.conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=97531)


@pytest.fixture(scope="module")
def model(ctx):
    from pulsar_timing_gibbsspec_amd.engine import DeviceModel
    g = golden("single_j1713.npz")
    gwid = np.asarray(g["gwid"])
    n_tm = g["T"].shape[1] - gwid.size
    return DeviceModel(ctx, [g["T"]], [g["Nvec"]], [g["r"]], [gwid], [np.full(n_tm, 1e-40)])


RHOMIN, RHOMAX = 1e-18, 1e-8


def _state(run):
    return [t.cpu().numpy() for t in (run.x, run.b, run.info, run.fail_count)]


def _launches(mdl, C, x0, plan, brec):
    """One FreeSpectrumChains run per entry of `plan` (launch lengths, the first from it0 = 0): the
    launches' x_rec and b_rec, then the final x, b, info and failure counts."""
    from pulsar_timing_gibbsspec_amd.engine import FreeSpectrumChains
    out = []
    for lens in plan:
        run = FreeSpectrumChains(mdl, RHOMIN, RHOMAX, C, x0)
        xs, bs = [], []
        for n in lens:
            xr, br = run.run(n, record_b_chains=brec)
            xs.append(xr.cpu().numpy())
            bs.append(br.cpu().numpy())
        out.append([np.concatenate(xs), np.concatenate(bs)] + _state(run))
    return out


def _both_scheds(ctx, fn):
    from pulsar_timing_gibbsspec_amd import _lib
    prev = ctx.get_option(_lib.OPT_SWEEP_SCHED)
    res, shapes = {}, []
    try:
        for sched in (2, 3):
            ctx.set_option(_lib.OPT_SWEEP_SCHED, sched)
            res[sched] = fn()
            shapes.append(ctx.get_option(_lib.OPT_LAST_SWEEP_SHAPE))
    finally:
        ctx.set_option(_lib.OPT_SWEEP_SCHED, prev)
    assert shapes == [2, 3]                      # the kernels that ran: one chain per wave, two
    return res


def _assert_same(one, two):
    for a, b in zip(one, two):
        assert a.shape == b.shape and np.array_equal(a, b)


PLAN = ((1,), (3, 4))


@pytest.mark.parametrize("brec", [None, 1])
@pytest.mark.parametrize("C", [2, 6, 10, 64])
def test_pair_diet_equals_one_chain_per_wave(ctx, model, C, brec):
    """1 sweep from it0 = 0; 3 sweeps and 4 more in a continued launch -- with every chain's b recorded
    and with GS_OPT_BREC_CHAINS = 1."""
    x0 = np.random.default_rng(21).uniform(-9, -4, (C, 30))
    res = _both_scheds(ctx, lambda: _launches(model, C, x0, PLAN, brec))
    for one, two in zip(res[2], res[3]):
        _assert_same(one, two)
        assert not two[4].any() and not two[5].any()      # no failed factorisation
        assert np.isfinite(two[0]).all() and np.isfinite(two[1]).all()
    assert res[3][1][1].shape[:2] == (7, C if brec is None else 1)


def test_pair_diet_three_pulsars(ctx):
    """Three consecutive pulsars of the simulated `indep` array with nM <= 16 timing-model columns (the
    pair kernel's tiled fixed block), GS_OPT_PSR_BASE at their first (non-zero) index, 4 chains each."""
    from pulsar_timing_gibbsspec_amd import _lib, synthetic
    from pulsar_timing_gibbsspec_amd.engine import DeviceModel
    ptas = synthetic.pulsar_ptas(synthetic.array_pta(kind="indep", seed=0))
    T = [p.get_basis()[0] for p in ptas]
    N = [p.get_ndiag({})[0] for p in ptas]
    R = [p.get_residuals()[0] for p in ptas]
    nM = np.array([t.shape[1] - 60 for t in T])
    runs = [p for p in range(1, len(nM) - 2) if (nM[p:p + 3] <= 16).all()]
    assert runs
    lo = runs[0]
    C = 4
    x0 = np.random.default_rng(22).uniform(-9, -4, (3 * C, 30))
    ctx.set_option(_lib.OPT_PSR_BASE, lo)
    try:
        model3 = DeviceModel(ctx, T[lo:lo + 3], N[lo:lo + 3], R[lo:lo + 3], [np.arange(60)] * 3,
                             [np.full(t.shape[1] - 60, 1e-40) for t in T[lo:lo + 3]])
        res = _both_scheds(ctx, lambda: _launches(model3, C, x0, PLAN, None))
    finally:
        ctx.set_option(_lib.OPT_PSR_BASE, 0)
    for one, two in zip(res[2], res[3]):
        for a, b in zip(one, two):
            assert a.shape == b.shape
            if a.shape[-1] == model3.ldb:        # b rows: columns >= m_p are never written
                for p in range(3):
                    rows, m = slice(p * C, (p + 1) * C), model3.m[p]
                    assert np.array_equal(a[..., rows, :m], b[..., rows, :m])
            else:
                assert np.array_equal(a, b)
        assert not two[4].any() and not two[5].any()


def _non_pd_run(model, C, x0, j, value, pin_b):
    """10 sweeps, then 5 with the model block's S[j][j] (S0 is NF x (NF + 1) row-major at the block's
    start) set to `value`, then 5 with the model restored.  pin_b: before the 5 failing sweeps chain 0's
    b on the first frequency is set to 1 (tau = 1: rho | b is rhomax to 1e-7 relative, phiinv 1e8) and
    every other chain's to 1e-12 (tau = 1e-24: rho = rhomin / U)."""
    from pulsar_timing_gibbsspec_amd.engine import FreeSpectrumChains
    run = FreeSpectrumChains(model, RHOMIN, RHOMAX, C, x0)
    out = [t.cpu().numpy() for t in run.run(10)]
    b10 = run.b.clone()
    saved = model.model.clone()
    try:
        if pin_b:
            f = torch.as_tensor(model.fidx_host[0][:2], device=run.b.device)
            run.b[0, f] = 1.0
            run.b[1:, f] = 1e-12
            b10 = run.b.clone()
        model.model[62 * j] = value
        out += [t.cpu().numpy() for t in run.run(5)]
        out += _state(run)
        mid = (run.b.clone(), run.info.cpu().numpy().copy(), run.fail_count.cpu().numpy().copy())
    finally:
        model.model.copy_(saved)
    out += [t.cpu().numpy() for t in run.run(5)]
    return out + _state(run), b10, mid


@pytest.mark.parametrize("j", [0, 21, 57])
def test_pair_diet_non_pd_same_pivot(ctx, model, j):
    """S[j][j] = -1e300 mid-run (test_fused_sweep_non_pd_mid_run_keeps_b's construction at three
    columns): every chain's draw fails at pivot j + 1, in both kernels, and keeps its b."""
    C = 4
    x0 = golden("single_j1713.npz")["x0"]
    res = _both_scheds(ctx, lambda: _non_pd_run(model, C, x0, j, -1e300, False))
    _assert_same(res[2][0], res[3][0])
    for out, b10, (b, info, cnt) in res.values():
        assert torch.equal(b, b10)                           # b kept through 5 failed draws
        assert (info == j + 1).all() and cnt.tolist() == [5] * C
        assert all(np.isfinite(a).all() for a in out)
        assert out[-1].tolist() == [5] * C and not np.array_equal(out[-3], b10.cpu().numpy())


def test_pair_diet_one_chain_of_a_pair_fails(ctx, model):
    """S[0][0] = -1e15 with chain 0's prior precision there pinned at 1e8 and its partner's (and the
    other chains') near 1e18: chain 0 fails at pivot 1 in each of the 5 sweeps and keeps its b while
    chains that share its wave and workgroup draw on; same info, counts and b in both kernels."""
    C = 6
    x0 = np.random.default_rng(23).uniform(-9, -4, (C, 30))
    res = _both_scheds(ctx, lambda: _non_pd_run(model, C, x0, 0, -1e15, True))
    _assert_same(res[2][0], res[3][0])
    for out, b10, (b, info, cnt) in res.values():
        assert info[0] == 1 and cnt[0] == 5 and torch.equal(b[0], b10[0])
        assert (cnt[1:] == 0).any() and not torch.equal(b[1:], b10[1:])
        assert all(np.isfinite(a).all() for a in out)


def test_pair_diet_prior_at_both_bounds(ctx, model):
    """x0 alternating between the prior's bounds over the frequencies (chain 0 from -9, chain 1 from -4,
    two more at random): the first draw's phiinv is 1e18 and 1e8 on neighbouring diagonal entries."""
    C = 4
    x0 = np.random.default_rng(24).uniform(-9, -4, (C, 30))
    x0[0, 0::2], x0[0, 1::2] = -9.0, -4.0
    x0[1, 0::2], x0[1, 1::2] = -4.0, -9.0
    res = _both_scheds(ctx, lambda: _launches(model, C, x0, PLAN, None))
    for one, two in zip(res[2], res[3]):
        _assert_same(one, two)
        assert not two[4].any() and np.isfinite(two[1]).all()
    # the first recorded row is x0 itself, and the draw made from it moved b off its start
    assert np.array_equal(res[3][0][0][0, :2], x0[:2])
