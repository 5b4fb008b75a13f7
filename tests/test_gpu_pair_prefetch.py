"""k_sweep_pair's draw tail (gibbs_tile2.h: both chains' row-group sums in registers, the next draw's
normals generated inside the solve and read back from the wave's LDS slot) against the one-chain
kernel: GS_OPT_SWEEP_SCHED = 3 equals = 2 bit for bit in x_rec, b_rec, the final state and info.

What the launches cover: a launch's first draw takes its normals inline (the slot is not valid yet);
`it0 = 0` runs pass 0, whose prefetch serves the same sweep's second draw; every later draw reads the
slot; a continued launch starts with an invalid slot again, so a 3 + 4 split must equal the same 7
sweeps in one launch (nothing prefetched leaks across launches, and the last sweep's prefetch is
dropped).  6 and 10 chains leave a part-filled 8-chain workgroup.

The inline path is also taken after a sweep whose draw was skipped because both chains' gates were
shut.  That cannot be forced here: the pair kernel runs on device Philox only (no injected uniforms),
and a shut gate needs a rho draw that repeats the previous value exactly.  The fallback it takes is the
code of a launch's first draw, which every case below runs.
"""
import numpy as np
import pytest

from tests.conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=4321)


@pytest.fixture(scope="module")
def model(ctx):
    from pulsar_timing_gibbsspec_amd.engine import DeviceModel
    g = golden("single_j1713.npz")
    gwid = np.asarray(g["gwid"])
    n_tm = g["T"].shape[1] - gwid.size
    return DeviceModel(ctx, [g["T"]], [g["Nvec"]], [g["r"]], [gwid], [np.full(n_tm, 1e-40)])


def _launches(ctx, model, rhomin, rhomax, C, x0, plan, brec):
    """One FreeSpectrumChains run per entry of `plan` (a tuple of launch lengths, the first from
    it0 = 0): every launch's x_rec and b_rec, then the final x, b, info."""
    from pulsar_timing_gibbsspec_amd.engine import FreeSpectrumChains
    out = []
    for lens in plan:
        run = FreeSpectrumChains(model, rhomin, rhomax, C, x0)
        xs, bs = [], []
        for n in lens:
            xr, br = run.run(n, record_b_chains=brec)
            xs.append(xr.cpu().numpy())
            bs.append(br.cpu().numpy())
        out.append((np.concatenate(xs), np.concatenate(bs), run.x.cpu().numpy(), run.b.cpu().numpy(),
                    run.info.cpu().numpy()))
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


PLAN = ((1,), (3, 4), (7,))


@pytest.mark.parametrize("brec", [None, 1])
@pytest.mark.parametrize("C", [2, 6, 10, 64])
def test_pair_tail_equals_one_chain_per_wave(ctx, model, C, brec):
    """1 sweep from it0 = 0; 3 sweeps from it0 = 0 and 4 more in a continued launch; the same 7 in one
    launch -- with every chain's b recorded and with GS_OPT_BREC_CHAINS = 1."""
    g = golden("single_j1713.npz")
    from tests.parity_data import single_replay
    R = single_replay(g)
    x0 = np.random.default_rng(11).uniform(-9, -5, (C, 30))
    res = _both_scheds(ctx, lambda: _launches(ctx, model, R["rhomin"], R["rhomax"], C, x0, PLAN, brec))
    for one, two in zip(res[2], res[3]):
        for a, b in zip(one, two):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert not two[-1].any()                 # no failed factorisation
    split, whole = res[3][1], res[3][2]
    for a, b in zip(split, whole):               # the 3 + 4 split against one launch of 7
        assert np.array_equal(a, b)
    assert res[3][1][1].shape[1] == (C if brec is None else 1)
    assert np.isfinite(res[3][2][0]).all() and np.isfinite(res[3][2][1]).all()


def test_pair_tail_three_pulsars(ctx):
    """Three consecutive pulsars of the simulated `indep` array whose timing models have nM <= 16
    columns (the pair kernel's tiled fixed block), GS_OPT_PSR_BASE at their first index (the prefetch's
    Philox counters carry the global pulsar index), 4 chains each, 3 + 4 sweeps and the 7 in one."""
    from pulsar_timing_gibbsspec_amd import _lib, synthetic
    from pulsar_timing_gibbsspec_amd.engine import DeviceModel
    ptas = synthetic.pulsar_ptas(synthetic.array_pta(kind="indep", seed=0))
    T = [p.get_basis()[0] for p in ptas]
    N = [p.get_ndiag({})[0] for p in ptas]
    R = [p.get_residuals()[0] for p in ptas]
    nM = np.array([t.shape[1] - 60 for t in T])
    runs = [p for p in range(len(nM) - 2) if (nM[p:p + 3] <= 16).all() and p > 0]
    assert runs
    lo = runs[0]
    C = 4
    x0 = np.random.default_rng(12).uniform(-9, -4, (3 * C, 30))
    ctx.set_option(_lib.OPT_PSR_BASE, lo)
    try:
        model3 = DeviceModel(ctx, T[lo:lo + 3], N[lo:lo + 3], R[lo:lo + 3], [np.arange(60)] * 3,
                             [np.full(t.shape[1] - 60, 1e-40) for t in T[lo:lo + 3]])
        res = _both_scheds(ctx, lambda: _launches(ctx, model3, 1e-18, 1e-8, C, x0, PLAN[1:], None))
    finally:
        ctx.set_option(_lib.OPT_PSR_BASE, 0)

    def same(a, b):
        if a.shape[-1] == model3.ldb:            # b rows: columns >= m_p are never written
            for p in range(3):
                rows, m = slice(p * C, (p + 1) * C), model3.m[p]
                assert np.array_equal(a[..., rows, :m], b[..., rows, :m])
        else:
            assert np.array_equal(a, b)

    for one, two in zip(res[2], res[3]):
        for a, b in zip(one, two):
            same(a, b)
        assert not two[-1].any()
    for a, b in zip(res[3][0], res[3][1]):
        same(a, b)
