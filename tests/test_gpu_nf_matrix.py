"""Every NF class of dispatch_nf (csrc/gibbs_bdraw.h) on every fixed-block layout and both
one-chain sweep shapes.

The kernels k_bdraw, k_lnlike_marg and k_sweep_freespec / k_sweep_freespec_rm exist in eight NF
classes (NFC = 20 / 40 / 60 fixed; NF at run time with NTC = NF/16 + 1 = 1..5), read the
fixed-prior block in tiles (NMX <= 16) or row-major (17 <= NMX <= 64), and the sweep runs in 4-wave
workgroups (one chain per wave) or 12-wave hand-off workgroups.  tests/nf_cases.NF_LIST x
nm in {0, 1, 16, 17, 33, 48, 64} puts each class on each layout, the last-tile edges NF mod 16 = 0
included.

References (tests/parity_data, oracle.gibbs_oracle), with the tolerances of tests/test_gpu_nf.py:
the x87 long-double Cholesky draw on the same normals (1e-9 normwise per draw), the oracle's
PulsarBlockGibbs loop on the same normals and uniforms (x: 1e-9), lnlike_fullmarg (1e-10
relative); two launch shapes of the same arithmetic are compared bit for bit."""
import numpy as np
import pytest

from oracle import gibbs_oracle as O
from tests import nf_cases as K
from tests.parity_data import exact_chol_draw_pre, normwise_rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=99)


def _model(ctx, NF, nm):
    from pulsar_timing_gibbsspec_amd.engine import DeviceModel
    T, N, r = K.pulsar(NF, nm)
    return DeviceModel(ctx, [T], [N], [r], [np.arange(NF)], [np.full(nm, 1e-40)]), T, N, r


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


# ------------------------------------------------------------------ 1. open-loop b draw
BDRAW_CASES = ([(NF, nm) for NF in K.NF_LIST for nm in (0, 16, 17, 64)]
               + [(NF, nm) for NF in (14, 40, 64) for nm in (1, 33)])   # one fixed row; a 1-row last chunk


def _bdraw_against_exact(ctx, NF, nm):
    model, T, N, r = _model(ctx, NF, nm)
    m = T.shape[1]
    assert model.NF == NF and model.NMX == nm
    rng = np.random.default_rng(NF + 100 * nm)
    C = 4
    ph = K.phiinv_rows(rng, C, NF)
    z = np.zeros((C, model.ldb))
    z[:, :m] = rng.standard_normal((C, m))
    b, info = model.bdraw(dev(ph), C, z=dev(z))
    b = b.cpu().numpy()
    assert not info.cpu().numpy().any()
    tl, order = K.exact(NF, nm)
    for c in range(C):
        phi = np.concatenate([ph[c], np.full(nm, 1e-40)])
        bx = exact_chol_draw_pre(tl, phi, z[c, :m], order)
        err = normwise_rel(b[c, :m], bx)
        assert err < 1e-9, (NF, nm, c, err)


@pytest.mark.parametrize("NF,nm", BDRAW_CASES)
def test_bdraw_matrix_matches_exact_draw(ctx, NF, nm):
    """gs_bdraw with injected normals, every chain against the exact long-double draw: each
    k_bdraw<NFC, NTC, .., 3> class with no fixed block, the tiled one (nm <= 16) and the
    row-major one (M.G[row * LD + f], M.R[row * NMX + mm]; 17, odd 33, the largest 64)."""
    from pulsar_timing_gibbsspec_amd import _lib
    assert ctx.get_option(_lib.OPT_BCAST) == 3
    _bdraw_against_exact(ctx, NF, nm)


@pytest.mark.parametrize("bcast", [0, 1, 2])
@pytest.mark.parametrize("NF", [20, 40, 60])
def test_bdraw_lane_row_variants_row_major_fixed_block(ctx, NF, bcast):
    """The lane-row variants k_bdraw<NFC, 0, .., 0 | 1 | 2> of the fixed NF with 17 fixed columns."""
    from pulsar_timing_gibbsspec_amd import _lib
    prev = ctx.get_option(_lib.OPT_BCAST)
    ctx.set_option(_lib.OPT_BCAST, bcast)
    try:
        _bdraw_against_exact(ctx, NF, 17)
    finally:
        ctx.set_option(_lib.OPT_BCAST, prev)


# ------------------------------------------------------------------ 2. marginalised likelihood
@pytest.mark.parametrize("nm", [0, 17, 64])
@pytest.mark.parametrize("NF", K.NF_LIST)
def test_lnlike_marg_matrix(ctx, NF, nm):
    """k_lnlike_marg<NFC, NTC> against lnlike_fullmarg (1e-10 relative): the model block staged in
    LDS below 64 KB and above it (nm = 64: 43 KB at NF = 2 up to 102 KB at NF = 64)."""
    model, T, N, r = _model(ctx, NF, nm)
    rng = np.random.default_rng(NF + 1000 * nm)
    C = 3
    ph = K.phiinv_rows(rng, C, NF)
    lnl, info = model.lnlike_marg(dev(ph), C)
    lnl = lnl.cpu().numpy()
    assert not info.cpu().numpy().any()
    TNT, d = K.tnt64(NF, nm)
    for c in range(C):
        phi = np.concatenate([1.0 / ph[c], np.full(nm, 1e40)])
        want = O.lnlike_fullmarg(r, N, TNT, d, 1.0 / phi, np.sum(np.log(phi)))
        assert abs(lnl[c] - want) <= 1e-10 * abs(want), (NF, nm, c, lnl[c], want, abs(lnl[c] - want) / abs(want))


# ------------------------------------------------------------------ 3. fused sweep, both one-chain shapes
# (NF, nm, LDS bytes of the 12-wave hand-off workgroup by launch_sweep_freespec's formula: the tiled
# model block + 12 x (tile scratch + 128 + 256) + 4 x 256 + 2 doubles).  All below the 160 KB
# (163840 B) a gfx950 workgroup may request, so none falls back to the 4-wave shape.
SWEEP_CASES = [(14, 16, 89744), (14, 33, 98464), (16, 17, 95888), (20, 16, 95888), (20, 17, 95888),
               (30, 16, 95888), (30, 33, 106784), (32, 0, 95760), (40, 16, 104080), (40, 48, 130320),
               (46, 17, 104608), (48, 17, 114320), (60, 16, 114320), (60, 33, 129040), (62, 16, 114320),
               (64, 16, 128144), (64, 33, 141872)]
LDS_OPTIN = 160 * 1024


def test_sweep_cases_cover_every_class_on_both_layouts(ctx):
    """The list above has each of the eight NF classes with a tiled (k_sweep_freespec) and a
    row-major (k_sweep_freespec_rm) fixed block, and the stated bytes are the launcher's: the tile
    stride from gs_model_tiled_stride, the scratch of gs_tile_scr."""
    seen = {}
    for NF, nm, lds in SWEEP_CASES:
        seen.setdefault(K.nf_class(NF), set()).add(nm > 16)
        NT = NF // 16 + 1
        scr = 336 + (16 * NT if NT > 4 else 64)
        want = (int(ctx.lib.gs_model_tiled_stride(NF, nm)) + 12 * (scr + 128 + 256) + 4 * 256 + 2) * 8
        assert lds == want and lds <= LDS_OPTIN, (NF, nm, lds, want)
    assert set(seen) == {(20, 0), (40, 0), (60, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5)}
    assert all(v == {False, True} for v in seen.values()), seen


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("NF,nm,lds12", SWEEP_CASES)
def test_sweep_matrix_handoff_equals_one_chain_per_wave_and_oracle(ctx, NF, nm, lds12, S):
    """FreeSpectrumChains on injected z0 / z / u, 29 chains (a full 16-chain hand-off workgroup whose
    four trios each carry an extra chain and a 13-chain one where only trio 0 does), S = 2 (an empty
    first third) and 4 sweeps: GS_OPT_SWEEP_SCHED = 1 (k_sweep_freespec[_rm]<NFC, NTC, 12, 3>) and
    2 (<.., 4, 3>) give every recorded row, the final state and info bit for bit.  Chains 0 (an own
    chain), 12 and 15 (the first and last extra), 28 (the partial workgroup's extra) of the
    hand-off run against the oracle's loop (x, 1e-9) and each b draw against the exact draw at the
    device's own state (1e-9)."""
    from pulsar_timing_gibbsspec_amd import _lib
    from pulsar_timing_gibbsspec_amd.engine import FreeSpectrumChains
    model, T, N, r = _model(ctx, NF, nm)
    m, n_f = T.shape[1], NF // 2
    C = 29
    rng = np.random.default_rng(7 * NF + nm + S)
    x0 = rng.uniform(-9, -4, (C, n_f))
    z = np.zeros((S + 1, C, model.ldb))
    z[:, :, :m] = rng.standard_normal((S + 1, C, m))
    U = rng.random((S, C, n_f))
    zd0, zd, Ud = dev(z[0]), dev(z[1:]), dev(U)
    out, shapes = [], []
    prev = ctx.get_option(_lib.OPT_SWEEP_SCHED)
    try:
        for sched in (1, 2):
            ctx.set_option(_lib.OPT_SWEEP_SCHED, sched)
            run = FreeSpectrumChains(model, 1e-18, 1e-8, C, x0)
            assert run.fused
            xr, br = run.run(S, z0_inj=zd0, z_inj=zd, u_inj=Ud)
            shapes.append(ctx.get_option(_lib.OPT_LAST_SWEEP_SHAPE))
            run.check_info()
            out.append([t.cpu().numpy() for t in (xr, br, run.x, run.b, run.info)])
    finally:
        ctx.set_option(_lib.OPT_SWEEP_SCHED, prev)
    assert shapes == [1, 2], (NF, nm, lds12, shapes)
    for i, (a, b) in enumerate(zip(*out)):
        if i in (1, 3):                          # b rows: column m of an nm = 0 model (ldb = NF + 1) is never written
            a, b = a[..., :m], b[..., :m]
        assert np.array_equal(a, b), i
    assert not out[0][-1].any()
    xr, br = out[0][0], out[0][1]
    TNT, d = K.tnt64(NF, nm)
    tl, order = K.exact(NF, nm)
    for c in (0, 12, 15, 28):
        want_x, _, _ = O.sweep_single(TNT, d, np.arange(NF), x0[c], 1e-18, 1e-8, z[:, c, :m], U[:, c], S,
                                      lambda x: O.phiinv_single(x, nm), draw="chol", order=order)
        ex = normwise_rel(xr[:, c], want_x)
        assert ex < 1e-9, (NF, nm, c, ex)
        # every recorded draw (row j: drawn with z[j] at x row j) and the final one against the exact
        # draw at the device's own x.  Not against the oracle's b: its fp64 draw is itself up to 1.2e-8
        # from the exact one at these states (NF = 40, nm = 48, x0 in (-9, -4)), and a fed-back b
        # chain amplifies rounding through phi = 10^(2x)
        for j in range(1, S):
            bx = exact_chol_draw_pre(tl, O.phiinv_single(xr[j, c], nm), z[j, c, :m], order)
            eb = normwise_rel(br[j, c, :m], bx)
            assert eb < 1e-9, (NF, nm, c, j, eb)
        bx = exact_chol_draw_pre(tl, O.phiinv_single(out[0][2][c], nm), z[S, c, :m], order)
        eb = normwise_rel(out[0][3][c, :m], bx)
        assert eb < 1e-9, (NF, nm, c, "final", eb)


# ------------------------------------------------------------------ 4. hand-off on several pulsars
def test_sweep_handoff_three_ragged_pulsars(ctx):
    """The 12-wave hand-off workgroups on three consecutive pulsars of the `indep` array (NF = 60)
    whose timing models mix 17 columns (row-major fixed block) with <= 16 (tiled) inside one
    NMX = 17 batch (model_tiled_view_psr per pulsar), a non-zero GS_OPT_PSR_BASE, device Philox,
    29 chains, 5 sweeps and a continued second launch, b recorded for chains < 5 only
    (GS_OPT_BREC_CHAINS: the extra chains record no b rows): bit for bit the recorded rows and the
    final state of the one-chain-per-wave shape on the written columns."""
    from pulsar_timing_gibbsspec_amd import _lib, synthetic
    from pulsar_timing_gibbsspec_amd.engine import DeviceModel, FreeSpectrumChains
    ptas = synthetic.pulsar_ptas(synthetic.array_pta(kind="indep", seed=0))
    T = [p.get_basis()[0] for p in ptas]
    N = [p.get_ndiag({})[0] for p in ptas]
    R = [p.get_residuals()[0] for p in ptas]
    nM = np.array([t.shape[1] - 60 for t in T])
    runs = [p for p in range(1, len(nM) - 2) if (nM[p:p + 3] == 17).any() and (nM[p:p + 3] <= 16).any()
            and nM[p:p + 3].max() == 17]
    assert runs
    lo = runs[0]
    C, S, BK = 29, 5, 5
    x0 = np.random.default_rng(11).uniform(-9, -4, (3 * C, 30))
    out, shapes = [], []
    prev = ctx.get_option(_lib.OPT_SWEEP_SCHED)
    ctx.set_option(_lib.OPT_PSR_BASE, lo)
    try:
        model3 = DeviceModel(ctx, T[lo:lo + 3], N[lo:lo + 3], R[lo:lo + 3], [np.arange(60)] * 3,
                             [np.full(n, 1e-40) for n in nM[lo:lo + 3]])
        assert model3.NMX == 17
        for sched in (1, 2):
            ctx.set_option(_lib.OPT_SWEEP_SCHED, sched)
            run = FreeSpectrumChains(model3, 1e-18, 1e-8, C, x0)
            xr, br = run.run(S, record_b_chains=BK)
            xr2, br2 = run.run(S, record_b_chains=BK)
            shapes.append(ctx.get_option(_lib.OPT_LAST_SWEEP_SHAPE))
            run.check_info()
            out.append([t.cpu().numpy() for t in (xr, br, xr2, br2, run.x, run.b, run.info)])
    finally:
        ctx.set_option(_lib.OPT_SWEEP_SCHED, prev)
        ctx.set_option(_lib.OPT_PSR_BASE, 0)
    assert shapes == [1, 2]
    assert out[0][1].shape == (S, 3 * BK, model3.ldb)
    for a, b in zip(*out):
        if a.shape[-1] == model3.ldb:            # b rows: columns >= m_p are never written
            k = a.shape[-2] // 3
            for p in range(3):
                rows, m = slice(p * k, (p + 1) * k), model3.m[p]
                assert np.array_equal(a[..., rows, :m], b[..., rows, :m])
        else:
            assert np.array_equal(a, b)
    assert not out[0][-1].any()
    # the chains moved, every pulsar's own way (a stale per-pulsar view would repeat a neighbour's draws)
    xf = out[0][4].reshape(3, C, 30)
    assert not np.array_equal(xf[0], xf[1]) and not np.array_equal(xf[1], xf[2])
    assert np.all(np.isfinite(out[0][5][:, :60]))
