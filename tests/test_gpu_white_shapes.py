"""Every white-noise kernel path of csrc/gibbs_white.hip against long-double references
(tests/white_ref.py) on seeded synthetic data: T ~ N(0,1) times per-column scales spanning
10^+-6, sigma in [1e-7, 1e-6], r ~ sigma; models are WhiteNoiseModel(prefix=False), NF = 2.

1. gs_white_tnt: all 23 instantiations -- k_white_syrk_mc<1..6>, k_white_syrk<1..16> (<1..6> under
   GS_SYRK_PAIRED), the k_white_tnt + k_white_tnr fallback (m >= 256) -- with ragged m in one
   launch, both x layouts, 9 chains, 3 backends (efac + tnequad / t2equad only / no parameter).
   Entrywise, with n the TOA count and u = 2^-53:
       |dTNT_ij| <= (n + 16) u sqrt(TNT_ii TNT_jj),   |dd_j| <= (n + 16) u sqrt(TNT_jj rNr),
   TNT == TNT.T exactly, and nothing outside each system's m x m / m range is written.
2. gs_white_resid, both kernels: |dy_t| <= (m + 2) u (|r_t| + sum_j |T_tj b_j|).
3. gs_white_mh with injected draws against white_mh_ref: bit-identical white columns, every other
   column untouched, n_acc and q_rec equal; nsteps_chain; the inclusive prior edge.
4. gs_white_mh on its own Philox stream against white_mh_philox (global pulsar index, chain_base,
   sweep, counter slots 3 s .. 3 s + 2).
5. gs_ecorr_epoch_sums, staged and unstaged groups, against long-double segment sums.

A Metropolis system may be skipped only on an accept/reject near-tie of the reference (margin <=
B, white_ref.white_mh_ref); the cap is zero skipped systems, and tests/test_white_ref.py pins on
the CPU that the committed seeds produce none.
"""
import numpy as np
import pytest

from tests import white_ref as W
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

MAX_SKIPPED = 0
GUARD = 64


@pytest.fixture(scope="module")
def gpu():
    if not gpu_available():
        pytest.skip("no GPU")
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib


def _context(gpu, per_sys, seed=1, psr_base=0):
    c = gpu.Context(0, seed=seed)
    c.set_option(gpu.OPT_X_PER_SYS, int(per_sys))
    c.set_option(gpu.OPT_PSR_BASE, int(psr_base))
    return c


@pytest.fixture(scope="module")
def ctxs(gpu):
    return {ps: _context(gpu, ps) for ps in (False, True)}


def _model(ctx, psr, white_lists, C):
    from pulsar_timing_gibbsspec_amd.white import WhiteNoiseModel
    return WhiteNoiseModel(ctx, [d["T"] for d in psr], [d["r"] for d in psr], [d["sigma"] for d in psr],
                           [d["backends"] for d in psr], [[0, 1]] * len(psr),
                           [np.full(d["T"].shape[1] - 2, 1e-40) for d in psr], white_lists, C, prefix=False)


def _dev(ctx, a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(ctx.device)


def _guarded(ctx, n, fill=np.nan, dtype=None):
    """(whole, view): an n-element buffer with GUARD sentinel elements on either side."""
    import torch
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype or torch.float64, device=ctx.device)
    return whole, whole[GUARD:GUARD + n]


# ================================================================== 1. SYRK
def _check_syrk(ctx, n_toa, m, per_sys):
    """One gs_white_tnt launch of syrk_case(n_toa, m) into NaN-filled, padded TNT / d."""
    psr, vals = W.syrk_case(n_toa, m)
    C = W.SYRK_C
    wm = _model(ctx, psr, W.SYRK_WHITE, C)
    x = W.layout_x(vals, W.SYRK_WHITE, C, W.SYRK_LDX, per_sys)
    # chain strides padded past the model's own so that writes outside a system's range land on NaN
    wm.tnt_cstride += 5
    wm.d_cstride += 3
    Tw, wm.TNT = _guarded(ctx, C * wm.tnt_cstride)
    dw, wm.d = _guarded(ctx, C * wm.d_cstride)
    wm.tnt(_dev(ctx, x), W.SYRK_LDX)
    Th, dh = Tw.cpu().numpy(), dw.cpu().numpy()
    written_T, written_d = np.zeros(Th.size, bool), np.zeros(dh.size, bool)
    worst = (0.0, 0.0)
    for p, d in enumerate(psr):
        mm = d["T"].shape[1]
        for c in range(C):
            o = GUARD + c * wm.tnt_cstride + int(wm.tnt_off[p])
            od = GUARD + c * wm.d_cstride + int(wm.d_off[p])
            written_T[o:o + mm * mm] = True
            written_d[od:od + mm] = True
            try:
                e = W.check_tnt(Th[o:o + mm * mm].reshape(mm, mm), dh[od:od + mm], d["T"], None, d["r"],
                                ref=W.syrk_ref(n_toa, m, p, c))
            except AssertionError as err:
                raise AssertionError((f"pulsar {p} (n_toa {d['T'].shape[0]}, m {mm}) chain {c}",) + err.args)
            worst = max(worst, e)
    assert np.isnan(Th[~written_T]).all(), "TNT written outside the systems' m x m ranges"
    assert np.isnan(dh[~written_d]).all(), "d written outside the systems' m ranges"
    return worst


SYRK_SHAPES = [(nb, m) for nb in range(1, 17) for m in W.syrk_ms(nb)]


@pytest.mark.parametrize("per_sys", [False, True], ids=["xchain", "xsys"])
@pytest.mark.parametrize("nb,m", SYRK_SHAPES, ids=[f"nb{nb}-m{m}" for nb, m in SYRK_SHAPES])
def test_syrk_every_instantiation(ctxs, monkeypatch, nb, m, per_sys):
    """Default route: k_white_syrk_mc<nb> for nb <= 6, k_white_syrk<nb> above (nb = 14 is the
    balanced instantiation whose last wave owns the diagonal tiles, nb = 16 needs the > 64 KB LDS
    opt-in).  70 TOAs = two 32-TOA chunks + 6 rows; 2 pulsars x 9 chains = 18 systems."""
    monkeypatch.delenv("GS_SYRK_PAIRED", raising=False)
    assert (m + 16) // 16 == nb
    _check_syrk(ctxs[per_sys], 70, m, per_sys)


PAIRED_SHAPES = [s for s in SYRK_SHAPES if s[0] <= 6]


@pytest.mark.parametrize("per_sys", [False, True], ids=["xchain", "xsys"])
@pytest.mark.parametrize("nb,m", PAIRED_SHAPES, ids=[f"nb{nb}-m{m}" for nb, m in PAIRED_SHAPES])
def test_syrk_paired_small_block_counts(ctxs, monkeypatch, nb, m, per_sys):
    """GS_SYRK_PAIRED=1: k_white_syrk<1..6>, the paired-row kernel at the block counts the default
    route gives to k_white_syrk_mc (odd nb: the middle wave owns one row, r1 == r2)."""
    monkeypatch.setenv("GS_SYRK_PAIRED", "1")
    _check_syrk(ctxs[per_sys], 70, m, per_sys)


@pytest.mark.parametrize("per_sys", [False, True], ids=["xchain", "xsys"])
@pytest.mark.parametrize("m", [256, 300])
def test_tnt_fallback_pair(ctxs, monkeypatch, m, per_sys):
    """m >= 256: k_white_tnt (one workgroup per lower tile pair) + k_white_tnr."""
    monkeypatch.delenv("GS_SYRK_PAIRED", raising=False)
    _check_syrk(ctxs[per_sys], 70, m, per_sys)


@pytest.mark.parametrize("n_toa", [1, 31, 32, 33, 64])
@pytest.mark.parametrize("m", [47, 143, 216, 256], ids=["mc3", "paired9", "bal14", "fallback"])
def test_tnt_toa_counts_around_the_chunk(ctxs, monkeypatch, m, n_toa):
    """TOA counts around the 32-TOA chunk (and a single TOA, whose only backend is the third) at
    one shape per kernel family."""
    monkeypatch.delenv("GS_SYRK_PAIRED", raising=False)
    _check_syrk(ctxs[True], n_toa, m, True)


# ================================================================== 2. residual GEMM
@pytest.mark.parametrize("valu", [False, True], ids=["mfma", "valu"])
@pytest.mark.parametrize("C", [1, 15, 16, 17])
@pytest.mark.parametrize("m", [1, 3, 4, 15, 16, 17, 76, 130])
def test_resid_matches_long_double(gpu, ctxs, monkeypatch, m, C, valu):
    """y = r - T b through the C-ABI (k_white_resid_mfma, or k_white_resid under GS_RESID_VALU):
    three ragged pulsars, b columns >= m NaN-filled (they must not be read), y NaN-prefilled."""
    if valu:
        monkeypatch.setenv("GS_RESID_VALU", "1")
    else:
        monkeypatch.delenv("GS_RESID_VALU", raising=False)
    ctx = ctxs[False]
    psr, b, ys, bounds = W.resid_case(m, C)
    P = len(psr)
    n = np.array([d["T"].shape[0] for d in psr], np.int64)
    toa_off = np.concatenate([[0], np.cumsum(n)])
    T_off = np.concatenate([[0], np.cumsum(n * m)])
    tdesc = np.stack([n, np.full(P, m), T_off[:-1], toa_off[:-1], np.zeros(P, np.int64), np.zeros(P, np.int64)],
                     axis=1).astype(np.int64)
    ldb, ldy = m + 3, int(toa_off[-1]) + 2
    bp = np.full((P * C, ldb), np.nan)
    bp[:, :m] = b
    yw, yv = _guarded(ctx, C * ldy)
    keep = [_dev(ctx, tdesc), _dev(ctx, np.concatenate([d["T"].T.ravel() for d in psr])),
            _dev(ctx, np.concatenate([d["r"] for d in psr])), _dev(ctx, bp)]
    gpu.check(ctx.lib.gs_white_resid(ctx.handle, P, C, int(n.max()), ldb, *[gpu.ptr(t) for t in keep], ldy,
                                     gpu.ptr(yv)), "gs_white_resid")
    yh = yw.cpu().numpy()
    y = yh[GUARD:GUARD + C * ldy].reshape(C, ldy)
    assert np.isnan(yh[:GUARD]).all() and np.isnan(yh[GUARD + C * ldy:]).all() and np.isnan(y[:, toa_off[-1]:]).all()
    for p in range(P):
        got = y[:, toa_off[p]:toa_off[p + 1]]
        assert np.isfinite(got).all(), p
        err = np.abs(np.asarray(got, W.L) - ys[p])
        assert np.all(err <= bounds[p]), (p, int(n[p]), float(np.max(err / bounds[p])))


# ================================================================== 3, 4. Metropolis kernel
class _MhRun:
    """One gs_white_mh launch over pulsars `psrs` and chains `chains` of white_ref.mh_case, y
    written into the model directly."""

    def __init__(self, ctx, per_sys, psrs=(0, 1, 2), chains=tuple(range(W.MH_C))):
        import torch
        psr, vals, _ = W.mh_case()
        self.ctx, self.per_sys, self.psrs, self.chains = ctx, per_sys, list(psrs), list(chains)
        self.C = C = len(chains)
        self.wl = [W.MH_WHITE[p] for p in psrs]
        self.wm = wm = _model(ctx, [psr[p] for p in psrs], self.wl, C)
        for i, p in enumerate(psrs):
            assert np.array_equal(wm.perm[i], np.arange(wm.perm[i].size))
            o = int(np.sum(wm.n_toa[:i]))
            wm.y[:, o:o + int(wm.n_toa[i])] = _dev(ctx, psr[p]["y"][self.chains])
        self.x0 = W.layout_x([vals[p][self.chains] for p in psrs], self.wl, C, W.MH_LDX, per_sys)
        self.n_sys = len(psrs) * C
        self.torch = torch

    def woff(self, i):
        return int(np.sum([len(w) for w in self.wl[:i]]))

    def run(self, steps, inj=None, nsteps=None, sweep=0, chain_base=0):
        torch, ctx = self.torch, self.ctx
        x = _dev(ctx, self.x0)
        q_rec = torch.full((steps, self.n_sys, 32), float("nan"), dtype=torch.float64, device=ctx.device)
        n_acc = torch.full((self.n_sys,), -1, dtype=torch.int32, device=ctx.device)
        self.wm.mh(x, W.MH_LDX, steps, sweep, chain_base,
                   nsteps_chain=None if nsteps is None else _dev(ctx, nsteps, torch.int32),
                   inj=None if inj is None else _dev(ctx, inj), q_rec=q_rec, n_acc=n_acc)
        return x.cpu().numpy(), q_rec.cpu().numpy(), n_acc.cpu().numpy()


def _compare_injected(run, refs, x, q_rec, n_acc):
    """Device output of an injected-draw launch against white_mh_ref per system."""
    C, per_sys = run.C, run.per_sys
    want = run.x0.copy()
    skipped = 0
    for i in range(len(run.psrs)):
        nw = len(run.wl[i])
        for c in range(C):
            sys = i * C + c
            xr, acc, q, margin, B = refs[sys]
            rows = (W.xrow(want, i, c, C, per_sys), W.xrow(x, i, c, C, per_sys))
            if np.any(margin <= B):          # near-tie: the fp64 sums may decide either way
                skipped += 1
                cols = [col for col, *_ in run.wl[i]]
                rows[0][cols] = rows[1][cols]
                continue
            for col, *_ in run.wl[i]:
                rows[0][col] = xr[col]
            assert n_acc[sys] == acc, (i, c, n_acc[sys], acc)
            n = q.shape[0]
            assert np.array_equal(q_rec[:n, sys, :nw], q), (i, c)
            assert np.isnan(q_rec[n:, sys]).all() and np.isnan(q_rec[:, sys, nw:]).all(), (i, c)
    assert skipped <= MAX_SKIPPED, skipped
    # white columns bit-identical, every other entry of x still the sentinel
    assert np.array_equal(x, want), np.argwhere(x != want)[:8]


@pytest.mark.parametrize("per_sys", [False, True], ids=["xchain", "xsys"])
def test_mh_injected_matches_reference(gpu, ctxs, per_sys):
    """Three pulsars in one launch (1 backend / efac only; 15 backends of 1, 63, 64, 65, ... TOAs
    with 32 parameters; 4 backends, one without a parameter, one with t2equad only), 6 chains
    (a partial 4-wave workgroup), 40 injected steps."""
    run = _MhRun(ctxs[per_sys], per_sys)
    _, _, inj = W.mh_case()
    _, refs = W.mh_refs(per_sys)
    out = run.run(W.MH_STEPS, inj=inj)
    _compare_injected(run, refs, *out)
    assert out[2].min() >= 0 and out[2].max() > 0


@pytest.mark.parametrize("per_sys", [False, True], ids=["xchain", "xsys"])
def test_mh_nsteps_chain(gpu, ctxs, per_sys):
    """Per-chain step counts (per system under GS_OPT_X_PER_SYS), 0 and the maximum included:
    steps past a chain's count do not apply (x, n_acc) and leave q_rec unwritten."""
    run = _MhRun(ctxs[per_sys], per_sys)
    _, _, inj = W.mh_case()
    ns = W.mh_nsteps(per_sys)
    _, refs = W.mh_refs(per_sys, nsteps=ns)
    _compare_injected(run, refs, *run.run(W.MH_STEPS, inj=inj, nsteps=ns))


@pytest.mark.parametrize("per_sys", [False, True], ids=["xchain", "xsys"])
def test_mh_prior_edge_is_inclusive(gpu, ctxs, per_sys):
    """wmax set to the exact fp64 value of a system's first proposal: evaluated and (u = 1e-300)
    accepted; wmax one ulp below another system's proposal: rejected, x unchanged."""
    run = _MhRun(ctxs[per_sys], per_sys)
    inj, wmax = W.mh_edge_case()
    for (p, i), v in wmax.items():
        run.wm.wmax[run.woff(p) + i] = v
    _, refs = W.mh_refs(per_sys, inj=inj, wmax=wmax)
    x, q_rec, n_acc = run.run(1, inj=inj)
    _compare_injected(run, refs, x, q_rec, n_acc)
    C = W.MH_C
    col_a, col_b = W.MH_WHITE[0][0][0], W.MH_WHITE[2][0][0]
    assert n_acc[0 * C + 2] == 1 and W.xrow(x, 0, 2, C, per_sys)[col_a] == wmax[(0, 0)]
    assert n_acc[2 * C + 4] == 0
    assert W.xrow(x, 2, 4, C, per_sys)[col_b] == W.xrow(run.x0, 2, 4, C, per_sys)[col_b]
    assert q_rec[0, 2 * C + 4, 0] == np.nextafter(wmax[(2, 0)], np.inf)


def _compare_philox(run, refs, x, q_rec, n_acc):
    C, per_sys = run.C, run.per_sys
    skipped = 0
    for i, p in enumerate(run.psrs):
        nw = len(run.wl[i])
        cols = [col for col, *_ in run.wl[i]]
        for ci, c in enumerate(run.chains):
            sys = i * C + ci
            (xr, acc, steps, w), (_, _, q, margin, B) = refs[(p, c)]
            if np.any(margin <= B):
                skipped += 1
                continue
            # the chosen parameter of every step: the lane of q_rec that moved off the current state
            base = q.copy()
            base[np.arange(len(w)), w] -= (steps[:, 2] * np.float64(0.05 * nw)) * steps[:, 0]
            assert np.array_equal(np.argmax(np.abs(q_rec[:, sys, :nw] - base), axis=1), w), (p, c)
            assert np.allclose(q_rec[:, sys, :nw], q, rtol=1e-12, atol=1e-12), (p, c)
            assert n_acc[sys] == acc, (p, c, n_acc[sys], acc)
            got = W.xrow(x, i, ci, C, per_sys)
            assert np.allclose(got[cols], xr[cols], rtol=1e-12, atol=1e-12), (p, c)
            rest = np.setdiff1d(np.arange(W.MH_LDX), cols if per_sys else [col for wl in run.wl for col, *_ in wl])
            assert np.all(got[rest] == W.SENTINEL), (p, c)
    assert skipped <= MAX_SKIPPED, skipped


@pytest.mark.parametrize("per_sys", [False, True], ids=["xchain", "xsys"])
def test_mh_philox_stream(gpu, per_sys):
    """inj = None: the kernel's own Philox draws (GS_OPT_PSR_BASE = 5, chain_base = 11, sweep = 3,
    a key with both words set) against white_mh_philox: chosen parameter per step exact, n_acc
    equal, x within rtol = atol = 1e-12 (the device-libm Box-Muller tolerance of
    test_gpu_red.py::test_red_mh_matches_oracle).  A launch over pulsars 1..2 and chains 2..5 with
    the bases moved accordingly is bit-identical to the matching rows of the full launch."""
    ctx = _context(gpu, per_sys, seed=W.MH_KEY_SEED, psr_base=W.MH_PSR_BASE)
    run = _MhRun(ctx, per_sys)
    _, refs = W.mh_philox_refs(per_sys)
    x, q_rec, n_acc = run.run(W.MH_STEPS, sweep=W.MH_SWEEP, chain_base=W.MH_CHAIN_BASE)
    _compare_philox(run, refs, x, q_rec, n_acc)
    assert 0 < n_acc.sum() < W.MH_STEPS * run.n_sys
    psrs, chains = (1, 2), (2, 3, 4, 5)
    ctx2 = _context(gpu, per_sys, seed=W.MH_KEY_SEED, psr_base=W.MH_PSR_BASE + psrs[0])
    sub = _MhRun(ctx2, per_sys, psrs, chains)
    xs, qs, ns = sub.run(W.MH_STEPS, sweep=W.MH_SWEEP, chain_base=W.MH_CHAIN_BASE + chains[0])
    C = W.MH_C
    for i, p in enumerate(psrs):
        cols = [col for col, *_ in W.MH_WHITE[p]]
        for ci, c in enumerate(chains):
            assert np.array_equal(W.xrow(xs, i, ci, len(chains), per_sys)[cols], W.xrow(x, p, c, C, per_sys)[cols])
            assert ns[i * len(chains) + ci] == n_acc[p * C + c]
            assert np.array_equal(qs[:, i * len(chains) + ci], q_rec[:, p * C + c], equal_nan=True), (p, c)


# ================================================================== 5. ECORR epoch sums
@pytest.mark.parametrize("first_big", [True, False], ids=["fallback-first", "staged-first"])
@pytest.mark.parametrize("ne", [1, 16, 17, 40])
@pytest.mark.parametrize("C", [1, 8, 9])
@pytest.mark.parametrize("kb", [48, 80])
def test_ecorr_epoch_sums_match_segment_sums(gpu, ctxs, kb, C, ne, first_big):
    """k_ecorr_epoch_sums: 16-epoch groups alternate between > 256 TOA entries (the unstaged
    fallback) and <= 256 (staged through LDS); Bx (T columns, zero columns, the d column) and Dg
    within (q_e + 16) u sum |terms| of the long-double segment sums, q_e the epoch's entry count."""
    import torch
    ctx = ctxs[False]
    e = W.epoch_case(kb, C, ne, first_big)
    d = e["psr"]
    wm = _model(ctx, [d], [W.ES_WHITE], C)
    assert np.array_equal(wm.perm[0], np.arange(wm.perm[0].size))
    Bw, Bv = _guarded(ctx, C * ne * kb)
    Dw, Dv = _guarded(ctx, C * ne)
    keep = [_dev(ctx, e["x"]), _dev(ctx, e["colmap"], torch.int32), _dev(ctx, e["eptr"], torch.int32),
            _dev(ctx, e["etoa"], torch.int32), _dev(ctx, e["eu"])]
    p = gpu.ptr
    gpu.check(ctx.lib.gs_ecorr_epoch_sums(
        ctx.handle, C, p(wm.wdesc), p(wm.wcol), p(wm.wkind), p(wm.wbk), p(keep[0]), W.ES_LDX, p(wm.T), W.ES_M,
        p(wm.sigma2), p(wm.bk), p(wm.r), ne, kb, e["dcol"], p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]),
        p(Bv), p(Dv)), "gs_ecorr_epoch_sums")
    Bh, Dh = Bw.cpu().numpy(), Dw.cpu().numpy()
    for h, n in ((Bh, C * ne * kb), (Dh, C * ne)):
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + n:]).all()
        assert np.isfinite(h[GUARD:GUARD + n]).all()
    Bx = Bh[GUARD:GUARD + C * ne * kb].reshape(C, ne, kb)
    Dg = Dh[GUARD:GUARD + C * ne].reshape(C, ne)
    eB = np.abs(np.asarray(Bx, W.L) - e["Bx"])
    eD = np.abs(np.asarray(Dg, W.L) - e["Dg"])
    assert np.all(eB <= e["bB"]), np.argwhere(eB > e["bB"])[:4]
    assert np.all(eD <= e["bD"]), np.argwhere(eD > e["bD"])[:4]
    unmapped = (e["colmap"] < 0) & (np.arange(kb) != e["dcol"])
    assert np.all(Bx[:, :, unmapped] == 0.0)

