"""The persistent shape of k_bdraw_tiled, and the PTA array kernels at other NF classes than 60.

gs_bdraw_tiled launches one resident round of workgroups when the classic grid (one workgroup per
pulsar and 16 chains) needs more than one; workgroup w then draws the (pulsar, 4-chain group) items
[w n / G, (w + 1) n / G) in pulsar-major order, restaging the model block where its range crosses a
pulsar.  GS_OPT_LAST_BDRAW_PERSIST reports G, so these tests can tell that the branch ran.  gs_bdraw
on the row-major blocks (k_bdraw, never persistent) is the same arithmetic: every b and info must
equal it bit for bit, and a system the ranges dropped would keep its sentinel.

References: the x87 long-double draw (tests/parity_data, 1e-9 normwise) on the device's own Philox
normals restated from the counters (oracle.philox4x32), oracle.lnlike_fullmarg (1e-10 relative),
and tests/hyper_ref.py for gs_hyper_mh (x entry for entry)."""
import numpy as np
import pytest

from oracle import gibbs_oracle as O
from tests import hyper_ref as H
from tests.parity_data import exact_chol_draw_pre, exact_tnt, normwise_rel

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 77
SENTINEL = 7.0
WPB, LOOP = 4, 4        # chains per item (GS_BDRAW_WPB) and items per classic workgroup (GS_BDRAW_LOOP)


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=SEED)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _array_model(ctx, models, NF):
    """DeviceModel of array pulsars (T = [M | F]): the free-spectrum columns follow the timing model's."""
    from pulsar_timing_gibbsspec_amd.engine import DeviceModel
    T = [m.get_basis() for m in models]
    N = [m.get_ndiag({}) for m in models]
    R = [m.residuals for m in models]
    nm = [t.shape[1] - NF for t in T]
    gwid = [n + np.arange(NF) for n in nm]
    return DeviceModel(ctx, T, N, R, gwid, [np.full(n, 1e-40) for n in nm]), T, N, R


def _ragged(kind, n=3, n_f=30):
    """n = 3 or 5 pulsars of the 45-pulsar array with ragged timing-model sizes: the smallest, one of
    17 columns (row-major fixed block), the largest <= 16 (tiled) [, the other of 17, a middle one]."""
    from pulsar_timing_gibbsspec_amd import synthetic
    pta = synthetic.array_pta(kind=kind, n_f=n_f, seed=0)
    nM = np.array([m.get_basis().shape[1] - 2 * n_f for m in pta.models])
    big = [int(i) for i in np.nonzero(nM == 17)[0]]
    small = [int(np.nonzero(nM == v)[0][0]) for v in sorted(set(nM[nM <= 16]))]
    assert len(small) >= 3 and len(big) >= 2
    sel = [small[0], big[0], small[-1], big[1], small[len(small) // 2]][:n]
    assert len({int(nM[i]) for i in sel[:3]}) == 3
    return [pta.models[i] for i in sel]


def _both_draws(ctx, model, C, phi, mask=None, sweep=3, chain_base=1000, lnl=None):
    """gs_bdraw on the row-major blocks and gs_bdraw_tiled on the tiled ones, device Philox, b
    pre-filled with a sentinel.  Returns [(b, info)] x 2 and the persistent workgroup count of the
    tiled launch; lnl (device tensor): attached to the tiled launch (gs_ctx_set_bdraw_lnl)."""
    from pulsar_timing_gibbsspec_amd import _lib
    lib, h = ctx.lib, ctx.handle
    out = []
    persist = None
    for tiled in (False, True):
        fn, mb = (lib.gs_bdraw_tiled, model.model_tiled) if tiled else (lib.gs_bdraw, model.model)
        b = torch.full((model.P * C, model.ldb), SENTINEL, dtype=torch.float64, device="cuda")
        info = torch.full((model.P * C,), -9, dtype=torch.int32, device="cuda")
        if tiled and lnl is not None:
            _lib.check(lib.gs_ctx_set_bdraw_lnl(h, _lib.ptr(lnl), _lib.ptr(model.model)), "attach")
        try:
            _lib.check(fn(h, model.P, C, model.NF, model.NMX, model.ldb, _lib.ptr(mb), _lib.ptr(model.fidx),
                          _lib.ptr(model.midx), _lib.ptr(model.nm_dev), _lib.ptr(phi), None, sweep, _lib.EV_B,
                          chain_base, _lib.ptr(mask), _lib.ptr(b), _lib.ptr(info)), "bdraw")
        finally:
            if tiled and lnl is not None:
                _lib.check(lib.gs_ctx_set_bdraw_lnl(h, None, None), "detach")
        if tiled:
            persist = ctx.get_option(_lib.OPT_LAST_BDRAW_PERSIST)
        out.append((b.cpu().numpy(), info.cpu().numpy()))
    return out, persist


def _philox_normals(model, p, chain, sweep, psr_base=0):
    """The normals bdraw_item draws for system (p, chain): lane l's counter (l, sweep, chain,
    (p + psr_base) << 8 | GS_EV_B) gives the Box-Muller pair (z of free-spectrum column fidx[l], z
    of fixed column midx[l])."""
    from pulsar_timing_gibbsspec_amd import _lib
    ctr = np.zeros((64, 4), np.uint32)
    ctr[:, 0] = np.arange(64)
    ctr[:, 1] = sweep & 0xffffffff
    ctr[:, 2] = chain & 0xffffffff
    ctr[:, 3] = ((p + psr_base) << 8) | _lib.EV_B
    key = np.repeat(np.array([[SEED & 0xffffffff, SEED >> 32]], np.uint32), 64, axis=0)
    n1, n2 = O.box_muller(*O.philox_uniform_pair(ctr, key))
    z = np.zeros(int(model.m[p]))
    z[model.fidx_host[p]] = n1[:model.NF]
    z[model.midx_host[p]] = n2[:int(model.nm[p])]
    return z


def _check_exact(model, T, N, R, b, phi_of, systems, sweep, chain_base):
    """b of the (p, c) systems against the exact long-double draw at 1e-9."""
    tl = {}
    for p, c in systems:
        if p not in tl:
            tl[p] = exact_tnt(T[p], N[p], R[p])
        m = int(model.m[p])
        ph = np.full(m, 1e-40)
        ph[model.fidx_host[p]] = phi_of(p, c)
        order = O.chol_order(m, model.fidx_host[p])
        z = _philox_normals(model, p, chain_base + c, sweep)
        bx = exact_chol_draw_pre(tl[p], ph, z, order)
        err = normwise_rel(b[p * b.shape[0] // model.P + c, :m], bx)
        assert err < 1e-9, (p, c, err)


def _assert_same(out, model, C, shut=None):
    """Bit equality of the two launches on the written columns; shut systems keep the sentinel."""
    (b0, i0), (b1, i1) = out
    assert np.array_equal(i0, i1)
    for p in range(model.P):
        rows, m = slice(p * C, (p + 1) * C), int(model.m[p])
        assert np.array_equal(b0[rows, :m], b1[rows, :m]), p
        open_ = np.ones(C, bool) if shut is None else ~shut
        assert not (b1[rows, :m][open_] == SENTINEL).any(), p     # every open system was drawn ...
        assert not i1[rows][open_].any(), p                       # ... and factorised
        if shut is not None:
            assert shut.any() and np.all(b1[rows][shut] == SENTINEL) and np.all(i1[rows][shut] == -9)


# ------------------------------------------------------------------ 1, 2. persistent ranges
C_PERSIST = 11003       # odd: a ragged last chain group; 3 x 688 classic workgroups, 8253 items


@pytest.mark.parametrize("P,C,classic", [(3, C_PERSIST, 3 * 688), (5, 4099, 5 * 257)])
def test_bdraw_tiled_persistent_ranges_equal_row_major_draw(ctx, P, C, classic):
    """k_bdraw_tiled<60, 0, 4, false, false> in its persistent shape on ragged pulsars (nM = 17,
    row-major, between tiled ones): 3 x 11003 chains (3 x 688 classic workgroups, 8253 items) and
    5 x 4099 (5 x 257, 5125 items), both more than a resident round of a 256-CU device, so G
    workgroups take uneven item ranges whose boundaries fall inside pulsars.  A G divisible by 3 (e.g.
    3 workgroups per CU) aligns the first case's pulsar boundaries with range boundaries; no
    plausible G = k x CUs is divisible by 5, so in the second case ranges cross pulsars mid-range
    (the restage, fi / mi / nM and the per-pulsar view change inside the item loop; asserted).
    b and info equal k_bdraw's bit for bit, unmasked and with ~30 % of the chains shut (those keep
    the sentinel); 0 < G < classic; the first and last chain of every pulsar and the chains either
    side of three range boundaries equal the exact draw on the restated Philox normals (1e-9)."""
    model, T, N, R = _array_model(ctx, _ragged("curn", P), 60)
    assert model.P == P and model.NMX == 17 and min(model.nm) <= 16 and model.model_tiled is not None
    sweep, chain_base = 3, 1000
    rng = np.random.default_rng(5)
    phi = 10.0 ** rng.uniform(12, 16, (P * C, 60))
    phid = dev(phi)
    nb = -(-C // WPB)
    assert classic == P * -(-nb // LOOP)
    out, G = _both_draws(ctx, model, C, phid, sweep=sweep, chain_base=chain_base)
    assert 0 < G < classic, (G, classic)
    _assert_same(out, model, C)
    n_items = P * nb
    assert n_items % G, (n_items, G)                   # uneven ranges
    crossing = [k for k in range(1, P) if (k * nb * G) % n_items]   # pulsar boundaries strictly inside a range
    assert crossing or P == 3, (G, n_items)
    systems = [(p, c) for p in range(P) for c in (0, C - 1)]
    for w in (G // 4, G // 2, (3 * G) // 4):           # items lo - 1 | lo of workgroup w's range
        lo = w * n_items // G
        assert 0 < lo < n_items
        systems += [((lo - 1) // nb, min(((lo - 1) % nb) * WPB + WPB - 1, C - 1)), (lo // nb, (lo % nb) * WPB)]
    assert len(set(systems)) == 2 * P + 6
    _check_exact(model, T, N, R, out[1][0], lambda p, c: phi[p * C + c], systems, sweep, chain_base)
    shut = rng.uniform(size=C) < 0.3
    out, G2 = _both_draws(ctx, model, C, phid, mask=dev((~shut).astype(np.int32), torch.int32), sweep=sweep,
                          chain_base=chain_base)
    assert G2 == G
    _assert_same(out, model, C, shut=shut)
    from pulsar_timing_gibbsspec_amd import _lib
    with pytest.raises(_lib.GibbsLibError):            # the option is read only
        ctx.set_option(_lib.OPT_LAST_BDRAW_PERSIST, 1)
    assert ctx.get_option(_lib.OPT_LAST_BDRAW_PERSIST) == G


def test_bdraw_tiled_persistent_lnl_output(ctx):
    """k_bdraw_tiled<60, 0, 4, false, true> in its persistent shape (the curn_plred sweep's gated
    draw): a curn_plred engine of the same three pulsars x 11003 chains, a mixed gate.  lnl_p of
    every system, drawn or shut, equals gs_lnlike_marg bit for bit, b of the shut systems is
    unchanged, the open ones are drawn."""
    from pulsar_timing_gibbsspec_amd import PTABlockGibbs, _lib, synthetic
    from pulsar_timing_gibbsspec_amd._lib import check, ptr
    pta = synthetic.PTA(_ragged("curn_plred"))
    C = C_PERSIST
    gb = PTABlockGibbs(pta, nchains=C, seed=11)
    x0 = np.concatenate([np.atleast_1d(p.sample()).ravel() for p in gb.params])
    eng = gb._new_engine(x0)
    m, lib, h = eng.model, eng.ctx.lib, eng.ctx.handle
    assert m.NMX == 17 and eng.hyper is not None and not eng.phi_shared
    rng = np.random.default_rng(6)
    eng.phiinv_F.copy_(dev(10.0 ** rng.uniform(12, 16, (m.P * C, m.NF))))
    eng.b.fill_(SENTINEL)
    want = torch.empty(m.P * C, dtype=torch.float64, device="cuda")
    check(lib.gs_lnlike_marg(h, m.P, C, m.NF, m.NMX, ptr(m.model), 0, ptr(m.nm_dev), ptr(eng.phiinv_F), ptr(want),
                             None), "gs_lnlike_marg")
    assert torch.isfinite(want).all()
    gate = torch.as_tensor((rng.uniform(size=C) >= 0.3).astype(np.int32), device="cuda")
    sys_open = gate.repeat(m.P).bool()
    eng.hyper.lnl_p.fill_(float("nan"))
    eng._bdraw(None, _lib.EV_B, gate)
    G = eng.ctx.get_option(_lib.OPT_LAST_BDRAW_PERSIST)
    nb = -(-C // WPB)
    assert 0 < G < m.P * -(-nb // LOOP), G
    assert eng.ctx.get_option(_lib.OPT_LAST_SWEEP_SHAPE) == 2
    assert torch.equal(eng.hyper.lnl_p, want)
    assert bool((~sys_open).any()) and bool((eng.b[~sys_open] == SENTINEL).all())
    m_sys = torch.as_tensor(m.m, device="cuda").repeat_interleave(C)
    cols = torch.arange(m.ldb, device="cuda")[None, :] < m_sys[:, None]        # the columns each system writes
    assert not bool(((eng.b == SENTINEL) & cols)[sys_open].any())
    assert not eng.info.cpu().numpy().any()


# ------------------------------------------------------------------ 3. array kernels at other NF
ARRAY_NF_CASES = ([(n_f, 3, n_f in (8, 10, 32)) for n_f in (7, 8, 10, 16, 20, 24, 30, 32)]         # NMX = 15: FX
                  + [(n_f, "ragged", n_f in (7, 16, 24)) for n_f in (7, 8, 10, 16, 24, 30, 32)]    # NMX = 17
                  + [(20, None, False)])                                                           # all 45: NMX = 17


@pytest.mark.parametrize("n_f,n_psr,phi_shared", ARRAY_NF_CASES)
def test_array_bdraw_tiled_any_nf(ctx, n_f, n_psr, phi_shared):
    """k_bdraw_tiled<NFC, NTC, 4, FX, LNLD> in every NF class (NF = 14, 16, 20, 32, 40, 48, 60, 64) on
    the curn array with the fixed blocks in tiles (the first three pulsars, NMX = 15: FX) and
    row-major (three ragged pulsars around one of 17 columns; n_f = 20 on all 45), 37 chains, both
    phiinv layouts: b and info equal gs_bdraw's bit for bit without and with the lnL output attached
    (LNLD); the lnL output equals gs_lnlike_marg bit for bit and lnlike_fullmarg to 1e-10 relative,
    and the first and last chain of every pulsar the exact draw (1e-9)."""
    from pulsar_timing_gibbsspec_amd import _lib, synthetic
    if n_psr == "ragged":
        models = _ragged("curn", 3, n_f)
    else:
        models = synthetic.array_pta(kind="curn", n_f=n_f, n_psr=n_psr, seed=0).models
    NF = 2 * n_f
    model, T, N, R = _array_model(ctx, models, NF)
    assert model.NMX == (15 if n_psr == 3 else 17) and model.model_tiled is not None
    C, sweep, chain_base = 37, 2, 50
    rng = np.random.default_rng(n_f)
    rows = C if phi_shared else model.P * C
    phi = 10.0 ** rng.uniform(12, 16, (rows, NF))
    phid = dev(phi)
    phi_full = dev(np.tile(phi, (model.P, 1))) if phi_shared else phid
    lnl = torch.full((model.P * C,), float("nan"), dtype=torch.float64, device="cuda")
    prev = ctx.get_option(_lib.OPT_PHI_PER_CHAIN)
    ctx.set_option(_lib.OPT_PHI_PER_CHAIN, int(phi_shared))
    try:
        plain, G0 = _both_draws(ctx, model, C, phid, sweep=sweep, chain_base=chain_base)
        with_lnl, G1 = _both_draws(ctx, model, C, phid, sweep=sweep, chain_base=chain_base, lnl=lnl)
    finally:
        ctx.set_option(_lib.OPT_PHI_PER_CHAIN, prev)
    assert G0 == 0 and G1 == 0                      # at most 45 x 3 workgroups: the classic grid
    _assert_same(plain, model, C)
    _assert_same(with_lnl, model, C)
    assert np.array_equal(plain[1][0], with_lnl[1][0])
    systems = [(p, c) for p in range(model.P) for c in (0, C - 1)]
    _check_exact(model, T, N, R, plain[1][0], lambda p, c: phi[c if phi_shared else p * C + c], systems, sweep,
                 chain_base)
    want = torch.empty_like(lnl)
    _lib.check(ctx.lib.gs_lnlike_marg(ctx.handle, model.P, C, NF, model.NMX, _lib.ptr(model.model), 0,
                                      _lib.ptr(model.nm_dev), _lib.ptr(phi_full), _lib.ptr(want), None),
               "gs_lnlike_marg")
    assert torch.equal(lnl, want)
    full = (lnl + model.lnl_constants().repeat_interleave(C)).cpu().numpy()
    for p, c in systems:
        TNT, d = O.tnt(T[p], N[p], R[p])
        ph = np.full(int(model.m[p]), 1e-40)
        ph[model.fidx_host[p]] = phi[c if phi_shared else p * C + c]
        ref = O.lnlike_fullmarg(R[p], N[p], TNT, d, ph, -np.sum(np.log(ph)))
        assert abs(full[p * C + c] - ref) <= 1e-10 * abs(ref), (p, c, full[p * C + c], ref,
                                                                abs(full[p * C + c] - ref) / abs(ref))


# ------------------------------------------------------------------ 4. hyper MH at other NF
@pytest.mark.parametrize("n_f,seed", H.MH_CASES)
def test_hyper_mh_any_nf_matches_numpy_block(n_f, seed):
    """k_hyper_mh<0, 1> (NF = 14) and <40, 0> on the 3-pulsar curn_plred array, 4 chains, 70 injected
    steps (the 64-step proposal table refilled once): x after the block equals the numpy
    restatement entry for entry and the accepted counts agree.  The committed draws have no step an
    fp64 likelihood could not decide (tests/test_nf_matrix_ref.py), so nothing is skipped."""
    from pulsar_timing_gibbsspec_amd import PTABlockGibbs
    pta, x0, rows, x_out, n_acc, n_tie = H.mh_case(n_f, seed)
    assert not n_tie.any()
    C = H.MH_CHAINS
    gb = PTABlockGibbs(pta, hypersample="conditional", redsample="mh", nchains=C, seed=3)
    assert np.array_equal(gb.get_hyper_param_indices(), H.hyper_indices(pta.param_names))
    eng = gb._new_engine(x0[0])
    assert eng.model.NF == 2 * n_f and eng.hyper_pl
    eng.x.copy_(dev(x0))
    eng.hyper_block(H.MH_STEPS, inj=dev(rows))
    got = eng.x.cpu().numpy()
    assert np.array_equal(got, x_out), np.argwhere(got != x_out)
    acc = eng.hyper.n_acc.cpu().numpy()
    assert np.array_equal(acc, n_acc), (acc, n_acc)
    assert np.all((0 < acc) & (acc < H.MH_STEPS))
