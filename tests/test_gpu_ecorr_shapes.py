"""The basis-ECORR kernels (csrc/gibbs_ecorr.hip) at every tile class, block width and epoch edge, against the
long-double references of tests/ecorr_ref.py (its cases: NF = 20 / 40 / 60 <-> k_ecorr_prefix NB = 3 / 4 / 5,
nM = 1 / 5 / 15 / 16 and NMX > nM, the unfused route with m_R = 37 / 47 / 95 <-> k_ecorr_schur NB = 3 / 3 / 6,
ne = 0 .. 65, a backend that owns no epoch).  Chain counts are no multiples of the 4-chain workgroup and
fill more than one.

* a. gs_ecorr_prefix, likelihood and block mode, shared operands at a 16-byte aligned and an 8-byte offset
  address and per-chain copies with an even and an odd chain stride: lnl bit-identical across the four and
  1e-9 max(1, |ref|) from prefix_ref, aux at rtol 1e-11 (1e-13 across the four), every section of the model
  block 1e-9 normwise, Rm zero outside [0, nM)^2, the block's tail zero;
* b. the three device forms of the likelihood 1e-7 max(1, |ref|) from the dense long-double lnlike_ref, the
  fused and the unfused model block 1e-9 normwise from each other, PulsarBlockGibbs.get_lnlikelihood with
  fixed and with sampled white noise, the two per-chain operand routes 1e-12 from each other;
* d. the Metropolis block on injected draws bit-identical to mh_ref's (no step exempt: tests/test_ecorr_ref.py
  holds every step's margin above 4e-9 max |lnL|), incremental steps against full evaluations on Philox draws;
* e. the b draw: conditional mean 1e-8 normwise from bdraw_ref, max |G^T Sigma G - I| < 1e-6, the E / R
  columns at ecid / rcol of a padded b, a mixed chain_mask on the unfused route.
  (c, the Schur kernel alone, is test_ecorr_schur_direct of tests/test_gpu_ecorr.py.)

Largest errors seen on the MI355X (each family over all its cases):
  a. lnl 1.1e-14 (bound 1e-9), aux 4.0e-16 (1e-11); block sections S0 2.3e-14, dF 4.4e-14, Gm 2.6e-14,
     hm 1.7e-14, Rm 1.1e-14, am 1.5e-15 (1e-9); lnl bit-identical and aux equal across the four forms;
  b. likelihood mode 2.8e-15, fused block 2.7e-15, unfused 1.8e-13 (1e-7); fused vs unfused block 5.7e-14
     (1e-9); PulsarBlockGibbs 5.3e-15 (1e-7); operand routes 2.0e-16 (1e-12);
  c. test_ecorr_schur_direct, every row (the tile-edge ones against schur_ref): 6.5e-16 entrywise (1e-12);
  d. every injected decision the reference's; incremental vs full lnl0 4.8e-13 (1e-9), stored state
     8.4e-15 (1e-11);
  e. conditional mean 1.9e-12 (1e-8), max |G^T Sigma G - I| 1.7e-12 (1e-6).
"""
import numpy as np
import pytest

from tests import ecorr_ref as E
from tests.conftest import gpu_available
from tests.parity_data import normwise_rel

pytestmark = pytest.mark.gpu

C_PREFIX = 6      # two workgroups, the second half full
RHO = (-9.0, -4.0)


@pytest.fixture(scope="module")
def ctx():
    if not gpu_available():
        pytest.skip("no GPU")
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=11)


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.array(a, order="C"), dtype=dtype or torch.float64, device="cuda")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _note(family, value):
    print(f"ECORR-SHAPES {family} {float(value):.3e}")


def _em(ctx, c, C, per_chain=False, ecid=None, ebk=None):
    from pulsar_timing_gibbsspec_amd.ecorr import EcorrModel
    return EcorrModel(ctx, c["T"], c["N"], c["r"], c["ecid"] if ecid is None else ecid,
                      c["ebk"] if ebk is None else ebk, c["gwid"], c["eind"], c["emin"], c["emax"], c["n_param"], C,
                      per_chain=per_chain)


def _white_list(c):
    names = c["names"]
    return [(int(j), 0 if names[j].endswith("efac") else 1, int(names[j].split("_b")[1].split("_")[0]),
             float(c["bounds"][names[j]][0]), float(c["bounds"][names[j]][1])) for j in c["wind"]]


def _white_models(ctx, c, C):
    from pulsar_timing_gibbsspec_amd.ecorr import white_ecorr_models
    return white_ecorr_models(ctx, c["T"], c["r"], c["sigma"], c["backends"], c["gwid"], _white_list(c), c["ecid"],
                              c["ebk"], c["eind"], c["emin"], c["emax"], c["n_param"], C)


# ------------------------------------------------------------------ a. the fused prefix
def _prefix_forms(ctx, em, c, X, ne, NMX=None, shared_only=False):
    """gs_ecorr_prefix on the first ne epochs of em's operands, both modes, in the four operand forms:
    [(lnl, aux, block (C x mstride), aux of the block mode)] and the host copies of the operands."""
    import torch
    from pulsar_timing_gibbsspec_amd._lib import check, ptr
    C, NF, KB, nM = X.shape[0], em.NF, em.ldbp, em.nm
    NMX = nM if NMX is None else NMX
    mstride = int(ctx.lib.gs_model_stride(NF, NMX))
    n1 = max(ne, 1)                                     # ne = 0: one-row dummies, never read
    Bp = em.Bp[:n1].contiguous()
    Dg, ebk = em.Dg[:n1].contiguous(), em.ebk[:n1].contiguous()
    Ap = em.Ap
    x, phf = _dev(X), _dev(E.phiinv_F(c, X))

    def run(Bx, Dgx, Apx, strides):
        out = []
        for lnl_mode in (True, False):
            lnl = torch.full((C,), np.nan, dtype=torch.float64, device="cuda")
            aux = torch.full((C, 4), np.nan, dtype=torch.float64, device="cuda")
            info = torch.full((C,), -1, dtype=torch.int32, device="cuda")
            # NMX > nM leaves rows nM.. of Gm / hm alone: zero there, as the reference has them
            model = torch.full((C, mstride), 0.0 if NMX > nM else np.nan, dtype=torch.float64, device="cuda")
            check(ctx.lib.gs_ecorr_prefix(ctx.handle, C, NF, NMX, nM, ne, KB, ptr(Bx), ptr(Dgx), ptr(ebk), em.n_bk,
                                          ptr(em.ecol), ptr(x), x.shape[1], ptr(Apx), ptr(phf) if lnl_mode else None,
                                          None if lnl_mode else ptr(model), ptr(aux), ptr(lnl) if lnl_mode else None,
                                          ptr(info), *strides), "gs_ecorr_prefix")
            assert int(info.abs().max()) == 0
            out += [lnl.cpu().numpy(), aux.cpu().numpy()] if lnl_mode else [model.cpu().numpy(), aux.cpu().numpy()]
        return out

    off = torch.zeros(n1 * KB + 1, dtype=torch.float64, device="cuda")
    off[1:] = Bp.reshape(-1)
    assert Bp.data_ptr() % 16 == 0 and off[1:].data_ptr() % 16 == 8
    outs = [run(Bp, Dg, Ap, (0, 0, 0)), run(off[1:], Dg, Ap, (0, 0, 0))]
    if not shared_only:
        for extra in (0, 1):
            cs = ne * KB + extra
            Bc = torch.zeros(C * cs, dtype=torch.float64, device="cuda")
            for ch in range(C):
                Bc[ch * cs:ch * cs + ne * KB] = Bp.reshape(-1)
            Dc = Dg.repeat(C).contiguous()
            Ac = Ap.reshape(1, -1).repeat(C, 1).contiguous()
            outs.append(run(Bc, Dc, Ac, (cs, ne, KB * KB)))
    host = (Bp.cpu().numpy()[:ne], Dg.cpu().numpy()[:ne], ebk.cpu().numpy()[:ne], Ap.cpu().numpy())
    return outs, host


def _check_prefix(c, X, outs, host, NF, nM, NMX):
    C = X.shape[0]
    Bn, Dn, En, An = host
    sizes = E.section_sizes(NF, NMX)
    cut, used = np.cumsum(sizes)[:-1], sum(sizes)
    lnl0, aux0, blk0, bax0 = outs[0]
    for lnl, aux, blk, bax in outs[1:]:
        assert np.array_equal(lnl, lnl0)
        np.testing.assert_allclose(aux, aux0, rtol=1e-13, atol=0)
        np.testing.assert_allclose(bax, bax0, rtol=1e-13, atol=0)
    refs = [E.prefix_ref(Bn, Dn, En, An, X[ch], c["eind"], E.phiinv_F(c, X[ch])[0], NF, nM, NMX) for ch in range(C)]
    want = np.array([float(r["lnl"]) for r in refs])
    err = np.abs(lnl0 - want) / np.maximum(1.0, np.abs(want))
    _note("a.lnl", err.max())
    assert err.max() < 1e-9, (lnl0, want)
    waux = _f64([r["aux_lnl"] for r in refs])
    _note("a.aux", np.max(np.abs(aux0 - waux) / np.maximum(np.abs(waux), 1e-300)))
    np.testing.assert_allclose(aux0, waux, rtol=1e-11, atol=0)
    wblk = _f64([r["block"] for r in refs])
    for lnl, aux, blk, bax in outs:
        np.testing.assert_allclose(bax, _f64([r["aux_block"] for r in refs]), rtol=1e-11, atol=0)
        for k, (got, ref) in enumerate(zip(np.split(blk[:, :used], cut, axis=1), np.split(wblk, cut, axis=1))):
            e = normwise_rel(got, ref)
            _note("a.block." + E.SECTIONS[k], e)
            assert e < 1e-9, (E.SECTIONS[k], e)
        assert not blk[:, used:].any()                  # the tail, as the kernel writes it
        Rm = np.split(blk[:, :used], cut, axis=1)[4].reshape(C, NMX, NMX)
        assert not Rm[:, nM:, :].any() and not Rm[:, :, nM:].any()


@pytest.mark.parametrize("name", E.FUSED)
def test_prefix_every_nb_and_nm(ctx, name):
    """NB = 3 / 4 / 5 and nM = 1 / 5 / 15 / 16 at the model's own ~35 epochs."""
    c = E.case(name)
    X = E.draws(c, C_PREFIX)
    em = _em(ctx, c, C_PREFIX)
    assert em.fused and em.ldbp == 16 * (1 + (c["NF"] + 16) // 16) and em.nm == c["nm"]
    outs, host = _prefix_forms(ctx, em, c, X, em.ne)
    _check_prefix(c, X, outs, host, em.NF, em.nm, em.nm)


@pytest.mark.parametrize("ne", (0,) + E.EDGE_NE)
@pytest.mark.parametrize("name", ("E20", "E40"))
def test_prefix_epoch_edges(ctx, name, ne):
    """The first ne epochs of a >= 65-epoch model at NB = 3 / 4: partial and exact 32-epoch shared chunks,
    8-epoch per-chain chunks and 64-epoch weight segments; ne = 0 (shared operands: one-row dummies, the
    kernel issues no epoch load) is the R system alone."""
    c = E.case(name)
    X = E.draws(c, C_PREFIX)
    em = _em(ctx, c, C_PREFIX)
    assert em.ne >= 65
    outs, host = _prefix_forms(ctx, em, c, X, ne, shared_only=ne == 0)
    _check_prefix(c, X, outs, host, em.NF, em.nm, em.nm)
    if ne == 0:
        assert not outs[0][1].any()


def test_prefix_nmx_above_nm(ctx):
    """M5 through the C-ABI with NMX = nM + 3: the fixed-block sections strided by NMX."""
    c = E.case("M5")
    X = E.draws(c, C_PREFIX)
    em = _em(ctx, c, C_PREFIX)
    outs, host = _prefix_forms(ctx, em, c, X, em.ne, NMX=em.nm + 3)
    _check_prefix(c, X, outs, host, em.NF, em.nm, em.nm + 3)


# ------------------------------------------------------------------ b. the likelihood's device forms
def _lnl_refs(c, X):
    out = []
    for x in X:
        phiinv, ld = E.phiinv_full(c, x)
        out.append(float(E.lnlike_ref(c["T"], c["N"], c["r"], phiinv, ld)[0]))
    return np.array(out)


@pytest.mark.parametrize("name", ("A20", "A40", "M1", "M15") + E.UNFUSED)
def test_lnlike_forms_match_dense_reference(ctx, name):
    """EcorrModel.lnlike through the likelihood mode, through the fused block + gs_lnlike_marg and through
    gs_ecorr_schur + gs_prefix_sys + gs_lnlike_marg (the only form when nm > 16) against lnlike_ref from
    (T, N, r); the fused and the unfused model block against each other."""
    c = E.case(name)
    C = 6
    X = E.draws(c, C)
    em = _em(ctx, c, C)
    assert em.fused == (name in E.FUSED) and em.mR == c["NF"] + c["nm"]
    ref = _lnl_refs(c, X)
    x, phf = _dev(X), _dev(E.phiinv_F(c, X))
    modes = ("lnl", "block", "unfused") if em.fused else ("unfused",)
    for mode in modes:
        em.fused = mode != "unfused"
        em.fused_lnl = mode == "lnl"
        got = em.lnlike(x, phf).cpu().numpy()
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        _note("b.lnlike." + mode, err.max())
        assert err.max() < 1e-7, (mode, got, ref)
    if name in E.FUSED:
        em.factor(x, fused=True)
        a = em.model.clone()
        em.factor(x, fused=False)
        sizes = E.section_sizes(em.NF, em.NMX)
        cut = np.cumsum(sizes)[:-1]
        A = a.view(C, -1).cpu().numpy()[:, :sum(sizes)]
        B = em.model.view(C, -1).cpu().numpy()[:, :sum(sizes)]
        for k, (sa, sb) in enumerate(zip(np.split(A, cut, axis=1), np.split(B, cut, axis=1))):
            _note("b.blocks", normwise_rel(sa, sb))
            assert normwise_rel(sa, sb) < 1e-9, E.SECTIONS[k]


@pytest.mark.parametrize("name", ("A20", "A40", "W20", "W40"))
def test_pulsar_block_gibbs_lnlikelihood(ctx, name):
    """PulsarBlockGibbs.get_lnlikelihood at NF = 20 / 40 with fixed white noise and with white noise
    sampled (gs_white_tnt -> gs_ecorr_gather -> the per-chain kernels at kb = 48 / 64), against lnlike_ref at
    that chain's N."""
    from pulsar_timing_gibbsspec_amd.pulsar_gibbs import PulsarBlockGibbs
    c = E.case(name)
    pta = c["pta"]
    gb = PulsarBlockGibbs(pta, nchains=4, seed=3)
    for x in E.draws(c, 3):
        params = pta.map_params(x)
        N = pta.get_ndiag(params)[0]
        phiinv, ld = pta.get_phiinv(params, logdet=True)[0]
        ref = float(E.lnlike_ref(c["T"], N, c["r"], phiinv, ld)[0])
        got = gb.get_lnlikelihood(x)
        _note("b.gibbs", abs(got - ref) / max(1.0, abs(ref)))
        assert abs(got - ref) < 1e-7 * max(1.0, abs(ref)), (name, got, ref)
    assert gb._em1.per_chain == c["white"] and gb._em1.ldbp == (48 if c["NF"] == 20 else 64)


@pytest.mark.parametrize("name", ("W20", "W40"))
def test_white_operand_routes_agree(ctx, name):
    """Per-chain operands by the full m x m SYRK + gs_ecorr_gather and by the R-column SYRK +
    gs_ecorr_epoch_sums: equal to 1e-12 (test_ecorr_white_operand_routes_agree at NF = 20 / 40)."""
    from pulsar_timing_gibbsspec_amd.ecorr import EcorrWhiteChains
    c = E.case(name)
    C = 6
    X = E.draws(c, C)
    wm, wmR, em = _white_models(ctx, c, C)
    run = EcorrWhiteChains(wm, em, c["gw"], c["gwid"], RHO[0], RHO[1], X[0], 1, 1, wmR=wmR)
    run.x.copy_(_dev(X))
    run._operands()
    A = [t.clone().cpu().numpy() for t in (em.Bp, em.Dg, em.Ap)]
    run.wmR = None
    run._operands()
    B = [t.cpu().numpy() for t in (em.Bp, em.Dg, em.Ap)]
    for a, b in zip(A, B):
        a, b = a.reshape(C, -1), b.reshape(C, -1)
        _note("b.routes", normwise_rel(a, b))
        assert normwise_rel(a, b) < 1e-12, normwise_rel(a, b)


# ------------------------------------------------------------------ d. the Metropolis block
@pytest.mark.parametrize("name", E.MH_CASES)
def test_mh_matches_reference(ctx, name):
    """EcorrModel.mh on injected rows, incremental steps on and off, against mh_ref: the final x
    bit-identical, the accept counts equal; EMPTY: backend 1 of 3 owns no epoch (nch = 0)."""
    import torch
    c = E.case(name)
    X0, inj, Xo, acc, marg, lmax = E.mh_case(name)
    assert marg.min() > E.MH_MARGIN_REL * lmax          # every step is compared
    C = X0.shape[0]
    em = _em(ctx, c, C)
    if name == "EMPTY":
        assert em.n_bk == 3 and em.eoff_host[1] == em.eoff_host[2] and em.eoff_host[-1] == em.ne
    phf = _dev(E.phiinv_F(c, X0))
    for inc in (True, False):
        em.incremental = inc
        x = _dev(X0).clone()
        n_acc = torch.zeros(C, dtype=torch.int32, device="cuda")
        em.mh(x, phf, inj.shape[0], inj=_dev(inj), n_acc=n_acc)
        assert np.array_equal(x.cpu().numpy(), Xo), (inc, np.abs(x.cpu().numpy() - Xo).max())
        assert np.array_equal(n_acc.cpu().numpy(), acc)
        assert int(em.pinfo.abs().max()) == 0


def _split_case(name):
    """E20 / E40 with backend 0 owning the first 67 epochs: backend 1's range starts off a multiple of 8
    and backend 0's crosses a 64-epoch weight segment."""
    c = dict(E.case(name))
    c["ebk"] = (np.arange(c["ne"]) >= 67).astype(np.int64)
    return c


@pytest.mark.parametrize("name", E.MH_CASES + ("E20", "E40"))
def test_incremental_steps_match_full(ctx, name):
    """Incremental Metropolis steps against a full evaluation per step on the same Philox draws, 72 steps
    (one REFRESH re-base), shared operands: identical decisions, lnl0 at rtol 1e-9, the stored state within
    1e-11 of a fresh T(x)."""
    from tests.test_gpu_ecorr import _mh_both_ways
    split = name in ("E20", "E40")
    c = _split_case(name) if split else E.case(name)
    C = 13
    X = np.repeat(E.mh_start(c, 1), C, axis=0)
    em = _em(ctx, c, C)
    if split:
        assert em.eoff_host[1] == 67
    (a, b), dev = _mh_both_ways(em, _dev(X), _dev(E.phiinv_F(c, X)), 72)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert a[2].max() > 0
    _note("d.lnl0", np.max(np.abs(a[1] - b[1]) / np.abs(b[1])))
    _note("d.state", dev)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-9, atol=0)
    assert dev < 1e-11, dev


@pytest.mark.parametrize("name", ("W20", "W40"))
def test_white_incremental_steps_match_full(ctx, name):
    """The same with per-chain operands, the chains at different white-noise states."""
    from tests.test_gpu_ecorr import _mh_both_ways
    c = E.case(name)
    C = 13
    X = E.draws(c, C)
    X[:, c["eind"]] = E.mh_start(c, C)[:, c["eind"]]
    wm, _, em = _white_models(ctx, c, C)
    x = _dev(X)
    wm.tnt(x, x.shape[1])
    em.gather(wm.TNT, wm.d, wm.tnt_cstride, wm.d_cstride)
    (a, b), dev = _mh_both_ways(em, x, _dev(E.phiinv_F(c, X)), 72)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    _note("d.lnl0", np.max(np.abs(a[1] - b[1]) / np.abs(b[1])))
    _note("d.state", dev)
    np.testing.assert_allclose(a[1], b[1], rtol=1e-9, atol=0)
    assert dev < 1e-11, dev


# ------------------------------------------------------------------ e. the b draw
SENTINEL = 123.25


def _check_bdraw(c, em, x, N, shuffled=None):
    """C = m + 1 chains at the state x: zero normals, then the unit vectors, into a sentinel-filled b with
    ldb = m + 3."""
    import torch
    m = c["m"]
    C = m + 1
    assert em.C == C
    X = np.broadcast_to(x, (C, x.size)).copy()
    Z = np.zeros((C, m))
    Z[1:] = np.eye(m)
    b = torch.full((C, m + 3), SENTINEL, dtype=torch.float64, device="cuda")
    em.bdraw(_dev(X), _dev(E.phiinv_F(c, X)), b, z=_dev(Z))
    B = b.cpu().numpy()
    assert np.all(B[:, m:] == SENTINEL) and not np.any(B[:, :m] == SENTINEL)
    phiinv, _ = E.phiinv_full(c, x)
    mean, Sig = E.bdraw_ref(c["T"], N, c["r"], phiinv)
    e = normwise_rel(B[0, :m], _f64(mean))
    _note("e.mean", e)
    assert e < 1e-8, e
    G = (B[1:, :m] - B[0, :m]).T
    g = np.abs(_f64(G.T.astype(E.L_) @ Sig @ G.astype(E.L_)) - np.eye(m)).max()
    _note("e.GtSG", g)
    assert g < 1e-6, g
    assert int(em.binfo.max()) == 0 and int(em.binfo.min()) == 0


@pytest.mark.parametrize("name", ("A20", "A40", "M1", "U17", "U35", "E40"))
def test_bdraw_is_exact_conditional(ctx, name):
    """Shared Bx (k_ecorr_bdraw_e<8>): the fused route (ldbx = 48 / 64, ~35 epochs and, E40, a partly
    filled second 64-epoch workgroup) and the unfused one (_jmap_r, dcol = m_R, ldbx = 48 / 96).  M1 hands
    the epoch columns over in a shuffled order."""
    c = E.case(name)
    x = E.draws(c, 1, seed=3)[0]
    ecid = ebk = None
    if name == "M1":
        perm = np.random.default_rng(3).permutation(c["ne"])
        ecid, ebk = c["ecid"][perm], c["ebk"][perm]
        assert not np.all(np.diff(ebk) >= 0)
    em = _em(ctx, c, c["m"] + 1, ecid=ecid, ebk=ebk)
    assert em.fused == (c["nm"] <= 16)
    _check_bdraw(c, em, x, c["N"])


def test_bdraw_per_chain_operands(ctx):
    """Per-chain Bx (k_ecorr_bdraw_e<1>, white noise sampled) at NF = 20, every chain at one N."""
    c = E.case("W20")
    x = E.draws(c, 1, seed=3)[0]
    C = c["m"] + 1
    wm, _, em = _white_models(ctx, c, C)
    xs = _dev(np.broadcast_to(x, (C, x.size)).copy())
    wm.tnt(xs, xs.shape[1])
    em.gather(wm.TNT, wm.d, wm.tnt_cstride, wm.d_cstride)
    assert em.per_chain and em.strides[0] == em.ne * 48
    N = c["pta"].get_ndiag(c["pta"].map_params(x))[0]
    _check_bdraw(c, em, x, N)


def test_bdraw_chain_mask_mixed_unfused(ctx):
    """A mixed chain_mask with 13 chains on the unfused route: masked chains keep their b (both the b_R
    scatter and the b_E draw), unmasked chains equal the unmasked draw."""
    import torch
    c = E.case("U17")
    m, C = c["m"], 13
    em = _em(ctx, c, C)
    assert not em.fused
    X = E.draws(c, C, seed=9)
    Z = np.random.default_rng(5).standard_normal((C, m))
    ref = torch.zeros(C, m, dtype=torch.float64, device="cuda")
    em.bdraw(_dev(X), _dev(E.phiinv_F(c, X)), ref, z=_dev(Z))
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1], np.int32)
    b = torch.full((C, m), SENTINEL, dtype=torch.float64, device="cuda")
    em.bdraw(_dev(X), _dev(E.phiinv_F(c, X)), b, z=_dev(Z), chain_mask=torch.as_tensor(mask, device="cuda"))
    B, R = b.cpu().numpy(), ref.cpu().numpy()
    for ch in range(C):
        if mask[ch]:
            assert np.array_equal(B[ch], R[ch]), ch
        else:
            assert np.all(B[ch] == SENTINEL), ch
