"""The setup kernels at every block edge and scratch path (needs an MI355X): TNT / d
(k_tnt_dd, k_tnr_dd behind gs_tnt_dd; k_tnt, k_tnr behind gs_tnt) and the fixed-prior prefix
(k_prefix_dd behind gs_prefix_dd, gs_prefix_sys, gs_prefix), called through the C ABI and compared
with the mpmath references of tests/setup_ref.py at the kernels' own precision.

The bounds are derived, not fitted (tests/test_setup_ref.py settles them on the CPU against a host
build of the same double-double header and against numpy fp64):
* gs_tnt_dd: |hi + lo - S| <= (n_toa + 16) 2^-104 M, M = sum of |terms| (Dot2's n u^2 plus a few
  u^2 per term from recip_dd / dd_mul_d); a lost low word is ~2^-53 M;
* gs_tnt: 72 * 2^-53 M (one rounding of T / N, 64 fused accumulations per block, two-sums);
* S0, dF: 1 ulp + 2^-70 (|A_fg| + sum |W_if| |W_ig|); the Schur diagonals of the cases cancel by
  4e3..3e5 (median per system), so an fp64-accurate prefix misses by >= 1e3 ulp;
* R, G, h: Higham's componentwise (nM + 4) u |R| |L^T| |R| (x 2 and x |W|, |e| for G, h).
Worst error / bound measured on an MI355X: gs_tnt_dd 0.057 (TNT), 0.013 (d); gs_tnt 0.073, 0.036;
S0 0.497, dF 0.499 and aux1 0.493 (the half ulp of the final rounding; the double-double part is
~1e-10 of its bound); R 0.137, G 0.25, h 0.139 (numpy fp64 gives the same R and G figures); aux0
0.071.  DESIGN.md, "Setup kernels", has the table.
"""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")
torch = pytest.importorskip("torch")

from tests import setup_ref as SR                      # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from pulsar_timing_gibbsspec_amd import _lib
    return _lib.Context(0, seed=5)


class Keep:
    """Device tensors that stay alive until the call's results are read (an inline
    `_lib.ptr(tensor)` would free the temporary and let the allocator alias the next one)."""

    def __init__(self):
        self.held = []

    def __call__(self, a, dtype=torch.float64):
        from pulsar_timing_gibbsspec_amd import _lib
        if a is None:
            return None
        t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()
        self.held.append(t)
        return _lib.ptr(t)

    def out(self, n, dtype=torch.float64, fill=float("nan")):
        """An output buffer of n elements and a guard tail, pre-filled."""
        t = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
        self.held.append(t)
        return t


def _show(what, ratio):
    print(f"[setup-shapes] {what}: worst error / bound = {ratio:.3g}")


# =================================================================================== TNT, d
def run_tnt(ctx, items, fn="gs_tnt_dd", m_max=None, tnt=True, tnt_lo=True, d=True, d_lo=True):
    """One call on a ragged batch.  Returns dict(TNT, TNT_lo, d, d_lo): lists of per-pulsar arrays
    (None where the output was passed as NULL) after checking that the guard tails kept their NaN."""
    from pulsar_timing_gibbsspec_amd import _lib
    K = Keep()
    desc, To, to, no, do = [], 0, 0, 0, 0
    for T, N, r in items:
        n, m = T.shape
        desc.append([n, m, To, to, no, do])
        To, to, no, do = To + n * m, to + n, no + m * m, do + m
    m_max = m_max or max(T.shape[1] for T, _, _ in items)
    dd = fn == "gs_tnt_dd"
    bufs = dict(TNT=K.out(no) if tnt else None, TNT_lo=K.out(no) if (dd and tnt_lo) else None,
                d=K.out(do) if d else None, d_lo=K.out(do) if (dd and d_lo) else None)
    args = [ctx.handle, len(items), m_max, K(np.array(desc, dtype=np.int64), torch.int64),
            K(np.concatenate([T.ravel() for T, _, _ in items])), K(np.concatenate([N for _, N, _ in items])),
            K(np.concatenate([r for _, _, r in items]))]
    P = _lib.ptr
    if dd:
        args += [P(bufs["TNT"]), P(bufs["TNT_lo"]), P(bufs["d"]), P(bufs["d_lo"])]
    else:
        args += [P(bufs["TNT"]), P(bufs["d"])]
    _lib.check(getattr(ctx.lib, fn)(*args), fn)
    torch.cuda.synchronize()
    out = {}
    for k, t in bufs.items():
        if t is None:
            out[k] = None
            continue
        a = t.cpu().numpy()
        assert np.all(np.isnan(a[-GUARD:])), f"{k}: guard tail written"
        parts, o = [], 0
        for T, _, _ in items:
            m = T.shape[1]
            sz = m * m if k.startswith("TNT") else m
            parts.append(a[o:o + sz].reshape((m, m) if k.startswith("TNT") else (m,)))
            o += sz
        out[k] = parts
    return out


@pytest.fixture(scope="module")
def tnt_dd_batch(ctx):
    return run_tnt(ctx, SR.tnt_inputs())


@pytest.fixture(scope="module")
def tnt_batch(ctx):
    return run_tnt(ctx, SR.tnt_inputs(), fn="gs_tnt")


def test_tnt_dd_accuracy(tnt_dd_batch):
    """A1.  Every element of the ragged batch: |hi + lo - S| <= (n_toa + 16) 2^-104 M and
    |hi - S| <= 1 ulp(S) + that; hi and lo exactly symmetric; the same for d.
    Worst ratio to the dd bound measured on an MI355X: TNT 0.0567, d 0.0134 (the host build of the
    same loops gives the same two figures)."""
    got = tnt_dd_batch
    worst = worst_d = 0.0
    for p, ((T, N, r), (S, M, Sd, Md)) in enumerate(zip(SR.tnt_inputs(), SR.tnt_reference())):
        n = T.shape[0]
        hi, lo, dh, dl = got["TNT"][p], got["TNT_lo"][p], got["d"][p], got["d_lo"][p]
        assert not np.isnan(hi).any() and not np.isnan(lo).any(), f"pulsar {p}: unwritten TNT elements"
        assert not np.isnan(dh).any() and not np.isnan(dl).any(), f"pulsar {p}: unwritten d elements"
        b, bd = (n + 16) * 2.0 ** -104 * M, (n + 16) * 2.0 ** -104 * Md
        e, ed = SR.err_dd(hi, lo, S), SR.err_dd(dh, dl, Sd)
        worst, worst_d = max(worst, float(np.max(e / b))), max(worst_d, float(np.max(ed / bd)))
        assert np.all(e <= b), (p, T.shape, float(np.max(e / b)))
        assert np.all(ed <= bd), (p, T.shape, float(np.max(ed / bd)))
        assert np.all(SR.err(hi, S) <= SR.ulp(S) + b), p
        assert np.all(SR.err(dh, Sd) <= SR.ulp(Sd) + bd), p
        assert np.array_equal(hi, hi.T) and np.array_equal(lo, lo.T), p
    _show("gs_tnt_dd TNT", worst)
    _show("gs_tnt_dd d", worst_d)


@pytest.mark.parametrize("null", ["TNT_lo", "d_lo", "both_lo", "TNT", "d"])
def test_tnt_dd_null_outputs(ctx, tnt_dd_batch, null):
    """A2.  NULL low words leave the hi outputs bit-identical; TNT = NULL still writes d and
    d = NULL still writes TNT."""
    kw = dict(TNT_lo=dict(tnt_lo=False), d_lo=dict(d_lo=False), both_lo=dict(tnt_lo=False, d_lo=False),
              TNT=dict(tnt=False, tnt_lo=False), d=dict(d=False, d_lo=False))[null]
    got = run_tnt(ctx, SR.tnt_inputs(), **kw)
    seen = 0
    for k in ("TNT", "TNT_lo", "d", "d_lo"):
        if got[k] is None:
            continue
        for a, b in zip(got[k], tnt_dd_batch[k]):
            assert np.array_equal(a, b), (null, k)          # NaN nowhere: array_equal is bitwise enough
            seen += 1
    assert seen >= 8


@pytest.mark.parametrize("fn", ["gs_tnt_dd", "gs_tnt"])
def test_tnt_batch_invariance_and_containment(ctx, tnt_dd_batch, tnt_batch, fn):
    """A3 / A4.  Each pulsar alone (m_max = its own m, offsets 0) gives the bits of its slice of the
    batch; every element of every block is written over the NaN pre-fill and the guard tail stays
    NaN (checked in run_tnt)."""
    batch = tnt_dd_batch if fn == "gs_tnt_dd" else tnt_batch
    for p, item in enumerate(SR.tnt_inputs()):
        alone = run_tnt(ctx, [item], fn=fn)
        for k, parts in alone.items():
            if parts is None:
                continue
            assert not np.isnan(batch[k][p]).any(), (fn, k, p)
            assert np.array_equal(parts[0], batch[k][p]), (fn, k, p, item[0].shape)


def test_tnt_mfma_accuracy(tnt_batch):
    """A4.  gs_tnt (fp64 MFMA, compensated block sums): |TNT - S| <= 72 * 2^-53 M and the same
    for d.  The kernel does not mirror, so no exact symmetry is asked.  Worst ratio measured on
    an MI355X: TNT 0.0726, d 0.0361."""
    worst = worst_d = 0.0
    for p, ((T, N, r), (S, M, Sd, Md)) in enumerate(zip(SR.tnt_inputs(), SR.tnt_reference())):
        hi, dh = tnt_batch["TNT"][p], tnt_batch["d"][p]
        assert not np.isnan(hi).any() and not np.isnan(dh).any(), p
        e, ed = SR.err(hi, S) / (72 * SR.U * M), SR.err(dh, Sd) / (72 * SR.U * Md)
        worst, worst_d = max(worst, float(e.max())), max(worst_d, float(ed.max()))
        assert np.all(e <= 1.0), (p, T.shape, float(e.max()))
        assert np.all(ed <= 1.0), (p, T.shape, float(ed.max()))
    _show("gs_tnt TNT", worst)
    _show("gs_tnt d", worst_d)


# =================================================================================== prefix
def run_prefix(ctx, NF, NMX, chains, fn="gs_prefix_dd", lo=True, shared=False):
    """chains: [n_chain][n_psr] systems (setup_ref.prefix_inputs dicts; fidx / midx / ph / shapes are
    taken from chain 0).  shared: pass chain 0 with strides 0 and n_chain = len(chains).
    Returns (blocks [n_psr, n_chain, stride], info [n_psr, n_chain]); the model buffer is
    pre-filled with NaN and its guard tail is checked."""
    from pulsar_timing_gibbsspec_amd import _lib
    K = Keep()
    n_chain, n_psr = len(chains), len(chains[0])
    desc, no, do = [], 0, 0
    for s in chains[0]:
        desc.append([s["m"], s["nM"], no, do])
        no, do = no + s["m"] ** 2, do + s["m"]
    src = chains[:1] if shared else chains

    def cat(key):
        return np.concatenate([np.asarray(s[key], dtype=np.float64).ravel() for ch in src for s in ch])

    def pad(key, width, dtype):
        a = np.zeros((n_psr, max(width, 1)), dtype=dtype)
        for p, s in enumerate(chains[0]):
            a[p, :len(s[key])] = s[key]
        return a

    ph = np.full((n_psr, max(NMX, 1)), 1e-40)
    for p, s in enumerate(chains[0]):
        ph[p, :NMX] = s["ph"]
    stride = int(ctx.lib.gs_model_stride(NF, NMX))
    n_sys = n_psr * n_chain
    model = K.out(n_sys * stride)
    info = K.out(n_sys, dtype=torch.int32, fill=-7)
    cs_t, cs_d = (0, 0) if (shared or n_chain == 1) else (no, do)
    P = _lib.ptr
    dsc = K(np.array(desc, dtype=np.int64), torch.int64)
    fidx = K(pad("fidx", NF, np.int32)[:, :NF], torch.int32)
    midx = K(pad("midx", NMX, np.int32), torch.int32)
    A, d = K(cat("A")), K(cat("d"))
    if fn == "gs_prefix_dd":
        rc = ctx.lib.gs_prefix_dd(ctx.handle, n_psr, n_chain, NF, NMX, dsc, cs_t, cs_d, A,
                                  K(cat("A_lo")) if lo else None, d, K(cat("d_lo")) if lo else None,
                                  fidx, midx, K(ph), P(model), P(info))
    elif fn == "gs_prefix_sys":
        rc = ctx.lib.gs_prefix_sys(ctx.handle, n_psr, n_chain, NF, NMX, dsc, cs_t, cs_d, A, d, fidx, midx,
                                   K(ph), P(model), P(info))
    else:
        assert n_chain == 1
        rc = ctx.lib.gs_prefix(ctx.handle, n_psr, NF, NMX, dsc, A, d, fidx, midx, K(ph), P(model), P(info))
    _lib.check(rc, fn)
    torch.cuda.synchronize()
    mb, inf = model.cpu().numpy(), info.cpu().numpy()
    assert np.all(np.isnan(mb[-GUARD:])), "model: guard tail written"
    assert np.all(inf[-GUARD:] == -7), "info: guard tail written"
    return mb[:-GUARD].reshape(n_psr, n_chain, stride), inf[:-GUARD].reshape(n_psr, n_chain)


def split_block(blk, NF, NMX):
    o = NF * (NF + 1)
    S0 = blk[:o].reshape(NF, NF + 1)
    dF = blk[o:o + NF]
    o += NF
    G = blk[o:o + NMX * (NF + 1)].reshape(NMX, NF + 1)
    o += NMX * (NF + 1)
    h = blk[o:o + NMX]
    o += NMX
    R = blk[o:o + NMX * NMX].reshape(NMX, NMX)
    o += NMX * NMX
    return dict(S0=S0, dF=dF, G=G, h=h, R=R, aux=blk[o:o + 2], tail=blk[o + 2:])


def check_block(blk, ref, NF, NMX, nM, tag):
    """Asserts B1-B4 on one model block; returns the worst error / bound per output."""
    assert not np.isnan(blk).any(), f"{tag}: unwritten elements in the model block"
    b = split_block(blk, NF, NMX)
    S0, dF = b["S0"][:, :NF], b["dF"]
    bS, bd = SR.s0_bound(ref)
    rS, rd = SR.err(S0, ref["S0"]) / bS, SR.err(dF, ref["dF"]) / bd
    assert np.all(rS <= 1.0), (tag, "S0", float(rS.max()), np.unravel_index(rS.argmax(), rS.shape))
    assert np.all(rd <= 1.0), (tag, "dF", float(rd.max()))
    assert np.array_equal(S0, S0.T), (tag, "S0 symmetry")
    assert np.array_equal(b["S0"][:, NF], dF), (tag, "S0 padding column")
    ratios = dict(S0=float(rS.max()), dF=float(rd.max()))
    if nM:
        bR, bG, bh = SR.ghr_bound(ref, nM)
        up = np.triu(np.ones((nM, nM), bool))
        rR = SR.err(b["R"][:nM, :nM], ref["R"])
        assert np.all(rR[~up] == 0.0), (tag, "R lower triangle")
        rR = rR[up] / bR[up]
        rG = SR.err(b["G"][:nM, :NF], ref["G"]) / bG
        rh = SR.err(b["h"][:nM], ref["h"]) / bh
        assert np.all(rR <= 1.0), (tag, "R", float(rR.max()))
        assert np.all(rG <= 1.0), (tag, "G", float(rG.max()))
        assert np.all(rh <= 1.0), (tag, "h", float(rh.max()))
        ratios.update(R=float(rR.max()), G=float(rG.max()), h=float(rh.max()))
    # aux: sum log L_ii in fp64, |e|^2 rounded from double-double
    if nM:
        with mp.workprec(SR.PREC):
            e0 = float(abs(mp.mpf(float(b["aux"][0])) - ref["logdet"]))
            e1 = float(abs(mp.mpf(float(b["aux"][1])) - ref["ee"]))
        b0, b1 = (nM + 4) * SR.U * ref["logabs"], np.spacing(ref["eex"]) + 2.0 ** -70 * ref["eex"]
        assert e0 <= b0, (tag, "aux0", e0 / b0)
        assert e1 <= b1, (tag, "aux1", e1 / b1)
        ratios.update(aux0=e0 / b0, aux1=e1 / b1)
    else:
        assert b["aux"][0] == 0.0 and b["aux"][1] == 0.0, (tag, "aux without a fixed block")
    # padding: exact zeros
    assert np.all(b["G"][nM:] == 0.0) and np.all(b["G"][:, NF] == 0.0), (tag, "G padding")
    assert np.all(b["h"][nM:] == 0.0), (tag, "h padding")
    assert np.all(b["R"][nM:] == 0.0) and np.all(b["R"][:, nM:] == 0.0), (tag, "R padding")
    assert np.all(b["tail"] == 0.0), (tag, "block tail")
    return ratios


def case_chain(name, variant=0):
    return [SR.prefix_inputs(name, p, variant) for p in range(len(SR.CASES[name]["nM"]))]


@pytest.fixture(scope="module")
def clean(ctx):
    """gs_prefix_dd of every case, n_chain = 1, computed once: name -> (blocks, info)."""
    out = {}

    def get(name):
        if name not in out:
            c = SR.CASES[name]
            out[name] = run_prefix(ctx, c["NF"], c["NMX"], [case_chain(name)])
        return out[name]
    return get


@pytest.mark.parametrize("name", list(SR.CASES))
def test_prefix_dd_against_mpmath(clean, name):
    """B1-B4 per system of every case (P0..P7 and P1ph, the case with phiinv_fixed = 10^U(-2, 2)):
    S0 / dF to 1 ulp + 2^-70 of the magnitude, exactly symmetric, padding column = dF; R, G, h to
    the componentwise fp64 bounds; aux; exact zeros in the padding and the tail; NaN pre-fill fully
    overwritten and the guard intact; info = 0."""
    c = SR.CASES[name]
    blocks, info = clean(name)
    assert np.all(info == 0)
    for p, nM in enumerate(c["nM"]):
        r = check_block(blocks[p, 0], SR.prefix_reference(name, p), c["NF"], c["NMX"], nM, f"{name}-{p}")
        _show(f"gs_prefix_dd {name}-{p}", max(r.values()))
        print(f"[setup-shapes]   {name}-{p}: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    if name == "P0":
        # no fixed block: S0 and dF are the rounded A_FF + A_lo and d_F + d_lo
        s = SR.prefix_inputs("P0", 0)
        F = s["fidx"]
        b = split_block(blocks[0, 0], 2, 0)
        assert np.array_equal(b["S0"][:, :2], s["A"][np.ix_(F, F)] + s["A_lo"][np.ix_(F, F)])
        assert np.array_equal(b["dF"], s["d"][F] + s["d_lo"][F])


@pytest.mark.parametrize("name", ["P1", "P4"])
def test_prefix_chains(ctx, clean, name):
    """B5.  Stride 0 with n_chain = 3: every chain's block has the bits of the n_chain = 1 result.
    Per-chain strides with a different A per chain: block (p, c) has the bits of that A run alone
    (in P4 each of the 6 systems has its own workspace slice; then once more with 9 chains)."""
    c = SR.CASES[name]
    NF, NMX = c["NF"], c["NMX"]
    blocks, _ = clean(name)
    chains = [case_chain(name, v) for v in range(3)]
    for fn in ("gs_prefix_dd", "gs_prefix_sys"):
        lo = fn == "gs_prefix_dd"
        base = blocks if lo else run_prefix(ctx, NF, NMX, chains[:1], lo=False)[0]
        got, info = run_prefix(ctx, NF, NMX, chains, fn=fn, lo=lo, shared=True)
        assert np.all(info == 0)
        for ch in range(3):
            assert np.array_equal(got[:, ch], base[:, 0]), (name, fn, "shared", ch)
    # P4 again with 9 chains = 18 slices: workgroups are dealt round-robin to the 8 XCDs, each
    # with its own L2, so two systems that wrongly shared a slice would only see each other's
    # writes from the same XCD, i.e. 8 systems apart
    for n_chain in ((3, 9) if name == "P4" else (3,)):
        chains = [case_chain(name, v) for v in range(n_chain)]
        got, info = run_prefix(ctx, NF, NMX, chains)
        assert np.all(info == 0)
        for v in range(n_chain):
            alone, _ = run_prefix(ctx, NF, NMX, [chains[v]])
            assert np.array_equal(got[:, v], alone[:, 0]), (name, "per-chain", n_chain, v)
            if v:
                assert not np.array_equal(got[:, v], got[:, 0])


def test_prefix_wrappers(ctx):
    """B6.  gs_prefix_sys and gs_prefix on P1 have the bits of gs_prefix_dd with TNT_lo = d_lo =
    NULL, and that result meets B1-B4 against a reference built from hi alone."""
    c = SR.CASES["P1"]
    NF, NMX = c["NF"], c["NMX"]
    ch = [case_chain("P1")]
    base, info = run_prefix(ctx, NF, NMX, ch, lo=False)
    assert np.all(info == 0)
    for fn in ("gs_prefix_sys", "gs_prefix"):
        got, info = run_prefix(ctx, NF, NMX, ch, fn=fn)
        assert np.all(info == 0)
        assert np.array_equal(got, base), fn
    for p, nM in enumerate(c["nM"]):
        check_block(base[p, 0], SR.prefix_reference("P1", p, use_lo=False), NF, NMX, nM, f"P1-{p} hi only")


def test_prefix_info(ctx, clean):
    """B7.  P1 with pulsar 1's A_MM indefinite from pivot 3 on, and a second chain whose pulsar 0
    holds a NaN: info = k + 1 at the first non-positive pivot k of the mpmath factorisation,
    non-zero for the NaN system, 0 elsewhere, and the other systems' blocks keep the bits of the
    clean run.  (Inputs the kernel is documented to flag.)"""
    c = SR.CASES["P1"]
    NF, NMX = c["NF"], c["NMX"]
    blocks, _ = clean("P1")
    base = case_chain("P1")
    with pytest.raises(SR.NotPositive) as e:
        SR.prefix_reference_of(SR.indefinite_system(), pivots_only=True)
    k = e.value.k
    assert k == SR.INDEF_K
    chains = [[base[0], SR.indefinite_system(), base[2]], [SR.nan_system(), base[1], base[2]]]
    got, info = run_prefix(ctx, NF, NMX, chains)
    assert info[1, 0] == k + 1
    assert info[0, 1] != 0
    for p, ch in ((0, 0), (2, 0), (1, 1), (2, 1)):
        assert info[p, ch] == 0, (p, ch)
        assert np.array_equal(got[p, ch], blocks[p, 0]), (p, ch)
