"""Long-double references and seeded synthetic cases for the white-noise kernels
(csrc/gibbs_white.hip): gs_white_tnt, gs_white_resid, gs_white_mh, gs_ecorr_epoch_sums.

Everything here runs on the CPU.  The references restate the kernels' operations in
np.longdouble on the same fp64 inputs; the case builders are shared by the GPU tests
(tests/test_gpu_white_shapes.py) and by the CPU self-tests (tests/test_white_ref.py), which pin
that no committed seed produces an accept/reject near-tie.

White parameters are given as the WhiteNoiseModel's white_list: [(x column, kind, backend, pmin,
pmax)] with kind 0 = efac, 1 = log10_tnequad, 2 = log10_t2equad.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import gibbs_oracle as O

L = np.longdouble
U = 2.0 ** -53
EFAC, TNEQUAD, T2EQUAD = 0, 1, 2
EV_WHITE = 7
SENTINEL = -12345.6789
PRIOR = {EFAC: (0.1, 5.0), TNEQUAD: (-8.5, -5.0), T2EQUAD: (-8.5, -5.0)}
START = {EFAC: (0.5, 2.0), TNEQUAD: (-8.0, -6.0), T2EQUAD: (-8.0, -6.0)}


# ================================================================== exact restatements
def _white_state(n_bk, white_list, xrow):
    """(ef2, t2, tn) per backend in long double; an absent parameter is efac 1, equad 0."""
    ef2, t2, tn = np.ones(n_bk, L), np.zeros(n_bk, L), np.zeros(n_bk, L)
    for col, kind, k, _, _ in white_list:
        _apply(kind, k, xrow[col], ef2, t2, tn)
    return ef2, t2, tn


def _apply(kind, k, v, ef2, t2, tn):
    v = L(v)
    if kind == EFAC:
        ef2[k] = v * v
    elif kind == TNEQUAD:
        tn[k] = L(10) ** (2 * v)
    else:
        t2[k] = L(10) ** (2 * v)


def exact_N(sigma2, bk, params):
    """N = ef^2 (sigma^2 + 10^(2 t2)) + 10^(2 tn) per TOA in long double.  params: iterable of
    (kind, backend, value); a backend without a parameter has efac 1 and equad 0."""
    bk = np.asarray(bk, np.int64)
    n_bk = int(bk.max()) + 1 if bk.size else 1
    params = list(params)
    if params:
        n_bk = max(n_bk, 1 + max(int(k) for _, k, _ in params))
    ef2, t2, tn = np.ones(n_bk, L), np.zeros(n_bk, L), np.zeros(n_bk, L)
    for kind, k, v in params:
        _apply(kind, k, v, ef2, t2, tn)
    return ef2[bk] * (np.asarray(sigma2, L) + t2[bk]) + tn[bk]


def params_of(white_list, xrow):
    return [(kind, k, xrow[col]) for col, kind, k, _, _ in white_list]


def exact_white_tnt(T, N, r):
    """(TNT, d, rNr) = (T^T N^-1 T, T^T N^-1 r, sum r^2 / N) in long double."""
    At = np.ascontiguousarray(np.asarray(T, L).T)     # (m, n): both operands contiguous along the TOAs
    w = 1 / np.asarray(N, L)
    rl = np.asarray(r, L)
    Aw = At * w[None, :]
    m = At.shape[0]
    TNT = np.zeros((m, m), L)
    for i in range(m):                                # lower triangle, mirrored
        TNT[i, :i + 1] = Aw[:i + 1] @ At[i]
        TNT[:i, i] = TNT[i, :i]
    return TNT, Aw @ rl, np.sum(rl * rl * w)


def tnt_bounds(TNT, rNr, n):
    """Entrywise bounds (n + 16) u sqrt(TNT_ii TNT_jj) and (n + 16) u sqrt(TNT_jj rNr): the
    any-order summation bound of n fp64 products through Cauchy-Schwarz, plus the roundings of
    N, 1/N and pow."""
    dg = np.sqrt(np.diag(TNT))
    return (n + 16) * U * np.outer(dg, dg), (n + 16) * U * dg * np.sqrt(rNr)


def check_tnt(TNTd, dd, T, N, r, symmetric=True, ref=None):
    """Assert the entrywise bounds and exact symmetry of a device (TNT, d) against the long-double
    reference at the exact N (ref: its precomputed exact_white_tnt); returns the largest
    error / bound ratios."""
    TNT, d, rNr = exact_white_tnt(T, N, r) if ref is None else ref
    assert np.isfinite(TNTd).all() and np.isfinite(dd).all(), "TNT / d not finite (unwritten entries?)"
    bT, bd = tnt_bounds(TNT, rNr, np.asarray(T).shape[0])
    eT = np.abs(np.asarray(TNTd, L) - TNT)
    ed = np.abs(np.asarray(dd, L) - d)
    bad = np.argwhere(eT > bT)
    assert bad.size == 0, ("TNT entry over its bound", tuple(bad[0]), float(eT[tuple(bad[0])]),
                           float(bT[tuple(bad[0])]), len(bad))
    badd = np.nonzero(ed > bd)[0]
    assert badd.size == 0, ("d entry over its bound", int(badd[0]), float(ed[badd[0]]), float(bd[badd[0]]))
    asym = np.argwhere(TNTd != TNTd.T) if symmetric else np.zeros(0)
    assert asym.size == 0, ("TNT not symmetric", tuple(asym[0]), len(asym))
    return float(np.max(eT / bT)), float(np.max(ed / bd))


def _backend_sum(sigma2, y, lo, hi, e, t, q):
    """(sum log N + y^2 / N, sum |log N| + y^2 / N) over TOAs [lo, hi), long double."""
    N = e * (sigma2[lo:hi] + t) + q
    lg, yy = np.log(N), y[lo:hi] * y[lo:hi] / N
    return np.sum(lg + yy), np.sum(np.abs(lg) + yy)


def white_mh_ref(x, white_list, sigma2, bk_off, y, steps, nsteps):
    """The steady-state white-noise Metropolis block (pulsar_gibbs.py:373-404) for one system.

    x: the system's row of x (fp64); sigma2, y: the pulsar's sigma^2 and y = r - T b with the TOAs
    grouped by backend, backend k in [bk_off[k], bk_off[k + 1]); steps: rows (scale, local
    parameter index, normal, uniform); nsteps: how many of them apply.

    A single-parameter proposal changes one backend's N, so lnlike1 - lnlike0 = -(S_k' - S_k) / 2
    with S_k = sum over the backend's TOAs of log N + y^2 / N, summed here in long double.  The
    proposal is x_old + (z * (0.05 n_w)) * scale in fp64 (numpy's rounding); outside the inclusive
    prior [lo, hi] it is rejected.  Returns (x, n_acc, q_rec, margin, B): the final row, the
    number of accepted steps, the proposal rows (current white values with the proposed one in
    place: the device's q_rec layout), |diff - log u| per step (inf outside the prior) and
    B = 4 n_k 2^-53 sum_i (|log N_i| + y_i^2 / N_i) over the touched backend, old plus new state:
    the forward error bound of fp64 sums of the same terms.  margin <= B marks a near-tie.
    """
    x = np.array(x, np.float64)
    nw, n_bk = len(white_list), len(bk_off) - 1
    s2, yl = np.asarray(sigma2, L), np.asarray(y, L)
    ef2, t2, tn = _white_state(n_bk, white_list, x)
    S = [_backend_sum(s2, yl, bk_off[k], bk_off[k + 1], ef2[k], t2[k], tn[k]) for k in range(n_bk)]
    xs = np.array([x[col] for col, *_ in white_list], np.float64)
    sig = np.float64(0.05 * nw)
    n_acc = 0
    q_rec = np.zeros((nsteps, nw))
    margin = np.full(nsteps, np.inf)
    B = np.zeros(nsteps)
    for st in range(nsteps):
        sc, w, z, u = (np.float64(v) for v in steps[st])
        w = int(w)
        xq = xs[w] + (z * sig) * sc
        q_rec[st] = xs
        q_rec[st, w] = xq
        _, kind, k, lo, hi = white_list[w]
        if not (lo <= xq <= hi):
            continue
        e, t, q = ef2.copy(), t2.copy(), tn.copy()
        _apply(kind, k, xq, e, t, q)
        new = _backend_sum(s2, yl, bk_off[k], bk_off[k + 1], e[k], t[k], q[k])
        diff = -(new[0] - S[k][0]) / 2
        logu = np.log(L(u))
        margin[st] = float(abs(diff - logu))
        B[st] = float(4 * (bk_off[k + 1] - bk_off[k]) * U * (new[1] + S[k][1]))
        if diff > logu:
            n_acc += 1
            ef2, t2, tn = e, t, q
            S[k] = new
            xs[w] = xq
    for (col, *_), v in zip(white_list, xs):
        x[col] = v
    return x, n_acc, q_rec, margin, B


def mh_scale(u):
    for edge, s in ((0.1, 0.1), (0.25, 0.5), (0.75, 1.0), (0.9, 3.0)):
        if u < edge:
            return s
    return 10.0


def philox_steps(nw, nsteps, key, sweep, chain, psr):
    """The device's draws of the white MH block: counters (3 s + {0, 1, 2}, sweep, chain,
    psr << 8 | GS_EV_WHITE) -> scale = gs_mh_scale(u1), w = min(int(u2 n_w), n_w - 1),
    z = sqrt(-2 log(1 - v1)) cos(2 pi v2), and the accept uniform."""
    key = np.asarray(key, np.uint32)
    out = np.zeros((nsteps, 4))
    for s in range(nsteps):
        pr = []
        for j in range(3):
            ctr = np.array([3 * s + j, sweep & 0xffffffff, chain & 0xffffffff,
                            ((psr << 8) | EV_WHITE) & 0xffffffff], np.uint32)
            pr.append([float(v) for v in O.philox_uniform_pair(ctr, key)])
        (u1, u2), (v1, v2), (u, _) = pr
        out[s] = (mh_scale(u1), min(int(u2 * nw), nw - 1), np.sqrt(-2.0 * np.log(1.0 - v1)) * np.cos(2 * np.pi * v2),
                  u)
    return out


def white_mh_philox(x, white_list, sigma2, bk_off, y, nsteps, key, sweep, chain, psr):
    """The same block driven by the device's Philox stream, written as the reference writes it:
    every step recomputes the whole likelihood -(sum log N + sum y^2 / N) / 2 over all TOAs and the
    uniform prior, in long double.  Returns (x, n_acc, steps, w per step)."""
    x = np.array(x, np.float64)
    nw, n_bk = len(white_list), len(bk_off) - 1
    bk = np.repeat(np.arange(n_bk), np.diff(bk_off))
    yl = np.asarray(y, L)
    steps = philox_steps(nw, nsteps, key, sweep, chain, psr)

    def lnlike(xr):
        N = exact_N(sigma2, bk, params_of(white_list, xr))
        return -(np.sum(np.log(N)) + np.sum(yl * yl / N)) / 2

    l0 = lnlike(x)
    n_acc = 0
    for sc, w, z, u in steps:
        col, _, _, lo, hi = white_list[int(w)]
        q = x.copy()
        q[col] = q[col] + (z * np.float64(0.05 * nw)) * sc
        if not (lo <= q[col] <= hi):
            continue
        l1 = lnlike(q)
        if l1 - l0 > np.log(L(u)):
            x, l0 = q, l1
            n_acc += 1
    return x, n_acc, steps, steps[:, 1].astype(int)


# ================================================================== synthetic cases
def synth_pulsar(rng, n_toa, m, backends):
    """T entries N(0,1) times per-column scales spanning 10^+-6, sigma in [1e-7, 1e-6], r ~ sigma."""
    scale = 10.0 ** rng.uniform(-6, 6, m)
    T = rng.standard_normal((n_toa, m)) * scale
    sigma = rng.uniform(1e-7, 1e-6, n_toa)
    r = rng.standard_normal(n_toa) * sigma
    return dict(T=T, r=r, sigma=sigma, backends=np.asarray(backends, np.int64))


def white_entry(col, kind, k):
    return (col, kind, k) + PRIOR[kind]


def draw_white(rng, white_list, n):
    """n start values of every parameter of white_list: (n, n_w)."""
    return np.stack([rng.uniform(*START[kind], n) for _, kind, *_ in white_list], axis=1) if white_list \
        else np.zeros((n, 0))


def layout_x(vals, white_lists, C, ldx, per_sys):
    """x holding vals[p][c, i] (parameter i of pulsar p, chain c): one row per chain with the
    pulsars' (disjoint) columns side by side, or one row per system (GS_OPT_X_PER_SYS).  Every
    other entry is SENTINEL."""
    P = len(white_lists)
    x = np.full((P * C if per_sys else C, ldx), SENTINEL)
    for p, wl in enumerate(white_lists):
        for i, (col, *_) in enumerate(wl):
            x[(p * C if per_sys else 0) + np.arange(C), col] = vals[p][:, i]
    return x


def xrow(x, p, c, C, per_sys):
    return x[p * C + c] if per_sys else x[c]


# ---- SYRK
SYRK_C = 9
SYRK_LDX = 12
# 3 backends: efac + tnequad, t2equad only, no parameter; the second pulsar's columns are disjoint
SYRK_WHITE = [[white_entry(1, EFAC, 0), white_entry(3, TNEQUAD, 0), white_entry(4, T2EQUAD, 1)],
              [white_entry(6, EFAC, 0), white_entry(8, TNEQUAD, 0), white_entry(10, T2EQUAD, 1)]]


def syrk_ms(nb):
    """Column counts reaching r-augmented block count nb = ceil((m + 1) / 16): odd m (4-byte DMA
    units), even m (16-byte units), and m = 16 (nb - 1): r alone in the last block."""
    return [16 * nb - 1, 16 * nb - 2] + ([16 * (nb - 1)] if nb > 1 else [])


@functools.lru_cache(maxsize=None)
def syrk_case(n_toa, m):
    """Two pulsars per launch, (n_toa, m) and (33, max(1, m - 5)): ragged m, a second T_off of
    either parity and a partial chunk.  Returns the pulsars and the white values (C, n_w) of each."""
    rng = np.random.default_rng([20, n_toa, m])
    shapes = [(n_toa, m), (33, max(1, m - 5))]
    # backend of TOA i: (i + 2) % 3 (unsorted: the model groups them; a 1-TOA pulsar has only backend 2)
    psr = [synth_pulsar(rng, n, mm, (np.arange(n) + 2) % 3) for n, mm in shapes]
    vals = [draw_white(rng, wl, SYRK_C) for wl in SYRK_WHITE]
    return psr, vals


@functools.lru_cache(maxsize=36)
def syrk_ref(n_toa, m, p, c):
    """exact_white_tnt of system (p, c) of syrk_case(n_toa, m) (the same for both x layouts)."""
    psr, vals = syrk_case(n_toa, m)
    d = psr[p]
    N = exact_N(d["sigma"] ** 2, d["backends"],
                [(kind, k, vals[p][c, i]) for i, (_, kind, k, _, _) in enumerate(SYRK_WHITE[p])])
    return exact_white_tnt(d["T"], N, d["r"])


# ---- residual
RESID_N = (1, 15, 16, 17, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def resid_case(m, C):
    """Three ragged pulsars of m columns; b (3 C, m) spans 10^+-3 per column.  Returns T, r lists,
    b and the long-double y = r - T b with its bound (m + 2) u (|r_t| + sum_j |T_tj b_j|)."""
    rng = np.random.default_rng([21, m, C])
    ns = [int(v) for v in rng.choice(RESID_N, 3, replace=False)]
    psr = [synth_pulsar(rng, n, m, np.zeros(n)) for n in ns]
    b = rng.standard_normal((3 * C, m)) * 10.0 ** rng.uniform(-3, 3, m)
    ys, bounds = [], []
    for p, d in enumerate(psr):
        Tl, bl = np.asarray(d["T"], L), np.asarray(b[p * C:(p + 1) * C], L)
        ys.append(np.asarray(d["r"], L)[None, :] - bl @ Tl.T)
        bounds.append((m + 2) * U * (np.abs(np.asarray(d["r"], L))[None, :] + np.abs(bl) @ np.abs(Tl).T))
    return psr, b, ys, bounds


# ---- Metropolis
MH_C = 6
MH_STEPS = 40
MH_LDX = 45
MH_KEY_SEED = (0x9e3779b9 << 32) | 0x7f4a7c15
MH_PSR_BASE, MH_CHAIN_BASE, MH_SWEEP = 5, 11, 3
MH_BK15 = [1, 63, 64, 65, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31]


def _mh_white_lists():
    """x columns 0, 1, 20, 44 are never white parameters (sentinels)."""
    cols = iter(c for c in range(MH_LDX) if c not in (0, 1, 20, 44))
    w0 = [white_entry(next(cols), EFAC, 0)]
    w1 = []
    for k in range(15):   # 15 backends, 32 parameters: efac + tnequad on every one, t2equad on two
        w1 += [white_entry(next(cols), EFAC, k), white_entry(next(cols), TNEQUAD, k)]
        if k in (3, 14):
            w1.append(white_entry(next(cols), T2EQUAD, k))
    # 4 backends: efac + tnequad, none, t2equad only, efac
    w2 = [white_entry(next(cols), EFAC, 0), white_entry(next(cols), TNEQUAD, 0),
          white_entry(next(cols), T2EQUAD, 2), white_entry(next(cols), EFAC, 3)]
    return [w0, w1, w2]


MH_WHITE = _mh_white_lists()
MH_BK_SIZES = [[37], MH_BK15, [9, 20, 14, 7]]


@functools.lru_cache(maxsize=None)
def mh_case(seed=22):
    """Three pulsars in one launch (TOAs sorted by backend): 37 TOAs / 1 backend / efac only;
    15 backends with sizes around the 64-lane stride and 32 parameters; 4 backends, one without
    a parameter and one with t2equad only.  y is fp64 noise of the size of sigma, per chain."""
    rng = np.random.default_rng(seed)
    psr = []
    for sizes in MH_BK_SIZES:
        d = synth_pulsar(rng, int(np.sum(sizes)), 3, np.repeat(np.arange(len(sizes)), sizes))
        d["bk_off"] = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        d["y"] = rng.standard_normal((MH_C, d["sigma"].size)) * d["sigma"] * rng.uniform(0.7, 1.6)
        psr.append(d)
    vals = [draw_white(rng, wl, MH_C) for wl in MH_WHITE]
    n_sys = 3 * MH_C
    inj = np.zeros((MH_STEPS, n_sys, 4))
    inj[..., 0] = rng.choice(O.MH_SIZES, (MH_STEPS, n_sys), p=O.MH_PROBS)
    for p, wl in enumerate(MH_WHITE):
        inj[:, p * MH_C:(p + 1) * MH_C, 1] = rng.integers(0, len(wl), (MH_STEPS, MH_C))
    inj[..., 2] = rng.standard_normal((MH_STEPS, n_sys))
    inj[..., 3] = rng.random((MH_STEPS, n_sys))
    return psr, vals, inj


def mh_nsteps(per_sys):
    """nsteps_chain of the per-chain-count case: per chain, or per system under X_PER_SYS; holds
    0 and the maximum."""
    base = np.array([0, MH_STEPS, 7, 1, 39, 13], np.int32)
    if not per_sys:
        return base
    return np.concatenate([base, base[::-1], np.roll(base, 2)]).astype(np.int32)


def mh_refs(per_sys, nsteps=None, inj=None, wmax=None):
    """white_mh_ref of every system of mh_case: list over sys = p * C + c of the ref's tuple."""
    psr, vals, inj0 = mh_case()
    inj = inj0 if inj is None else inj
    x = layout_x(vals, MH_WHITE, MH_C, MH_LDX, per_sys)
    out = []
    for p, d in enumerate(psr):
        wl = list(MH_WHITE[p])
        if wmax is not None:
            wl = [e[:4] + (wmax.get((p, i), e[4]),) for i, e in enumerate(wl)]
        for c in range(MH_C):
            sys = p * MH_C + c
            n = inj.shape[0] if nsteps is None else int(nsteps[sys if per_sys else c])
            out.append(white_mh_ref(xrow(x, p, c, MH_C, per_sys), wl, d["sigma"] ** 2, d["bk_off"], d["y"][c],
                                    inj[:, sys], n))
    return x, out


def mh_edge_case():
    """Prior-edge case: one step.  System (0, 2) proposes exactly its pulsar's wmax (inclusive:
    evaluated and, with u = 1e-300, accepted); system (2, 4) proposes one ulp above its wmax
    (rejected).  Returns (inj, {(pulsar, parameter): wmax})."""
    psr, vals, _ = mh_case()
    inj = np.zeros((1, 3 * MH_C, 4))
    inj[0, :] = (1.0, 0.0, 0.25, 1e-300)
    q_in = vals[0][2, 0] + (0.25 * np.float64(0.05 * 1)) * 1.0
    q_out = vals[2][4, 0] + (0.25 * np.float64(0.05 * 4)) * 1.0
    return inj, {(0, 0): float(q_in), (2, 0): float(np.nextafter(q_out, -np.inf))}


def mh_philox_refs(per_sys, chains=range(MH_C), psrs=range(3)):
    """white_mh_philox of the systems of mh_case at the committed key / sweep / bases, and
    white_mh_ref on the same steps (for q_rec, margins and bounds)."""
    psr, vals, _ = mh_case()
    x = layout_x(vals, MH_WHITE, MH_C, MH_LDX, per_sys)
    key = np.array([MH_KEY_SEED & 0xffffffff, MH_KEY_SEED >> 32], np.uint32)
    out = {}
    for p in psrs:
        d = psr[p]
        for c in chains:
            a = (xrow(x, p, c, MH_C, per_sys), MH_WHITE[p], d["sigma"] ** 2, d["bk_off"], d["y"][c])
            ph = white_mh_philox(*a, MH_STEPS, key, MH_SWEEP, MH_CHAIN_BASE + c, MH_PSR_BASE + p)
            out[(p, c)] = (ph, white_mh_ref(*a, ph[2], MH_STEPS))
    return x, out


# ---- ECORR epoch sums
ES_M = 7
ES_WHITE = [white_entry(0, EFAC, 0), white_entry(2, TNEQUAD, 0), white_entry(3, T2EQUAD, 1)]
ES_LDX = 5


@functools.lru_cache(maxsize=None)
def epoch_case(kb, C, ne, first_big):
    """One pulsar, ne epochs in groups of 16: groups alternate between more than 256 TOA entries
    (the unstaged fallback) and at most 256 (staged through LDS), starting with first_big.
    Returns the pulsar, x, the CSR lists, colmap / dcol and the long-double Bx, Dg with their
    bounds (q_e + 16) u sum |terms|."""
    rng = np.random.default_rng([23, kb, C, ne, int(first_big)])
    sizes = []
    for e in range(ne):
        big = (e // 16) % 2 == (0 if first_big else 1)
        n_in_group = min(16, ne - 16 * (e // 16))
        sizes.append(int(rng.integers(1, 6)) if not big else 257 // n_in_group + 1 + int(rng.integers(0, 3)))
    n_ent = int(np.sum(sizes))
    n_toa = n_ent + 5
    d = synth_pulsar(rng, n_toa, ES_M, np.sort(np.arange(n_toa) % 3))
    eptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    etoa = rng.permutation(n_toa)[:n_ent].astype(np.int32)
    eu = rng.uniform(0.5, 1.5, n_ent) * rng.choice([-1.0, 1.0], n_ent)
    colmap = np.full(kb, -1, np.int32)
    colmap[:2 * ES_M:2] = rng.permutation(ES_M)      # T columns at even j, zero columns between
    dcol = kb - 3
    x = layout_x([draw_white(rng, ES_WHITE, C)], [ES_WHITE], C, ES_LDX, False)
    Bx, Dg = np.zeros((C, ne, kb), L), np.zeros((C, ne), L)
    bB, bD = np.zeros((C, ne, kb)), np.zeros((C, ne))
    Tl, rl, ul = np.asarray(d["T"], L), np.asarray(d["r"], L), np.asarray(eu, L)
    for c in range(C):
        N = exact_N(d["sigma"] ** 2, d["backends"], params_of(ES_WHITE, x[c]))
        for e in range(ne):
            q = slice(eptr[e], eptr[e + 1])
            t = etoa[q]
            wgt = ul[q] / N[t]
            f = (sizes[e] + 16) * U
            for j in range(kb):
                v = Tl[t, colmap[j]] if colmap[j] >= 0 else (rl[t] if j == dcol else None)
                if v is not None:
                    Bx[c, e, j] = np.sum(v * wgt)
                    bB[c, e, j] = f * float(np.sum(np.abs(v * wgt)))
            Dg[c, e] = np.sum(ul[q] * wgt)
            bD[c, e] = f * float(np.sum(np.abs(ul[q] * wgt)))
    return dict(psr=d, x=x, eptr=eptr, etoa=etoa, eu=eu, colmap=colmap, dcol=dcol, sizes=sizes,
                Bx=Bx, Dg=Dg, bB=bB, bD=bD)
