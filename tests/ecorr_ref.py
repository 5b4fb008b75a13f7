"""Long-double references of the basis-ECORR kernels (csrc/gibbs_ecorr.hip) and the committed cases of
tests/test_gpu_ecorr_shapes.py / tests/test_ecorr_ref.py.  Plain numpy in x87 long double (as
tests/parity_data.exact_tnt); numpy.linalg does not take long double, so the Cholesky and the triangular
solves are written out.  Nothing here imports or calls the device library.

Operand layout (ecorr.EcorrModel, k_ecorr_prefix): the columns of Bp (ne x KB) and Ap (KB x KB), KB =
16 (1 + ceil((NF + 1) / 16)), are [M (nM <= 16, padded to 16) | F (NF) | d | pad]; Ap is TNT of that
ordering with phiinv_M on the M diagonal, d as row / column 16 + NF, (d, d) = 0 and 1 on every padded
diagonal.  a = Dg + 1 / phi_E, P = Bp^T diag(1/a) Bp, T = Ap - P.

Cases (name: NF, nm, route, backends): A20 / A40 (NB = 3 / 4 of k_ecorr_prefix), M1 / M15 / M5 (nM < 16),
U17 / U27 / U35 (the unfused route: k_ecorr_schur NB = 3 / 3 / 6), E20 / E40 (>= 65 epochs, whose rows the
staging-edge tests truncate), and W20 / W40 (white noise sampled: per-chain operands).  Each is built once
per session from synthetic.ecorr_pulsar_pta with a fixed seed and never modified."""
from functools import lru_cache

import numpy as np

L_ = np.longdouble
PSR = "J1713+0747"

#        name: (n_f, n_tm, n_epoch, n_backends, seed, white_vary)
CASES = {
    "A20": (10, 16, 40, 2, 11, False),
    "A40": (20, 16, 40, 2, 12, False),
    "M1": (10, 1, 40, 4, 13, False),
    "M15": (20, 15, 40, 3, 14, False),
    "M5": (30, 5, 40, 3, 15, False),
    "U17": (10, 17, 40, 2, 16, False),
    "U27": (10, 27, 40, 2, 17, False),
    "U35": (30, 35, 40, 2, 18, False),
    "E20": (10, 16, 90, 2, 19, False),
    "E40": (20, 16, 90, 2, 20, False),
    "W20": (10, 16, 40, 2, 21, True),
    "W40": (20, 16, 40, 2, 22, True),
}
FUSED = ("A20", "A40", "M1", "M15", "M5")
UNFUSED = ("U17", "U27", "U35")
EDGE_NE = (1, 7, 8, 9, 63, 64, 65)
MH_CASES = ("A20", "A40", "M1", "EMPTY")
MH_CHAINS, MH_STEPS = 6, 40
# a Metropolis decision of the device is the reference's when the reference's margin |delta - log u| exceeds
# twice the 1e-9 relative likelihood tolerance on each of the two values compared
MH_MARGIN_REL = 4e-9


# ------------------------------------------------------------------ long-double linear algebra
def chol(A):
    """Lower Cholesky factor of a long-double SPD matrix (column form)."""
    A = np.asarray(A, dtype=L_)
    m = A.shape[0]
    L = np.zeros_like(A)
    for k in range(m):
        v = A[k:, k] - L[k:, :k] @ L[k, :k]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[k, k] = np.sqrt(v[0])
        L[k + 1:, k] = v[1:] / L[k, k]
    return L


def solve_lower(L, B):
    """L^-1 B (forward substitution; B a vector or a matrix of columns)."""
    B = np.asarray(B, dtype=L_)
    Y = np.zeros_like(B)
    for k in range(L.shape[0]):
        Y[k] = (B[k] - L[k, :k] @ Y[:k]) / L[k, k]
    return Y


def solve_lower_t(L, B):
    """L^-T B (back substitution)."""
    B = np.asarray(B, dtype=L_)
    X = np.zeros_like(B)
    for k in range(L.shape[0] - 1, -1, -1):
        X[k] = (B[k] - L[k + 1:, k] @ X[k + 1:]) / L[k, k]
    return X


def _phi_E(xrow, ecol, ebk):
    """phi of every epoch from the chain's log10_ecorr values (phi = 10**(2 x), as ec_phi)."""
    ph = L_(10.0) ** (L_(2.0) * np.asarray(xrow, dtype=L_)[np.asarray(ecol)])
    return ph[np.asarray(ebk, np.int64)] if np.size(ebk) else np.zeros(0, dtype=L_)


# ------------------------------------------------------------------ kernels' references
def prefix_ref(Bp, Dg, ebk, Ap, xrow, ecol, phiinv_F, NF, nM, NMX):
    """k_ecorr_prefix from its operands (any float dtype, carried in long double).  Returns a dict:

    likelihood mode: ``lnl`` = (P_dd + dd^T S^-1 dd - log det S + sum log phiinv_F) / 2 with S = T_RR +
    diag(0_M, phiinv_F) over the 16 + NF columns [M | F] and dd = T_Rd, ``aux_lnl`` = (sum log a, 0,
    sum log phi_E, P_dd);
    block mode (the kernel's epilogue, gs_prefix layout): T_MM = L_M L_M^T, W = L_M^-1 T_M[F d],
    S = T_[F d][F d] - W^T W; ``S0`` (NF x (NF + 1): S_FF | S_Fd), ``dF`` = S_Fd, ``Gm`` (NMX x (NF + 1):
    rows < nM of L_M^-T W over F, column NF zero), ``hm`` (NMX: rows < nM of L_M^-T W_d), ``Rm`` (NMX x NMX:
    L_M^-T on [0, nM)^2, upper), ``am`` = (sum log diag L_M over nM, |W_d|^2), ``aux_block`` = (sum log a,
    P_dd, sum log phi_E, 0); ``block`` is the sections concatenated in the block's order.
    ``T`` is Ap - P itself."""
    Bp, Dg, Ap = (np.asarray(v, dtype=L_) for v in (Bp, Dg, Ap))
    ph = _phi_E(xrow, ecol, ebk)
    a = Dg + 1 / ph
    P = Bp.T @ (Bp / a[:, None])
    T = Ap - P
    R = dc = 16 + NF
    phF = np.asarray(phiinv_F, dtype=L_)
    sla, slp, pdd = np.sum(np.log(a)), np.sum(np.log(ph)), P[dc, dc]
    out = {"T": T, "aux_lnl": np.array([sla, 0, slp, pdd], dtype=L_),
           "aux_block": np.array([sla, pdd, slp, 0], dtype=L_)}
    # likelihood mode
    S = T[:R, :R].copy()
    S[np.arange(16, R), np.arange(16, R)] += phF
    L = chol(S)
    y = solve_lower(L, T[:R, dc])
    out["lnl"] = (pdd + y @ y - 2 * np.sum(np.log(np.diag(L))) + np.sum(np.log(phF))) / 2
    # block mode
    LM = chol(T[:16, :16])
    W = solve_lower(LM, T[:16, 16:dc + 1])
    G = solve_lower_t(LM, W)
    Sb = T[16:dc + 1, 16:dc + 1] - W.T @ W
    V = solve_lower_t(LM, np.eye(16, dtype=L_))       # L_M^-T, upper
    S0 = Sb[:NF, :NF + 1].copy()
    Gm = np.zeros((NMX, NF + 1), dtype=L_)
    Gm[:nM, :NF] = G[:nM, :NF]
    hm = np.zeros(NMX, dtype=L_)
    hm[:nM] = G[:nM, NF]
    Rm = np.zeros((NMX, NMX), dtype=L_)
    Rm[:nM, :nM] = V[:nM, :nM]
    am = np.array([np.sum(np.log(np.diag(LM)[:nM])), W[:, NF] @ W[:, NF]], dtype=L_)
    out.update(S0=S0, dF=Sb[:NF, NF].copy(), Gm=Gm, hm=hm, Rm=Rm, am=am)
    out["block"] = np.concatenate([out[k].ravel() for k in SECTIONS])
    return out


SECTIONS = ("S0", "dF", "Gm", "hm", "Rm", "am")


def section_sizes(NF, NMX):
    return [NF * (NF + 1), NF, NMX * (NF + 1), NMX, NMX * NMX, 2]


def schur_ref(Bx, Dg, ebk, xrow, xcol, A, dR, mR):
    """k_ecorr_schur: (TNT = A - B^T diag(1/a) B, d = dR - B^T (d_E / a), aux = (sum log a,
    sum d_E^2 / a, sum log phi_E, 0)) with B = Bx[:, :mR], d_E = Bx[:, mR]."""
    Bx, Dg, A, dR = (np.asarray(v, dtype=L_) for v in (Bx, Dg, A, dR))
    ph = _phi_E(xrow, xcol, ebk)
    a = Dg + 1 / ph
    B, dE = Bx[:, :mR], Bx[:, mR]
    TNT = A - B.T @ (B / a[:, None])
    d = dR - B.T @ (dE / a)
    return TNT, d, np.array([np.sum(np.log(a)), np.sum(dE * dE / a), np.sum(np.log(ph)), 0], dtype=L_)


def exact_tnt(T, N, r):
    Tl = np.asarray(T, dtype=L_)
    w = 1 / np.asarray(N, dtype=L_)
    return Tl.T @ (Tl * w[:, None]), Tl.T @ (np.asarray(r, dtype=L_) * w)


def white_const(N, r):
    """-1/2 (sum log N + r^T N^-1 r)."""
    N, r = np.asarray(N, dtype=L_), np.asarray(r, dtype=L_)
    return -(np.sum(np.log(N)) + np.sum(r * r / N)) / 2


def lnlike_ref(T, N, r, phiinv, logdet_phi, fixed=None):
    """get_lnlikelihood_fullmarg (oracle.gibbs_oracle.lnlike_fullmarg) with TNT, the Cholesky and the
    solve in long double: (lnL, lnL without the chain-independent constants).  The second value is in
    k_ecorr_accept's convention, lnl + (aux1 - aux0 - aux2) / 2 = lnL + (sum log N + r^T N^-1 r) / 2 -
    sum_M log phiinv_M / 2 over the fixed-prior columns ``fixed`` (None: no such column)."""
    TNT, d = exact_tnt(T, N, r)
    phiinv = np.asarray(phiinv, dtype=L_)
    L = chol(TNT + np.diag(phiinv))
    y = solve_lower(L, d)
    ll = white_const(N, r)
    full = ll + (y @ y - 2 * np.sum(np.log(np.diag(L))) - L_(logdet_phi)) / 2
    cM = np.sum(np.log(phiinv[np.asarray(fixed)])) / 2 if fixed is not None and np.size(fixed) else L_(0)
    return full, full - ll - cM


def lnlike_ecorr_ref(T, N, r, ecid, phiinv, logdet_phi):
    """The same value with the epoch columns eliminated first (oracle.gibbs_oracle.lnlike_ecorr_marg)."""
    TNT, d = exact_tnt(T, N, r)
    phiinv = np.asarray(phiinv, dtype=L_)
    ecid = np.asarray(ecid)
    rc = np.setdiff1d(np.arange(TNT.shape[0]), ecid)
    a = np.diag(TNT)[ecid] + phiinv[ecid]
    B, dE = TNT[np.ix_(ecid, rc)], d[ecid]
    S = TNT[np.ix_(rc, rc)] - B.T @ (B / a[:, None]) + np.diag(phiinv[rc])
    dR = d[rc] - B.T @ (dE / a)
    L = chol(S)
    y = solve_lower(L, dR)
    ld = np.sum(np.log(a)) + 2 * np.sum(np.log(np.diag(L)))
    return white_const(N, r) + (np.sum(dE * dE / a) + y @ y - ld - L_(logdet_phi)) / 2


def bdraw_ref(T, N, r, phiinv):
    """(Sigma^-1 d, Sigma) of update_b in long double, Sigma = TNT + diag(phiinv) over all m columns."""
    TNT, d = exact_tnt(T, N, r)
    Sig = TNT + np.diag(np.asarray(phiinv, dtype=L_))
    L = chol(Sig)
    return solve_lower_t(L, solve_lower(L, d)), Sig


def mh_ref(lnl_of_x, x, ecol, emin, emax, steps):
    """update_ecorr_params (as oracle.gibbs_oracle.white_mh states the white block) on injected (scale,
    parameter, normal, uniform) rows: q[ecol[p]] = x + (z (0.05 n_e)) scale in float64 (the reference's and
    the device's rounding), Uniform prior box, accept when lnl_of_x(q) - lnl_of_x(x) > log u (the
    difference in long double).  Returns (x, accepted steps, |delta - log u| of every step -- inf outside
    the prior --, the largest |lnL| met)."""
    x = np.array(x, dtype=np.float64)
    n_e = len(ecol)
    l0 = lnl_of_x(x)
    lmax, n_acc, margins = abs(l0), 0, []
    for scale, par, z, u in steps:
        p = int(par)
        q = x.copy()
        q[ecol[p]] = x[ecol[p]] + (np.float64(z) * (0.05 * n_e)) * np.float64(scale)
        lu = np.log(np.float64(u))
        if not emin[p] <= q[ecol[p]] <= emax[p]:
            margins.append(np.inf)
            continue
        l1 = lnl_of_x(q)
        lmax = max(lmax, abs(l1))
        margins.append(float(abs((l1 - l0) - L_(lu))))
        if l1 - l0 > lu:
            x, l0, n_acc = q, l1, n_acc + 1
    return x, n_acc, np.array(margins), float(lmax)


# ------------------------------------------------------------------ operands (ecorr.EcorrModel's, on the host)
def operands(TNT, d, ecid, gwid, phfix=1e-40):
    """EcorrModel's chain-independent operands from (TNT, d) of any float dtype, ecid already grouped by
    backend: dict with rc, mcols (the fixed-prior columns), Bx / A / dR (the R-ordered Schur operands,
    ldbx = 16 ceil((mR + 2) / 16)), Dg and, when nm <= 16, the reordered Bp / Ap (KB columns)."""
    dt = TNT.dtype
    m = TNT.shape[0]
    ecid, gwid = np.asarray(ecid, np.int64), np.asarray(gwid, np.int64)
    NF, ne = gwid.size, ecid.size
    rc = np.setdiff1d(np.arange(m), ecid)
    mR = rc.size
    mcols = np.array([c for c in rc if c not in set(gwid.tolist())], np.int64)
    nm = mcols.size
    ldbx = 16 * ((mR + 2 + 14) // 16)
    Bx = np.zeros((ne, ldbx), dtype=dt)
    Bx[:, :mR] = TNT[np.ix_(ecid, rc)]
    Bx[:, mR] = d[ecid]
    out = dict(rc=rc, mcols=mcols, mR=mR, nm=nm, NF=NF, ne=ne, ldbx=ldbx, Bx=Bx, Dg=np.diag(TNT)[ecid].copy(),
               A=TNT[np.ix_(rc, rc)].copy(), dR=d[rc].copy())
    if nm <= 16:
        KB = 16 * (1 + (NF + 1 + 15) // 16)
        cols = np.concatenate([mcols, gwid])
        idx = np.concatenate([np.arange(nm), 16 + np.arange(NF)])
        Bp = np.zeros((ne, KB), dtype=dt)
        Bp[:, idx] = TNT[np.ix_(ecid, cols)]
        Bp[:, 16 + NF] = d[ecid]
        Ap = np.zeros((KB, KB), dtype=dt)
        Ap[np.ix_(idx, idx)] = TNT[np.ix_(cols, cols)]
        Ap[16 + NF, idx] = d[cols]
        Ap[idx, 16 + NF] = d[cols]
        Ap[np.arange(nm), np.arange(nm)] += np.broadcast_to(np.asarray(phfix, dtype=dt), (nm,))
        pad = np.concatenate([np.arange(nm, 16), np.arange(17 + NF, KB)])
        Ap[pad, pad] = 1
        out.update(KB=KB, Bp=Bp, Ap=Ap)
    return out


# ------------------------------------------------------------------ the cases
def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@lru_cache(maxsize=None)
def case(name):
    """The model of a case: dict with pta, T, N (at the default white noise), r, names, ecid, ebk (backend of
    each epoch column), gwid, eind / gw (the x columns of log10_ecorr / log10_rho), emin / emax, NF, nm, ne,
    m, n_param, fixed (the timing-model columns) and, with white noise sampled, wind / sigma / backends."""
    from pulsar_timing_gibbsspec_amd import synthetic
    if name == "EMPTY":
        return _empty_case()
    n_f, n_tm, n_epoch, n_bk, seed, wv = CASES[name]
    pta = synthetic.ecorr_pulsar_pta(PSR, seed=seed, n_f=n_f, n_tm=n_tm, n_epoch=n_epoch, n_backends=n_bk,
                                     white_vary=wv)
    names = pta.param_names
    ebk = np.asarray(pta.signals[f"{PSR}_basis_ecorr"].epoch_backend, np.int64)
    ne = ebk.size
    T, r = pta.get_basis()[0], pta.get_residuals()[0]
    bounds = {p.name: (p.pmin, p.pmax) for p in pta.params}
    x_def = np.array([1.0 if n.endswith("efac") else -7.0 for n in names])
    N = pta.get_ndiag(pta.map_params(x_def))[0] if wv else pta.get_ndiag()[0]
    eind = np.array([i for i, n in enumerate(names) if "ecorr" in n])
    c = dict(name=name, pta=pta, T=T, N=N, r=r, names=names, ecid=np.arange(ne), ebk=ebk,
             gwid=ne + np.arange(2 * n_f), eind=eind, gw=np.array([i for i, n in enumerate(names) if "rho" in n]),
             emin=np.array([bounds[names[i]][0] for i in eind], float),
             emax=np.array([bounds[names[i]][1] for i in eind], float), NF=2 * n_f, nm=n_tm, ne=ne,
             m=T.shape[1], n_param=len(names), fixed=ne + 2 * n_f + np.arange(n_tm), n_bk=n_bk, white=wv)
    assert T.shape[1] == ne + 2 * n_f + n_tm and np.all(np.diff(ebk) >= 0)
    if wv:
        w = pta.models[0].white[0]
        c.update(wind=np.array([i for i, n in enumerate(names) if "efac" in n or "equad" in n]),
                 sigma=w.sigma, backends=w.backends, bounds=bounds)
    _freeze(T, N, r)
    return c


def _empty_case():
    """A20's pulsar with three ECORR parameters of which backend 1 owns no epoch (the second backend's epochs
    are handed to parameter 2): x = [log10_ecorr (3) | log10_rho (10)]."""
    a = case("A20")
    c = dict(a)
    ebk = np.where(a["ebk"] == 1, 2, 0)
    c.update(name="EMPTY", pta=None, ebk=ebk, eind=np.arange(3), gw=3 + np.arange(a["NF"] // 2), n_bk=3,
             emin=np.full(3, a["emin"][0]), emax=np.full(3, a["emax"][0]), n_param=3 + a["NF"] // 2,
             names=None)
    return c


def draws(c, C, seed=0):
    """C rows of x for case c: log10_ecorr in (-7.5, -5.5), log10_rho in (-8, -5), efac in (0.5, 2),
    log10_tnequad in (-8, -6)."""
    rng = np.random.default_rng([seed, len(c["name"]), c["NF"], c["nm"]])
    X = np.zeros((C, c["n_param"]))
    X[:, c["eind"]] = rng.uniform(-7.5, -5.5, (C, c["eind"].size))
    X[:, c["gw"]] = rng.uniform(-8.0, -5.0, (C, c["gw"].size))
    if c.get("white"):
        for j in c["wind"]:
            X[:, j] = rng.uniform(0.5, 2.0, C) if c["names"][j].endswith("efac") else rng.uniform(-8.0, -6.0, C)
    return X


def phiinv_F(c, X):
    return 1.0 / np.repeat(10.0 ** (2.0 * np.atleast_2d(X)[:, c["gw"]]), 2, axis=1)


def phiinv_full(c, xrow):
    """(phiinv over all m columns, log det phi) at a chain's x, as PTA.get_phiinv states it."""
    ph = np.full(c["m"], 1e40)
    ph[c["ecid"]] = np.array([10.0 ** (2.0 * float(xrow[e])) for e in c["eind"]])[c["ebk"]]
    ph[c["gwid"]] = np.repeat(10.0 ** (2.0 * xrow[c["gw"]]), 2)
    return 1.0 / ph, float(np.sum(np.log(ph)))


@lru_cache(maxsize=None)
def tnt64(name):
    """(TNT, d) in float64 (oracle.gibbs_oracle.tnt) of a case at its default white noise."""
    from oracle import gibbs_oracle as O
    c = case(name)
    out = O.tnt(c["T"], c["N"], c["r"])
    _freeze(*out)
    return out


@lru_cache(maxsize=None)
def tnt_exact(name):
    c = case(name)
    out = exact_tnt(c["T"], c["N"], c["r"])
    _freeze(*out)
    return out


@lru_cache(maxsize=None)
def host_operands(name, exact=False):
    """operands() of a case from the float64 (or the long-double) TNT; read-only."""
    c = case(name)
    out = operands(*(tnt_exact(name) if exact else tnt64(name)), c["ecid"], c["gwid"])
    _freeze(*(v for v in out.values() if isinstance(v, np.ndarray)))
    return out


def mh_inj(c, C=MH_CHAINS, n_steps=MH_STEPS, seed=0):
    """Injected (scale, parameter, normal, uniform) rows (n_steps, C, 4) of a case."""
    from oracle import gibbs_oracle as O
    rng = np.random.default_rng([seed + 77, c["NF"], c["nm"], c["n_bk"]])
    inj = np.zeros((n_steps, C, 4))
    inj[..., 0] = rng.choice(O.MH_SIZES, (n_steps, C), p=O.MH_PROBS)
    inj[..., 1] = rng.integers(0, c["n_bk"], (n_steps, C))
    inj[..., 2] = rng.standard_normal((n_steps, C))
    inj[..., 3] = rng.uniform(0.0, 1.0, (n_steps, C))
    return inj


def mh_start(c, C=MH_CHAINS):
    """Starting rows of the Metropolis cases: near the injected ECORR level, where steps are accepted."""
    X = draws(c, C, seed=5)
    X[:, c["eind"]] = np.random.default_rng(c["n_bk"]).uniform(-6.8, -6.0, (C, c["eind"].size))
    return X


@lru_cache(maxsize=None)
def mh_case(name):
    """The Metropolis block of a case in long double on the float64 operands the device holds: (X0, inj,
    X_out, n_acc, margins (C, steps), max |lnL|)."""
    c = case(name)
    base = "A20" if name == "EMPTY" else name
    op = host_operands(base)
    X0, inj = mh_start(c), mh_inj(c)
    ecol = c["eind"]
    Xo, acc, marg, lmax = [], [], [], 0.0
    for ch in range(X0.shape[0]):
        phF = phiinv_F(c, X0[ch])[0]

        def lnl(x, phF=phF):
            return _prefix_lnl(op, c["ebk"], x, ecol, phF, c["NF"])

        xo, na, mg, lm = mh_ref(lnl, X0[ch], ecol, c["emin"], c["emax"], inj[:, ch])
        Xo.append(xo), acc.append(na), marg.append(mg)
        lmax = max(lmax, lm)
    out = X0, inj, np.array(Xo), np.array(acc), np.array(marg), lmax
    _freeze(*out[:5])
    return out


def _prefix_lnl(op, ebk, x, ecol, phF, NF):
    """lnl + (aux1 - aux0 - aux2) / 2 of the likelihood mode (prefix_ref without the block sections)."""
    Bp, Dg, Ap = (np.asarray(op[k], dtype=L_) for k in ("Bp", "Dg", "Ap"))
    ph = _phi_E(x, ecol, ebk)
    a = Dg + 1 / ph
    T = Ap - Bp.T @ (Bp / a[:, None])
    R = dc = 16 + NF
    S = T[:R, :R].copy()
    phF = np.asarray(phF, dtype=L_)
    S[np.arange(16, R), np.arange(16, R)] += phF
    L = chol(S)
    y = solve_lower(L, T[:R, dc])
    lnl = (-T[dc, dc] + y @ y - 2 * np.sum(np.log(np.diag(L))) + np.sum(np.log(phF))) / 2
    return lnl - (np.sum(np.log(a)) + np.sum(np.log(ph))) / 2
