"""mpmath references and the committed cases for the setup kernels: TNT / d (gs_tnt_dd, gs_tnt)
and the fixed-prior prefix (gs_prefix_dd, gs_prefix_sys, gs_prefix).

Everything here runs on the CPU; inputs are synthetic and seeded.  The references work at
PREC = 320 bits (the device carries ~106), each is computed once per session (lru_cache) and
returned read-only: values that must be compared below fp64 resolution stay mpmath numbers in
object arrays, and `err` / `err_dd` subtract in mpmath before rounding the difference.

tests/test_setup_ref.py pins what the device tolerances rely on (the host build of the same
double-double header on these cases, their cancellation, numpy fp64 against the fp64 bounds);
tests/test_gpu_setup_shapes.py runs the kernels.
"""
from functools import lru_cache

import numpy as np

try:
    import mpmath as mp
except ImportError:                                    # the test modules importorskip first
    mp = None

PREC = 320
U = 2.0 ** -53

# ---------------------------------------------------------------------------------- TNT, d
# (n_toa, m): m_max = 65 -> nb = 5 blocks of 16 and two 64-column blocks for d; n_toa straddles
# the 4-wave stride, the 64-TOA chunk and the 256-TOA wave stride
TNT_SHAPES = ((1, 1), (3, 15), (63, 16), (64, 17), (65, 33), (130, 64), (257, 65), (300, 48))


@lru_cache(maxsize=None)
def tnt_inputs():
    """[(T (n, m), N (n), r (n))]: column scales 10^U(-3, 6), N = 10^U(-14, -11), r ~ 1e-6; some
    columns are exact copies of others (sums without cancellation off the diagonal, one pair
    across a 16-column block edge)."""
    rng = np.random.default_rng(20240)
    out = []
    for n, m in TNT_SHAPES:
        T = rng.standard_normal((n, m)) * 10.0 ** rng.uniform(-3, 6, m)
        if m >= 3:
            T[:, m - 1] = T[:, 0]
        if m >= 20:
            T[:, 17] = T[:, 3]
        N = 10.0 ** rng.uniform(-14, -11, n)
        r = 1e-6 * rng.standard_normal(n)
        for a in (T, N, r):
            a.setflags(write=False)
        out.append((T, N, r))
    return tuple(out)


@lru_cache(maxsize=None)
def tnt_reference():
    """Per pulsar (S, M, Sd, Md): S[i, j] = sum_t T_ti T_tj / N_t (object array of mpf, symmetric),
    M the same sum of absolute values (float64); Sd, Md for d with r in place of T_tj."""
    out = []
    with mp.workprec(PREC):
        for T, N, r in tnt_inputs():
            n, m = T.shape
            w = [1 / mp.mpf(float(x)) for x in N]
            cols = [[mp.mpf(float(T[t, j])) for t in range(n)] for j in range(m)]
            ucols = [[c[t] * w[t] for t in range(n)] for c in cols]
            rr = [mp.mpf(float(x)) for x in r]
            S = np.empty((m, m), dtype=object)
            M = np.empty((m, m))
            Sd = np.empty(m, dtype=object)
            Md = np.empty(m)
            for i in range(m):
                for j in range(i, m):
                    terms = [a * b for a, b in zip(ucols[i], cols[j])]
                    S[i, j] = S[j, i] = mp.fsum(terms)
                    M[i, j] = M[j, i] = float(mp.fsum(terms, absolute=True))
                terms = [a * b for a, b in zip(ucols[i], rr)]
                Sd[i] = mp.fsum(terms)
                Md[i] = float(mp.fsum(terms, absolute=True))
            for a in (S, M, Sd, Md):
                a.setflags(write=False)
            out.append((S, M, Sd, Md))
    return tuple(out)


def _sub(a, b):
    with mp.workprec(PREC):
        return float(abs(mp.mpf(float(a)) - b))


def _sub2(a, lo, b):
    with mp.workprec(PREC):
        return float(abs(mp.mpf(float(a)) + mp.mpf(float(lo)) - b))


_err = np.frompyfunc(_sub, 2, 1)
_err2 = np.frompyfunc(_sub2, 3, 1)


def err(got, ref):
    """|got - ref| elementwise, subtracted in mpmath (ref: object array of mpf)."""
    return np.asarray(_err(np.asarray(got, dtype=np.float64), ref), dtype=np.float64)


def err_dd(hi, lo, ref):
    """|hi + lo - ref| elementwise, in mpmath."""
    return np.asarray(_err2(np.asarray(hi, np.float64), np.asarray(lo, np.float64), ref), dtype=np.float64)


def to_float(ref):
    return np.asarray(ref, dtype=np.float64) if ref.dtype != object else \
        np.array([float(x) for x in ref.ravel()]).reshape(ref.shape)


def ulp(ref):
    """Spacing of fp64 at |ref| (ref: object array of mpf or floats)."""
    return np.spacing(np.abs(to_float(np.asarray(ref))))


# ---------------------------------------------------------------------------------- prefix
# name -> NF, NMX, nM per pulsar, n_chain, phiinv_fixed mode.  Scratch = 2 NMX^2 + 2 NMX (NF + 1)
# doubles: LDS up to 19968 (64 KiB without, 156 KiB with the attribute call), workspace above.
CASES = {
    "P0": dict(NF=2, NMX=0, nM=(0,), n_chain=1, ph="tm"),            # no fixed block
    "P1": dict(NF=20, NMX=16, nM=(16, 5, 0), n_chain=1, ph="tm"),    # 1184: plain LDS, ragged
    "P1ph": dict(NF=20, NMX=16, nM=(16, 5), n_chain=1, ph="wide"),   # phiinv_fixed = 10^U(-2, 2)
    "P2": dict(NF=60, NMX=64, nM=(64, 17), n_chain=1, ph="tm"),      # 16000: LDS by attribute
    "P3": dict(NF=60, NMX=73, nM=(73,), n_chain=1, ph="tm"),         # 19564: largest LDS shape
    "P4": dict(NF=60, NMX=74, nM=(74, 9), n_chain=3, ph="tm"),       # 19980: first workspace shape
    "P5": dict(NF=2, NMX=128, nM=(128,), n_chain=1, ph="tm"),        # widest block
    "P6": dict(NF=254, NMX=3, nM=(3,), n_chain=1, ph="tm"),          # packed-index decode, max NF
    "P7": dict(NF=126, NMX=64, nM=(64, 30), n_chain=1, ph="tm"),     # workspace with NF > 64
}
LDS_DOUBLES = 19968


def scratch_doubles(NF, NMX):
    return 2 * NMX * NMX + 2 * NMX * (NF + 1)


def systems(name):
    """[(case, pulsar)] of a case."""
    return [(name, p) for p in range(len(CASES[name]["nM"]))]


@lru_cache(maxsize=None)
def prefix_inputs(name, p, variant=0):
    """One system of a case: dict(A, A_lo (m, m), d, d_lo (m), fidx (NF), midx (nM), ph (NMX),
    m, nM).  variant > 0: another draw of the same shape (a different A per chain)."""
    c = CASES[name]
    NF, NMX, nM = c["NF"], c["NMX"], c["nM"][p]
    ci = sorted(CASES).index(name)
    m = NF + nM
    # interleaved, unsorted column assignment; the same for every variant (fidx / midx are per pulsar)
    perm = np.random.default_rng([ci, p, 76]).permutation(m)
    rng = np.random.default_rng([ci, p, variant, 77])
    midx, fidx = perm[:nM].astype(np.int32), perm[nM:].astype(np.int32)
    Tm = rng.standard_normal((4 * m, m))
    if nM:
        Tm[:, fidx] += Tm[:, midx] @ rng.standard_normal((nM, NF)) * 30.0
    Tm *= 10.0 ** rng.uniform(-3, 3, m)
    A = Tm.T @ Tm
    A = (A + A.T) / 2
    A_lo = A * rng.uniform(-1, 1, (m, m)) * 2.0 ** -54
    A_lo = (A_lo + A_lo.T) / 2
    d = Tm.T @ rng.standard_normal(4 * m)
    d_lo = d * rng.uniform(-1, 1, m) * 2.0 ** -54
    ph = np.full(NMX, 1e-40) if c["ph"] == "tm" else 10.0 ** rng.uniform(-2, 2, NMX)
    out = dict(A=A, A_lo=A_lo, d=d, d_lo=d_lo, fidx=fidx, midx=midx, ph=ph, m=m, nM=nM, NF=NF, NMX=NMX)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


class NotPositive(Exception):
    def __init__(self, k):
        self.k = k


def prefix_reference_of(s, use_lo=True, use_ph=True, pivots_only=False):
    """The prefix of one system in mpmath, from A = A + A_lo, d = d + d_lo (hi alone with
    use_lo=False).  Raises NotPositive(k) at the first non-positive (or NaN) pivot k.

    Returns S0 (NF, NF), dF (NF), R (nM, nM), G (nM, NF), h (nM), ee, logdet as mpf (object
    arrays / scalars), their rounded fp64 copies under the same name + "x", and the magnitudes
    the bounds are relative to (float64): S0mag, dFmag, Rmag = |R| |L^T| |R|,
    Gmag = Rmag |W|, hmag = Rmag |e|, logabs = sum |log L_ii|, cancel (NF): (A_ff + sum W^2) / S0_ff.
    """
    NF, nM, m = s["NF"], s["nM"], s["m"]
    Mi, Fi = s["midx"], s["fidx"]
    with mp.workprec(PREC):
        def a(i, j):
            v = mp.mpf(float(s["A"][i, j]))
            return v + mp.mpf(float(s["A_lo"][i, j])) if use_lo else v

        def dv(i):
            v = mp.mpf(float(s["d"][i]))
            return v + mp.mpf(float(s["d_lo"][i])) if use_lo else v

        # Cholesky of A_MM + diag(ph), row by row; the first non-positive pivot is the same k
        # as in the kernel's right-looking order (pivot k is the k-th Schur diagonal either way)
        L = []
        for i in range(nM):
            row = []
            for j in range(i + 1):
                v = a(Mi[i], Mi[j]) - mp.fdot(row[:j], L[j][:j]) if j < i else \
                    a(Mi[i], Mi[i]) + (mp.mpf(float(s["ph"][i])) if use_ph else 0) - mp.fdot(row, row)
                if j < i:
                    row.append(v / L[j][j])
                else:
                    if not v > 0:
                        raise NotPositive(i)
                    row.append(mp.sqrt(v))
            L.append(row)
        if pivots_only:
            return None
        # W columns f < NF, e = column NF
        Wc = []
        for f in range(NF + 1):
            col = []
            for i in range(nM):
                b = a(Mi[i], Fi[f]) if f < NF else dv(Mi[i])
                col.append((b - mp.fdot(L[i][:i], col)) / L[i][i])
            Wc.append(col)
        e = Wc[NF]
        S0 = np.empty((NF, NF), dtype=object)
        dF = np.empty(NF, dtype=object)
        for f in range(NF):
            for g in range(f, NF):
                S0[f, g] = S0[g, f] = a(Fi[f], Fi[g]) - mp.fdot(Wc[f], Wc[g])
            dF[f] = dv(Fi[f]) - mp.fdot(Wc[f], e)
        ee = mp.fdot(e, e)
        logs = [mp.log(L[i][i]) for i in range(nM)]
        logdet = mp.fsum(logs)
        # Linv lower; column mm of it (rows mm..) is row mm of R = L^-T (columns mm..)
        Lic = []
        for j in range(nM):
            col = [1 / L[j][j]]
            for i in range(j + 1, nM):
                col.append(-mp.fdot(L[i][j:i], col) / L[i][i])
            Lic.append(col)
        R = np.empty((nM, nM), dtype=object)
        R[...] = mp.mpf(0)
        G = np.empty((nM, NF), dtype=object)
        h = np.empty(nM, dtype=object)
        for mm in range(nM):
            for j in range(mm, nM):
                R[mm, j] = Lic[mm][j - mm]
            for f in range(NF):
                G[mm, f] = mp.fdot(Lic[mm], Wc[f][mm:])
            h[mm] = mp.fdot(Lic[mm], e[mm:])
        Lx = np.zeros((nM, nM))
        for i in range(nM):
            Lx[i, :i + 1] = [float(x) for x in L[i]]
        Wx = np.array([[float(x) for x in col] for col in Wc]).T.reshape(nM, NF + 1)
        AFF = np.array([[float(a(Fi[f], Fi[g])) for g in range(NF)] for f in range(NF)])
        dFF = np.array([float(dv(Fi[f])) for f in range(NF)])
    Rx = to_float(R)
    aW = np.abs(Wx)
    S0mag = np.abs(AFF) + aW[:, :NF].T @ aW[:, :NF]
    dFmag = np.abs(dFF) + aW[:, :NF].T @ aW[:, NF]
    Rmag = np.abs(Rx) @ np.abs(Lx.T) @ np.abs(Rx)
    S0x = to_float(S0)
    out = dict(
        S0=S0, dF=dF, R=R, G=G, h=h, ee=ee, logdet=logdet,
        S0x=S0x, dFx=to_float(dF), Rx=Rx, Gx=to_float(G), hx=to_float(h), eex=float(ee), logdetx=float(logdet),
        Lx=Lx, Wx=Wx, S0mag=S0mag, dFmag=dFmag, Rmag=Rmag,
        Gmag=Rmag @ aW[:, :NF], hmag=Rmag @ aW[:, NF], logabs=float(sum(abs(float(x)) for x in logs)),
        cancel=np.diag(S0mag) / np.abs(np.diag(S0x)))
    for k, v in out.items():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def prefix_reference(name, p, use_lo=True):
    return prefix_reference_of(prefix_inputs(name, p), use_lo=use_lo)


INDEF_K = 3


@lru_cache(maxsize=None)
def indefinite_system():
    """P1's pulsar 1 with A_MM indefinite from pivot INDEF_K on: that pivot's Schur diagonal
    L_kk^2 is replaced by -L_kk^2 (a documented, flagged input: info = k + 1)."""
    s = dict(prefix_inputs("P1", 1))
    k = int(s["midx"][INDEF_K])
    A = s["A"].copy()
    A[k, k] -= 2.0 * prefix_reference("P1", 1)["Lx"][INDEF_K, INDEF_K] ** 2
    A.setflags(write=False)
    s["A"] = A
    return s


@lru_cache(maxsize=None)
def nan_system():
    """P1's pulsar 0 with a NaN in A_MM."""
    s = dict(prefix_inputs("P1", 0))
    A = s["A"].copy()
    k = int(s["midx"][0])
    A[k, k] = np.nan
    A.setflags(write=False)
    s["A"] = A
    return s


# ------------------------------------------------------------------------------ the bounds
def s0_bound(ref):
    """S0, dF: 1 ulp(ref) + 2^-70 (|A_fg| + sum_i |W_if| |W_ig|)."""
    return ulp(ref["S0"]) + 2.0 ** -70 * ref["S0mag"], ulp(ref["dF"]) + 2.0 ** -70 * ref["dFmag"]


# Higham's componentwise bound for the inverse of the triangular L^T computed by substitution,
# |R - L^-T| <= c u |R| |L^T| |R|, with one more rounding for the fp64 copy of L and the product
R_CONST = 1.0   # x (nM + 4) u
G_CONST = 2.0   # x (nM + 4) u


def ghr_bound(ref, nM):
    c = (nM + 4) * U
    return R_CONST * c * ref["Rmag"], G_CONST * c * ref["Gmag"], G_CONST * c * ref["hmag"]


def numpy_ghr(ref):
    """Plain numpy fp64 R = L^-T (back substitution, column by column), G = R W, h = R e from
    the rounded L and W: what the fp64 bounds are settled against."""
    Lx, Wx = ref["Lx"], ref["Wx"]
    nM = Lx.shape[0]
    R = np.zeros((nM, nM))
    for j in range(nM):
        for i in range(j, -1, -1):
            sv = (1.0 if i == j else 0.0) - Lx[i + 1:j + 1, i] @ R[i + 1:j + 1, j]
            R[i, j] = sv / Lx[i, i]
    NF = Wx.shape[1] - 1
    return R, R @ Wx[:, :NF], R @ Wx[:, NF]
