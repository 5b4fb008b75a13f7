"""What the device tolerances of tests/test_gpu_setup_shapes.py rely on, pinned on the CPU for
every committed case of tests/setup_ref.py (no GPU):

* a host build of csrc/gibbs_dd.h running the kernels' own loops (k_tnt_dd / k_tnr_dd's Dot2 of
  exact products; k_prefix_dd's recurrence, the `schur` port of tests/test_dd_host.py) meets the
  double-double bounds against mpmath with a wide margin, and its rounded hi is within half an
  ulp: the bounds are not tight for a correct kernel;
* the Schur diagonals cancel by at least 1e3 (the median diagonal of every system with a fixed
  block), so an fp64-accurate prefix misses the S0 bound by orders of magnitude: the bounds are
  not loose for a wrong one;
* plain numpy fp64 meets the fp64 bounds on G, h and R.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from tests import setup_ref as SR                      # noqa: E402
from tests.test_dd_host import HARNESS, HDR            # noqa: E402

# k_tnt_dd's accumulation (one Dot2 over t per element) and k_tnr_dd's (four Dot2 striding t by 4,
# joined by dd_add), with recip_dd as in gibbs_prefix.hip
EXTRA = r"""
static inline gs_dd recip_dd(double N) { const double w = 1.0 / N; return {w, fma(-N, w, 1.0) / N}; }
extern "C" {
void tnt_dd(int n, int m, const double* T, const double* N, const double* r, double* hi, double* lo,
            double* dh, double* dl) {
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < m; ++j) {
      gs_dot2 acc;
      for (int t = 0; t < n; ++t) acc.fma_ddd(dd_mul_d(recip_dd(N[t]), T[t * m + i]), T[t * m + j]);
      const gs_dd v = acc.get(); hi[i * m + j] = v.hi; lo[i * m + j] = v.lo;
    }
    gs_dd s = {0.0, 0.0};
    for (int w = 0; w < 4; ++w) {
      gs_dot2 acc;
      for (int t = w; t < n; t += 4) acc.fma_ddd(dd_mul_d(recip_dd(N[t]), r[t]), T[t * m + i]);
      s = w ? dd_add(s, acc.get()) : acc.get();
    }
    dh[i] = s.hi; dl[i] = s.lo;
  }
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("setup_dd")
    src = open(HDR).read().replace("#include <hip/hip_runtime.h>", "").replace("#pragma once", "")
    (d / "gibbs_dd_host.h").write_text(src)
    (d / "h.cpp").write_text(HARNESS + EXTRA)
    so = d / "libsetupdd.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
                    "-o", str(so), str(d / "h.cpp")], check=True, cwd=d)
    return C.CDLL(str(so))


def _P(a):
    return a.ctypes.data_as(C.c_void_p)


def test_cases_cover_the_three_scratch_regimes():
    sd = {k: SR.scratch_doubles(c["NF"], c["NMX"]) for k, c in SR.CASES.items()}
    assert sd["P0"] == 0 and sd["P1"] * 8 <= 64 * 1024
    assert 64 * 1024 < sd["P2"] * 8 <= 156 * 1024
    assert sd["P3"] == 19564 <= SR.LDS_DOUBLES < sd["P4"] == 19980
    assert sd["P3"] == max(SR.scratch_doubles(60, n) for n in range(129) if SR.scratch_doubles(60, n) <= SR.LDS_DOUBLES)
    assert sd["P7"] > SR.LDS_DOUBLES and SR.CASES["P7"]["NF"] > 64
    assert SR.CASES["P6"]["NF"] == 254 and SR.CASES["P5"]["NMX"] == 128
    for c in SR.CASES.values():
        assert max(c["nM"]) == c["NMX"]
    # interleaved: the fixed columns are neither first nor contiguous
    s = SR.prefix_inputs("P1", 0)
    assert sorted(s["midx"]) != list(range(s["nM"])) and np.any(np.diff(np.sort(s["midx"])) > 1)
    assert sorted(np.concatenate([s["midx"], s["fidx"]])) == list(range(s["m"]))
    # the ragged TNT batch
    ms = [m for _, m in SR.TNT_SHAPES]
    assert max(ms) == 65 and (max(ms) + 15) // 16 == 5 and (max(ms) + 63) // 64 == 2
    for T, N, r in SR.tnt_inputs():
        if T.shape[1] >= 3:
            assert np.array_equal(T[:, -1], T[:, 0])


def test_host_tnt_loop_meets_the_dd_bound(lib):
    """The kernels' accumulation on the host against mpmath on the committed batch:
    |hi + lo - S| <= (n + 16) 2^-104 M with the worst ratio far below 1 (measured 0.057 for TNT,
    0.013 for d), and hi within half an ulp."""
    worst = worst_d = 0.0
    for (T, N, r), (S, M, Sd, Md) in zip(SR.tnt_inputs(), SR.tnt_reference()):
        n, m = T.shape
        hi, lo, dh, dl = np.zeros((m, m)), np.zeros((m, m)), np.zeros(m), np.zeros(m)
        lib.tnt_dd(n, m, _P(np.ascontiguousarray(T)), _P(N), _P(r), _P(hi), _P(lo), _P(dh), _P(dl))
        b, bd = (n + 16) * 2.0 ** -104 * M, (n + 16) * 2.0 ** -104 * Md
        worst = max(worst, float(np.max(SR.err_dd(hi, lo, S) / b)))
        worst_d = max(worst_d, float(np.max(SR.err_dd(dh, dl, Sd) / bd)))
        assert np.all(SR.err(hi, S) <= 0.5 * SR.ulp(S) + b)
        assert np.all(SR.err(dh, Sd) <= 0.5 * SR.ulp(Sd) + bd)
        # a lost low word is ~2^-53 M: it would miss the bound by this factor on most elements
        assert np.median(np.abs(lo) / b) > 1e6 or n * m < 16
    print(f"host tnt_dd worst ratio {worst:.3g}, d {worst_d:.3g}")
    assert worst < 0.25 and worst_d < 0.25


ALL_SYSTEMS = [s for name in SR.CASES for s in SR.systems(name)]


def _host_schur(lib, s, use_lo=True):
    """k_prefix_dd's recurrence on the host: fixed columns first, d as an extra F row / column."""
    m, nM, NF = s["m"], s["nM"], s["NF"]
    perm = np.concatenate([s["midx"], s["fidx"]]).astype(int)
    A = np.zeros((m + 1, m + 1))
    Al = np.zeros((m + 1, m + 1))
    A[:m, :m] = s["A"][np.ix_(perm, perm)]
    A[:m, m] = A[m, :m] = s["d"][perm]
    if use_lo:
        Al[:m, :m] = s["A_lo"][np.ix_(perm, perm)]
        Al[:m, m] = Al[m, :m] = s["d_lo"][perm]
    with mp.workprec(SR.PREC):                         # dd_add_d(A_ii, ph): here the rounded exact sum
        for i in range(nM):
            v = mp.mpf(float(A[i, i])) + mp.mpf(float(Al[i, i])) + mp.mpf(float(s["ph"][i]))
            A[i, i] = float(v)
            Al[i, i] = float(v - mp.mpf(A[i, i]))
    out = np.zeros(2 * (NF + 1) * (NF + 1))
    lib.schur(m + 1, nM, _P(np.ascontiguousarray(A)), _P(np.ascontiguousarray(Al)), _P(out))
    out = out.reshape(NF + 1, NF + 1, 2)
    return out[..., 0], out[..., 1]


@pytest.mark.parametrize("name,p", ALL_SYSTEMS, ids=[f"{n}-{p}" for n, p in ALL_SYSTEMS])
def test_host_prefix_and_case_properties(lib, name, p):
    """Per committed system: the host port's S0, dF and |e|^2 are within 2^-70 of the magnitude
    (measured: at most 1.9e-10 of that bound, 1.6e-31 of the magnitude) and their rounded hi within
    0.5 ulp + that; where there is a fixed block under the timing-model prior 1e-40, the Schur
    diagonals' cancellation (|A_ff| + sum W_if^2) / |S0_ff| has a median >= 1e3 (measured medians
    4.4e3 .. 3.1e5; the smallest single diagonal is 186, one of P6's 254 columns against 3 fixed
    ones); numpy fp64 meets the R, G, h bounds as derived (worst ratio 0.25, G of P6), so the
    constants are not widened."""
    s = SR.prefix_inputs(name, p)
    ref = SR.prefix_reference(name, p)
    NF, nM = s["NF"], s["nM"]
    hi, lo = _host_schur(lib, s)
    bS, bd = 2.0 ** -70 * ref["S0mag"], 2.0 ** -70 * ref["dFmag"]
    eS = SR.err_dd(hi[:NF, :NF], lo[:NF, :NF], ref["S0"])
    ed = SR.err_dd(hi[:NF, NF], lo[:NF, NF], ref["dF"])
    assert np.all(eS <= bS) and np.all(ed <= bd)
    assert np.all(SR.err(hi[:NF, :NF], ref["S0"]) <= 0.5 * SR.ulp(ref["S0"]) + bS)
    assert np.all(SR.err(hi[:NF, NF], ref["dF"]) <= 0.5 * SR.ulp(ref["dF"]) + bd)
    with mp.workprec(SR.PREC):
        assert abs(-(mp.mpf(hi[NF, NF]) + mp.mpf(lo[NF, NF])) - ref["ee"]) <= 2.0 ** -70 * ref["ee"]
    print(f"{name}-{p}: dd err / 2^-70 mag {float(np.max(eS / bS)):.3g}, cancel "
          f"{ref['cancel'].min():.3g}..{ref['cancel'].max():.3g}, median {np.median(ref['cancel']):.3g}")
    if nM == 0:
        # nothing to cancel: S0 and dF are the rounded A_FF and d_F
        assert np.all(ref["cancel"] == 1.0)
        with mp.workprec(SR.PREC):
            F = s["fidx"]
            assert ref["S0x"][0, 1] == float(mp.mpf(float(s["A"][F[0], F[1]])) + mp.mpf(float(s["A_lo"][F[0], F[1]])))
        assert ref["eex"] == 0.0 and ref["logdetx"] == 0.0
    elif SR.CASES[name]["ph"] == "tm":
        assert np.median(ref["cancel"]) >= 1e3
    else:
        # phiinv_fixed = 10^U(-2, 2) damps the fixed directions, so less cancels; what the device
        # test relies on here is that the diagonal term matters: without it S0 moves by far more
        # than the bound
        bare = SR.prefix_reference_of(s, use_ph=False)
        shift = SR.err(bare["S0x"], ref["S0"]) / SR.s0_bound(ref)[0]
        assert np.median(shift) > 1e6
    # fp64 outputs: numpy fp64 of the same formulas against the bounds
    if nM:
        R, G, h = SR.numpy_ghr(ref)
        bR, bG, bh = SR.ghr_bound(ref, nM)
        up = np.triu(np.ones((nM, nM), bool))
        rr = float(np.max(SR.err(R, ref["R"])[up] / bR[up]))
        rg = float(np.max(SR.err(G, ref["G"]) / bG))
        rh = float(np.max(SR.err(h, ref["h"]) / bh))
        print(f"{name}-{p}: numpy fp64 / bound: R {rr:.3g}, G {rg:.3g}, h {rh:.3g}")
        assert max(rr, rg, rh) <= 1.0                  # the constants stand as derived
        assert np.all(np.tril(R, -1) == 0.0)


def test_hi_only_reference_differs_from_the_dd_one():
    """The wrappers' reference (hi alone) is a different number from the dd one: dropping A_lo
    moves S0 by far more than the bound, so a kernel that ignored TNT_lo would be seen."""
    ref, ref_hi = SR.prefix_reference("P1", 0), SR.prefix_reference("P1", 0, use_lo=False)
    shift = SR.err(ref_hi["S0x"], ref["S0"]) / SR.s0_bound(ref)[0]
    assert np.median(shift) > 10


def test_indefinite_system_is_flagged_at_its_first_bad_pivot():
    s = SR.indefinite_system()
    with pytest.raises(SR.NotPositive) as e:
        SR.prefix_reference_of(s, pivots_only=True)
    assert e.value.k == 3
    with pytest.raises(SR.NotPositive) as e:
        SR.prefix_reference_of(SR.nan_system(), pivots_only=True)
    assert e.value.k == 0
