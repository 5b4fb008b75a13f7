// b|rho conditional, the batched draws (gfx950, fp64): k_bdraw, k_bdraw_wide, k_model_tile.  The draws
// on precomputed tiled blocks are in gibbs_bdraw_tiled.hip, the marginalised likelihood and the hyper
// MH block in gibbs_lnlike.hip, the fused sweeps in gibbs_sweep.hip; gibbs_bdraw.h is what they share.
//
// Algorithm: Sigma = TNT + diag(phiinv) is factorised with the
// fixed-prior columns (timing model, phiinv constant) first.  That prefix of
// the Cholesky does not change between sweeps, so it is done once per model by
// gs_prefix; each sweep only factorises the NF x NF Schur block
// S = S0 + diag(phiinv_F) (NF = 2 n_f <= 64), one wavefront per system:
//
//   lane i owns row i of the SYMMETRIC trailing matrix in registers a[0..NF-1].
//   Right-looking step k: pivot broadcast by v_readlane, lanes > k scale their
//   a[k] into L[i][k], every lane > k applies a[j] -= L[i][k] L[j][k] for
//   j > k with L[j][k] broadcast from lane j.  Because the update is applied to
//   the whole symmetric trailing block, lane i ends up holding row i of L
//   (a[j<i]) AND, unscaled, column i of L (a[j>i] = L[j][i] L[i][i]), so both
//   triangular solves are lane-local AXPYs on a broadcast scalar: no LDS, no
//   shuffles, no barriers.
//
// Reference: PulsarBlockGibbs.update_b pulsar_gibbs.py:489-520 (SVD draw);
// the draw law is identical (b ~ N(Sigma^-1 d, Sigma^-1)); with injected normals
// rotated by the oracle (z' = L^T U S^-1/2 z) the samples coincide.
#include "gibbs_bdraw.h"

namespace {

// ------------------------------------------------------------ batched b draw, wide timing model
// 64 < nM <= 128 fixed-prior columns (NF <= 64): the model block (R alone is up to 128 KB) is
// read from global memory / L2, z_M rows 64.. come from Philox slot 64 + lane (or injected),
// and rows >= 64 of x_M are stored by the factorisation routine itself.
template <int NTC, int WPB>
__global__ __launch_bounds__(64 * WPB, 2) void k_bdraw_wide(BdrawArgs A) {
  extern __shared__ double lds[];
  const int NF = A.NF;
  const int wave = gs_wave_id(), lane = threadIdx.x & 63;
  const int nb = (A.n_chain + WPB - 1) / WPB;
  const int p = blockIdx.x / nb;
  const int c = (blockIdx.x % nb) * WPB + wave;
  if (c >= A.n_chain) return;
  const int64_t sys = (int64_t)p * A.n_chain + c;
  if (A.chain_mask && A.chain_mask[A.mask_per_sys ? sys : (int64_t)c] == 0) return;
  const ModelLds M = model_view(A.model + (A.model_per_sys ? sys : (int64_t)p) * A.mstride, NF, A.NMX);
  const int nM = __builtin_amdgcn_readfirstlane(A.nm[p]);  // uniform: SGPR
  const int32_t* mrow = A.midx + (int64_t)p * A.NMX;
  const int fi = lane < NF ? A.fidx[p * NF + lane] : 0;
  const int mi = lane < nM ? mrow[lane] : 0;
  const int mia = 64 + lane < nM ? mrow[64 + lane] : 0;
  const double phinv = lane < NF ? A.phiinv_F[(A.phi_per_chain ? (int64_t)c : sys) * NF + lane] : 0.0;
  double zF = 0.0, zM = 0.0, zMa = 0.0;
  if (A.z) {
    zF = lane < NF ? A.z[sys * A.ldb + fi] : 0.0;
    zM = lane < nM ? A.z[sys * A.ldb + mi] : 0.0;
    zMa = 64 + lane < nM ? A.z[sys * A.ldb + mia] : 0.0;
  } else {
    const long long sw = gs_sweep(A.sweep, A.sweep_dev);
    gs_normal2(gs_counter(lane, sw, A.chain_base + c, p + A.psr_base, A.event), A.key, zF, zM);
    double unused;
    gs_normal2(gs_counter(64 + lane, sw, A.chain_base + c, p + A.psr_base, A.event), A.key, zMa, unused);
  }
  double bF = 0.0, bM = 0.0;
  double* scr = lds + wave * gs_tile_scr(NF);
  const int fail =
      bdraw_tile_wide<NTC>(M, A.NMX, nM, lane, phinv, zF, zM, zMa, bF, bM, scr, NF, A.b + sys * A.ldb, mrow);
  bdraw_store(A, sys, NF, nM, fi, mi, lane, fail, bF, bM);
}

template <int NFC, int NTC, int WPB, int BC>
__global__ __launch_bounds__(64 * WPB, GS_MINW(BC, NFC, NTC)) void k_bdraw(BdrawArgs A) {
  extern __shared__ double lds[];
  const int NF = NFC ? NFC : A.NF;
  const int wave = gs_wave_id(), lane = threadIdx.x & 63;
  const int nb = (A.n_chain + WPB - 1) / WPB;
  if (A.model_per_sys) {
    // per-system models (white-noise runs, TNT differs per chain): read from global memory (L2)
    const int p = blockIdx.x / nb;
    const int c = (blockIdx.x % nb) * WPB + wave;
    if (c >= A.n_chain) return;
    const int nM = __builtin_amdgcn_readfirstlane(A.nm[p]);  // uniform: SGPR
    const int fi = lane < NF ? A.fidx[p * NF + lane] : 0;
    const int mi = lane < nM ? A.midx[p * A.NMX + lane] : 0;
    const int64_t sys = (int64_t)p * A.n_chain + c;
    bdraw_item<NFC, NTC, BC>(A, model_view(A.model + sys * A.mstride, NF, A.NMX), p, c, NF, nM, fi, mi,
                             lds + wave * GS_SCR_DOUBLES(BC, NF), lane);
    return;
  }
  // shared pulsar model: staged once per workgroup for GS_BDRAW_LOOP chain groups of the pulsar
  const int nbl = (nb + GS_BDRAW_LOOP - 1) / GS_BDRAW_LOOP;
  const int p = blockIdx.x / nbl;
  const int g0 = (blockIdx.x % nbl) * GS_BDRAW_LOOP;
  const int nM = __builtin_amdgcn_readfirstlane(A.nm[p]);  // uniform: SGPR
  const int fi = lane < NF ? A.fidx[p * NF + lane] : 0;
  const int mi = lane < nM ? A.midx[p * A.NMX + lane] : 0;
  stage_model(lds, A.model + (int64_t)p * A.mstride, A.mstride);
  const ModelLds M = model_view(lds, NF, A.NMX);
  double* scr = lds + A.mstride + wave * GS_SCR_DOUBLES(BC, NF);
#pragma unroll 1
  for (int r = 0; r < GS_BDRAW_LOOP; ++r) {
    const int c = (g0 + r) * WPB + wave;
    if (c >= A.n_chain) break;
    bdraw_item<NFC, NTC, BC>(A, M, p, c, NF, nM, fi, mi, scr, lane);
  }
}

// ------------------------------------------------------------ tiled shared models (gs_bdraw_tiled)
// Register-tile copies of n_psr shared model blocks (one workgroup per pulsar, the fused sweep's
// stage_model_tiled writing to global memory), once per white-noise state.
__global__ void k_model_tile(const double* __restrict__ model, int64_t mstride, int NF, int NMX,
                             const int32_t* __restrict__ nm, double* __restrict__ tiled, int64_t tstride) {
  const int p = blockIdx.x;
  stage_model_tiled(tiled + p * tstride, model + p * mstride, NF, NMX, nm[p]);
}

template <int WPB>
int dispatch_nf_bdraw(int NF, int bc, dim3 grid, size_t lds, hipStream_t s, const BdrawArgs& a) {
  return dispatch_nf(NF, [&](auto nfc, auto ntc) {
    constexpr int NFC = decltype(nfc)::value, NTC = decltype(ntc)::value;
    GS_LANE_ROW_CASES(k_bdraw)
    return launch_lds(k_bdraw<NFC, NTC, WPB, 3>, grid, 64 * WPB, lds, s, a);
  });
}

}  // namespace

int launch_bdraw(hipStream_t s, const BdrawArgs& a) {
  if (a.NMX > 64) {
    constexpr int WPB = GS_SWEEP_WPB;
    const int nb = (a.n_chain + WPB - 1) / WPB;
    dim3 grid((unsigned)(a.n_psr * nb));
    const size_t lds = (size_t)gs_tile_scr(a.NF) * WPB * sizeof(double);
    return dispatch_nt(a.NF, [&](auto, auto ntc) {
      return launch_lds(k_bdraw_wide<decltype(ntc)::value, WPB>, grid, 64 * WPB, lds, s, a);
    });
  }
  constexpr int WPB = GS_BDRAW_WPB;
  const int nb = (a.n_chain + WPB - 1) / WPB;
  dim3 grid((unsigned)(a.n_psr * (a.model_per_sys ? nb : (nb + GS_BDRAW_LOOP - 1) / GS_BDRAW_LOOP)));
  const bool fixed = a.NF == 20 || a.NF == 40 || a.NF == 60;
  const size_t mlds = a.model_per_sys ? 0 : (size_t)a.mstride;
  const size_t lds = (mlds + (fixed ? GS_SCR_DOUBLES(a.bcast, a.NF) : gs_tile_scr(a.NF)) * WPB) *
                     sizeof(double);
  return dispatch_nf_bdraw<WPB>(a.NF, a.bcast, grid, lds, s, a);
}

int launch_model_tile(hipStream_t s, const double* model, int n_psr, int NF, int NMX, const int32_t* nm,
                      double* tiled) {
  if (n_psr == 0) return 0;
  hipLaunchKernelGGL(k_model_tile, dim3((unsigned)n_psr), dim3(256), 0, s, model, model_stride_doubles(NF, NMX), NF,
                     NMX, nm, tiled, model_tiled_doubles(NF, NMX));
  return 0;
}
