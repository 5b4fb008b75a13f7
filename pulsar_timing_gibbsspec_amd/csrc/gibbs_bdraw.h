// What the b-draw family's translation units share (gibbs_bdraw.hip, gibbs_bdraw_tiled.hip,
// gibbs_lnlike.hip, gibbs_sweep.hip): the model-block views and their staging, one b|rho draw of a
// wavefront's system (bdraw_wave, bdraw_sys, bdraw_item), the lnL value, and the launchers' helpers.
// Everything sits in the anonymous namespace, as the kernels do: each unit gets its own copy.
#pragma once
#include <cmath>
#include <type_traits>

#include "gibbs_common.h"
#include "gibbs_internal.h"
#include "gibbs_tile.h"
#include "gibbs_tile2.h"

#ifndef GS_SWEEP_MINW
#define GS_SWEEP_MINW 2
#endif

// min waves per SIMD (launch bounds) of the tile variant: 3 (<= 168 VGPRs).  Round 2 measured 3
// slower than 2 (3.05 vs 2.85 ms per launch: 35 spilled VGPRs, 54 spilled SGPRs at 207 VGPRs).
// Round 3 (r03f, MI355X, NF = 60, 4096 chains, interleaved A/B): with the tiled model block (no
// SGPR spills, 196 VGPRs) and z_F / the previous b parked in LDS (186 VGPRs) the 3-wave build
// spills 13 VGPRs, all outside the sweep's inner body, and runs 2.235 vs 2.281-2.287 ms per
// launch.  The run-time-NF instantiations with 4-5 tile rows keep 2 (24 / 84 spills at 3).
#ifndef GS_TILE_MINW
#define GS_TILE_MINW 3
#endif
#define GS_MINW(bc, nfc, ntc) \
  (((bc) == GS_BCAST_TILE || (nfc) == 0) ? (((nfc) == 0 && (ntc) >= 4) ? 2 : GS_TILE_MINW) : GS_SWEEP_MINW)

#ifndef GS_BCAST_CHUNK
#define GS_BCAST_CHUNK 8
#endif

// GS_PAIR_WPB: waves (chain pairs) per workgroup
#ifndef GS_PAIR_WPB
#define GS_PAIR_WPB 4
#endif

namespace {

// An SGPR copy of a compile-time index the compiler cannot see through: keeps
// the per-step lane masks (lane == k, lane > k) from being CSE'd across the
// fully unrolled factorisation and held live (3 x NF 64-bit masks -> SGPR spills).
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

struct ModelLds {
  const double* S0;  // NF x (NF+1)
  const double* dF;  // NF
  const double* G;   // NMX x (NF+1)
  const double* h;   // NMX
  const double* R;   // NMX x NMX
};

template <bool FX>
__device__ __forceinline__ ModelTiled model_tiled_view(const double* base, int NF, int NMX) {
  ModelTiled m;
  m.S = base;
  m.fixt = FX;  // == model_tiled_fix(NMX): the launcher picks the instantiation
  if (FX) {
    m.G = base + model_tiled_g_offset(NF);
    m.R = base + model_tiled_r_offset(NF, NMX);
    m.h = base + model_tiled_h_offset(NF, NMX);
  } else {  // row-major G | h | R after S'
    m.G = base + model_tiled_g_offset(NF);
    m.h = m.G + (int64_t)NMX * (NF + 1);
    m.R = m.h + NMX;
  }
  return m;
}
// The view of a block staged with the pulsar's own layout (FX: the batch's NMX <= 16, all tiled);
// returns the NMX the tile core indexes the block with.
template <bool FX>
__device__ __forceinline__ ModelTiled model_tiled_view_psr(const double* base, int NF, int NMX, int nM, int& NMXe) {
  if (FX) {
    NMXe = NMX;
    return model_tiled_view<true>(base, NF, NMX);
  }
  NMXe = model_tiled_layout(NMX, nM);
  return model_tiled_fix(NMXe) ? model_tiled_view<true>(base, NF, NMXe) : model_tiled_view<false>(base, NF, NMX);
}

__device__ __forceinline__ ModelLds model_view(const double* base, int NF, int NMX) {
  ModelLds m;
  m.S0 = base;
  m.dF = m.S0 + NF * (NF + 1);
  m.G = m.dF + NF;
  m.h = m.G + NMX * (NF + 1);
  m.R = m.h + NMX;
  return m;
}

// One b|rho draw for the wavefront's system.  Inputs per lane: phinv (lane < NF),
// zF (lane < NF), zM (lane < nM).  Outputs: bF (lane < NF), bM (lane < nM).
// Returns the 1-based index of the first non-positive pivot (0 = ok), uniform.
template <int NF, int BC>
__device__ __forceinline__ int bdraw_wave(const ModelLds& M, int NMX, int nM, int lane,
                                          double phinv, double zF, double zM, double& bF,
                                          double& bM, double* __restrict__ scr) {
  const bool act = lane < NF;
  const int row = act ? lane : 0;
  double a[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const double v = act ? M.S0[row * (NF + 1) + j] : 0.0;
    a[j] = (opaque(j) == lane) ? v + phinv : v;
  }
  // ---- right-looking Cholesky, symmetric trailing update
  double dinv = 0.0;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int kk = opaque(k);
    const double piv = rdlane(a[k], k);
    const double rs = rsqrt(piv);
    dinv = (lane == kk) ? rs : dinv;
    const double lk = a[k] * rs;
    const bool below = lane > kk;
    const double f = below ? lk : 0.0;
    a[k] = below ? lk : a[k];
    if constexpr (BC == GS_BCAST_READLANE) {
#pragma unroll
      for (int j = k + 1; j < NF; ++j) {
        a[j] = fma(-f, rdlane(a[k], j), a[j]);
        // bound the broadcasts in flight (each holds 2 SGPRs until its FMA)
        if (((j - k) % GS_BCAST_CHUNK) == 0) __builtin_amdgcn_sched_barrier(0);
      }
    } else if constexpr (BC == GS_BCAST_BATCH) {
      // batches of GS_BCAST_CHUNK broadcasts into distinct SGPR pairs, then the
      // FMAs: the readlane -> SGPR-read wait states overlap instead of a s_nop
      // per pair.  Constant trip counts so the inner loops unroll before k's.
#pragma unroll
      for (int j0 = 0; j0 < NF; j0 += GS_BCAST_CHUNK) {
        if (j0 + GS_BCAST_CHUNK - 1 > k) {
          double l[GS_BCAST_CHUNK];
#pragma unroll
          for (int q = 0; q < GS_BCAST_CHUNK; ++q)
            if (j0 + q > k && j0 + q < NF) l[q] = rdlane(a[k], j0 + q);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < GS_BCAST_CHUNK; ++q)
            if (j0 + q > k && j0 + q < NF) a[j0 + q] = fma(-f, l[q], a[j0 + q]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
      // column k through the wave's LDS slot: one ds_write_b64 per lane, then
      // same-address (broadcast) ds_read_b128 pairs; DS ops of a wave are in order.
      scr[lane] = f;
      wave_lds_sync();
#pragma unroll
      for (int j = (k + 1) & ~1; j < NF; j += 2) {
        const double2 v = *reinterpret_cast<const double2*>(scr + j);
        if (j > k) a[j] = fma(-f, v.x, a[j]);
        a[j + 1] = fma(-f, v.y, a[j + 1]);
        if ((((j - k) >> 1) % (GS_BCAST_CHUNK / 2)) == 0) __builtin_amdgcn_sched_barrier(0);
      }
      wave_lds_sync();
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // first non-positive pivot: lane k's dinv = rsqrt(pivot k) is NaN/inf/<=0
  const unsigned long long badm = __ballot(act && !(dinv > 0.0 && dinv < __builtin_inf()));
  const int fail = badm ? (__ffsll((long long)badm)) : 0;
  // ---- forward solve L y = dF (column AXPY)
  double r = act ? M.dF[row] : 0.0;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int kk = opaque(k);
    const double yk = rdlane(r * dinv, k);
    r = (lane == kk) ? yk : ((lane > kk) ? fma(-a[k], yk, r) : r);
  }
  // ---- back solve L^T x = y + zF; lane i < k holds L[k][i] L[i][i] in a[k]
  const double w = r + zF;
  double acc = 0.0, gacc = 0.0;
  const bool actm = lane < nM;
  const int mrow = actm ? lane : 0;
#pragma unroll
  for (int k = NF - 1; k >= 0; --k) {
    const int kk = opaque(k);
    const double xk = rdlane((w - dinv * acc) * dinv, k);
    bF = (lane == kk) ? xk : bF;
    acc = (lane < kk) ? fma(a[k], xk, acc) : acc;
    gacc = fma(actm ? M.G[mrow * (NF + 1) + k] : 0.0, xk, gacc);
  }
  // ---- fixed-prior block: x_M = h + R z_M - G x_F
  double v = actm ? M.h[mrow] - gacc : 0.0;
  for (int j = 0; j < nM; ++j) {
    const double zj = rdlane(zM, j);
    v = fma(actm ? M.R[mrow * NMX + j] : 0.0, zj, v);
  }
  if (actm) bM = v;
  return fail;
}

// One b|rho draw with the variant BC (tile MFMA or lane-row broadcast).  NFC > 0: the
// fixed-NF instantiations (20 / 40 / 60, every variant); NFC == 0: any even NF < 16 NTC at
// run time (tile variant only).
// LNLD (tile variant only): also leave gs_lnlike_marg's y and pivots in scr (lnl_terms).
template <int NFC, int NTC, int BC, bool PR = false, bool LNLD = false, typename ModelT>
__device__ __forceinline__ int bdraw_sys(const ModelT& M, int NMX, int nM, int lane, double phinv,
                                         double zF, double zM, double& bF, double& bM, double* scr, int NF) {
  if constexpr (NFC == 0 || BC == GS_BCAST_TILE)
    return bdraw_tile_nf<NFC, NTC, LNLD ? 2 : 0, PR>(M, NMX, nM, lane, phinv, zF, zM, bF, bM, scr, NF);
  else {
    static_assert(!LNLD, "the likelihood terms come with the tile variant only");
    return bdraw_wave<NFC, BC>(M, NMX, nM, lane, phinv, zF, zM, bF, bM, scr);
  }
}

// Copy a pulsar's model block into LDS (whole workgroup), 16 bytes per lane and access: model
// blocks are a 16-byte multiple of doubles (model_stride_doubles) at 16-byte aligned offsets.
// By LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no ds_write), each wave-instruction
// filling 1 KB of the block lane-linearly.
typedef __attribute__((address_space(3))) void* gs_lds_vptr;
__device__ __forceinline__ void stage_model(double* lds, const double* g, int64_t n) {
  const int n2 = (int)(n >> 1);
  const int wave = gs_wave_id(), lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int base = wave * 64; base < n2; base += nw * 64) {
    if (base + lane < n2)
      __builtin_amdgcn_global_load_lds((const void*)(g + 2 * (base + lane)), (gs_lds_vptr)(lds + 2 * base), 16, 0,
                                       0);
  }
  gs_wait_dma();
  __syncthreads();
}

// The fused sweep's model block in the register-tile layout (gibbs_tile.h ModelTiled,
// gibbs_internal.h model_tiled_*), built in LDS once per launch from the row-major block in
// global memory (L2): one double per thread and step, amortised over the launch's sweeps.
// Values are copied (or negated, G) exactly, so the draws are bit-identical to the row-major path.
// NMX: the batch's fixed-column count (the row-major block's strides); the LDS layout is the
// pulsar's own, model_tiled_layout(NMX, nM).
__device__ void stage_model_tiled(double* __restrict__ L, const double* __restrict__ g, int NF, int NMX, int nM) {
  const int NML = model_tiled_layout(NMX, nM);
  const int NT = model_tiled_nt(NF), LD = NF + 1, nP = model_tiled_np(NML);
  const bool fixt = model_tiled_fix(NML);
  const int oG = (int)model_tiled_g_offset(NF), n = (int)model_tiled_doubles(NF, NMX);
  const int oR = fixt ? (int)model_tiled_r_offset(NF, NML) : n, oH = fixt ? (int)model_tiled_h_offset(NF, NML) : n;
  const double* S0 = g;  // NF x (NF + 1), column NF = dF
  const double* G = g + NF * LD + NF;
  const double* h = G + NMX * LD;
  const double* R = h + NMX;
  for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
    const int l = idx & 63, s = (idx >> 6) & 3, q = l >> 4, c = l & 15;
    double v = 0.0;
    if (idx < oG) {  // S': tile (I, J), I <= J, row-major over the upper triangle of tiles
      int t = idx >> 8, I = 0;
      while (t >= NT - I) t -= NT - I++;
      const int J = I + t, r = 16 * I + 4 * s + q, col = 16 * J + c;
      if (r < NF && col < NF)
        v = S0[r * LD + col];
      else if (r < NF && col == NF)
        v = S0[r * LD + NF];  // dF on the augmented column ...
      else if (r == NF && col < NF)
        v = S0[col * LD + NF];  // ... and row
      else if (r == col)
        v = 1.0;  // identity padding (the augmented pivot too)
    } else if (!fixt) {  // row-major G | h | R, copied as they are
      const int k = idx - oG;
      if (k < NMX * LD + NMX + NMX * NMX) v = G[k];
    } else if (idx < oR) {  // G' = -G: chunk P (rows 16 P + c), tile column J
      const int k = idx - oG, P = k / (NT * 256), J = (k >> 8) % NT;
      const int row = 16 * P + c, f = 16 * J + 4 * s + q;
      if (row < nM && f < NF) v = -G[row * LD + f];
    } else if (idx < oH) {  // R': chunk pair (P, Q >= P)
      int t = (idx - oR) >> 8, P = 0;
      while (t >= nP - P) t -= nP - P++;
      const int Q = P + t, row = 16 * P + c, mm = 16 * Q + 4 * s + q;
      if (row < nM && mm < nM) v = R[row * NMX + mm];
    } else {
      const int k = idx - oH;
      if (k < NML) v = h[k];
    }
    L[idx] = v;
  }
  __syncthreads();
}

// ------------------------------------------------------------ batched b draw
// Issue priorities in k_bdraw / k_bdraw_tiled: on since the 4-group loop made its waves long-lived
// (r03l: CURN k_bdraw 0.535/0.526 vs 0.549/0.535 ms, CURN + red 0.540/0.540 vs 0.554/0.551; round 2's
// one-draw waves lost 25 % with them)
#ifndef GS_BDRAW_PR
#define GS_BDRAW_PR true
#endif
// Chain groups per workgroup (shared model: staged once for all of them).  Measured on MI355X
// (r03h, CURN line, 2048 chains x 45 pulsars, k_bdraw per launch): 1 -> 0.563-0.570 ms, 4 -> 0.545,
// 8 -> 0.566 (fewer, longer workgroups: the last round of the grid runs part-empty).
#ifndef GS_BDRAW_LOOP
#define GS_BDRAW_LOOP 4
#endif
// The marginalised lnL of a factorised system, 1/2 (ee + yy - 2 lm - ldS) + 1/2 sum_F log phiinv_F
// (-inf after a failed pivot): yy = |y|^2 and ldS = log det S from the tile core (lnl_terms), lm = sum
// log diag L_M and ee = |L_M^-1 d_M|^2 the model block's constants (model_aux_offset: {lm, ee}), and
// lph = sum_F log phiinv_F from lnl_phi_sum, which the whole wave calls (act: lane < NF).
// GS_LNL_VALUE is the only copy of the formula: k_lnlike_marg, the b draw's lnL output and k_hyper_mh's
// in-kernel values are bit-identical because all three expand it on the same sums.
__device__ __forceinline__ double lnl_phi_sum(bool act, double phinv) {
  double lph = act ? gs_log_lnl(phinv) : 0.0;  // phinv > 0 (lnl_terms)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lph += __shfl_xor(lph, o);
  return lph;
}
// (A macro, not a function: ee and lm are named in memory by two of the callers and read only if !fail,
// and the three kernels' code is only unchanged if each operand is evaluated where the formula uses it.)
#define GS_LNL_VALUE(fail, ee, lm, yy, ldS, lph) \
  ((fail) ? -__builtin_inf() : 0.5 * ((ee) + (yy)-2.0 * (lm) - (ldS)) + 0.5 * (lph))
// lnl[sys] of the b draw (gs_ctx_set_bdraw_lnl), the model constants from the row-major blocks
__device__ __forceinline__ void bdraw_lnl_store(const BdrawArgs& A, int p, int64_t sys, int NF, int lane, double phinv,
                                                int fail, double yy, double lp) {
  const double lph = lnl_phi_sum(lane < NF, phinv);
  if (lane == 0) {
    const double* aux = A.lnl_model + (int64_t)p * A.lnl_mstride + model_aux_offset(NF, A.NMX);
    A.lnl[sys] = GS_LNL_VALUE(fail, aux[1], aux[0], yy, lp, lph);
  }
}

// The draw's write-back: b rows (a failed factorisation -- non-PD Sigma, wave-uniform -- keeps the
// previous b and counts in fail_count), info.
__device__ __forceinline__ void bdraw_store(const BdrawArgs& A, int64_t sys, int NF, int nM, int fi, int mi, int lane,
                                            int fail, double bF, double bM) {
  if (!fail) {
    if (lane < NF) A.b[sys * A.ldb + fi] = bF;
    if (lane < nM) A.b[sys * A.ldb + mi] = bM;
  } else if (A.fail_count && lane == 0) {
    A.fail_count[sys] += 1;
  }
  if (A.info && lane == 0) A.info[sys] = fail;
}

// one (pulsar p, chain c) system of k_bdraw.  LNLD: also lnl[sys] = gs_lnlike_marg's value at the
// same phiinv (bit-identical: the same factorisation and accumulation, the model constants from the
// row-major block A.lnl_model) -- the PTA hyper block's lnL_p seed for the next sweep -- for the
// systems the gate skips as well (likelihood mode on the already staged block: no second launch).
template <int NFC, int NTC, int BC, bool LNLD = false, typename ModelT>
__device__ __forceinline__ void bdraw_item(const BdrawArgs& A, const ModelT& M, int p, int c, int NF, int nM, int fi,
                                           int mi, double* scr, int lane, int NMXe = -1) {
  if (NMXe < 0) NMXe = A.NMX;  // the NMX the block is indexed with (model_tiled_view_psr)
  const int64_t sys = (int64_t)p * A.n_chain + c;
  const bool shut = A.chain_mask && A.chain_mask[A.mask_per_sys ? sys : (int64_t)c] == 0;  // gate closed: keep b
  if constexpr (!LNLD) {
    if (shut) return;
  }
  const double phinv = lane < NF ? A.phiinv_F[(A.phi_per_chain ? (int64_t)c : sys) * NF + lane] : 0.0;
  if constexpr (LNLD) {
    if (shut) {  // no draw, but the lnL at this phiinv all the same (likelihood mode: no solves)
      double yy = 0.0, lp = 0.0;
      const int fail =
          bdraw_tile_nf<NFC, NTC, 1, GS_BDRAW_PR>(M, NMXe, nM, lane, phinv, 0.0, 0.0, yy, lp, scr, NF);
      bdraw_lnl_store(A, p, sys, NF, lane, phinv, fail, yy, lp);
      return;
    }
  }
  double zF = 0.0, zM = 0.0;
  if (A.z) {
    zF = lane < NF ? A.z[sys * A.ldb + fi] : 0.0;
    zM = lane < nM ? A.z[sys * A.ldb + mi] : 0.0;
  } else {
    gs_normal2(gs_counter(lane, gs_sweep(A.sweep, A.sweep_dev), A.chain_base + c, p + A.psr_base, A.event), A.key, zF,
               zM);
  }
  double bF = 0.0, bM = 0.0;
  const int fail = bdraw_sys<NFC, NTC, BC, GS_BDRAW_PR, LNLD>(M, NMXe, nM, lane, phinv, zF, zM, bF, bM, scr, NF);
  bdraw_store(A, sys, NF, nM, fi, mi, lane, fail, bF, bM);
  if constexpr (LNLD) {
    double yy, lp;
    lnl_terms(scr, lane, NF, yy, lp);
    bdraw_lnl_store(A, p, sys, NF, lane, phinv, fail, yy, lp);
  }
}

// Launch `kernel`; dynamic LDS above 64 KB (nm up to 64: model blocks up to 95 KB) needs the kernel
// attribute first.
template <typename K>
int set_lds(K kernel, size_t lds) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
         hipSuccess;
}
template <typename K, typename ArgsT>
int launch_lds(K kernel, dim3 grid, int threads, size_t lds, hipStream_t s, const ArgsT& a) {
  if (lds > 65536 && set_lds(kernel, lds)) return 2;
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, s, a);
  return 0;
}

// The instantiation of a b-draw kernel for NF: NF in {20, 40, 60} at compile time (NFC = NF, NTC = 0);
// any other even NF <= 64 at run time, one instantiation per tile count (NFC = 0, NTC = NF / 16 + 1; the
// tile variant only).  f(integral_constant NFC, integral_constant NTC) launches it and returns the
// launch's status; 1 for an NF that no kernel takes.
template <int N>
using gs_int = std::integral_constant<int, N>;
// dispatch_nt: the run-time half alone (every even NF <= 64 by its tile count), for kernels without
// fixed-NF instantiations (k_bdraw_wide).
template <typename F>
int dispatch_nt(int NF, F&& f) {
  if (NF <= 0 || NF > 64 || (NF & 1)) return 1;
  switch (NF / 16 + 1) {
    case 1: return f(gs_int<0>(), gs_int<1>());
    case 2: return f(gs_int<0>(), gs_int<2>());
    case 3: return f(gs_int<0>(), gs_int<3>());
    case 4: return f(gs_int<0>(), gs_int<4>());
    default: return f(gs_int<0>(), gs_int<5>());
  }
}
template <typename F>
int dispatch_nf(int NF, F&& f) {
  switch (NF) {
    case 20: return f(gs_int<20>(), gs_int<0>());
    case 40: return f(gs_int<40>(), gs_int<0>());
    case 60: return f(gs_int<60>(), gs_int<0>());
    default: return dispatch_nt(NF, f);
  }
}

// The lane-row broadcast variants (GS_OPT_BCAST 0 / 1 / 2) exist for the fixed NF only.
#define GS_LANE_ROW_CASES(KERNEL)                                                                     \
  if constexpr (NFC > 0) {                                                                            \
    switch (bc) {                                                                                     \
      case 0: return launch_lds(KERNEL<NFC, 0, WPB, 0>, grid, 64 * WPB, lds, s, a);                    \
      case 1: return launch_lds(KERNEL<NFC, 0, WPB, 1>, grid, 64 * WPB, lds, s, a);                    \
      case 2: return launch_lds(KERNEL<NFC, 0, WPB, 2>, grid, 64 * WPB, lds, s, a);                    \
      default: break;                                                                                 \
    }                                                                                                 \
  }

static int device_cus() {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0)
      ncu = 256;
  }
  return ncu;
}
// Largest dynamic LDS a workgroup may request (hipFuncSetAttribute opt-in limit; 160 KB on gfx950).
static size_t device_lds_optin() {
  static int lim = 0;
  if (!lim) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&lim, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || lim <= 0)
      lim = 160 * 1024;
  }
  return (size_t)lim;
}
}  // namespace
