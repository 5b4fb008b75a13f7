// The b draws on precomputed tiled model blocks (gs_bdraw_tiled; gfx950, fp64): k_bdraw_tiled, one
// chain per wave, and k_bdraw_pair, two.
#include "gibbs_bdraw.h"

namespace {

// k_bdraw on precomputed tiled blocks: each workgroup DMA-stages its pulsar's tile-layout block
// (30.8 KB at NF = 60, nm = 16, against 40.5 KB row-major) for GS_BDRAW_LOOP chain groups, and
// the draw loads its tiles lane-linearly (tile variant only).
template <int NFC, int NTC, int WPB, bool FX, bool LNLD>
__global__ __launch_bounds__(64 * WPB, GS_MINW(GS_BCAST_TILE, NFC, NTC)) void k_bdraw_tiled(BdrawArgs A) {
  extern __shared__ double lds[];
  const int NF = NFC ? NFC : A.NF;
  const int wave = gs_wave_id(), lane = threadIdx.x & 63;
  const int nb = (A.n_chain + WPB - 1) / WPB;
  double* scr = lds + A.mstride + wave * gs_tile_scr(NF);
  if (A.persist) {
    // one round of workgroups (A.persist = CUs x resident workgroups per CU), workgroup w taking the
    // (pulsar, chain group) items [w n / G, (w + 1) n / G) in pulsar-major order: every workgroup
    // draws the same number of groups, restaging the model only where its range crosses a pulsar
    const int64_t n_items = (int64_t)A.n_psr * nb;
    const int64_t w = blockIdx.x;
    const int64_t lo = w * n_items / A.persist, hi = (w + 1) * n_items / A.persist;
    int cur = -1, nM = 0, fi = 0, mi = 0, NMXe = A.NMX;
    ModelTiled M;
#pragma unroll 1
    for (int64_t it = lo; it < hi; ++it) {
      const int p = (int)(it / nb), grp = (int)(it % nb);
      if (p != cur) {  // uniform over the workgroup
        if (cur >= 0) __syncthreads();  // every wave is done with the previous block
        stage_model(lds, A.model + (int64_t)p * A.mstride, A.mstride);
        cur = p;
        nM = __builtin_amdgcn_readfirstlane(A.nm[p]);
        fi = lane < NF ? A.fidx[p * NF + lane] : 0;
        mi = lane < nM ? A.midx[p * A.NMX + lane] : 0;
        M = model_tiled_view_psr<FX>(lds, NF, A.NMX, nM, NMXe);
      }
      const int c = grp * WPB + wave;
      if (c < A.n_chain) bdraw_item<NFC, NTC, GS_BCAST_TILE, LNLD>(A, M, p, c, NF, nM, fi, mi, scr, lane, NMXe);
    }
    return;
  }
  const int nbl = (nb + GS_BDRAW_LOOP - 1) / GS_BDRAW_LOOP;
  const int p = blockIdx.x / nbl;
  const int g0 = (blockIdx.x % nbl) * GS_BDRAW_LOOP;
  const int nM = __builtin_amdgcn_readfirstlane(A.nm[p]);  // uniform: SGPR
  const int fi = lane < NF ? A.fidx[p * NF + lane] : 0;
  const int mi = lane < nM ? A.midx[p * A.NMX + lane] : 0;
  stage_model(lds, A.model + (int64_t)p * A.mstride, A.mstride);
  int NMXe;
  const ModelTiled M = model_tiled_view_psr<FX>(lds, NF, A.NMX, nM, NMXe);
#pragma unroll 1
  for (int r = 0; r < GS_BDRAW_LOOP; ++r) {
    const int c = (g0 + r) * WPB + wave;
    if (c >= A.n_chain) break;
    bdraw_item<NFC, NTC, GS_BCAST_TILE, LNLD>(A, M, p, c, NF, nM, fi, mi, scr, lane, NMXe);
  }
}

// ------------------------------------------------------------ b draws, two chains per wave
// gs_bdraw_tiled at NF = 60 without the lnL output (GS_OPT_SWEEP_SCHED = 3, or the cost model where the
// pairs fill 2 waves per SIMD): each wave draws chains c, c + 1 of one pulsar together
// (gibbs_tile2.h bdraw_tile_pair60: both chains' diagonal eliminations in one paired register set),
// bit-identical to bdraw_item's draws -- same normals (counters per chain), same tile core per chain; a
// shut chain (chain_mask) has its draw discarded and nothing written, as bdraw_item skips it.  Pulsars
// whose fixed block is row-major (nM > 16) run bdraw_item for each chain in turn.  Persistent ranges
// of (pulsar, group of 2 WPB chains) items as k_bdraw_tiled; n_chain is even.
// A wave's LDS after the model block (doubles): the chains' tile scratches, then their z_M slots.  The
// kernel's pointers and the launcher's size both come from here.
struct BdrawPairLds {
  static constexpr int scr0 = 0, scr1 = gs_tile_scr(60), zm = 2 * gs_tile_scr(60), total = zm + 2 * 64;
};
constexpr int GS_BPAIR_SCR = BdrawPairLds::total;
// cost of a row-major pulsar's item (paired items = 10).  Measured on the 45-pulsar curn array (r06g2/3,
// every chain drawing): 0.474 ms per launch at 13, 0.441-0.445 at 15, 0.461-0.464 at 18, against
// 0.444-0.445 for k_bdraw_tiled and 0.554 unweighted (r06s)
#ifndef GS_BPAIR_RM_COST
#define GS_BPAIR_RM_COST 15
#endif

template <int WPB>
__global__ __launch_bounds__(64 * WPB, 2) void k_bdraw_pair(BdrawArgs A) {
  extern __shared__ double lds[];
  constexpr int NF = 60, CPB = 2 * WPB;
  const int wave = gs_wave_id(), lane = threadIdx.x & 63;
  const int nb = (A.n_chain + CPB - 1) / CPB;
  double* wl = lds + A.mstride + (int64_t)wave * GS_BPAIR_SCR;
  double* const scr[2] = {wl + BdrawPairLds::scr0, wl + BdrawPairLds::scr1};
  double* zmslot = wl + BdrawPairLds::zm;
  // persistent ranges weighted by cost: an item of a pulsar whose fixed block is row-major (drawn one
  // chain at a time) costs GS_BPAIR_RM_COST / 10 of a paired one, so the workgroups covering such
  // pulsars take fewer items (without the weights they ran ~1.3x longer than the rest, r06s)
  const int64_t G = A.persist ? A.persist : (int64_t)gridDim.x;
  auto cost = [&](int q) -> int {
    if (!A.persist) return 1;  // one item per workgroup
    const int nq = __builtin_amdgcn_readfirstlane(A.nm[q]);
    return model_tiled_fix(model_tiled_layout(A.NMX, nq)) ? 10 : GS_BPAIR_RM_COST;
  };
  int64_t tot = 0;
#pragma unroll 1
  for (int q = 0; q < A.n_psr; ++q) tot += (int64_t)nb * cost(q);
  const int64_t c_lo = blockIdx.x * tot / G, c_hi = (blockIdx.x + 1) * tot / G;
  int cur = -1, nM = 0, fi = 0, mi = 0, NMXe = A.NMX;
  ModelTiled M;
  int64_t P0 = 0;
#pragma unroll 1
  for (int p = 0; p < A.n_psr && P0 < c_hi; ++p) {
    const int cp = cost(p);
    const int64_t P1 = P0 + (int64_t)nb * cp;
    // items grp with start P0 + grp cp in [c_lo, c_hi)
    const int g0 = c_lo > P0 ? (int)((c_lo - P0 + cp - 1) / cp) : 0;
    const int g1 = P1 > c_lo ? (int)min((int64_t)nb, (c_hi - P0 + cp - 1) / cp) : 0;
    P0 = P1;
#pragma unroll 1
  for (int grp = g0; grp < g1; ++grp) {
    if (p != cur) {  // uniform over the workgroup (as k_bdraw_tiled's persistent loop)
      if (cur >= 0) __syncthreads();
      stage_model(lds, A.model + (int64_t)p * A.mstride, A.mstride);
      cur = p;
      nM = __builtin_amdgcn_readfirstlane(A.nm[p]);
      fi = lane < NF ? A.fidx[p * NF + lane] : 0;
      mi = lane < nM ? A.midx[p * A.NMX + lane] : 0;
      M = model_tiled_view_psr<false>(lds, NF, A.NMX, nM, NMXe);
    }
    const int c0 = grp * CPB + 2 * wave;
    if (c0 >= A.n_chain) continue;
    if (!M.fixt) {  // row-major fixed block (nM > 16): one chain at a time
      bdraw_item<60, 0, GS_BCAST_TILE, false>(A, M, p, c0, NF, nM, fi, mi, scr[0], lane, NMXe);
      bdraw_item<60, 0, GS_BCAST_TILE, false>(A, M, p, c0 + 1, NF, nM, fi, mi, scr[0], lane, NMXe);
      continue;
    }
    const int64_t sys0 = (int64_t)p * A.n_chain + c0;
    bool shut[2];
    double phinv[2], zF[2], zM[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int64_t sys = sys0 + ch;
      const int c = c0 + ch;
      shut[ch] = A.chain_mask && A.chain_mask[A.mask_per_sys ? sys : (int64_t)c] == 0;
    }
    if (shut[0] && shut[1]) continue;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int64_t sys = sys0 + ch;
      const int c = c0 + ch;
      // a shut chain draws on a unit prior (its draw is discarded): no read of its phiinv row
      phinv[ch] = shut[ch] ? (lane < NF ? 1.0 : 0.0)
                           : (lane < NF ? A.phiinv_F[(A.phi_per_chain ? (int64_t)c : sys) * NF + lane] : 0.0);
      if (A.z) {
        zF[ch] = lane < NF ? A.z[sys * A.ldb + fi] : 0.0;
        zM[ch] = lane < nM ? A.z[sys * A.ldb + mi] : 0.0;
      } else {
        gs_normal2(gs_counter(lane, gs_sweep(A.sweep, A.sweep_dev), A.chain_base + c, p + A.psr_base, A.event), A.key,
                   zF[ch], zM[ch]);
      }
    }
    double bF[2], bM[2];
    int f[2];
    bdraw_tile_pair60<GS_BDRAW_PR>(M, NMXe, nM, lane, phinv, zF, zM, bF, bM, scr, zmslot, f);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      if (!shut[ch]) bdraw_store(A, sys0 + ch, NF, nM, fi, mi, lane, f[ch], bF[ch], bM[ch]);
    }
  }
  }
}

}  // namespace

// k_bdraw_pair where it applies (NF = 60, no lnL output, an even chain count) and its waves fill 2 per
// SIMD (n_psr x n_chain / 2 >= 8 waves per CU), or where GS_OPT_SWEEP_SCHED = 3 asks; 2 forces the
// one-chain kernel
// GS_BDRAW_PAIR (off): the cost model picks k_bdraw_pair where its pairs fill 2 waves per SIMD.
// Measured (r06s, curn engine, every chain drawing): 0.430 vs 0.4375-0.468 ms per launch on 3 pulsars
// x 30720 chains (all nM <= 16), but 0.554 vs 0.444-0.473 ms on the 45-pulsar array, whose two nM = 17
// pulsars draw one chain at a time inside the pair kernel and left the persistent ranges that cover
// them longer than the rest; with the ranges weighted by item cost (GS_BPAIR_RM_COST) 0.441-0.445 vs
// 0.444-0.445 ms (r06g3) -- within the noise, so it stays opt-in.  GS_OPT_SWEEP_SCHED = 3 runs it
// (bit-identical).
#ifndef GS_BDRAW_PAIR
#define GS_BDRAW_PAIR 0
#endif
static bool bdraw_pair_wins(const BdrawArgs& a) {
  if (a.NF != 60 || a.lnl || (a.n_chain & 1) || a.model_per_sys) return false;
  if (a.sched == 3) return true;
  if (a.sched || !GS_BDRAW_PAIR) return false;
  return (double)a.n_psr * (a.n_chain / 2) >= 8.0 * device_cus();
}
// The persistent shape's workgroup count -- one round of resident workgroups (CUs x workgroups per CU)
// -- when the classic grid of n_wg workgroups needs more than one round; 0: launch the classic grid.
template <typename K>
static int persistent_wgs(K kern, int threads, size_t lds, int64_t n_wg) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds) != hipSuccess || per_cu <= 0) return 0;
  const int resident = per_cu * device_cus();
  return n_wg > (int64_t)resident ? resident : 0;
}
int launch_bdraw_tiled(hipStream_t s, const BdrawArgs& a0, int* shape, int* persist) {
  constexpr int WPB = GS_BDRAW_WPB;
  BdrawArgs a = a0;
  *persist = 0;
  if (bdraw_pair_wins(a)) {
    constexpr int PW = GS_PAIR_WPB;
    const size_t lds = ((size_t)a.mstride + (size_t)PW * GS_BPAIR_SCR) * sizeof(double);
    if (lds <= device_lds_optin()) {
      auto kern = k_bdraw_pair<PW>;
      if (lds > 65536 && set_lds(kern, lds)) return 2;
      const int64_t items = (int64_t)a.n_psr * ((a.n_chain + 2 * PW - 1) / (2 * PW));
      a.persist = persistent_wgs(kern, 64 * PW, lds, items);
      hipLaunchKernelGGL(kern, dim3((unsigned)(a.persist ? a.persist : items)), dim3(64 * PW), lds, s, a);
      *shape = 3;
      *persist = a.persist;
      return 0;
    }
  }
  *shape = 2;
  const int nb = (a.n_chain + WPB - 1) / WPB;
  const int64_t nwg = (int64_t)a.n_psr * ((nb + GS_BDRAW_LOOP - 1) / GS_BDRAW_LOOP);
  const size_t lds = ((size_t)a.mstride + (size_t)gs_tile_scr(a.NF) * WPB) * sizeof(double);
  static const int persist_env = getenv("GS_BDRAW_PERSIST") ? atoi(getenv("GS_BDRAW_PERSIST")) : 1;
  auto launch = [&](auto kern) {
    if (lds > 65536 && set_lds(kern, lds)) return 2;
    if (persist_env) a.persist = persistent_wgs(kern, 64 * WPB, lds, nwg);
    dim3 grid((unsigned)(a.persist ? a.persist : nwg));
    hipLaunchKernelGGL(kern, grid, dim3(64 * WPB), lds, s, a);
    *persist = a.persist;
    return 0;
  };
  const bool fx = model_tiled_fix(a.NMX);
  return dispatch_nf(a.NF, [&](auto nfc, auto ntc) {
    constexpr int NFC = decltype(nfc)::value, NTC = decltype(ntc)::value;
    if (fx)
      return a.lnl ? launch(k_bdraw_tiled<NFC, NTC, WPB, true, true>)
                   : launch(k_bdraw_tiled<NFC, NTC, WPB, true, false>);
    return a.lnl ? launch(k_bdraw_tiled<NFC, NTC, WPB, false, true>)
                 : launch(k_bdraw_tiled<NFC, NTC, WPB, false, false>);
  });
}
