// The fused free-spectrum sweeps (gfx950, fp64): rho|b and the gated b|rho draw of n_sweeps sweeps in
// one launch -- k_sweep_freespec / k_sweep_freespec_rm (one chain per wave, or the 12-wave hand-off
// shape), k_sweep_pair (two chains per wave) -- the cost model that picks the shape, and
// k_rho_analytic.  The draw itself is gibbs_bdraw.h's bdraw_sys on gibbs_tile.h / gibbs_tile2.h.
#include "gibbs_bdraw.h"

namespace {

// ------------------------------------------------------------ fused sweep
// The analytic rho|b law of one frequency (pulsar_gibbs.py:208-216, 236) for the fused sweeps: from
// tau = (b_sin^2 + b_cos^2) / 2 and the uniform U, xnew = 0.5 log10 rho and phinv = 1 / rho; both 0 on a
// lane that is not `act`.  irhomin / irhomax: the reciprocals of the prior bounds.  Called by the whole
// wave (the ballot).  k_rho_analytic keeps the exact-libm law.
struct RhoDraw {
  double xnew, phinv;
};
__device__ __forceinline__ RhoDraw rho_given_b(double tau, double U, double rhomin, double rhomax, double irhomin,
                                               double irhomax, bool act) {
#if GS_FAST_MATH
  // the reference's expressions with its divisions by the prior bounds as products with
  // their reciprocals, tau / den and den / tau by v_rcp_f64 + two Newton steps, and
  // the short log (gibbs_common.h): ~2 ulp per value, ~150 fewer VALU per draw
  const double t1 = tau * irhomax;
  const double arg = t1 - tau * irhomin;
#else
  const double t1 = tau / rhomax;
  const double arg = t1 - (tau / rhomin);
#endif
  // 1 - exp(arg) rounds to exactly 1 for arg < -37.5: skip the exp when every
  // lane is there (the usual case, tau >> rhomin)
  double hi = 1.0;
  if (__ballot(act && !(arg < -40.0))) hi = 1 - exp(arg);
  const double eta = 0.0 + hi * U;
#if GS_FAST_MATH
  const double den = t1 - gs_log_pos(1 - eta);
  const double rho = tau * rcp_nr2(den);
  const double xnew = act ? gs_log_pos(rho) * 0x1.bcb7b1526e50ep-3 : 0.0;  // 0.5 log10 rho
  // phiinv = 1/rho = den / tau
  const double phinv = act ? den * rcp_nr2(tau) : 0.0;
#else
  const double den = t1 - log(1 - eta);
  const double rho = tau / den;
  const double xnew = act ? 0.5 * log10(rho) : 0.0;
  // phiinv of the new rho: 1/rho (rcp + two Newton steps) instead of the
  // reference's 1/10**(2 x) round trip through log10 (equal to a few ulp)
  const double phinv = act ? rcp_nr2(rho) : 0.0;
#endif
  return {xnew, phinv};
}

// FX: the tiled model block's fixed-prior part in tiles (nm <= 16, k_sweep_freespec) or row-major
// (k_sweep_freespec_rm): a compile-time choice, so each kernel carries only its own fixed-block
// code (both in one kernel cost the headline 7 more spilled VGPRs, +1.2 %, r03j).  Read by the tile
// variant only: the lane-row variants have no k_sweep_freespec_rm.
template <int NFC, int NTC, int WPB, int BC, bool FX>
__device__ __forceinline__ void sweep_freespec_body(const SweepArgs& A) {
  extern __shared__ double lds[];
  const int NF = NFC ? NFC : A.NF;
  const int NFR = NF / 2;
  const int wave = gs_wave_id(), lane = threadIdx.x & 63;
  // tile variant: the model block in the register-tile layout (stage_model_tiled); the lane-row
  // broadcast variants read the row-major block
  constexpr bool TL = BC == GS_BCAST_TILE || NFC == 0;
  // BAL (12-wave workgroups = 3 waves on each SIMD of a CU, tile variant): 16 chains per
  // workgroup, waves 0..11 own chains 0..11 and each trio (waves 3e, 3e+1, 3e+2) runs chain 12 + e
  // in thirds of the sweeps, handed from wave to wave through LDS -- every wave draws 4/3 chains,
  // so 4096 chains fill the 3072 wave slots of a 3-waves/SIMD launch in one round instead of a
  // full round plus a third of a round at 1 wave/SIMD.
  constexpr bool BAL = TL && WPB == 12;
  constexpr int CPB = BAL ? 16 : WPB;  // chains per workgroup
  static_assert(BAL == (WPB == SweepLds::HANDOFF_WPB), "the hand-off shape is the tile variant's 12-wave workgroup");
  const int nb = (A.n_chain + CPB - 1) / CPB;
  const int p = blockIdx.x / nb;
  const int cblk = (blockIdx.x % nb) * CPB;
  const int c_own = cblk + wave;
  const int nM = __builtin_amdgcn_readfirstlane(A.nm[p]);  // uniform: SGPR
  int64_t mlds;
  if constexpr (BAL) {  // hand-off flags (the staging's barrier orders this before any use)
    if (threadIdx.x < SweepLds::TRIOS)
      reinterpret_cast<int*>(lds + model_tiled_doubles(NF, A.NMX) +
                             GS_SWEEP_LDS_FLAGS(GS_SCR_DOUBLES(BC, NF), WPB))[threadIdx.x] = 0;
  }
  if constexpr (TL) {
    stage_model_tiled(lds, A.model + (int64_t)p * A.mstride, NF, A.NMX, nM);
    mlds = model_tiled_doubles(NF, A.NMX);
  } else {
    stage_model(lds, A.model + (int64_t)p * A.mstride, A.mstride);
    mlds = A.mstride;
  }
  if (c_own >= A.n_chain) return;  // (then no extra chain either: 12 + e > wave)
  using ModelT = typename std::conditional<TL, ModelTiled, ModelLds>::type;
  ModelT M;
  int NMXe = A.NMX;  // the NMX the staged block is indexed with (its own layout, model_tiled_view_psr)
  if constexpr (TL) {
    M = model_tiled_view_psr<FX>(lds, NF, A.NMX, nM, NMXe);
  } else {
    M = model_view(lds, NF, A.NMX);
  }
  const int64_t n_sys = (int64_t)A.n_psr * A.n_chain;
  const bool act = lane < NF, actm = lane < nM;
  const int kf = act ? (lane >> 1) : 0;  // frequency of this lane
  const int fi = act ? A.fidx[p * NF + lane] : 0;
  const int mi = actm ? A.midx[p * A.NMX + lane] : 0;
  // the workgroup's LDS after the model block (SweepLds; the launcher asks for mlds + GS_SWEEP_LDS_TOTAL)
  using L = SweepLds;
  double* scr = lds + mlds + wave * GS_SCR_DOUBLES(BC, NF);
  // previous b (failed draws)
  double* bsave = lds + mlds + GS_SWEEP_LDS_SAVE(GS_SCR_DOUBLES(BC, NF), WPB) + wave * L::SAVE;
  // BAL: the wave's parked own-chain state (x, bF, bM, fail) while it runs the extra chain, and
  // the trio's hand-off slot of the extra chain (+ its progress flag), after the save slots
  double* park = lds + mlds + GS_SWEEP_LDS_PARK(GS_SCR_DOUBLES(BC, NF), WPB) + wave * L::STATE;
  double* hand = lds + mlds + GS_SWEEP_LDS_HAND(GS_SCR_DOUBLES(BC, NF), WPB) + (wave / 3) * L::STATE;
  int* hflag =
      reinterpret_cast<int*>(lds + mlds + GS_SWEEP_LDS_FLAGS(GS_SCR_DOUBLES(BC, NF), WPB)) + wave / 3;
  GS_PH_INIT(scr)

  const double rhomin = A.rhomin, rhomax = A.rhomax;
  const double irhomin = 1.0 / rhomin, irhomax = 1.0 / rhomax;
  const int64_t xr_step = n_sys * NFR;
  const int64_t br_step = (A.brec_nc == 0 ? n_sys : (int64_t)A.n_psr * A.brec_nc) * A.ldb;
  // segments (uniform per wave): chain, sweep range, where the state comes from / goes to
  // (0 global state arrays, 1 the wave's park slot, 2 the trio's hand-off slot)
  const int S = A.n_sweeps, s1 = S / 3, s2 = 2 * S / 3, t = wave % 3;
  const int c_ext = cblk + 12 + wave / 3;
  const bool ext = BAL && c_ext < A.n_chain;
  const int nseg = ext ? (t == 0 ? 2 : 3) : 1;
#pragma unroll 1
  for (int seg = 0; seg < nseg; ++seg) {
    int c = c_own, sw_a = 0, sw_b = S, src = 0, dst = 0, need = 0;
    if (ext) {
      if (t == 0) {  // extra [0, s1) -> hand-off, then own [0, S)
        if (seg == 0) { c = c_ext; sw_b = s1; dst = 2; }
      } else {       // own [0, sN) -> park, extra [sN, sN') from / to hand-off, own [sN, S) from park
        const int sa = t == 1 ? s1 : s2, sb = t == 1 ? s2 : S;
        if (seg == 0) { sw_b = sa; dst = 1; }
        if (seg == 1) { c = c_ext; sw_a = sa; sw_b = sb; src = 2; dst = t == 1 ? 2 : 0; need = t; }
        if (seg == 2) { sw_a = sa; src = 1; }
      }
    }
    const int64_t sys = (int64_t)p * A.n_chain + c;
    const long long gchain = A.chain_base + c;
    double x = 0.0, bF = 0.0, bM = 0.0;
    int fail = 0;
    // dead (wave-uniform): the hand-off of the extra chain did not arrive in time, or arrived
    // poisoned by an earlier dead third -- the segment's sweeps are skipped, nothing stale is
    // recorded or stored, and the chain ends with info = -1 (the host raises on it)
    bool dead = false;
    if (src == 0) {
      x = act ? A.x_state[sys * NFR + kf] : 0.0;
      bF = act ? A.b_state[sys * A.ldb + fi] : 0.0;
      bM = actm ? A.b_state[sys * A.ldb + mi] : 0.0;
    } else {
      double* slot = src == 1 ? park : hand;
      if (src == 2) {
        // wait for the trio's previous third of the extra chain (its waves are co-resident: same
        // workgroup); bounded, so a logic error cannot hang the device -- and on expiry the chain
        // is marked failed instead of continuing from a stale slot
        const int limit = A.dbg_handoff ? (1 << 16) : (1 << 24);
        int spins = 0;
        while (__hip_atomic_load(hflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < need) {
          __builtin_amdgcn_s_sleep(2);
          if (++spins > limit) {
            dead = true;
            break;
          }
        }
      }
      if (!dead) {
        gtile::lds_fence();
        x = slot[lane];
        bF = slot[64 + lane];
        bM = slot[128 + lane];
        fail = (int)slot[192];
        dead = fail < 0;
      }
    }
    if (dead) sw_b = sw_a;
    // record pointers of this lane, advanced by one sweep's rows per iteration: x rows of every
    // system; b rows of every system, or of the first brec_nc chains of each pulsar, compact
    double* xrp = (A.x_rec && act && !(lane & 1)) ? A.x_rec + sw_a * xr_step + sys * NFR + kf : nullptr;
    const bool brec = A.b_rec && (A.brec_nc == 0 || c < A.brec_nc);
    const int64_t brow0 = A.brec_nc == 0 ? sys : (int64_t)p * A.brec_nc + c;
    double* bFp = (brec && act) ? A.b_rec + sw_a * br_step + brow0 * A.ldb + fi : nullptr;
    double* bMp = (brec && actm) ? A.b_rec + sw_a * br_step + brow0 * A.ldb + mi : nullptr;
#pragma unroll 1
  for (int sw = sw_a; sw < sw_b; ++sw) {
    const long long ii = A.it0 + sw;
    const int64_t rec = (int64_t)sw * n_sys + sys;
    GS_PH_BEGIN
    // record-before-update (pulsar_gibbs.py:658-659)
    if (xrp) *xrp = x;
    if (bFp) *bFp = bF;
    if (bMp) *bMp = bM;
    xrp = xrp ? xrp + xr_step : nullptr;
    bFp = bFp ? bFp + br_step : nullptr;
    bMp = bMp ? bMp + br_step : nullptr;
    // pass 0: first b draw from xs at global sweep 0 (pulsar_gibbs.py:661-662);
    // pass 1: rho|b then the gated b draw.  One bdraw_wave call site.
#pragma unroll 1
    for (int pass = (ii == 0) ? 0 : 1; pass < 2; ++pass) {
      const double* zinj = A.z0_inj;
      int ev = GS_EV_B0;
      double phinv = 0.0;
      int64_t zrow = sys;
      if (pass == 1) {
        if constexpr (GS_RHO_PRIO > 0) __builtin_amdgcn_s_setprio(GS_RHO_PRIO);
        // rho|b analytic (pulsar_gibbs.py:208-216, 236)
        const double partner = __shfl_xor(bF, 1);
        const double be = (lane & 1) ? partner : bF, bo = (lane & 1) ? bF : partner;
        // tau = (b_sin^2 + b_cos^2) / 2 rounded as numpy (pulsar_gibbs.py:208-209): no fma contraction
        const double tau = gs_add_rn(gs_mul_rn(be, be), gs_mul_rn(bo, bo)) / 2;
        double U;
        if (A.u_inj) {
          U = act ? A.u_inj[rec * NFR + kf] : 0.5;
        } else {
          double u2;
          gs_uniform2(gs_counter(kf, ii, gchain, p + A.psr_base, GS_EV_RHO), A.key, U, u2);
        }
        const RhoDraw rd = rho_given_b(tau, U, rhomin, rhomax, irhomin, irhomax, act);
        const double xnew = rd.xnew;
        phinv = rd.phinv;
        // gate: all(xnew != x_old[-1])  (pulsar_gibbs.py:697)
        const double xlast = rdlane(x, NF - 1);
        const bool same = act && (xnew == xlast);
        const bool gate = __ballot(same) == 0ull;
        x = xnew;
        if constexpr (GS_RHO_PRIO > 0) __builtin_amdgcn_s_setprio(GS_BASE_PRIO);
        if (!gate) break;
        zinj = A.z_inj;
        ev = GS_EV_B;
        zrow = rec;
      }
      GS_PH(6)
      double zF, zM;
      if (zinj) {
        zF = act ? zinj[zrow * A.ldb + fi] : 0.0;
        zM = actm ? zinj[zrow * A.ldb + mi] : 0.0;
      } else {
        gs_normal2(gs_counter(lane, ii, gchain, p + A.psr_base, ev), A.key, zF, zM);
      }
      if (pass == 0) phinv = act ? 1.0 / pow(10.0, 2.0 * x) : 0.0;  // first draw from xs
      GS_PH(7)
      // a failed factorisation (non-PD Sigma, wave-uniform) keeps the previous b: no NaN ever
      // enters the state (the reference's LinAlgError branch, pulsar_gibbs.py:507-516).  The
      // previous b waits in the wave's LDS save slot, not in 4 VGPRs across the draw.
      bsave[lane] = bF;
      bsave[64 + lane] = bM;
      const int f = bdraw_sys<NFC, NTC, BC, true>(M, NMXe, nM, lane, phinv, zF, zM, bF, bM, scr, NF);
      if (f) {
        gtile::lds_fence();
        bF = bsave[lane];
        bM = bsave[64 + lane];
        if (!fail) fail = f;
        if (A.fail_count && lane == 0) A.fail_count[sys] += 1;
      }
    }
  }
    if (dst == 0) {
      if (!dead) {
        if (act && !(lane & 1)) A.x_state[sys * NFR + kf] = x;
        if (act) A.b_state[sys * A.ldb + fi] = bF;
        if (actm) A.b_state[sys * A.ldb + mi] = bM;
      }
      if (A.info && lane == 0) A.info[sys] = dead ? -1 : fail;
    } else {
      double* slot = dst == 1 ? park : hand;
      gtile::lds_fence();
      slot[lane] = x;
      slot[64 + lane] = bF;
      slot[128 + lane] = bM;
      if (lane == 0) slot[192] = dead ? -1.0 : (double)fail;
      gtile::lds_fence();
      // (GS_OPT_DEBUG_HANDOFF: workgroup 0's first trio never publishes its first third, so the
      // test sees the wait expire)
      const bool skip = A.dbg_handoff && blockIdx.x == 0 && wave == 0;
      if (dst == 2 && !skip) __hip_atomic_store(hflag, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  GS_PH_FLUSH(scr)
}

template <int NFC, int NTC, int WPB, int BC>
__global__ __launch_bounds__(64 * WPB, GS_MINW(BC, NFC, NTC)) void k_sweep_freespec(SweepArgs A) {
  sweep_freespec_body<NFC, NTC, WPB, BC, true>(A);
}
template <int NFC, int NTC, int WPB, int BC>
__global__ __launch_bounds__(64 * WPB, GS_MINW(BC, NFC, NTC)) void k_sweep_freespec_rm(SweepArgs A) {
  sweep_freespec_body<NFC, NTC, WPB, BC, false>(A);
}

// ------------------------------------------------------------ fused sweep, two chains per wave
// GS_OPT_SWEEP_SCHED = 3 (and the cost model's choice where it applies, launch_sweep_freespec): the
// same sweep as sweep_freespec_body for NF = 60 on the tiled model block (nm <= 16) with device Philox,
// each wavefront running chains c, c + 1 side by side and drawing their b together
// (gibbs_tile2.h bdraw_tile_pair60).  Every draw, uniform and record is the one-chain kernel's bit for
// bit: the Philox counters are per chain, a chain whose gate is shut has its (computed) draw discarded
// exactly where the one-chain kernel skips it, and a failed factorisation keeps that chain's b.
// 2 waves per SIMD (both chains' tiles: ~200 VGPRs): 4096 chains are 2048 waves, one round.
// A wave's LDS after the model block (doubles); the kernel's pointers and the launcher's size both come
// from here.
struct SweepPairLds {
  // a chain's stride in each slot: a row of 64 lanes; b = bF | bM; the prefetched normals and z_M as
  // gibbs_tile2.h indexes them (pair_prefetch_read: 80 per chain, bdraw_tile_pair60's zmslot: 64)
  static constexpr int ROW = 64, B = 2 * ROW, PF = 80;
  static constexpr int scr0 = 0, scr1 = gs_tile_scr(60);  // the chains' tile scratches
  static constexpr int bsave = 2 * gs_tile_scr(60);        // [2][B]: their previous b (failed or shut draws)
  static constexpr int zm = bsave + 2 * B;                 // [2][ROW]: their z_M during the draw
  static constexpr int xpark = zm + 2 * ROW;               // [2][ROW]: their x during the draw (not in VGPRs)
  static constexpr int pf = xpark + 2 * ROW;  // [2][PF]: the next draw's normals (PairPrefetch's slot)
  static constexpr int total = pf + 2 * PF;
};
constexpr int GS_PAIR_SCR = SweepPairLds::total;
// GS_PAIR_RHO_PRIO: issue priority of the pair kernel's rho step (the one-chain kernels: GS_RHO_PRIO = 0).
// Measured on the headline (r06x, 4 interleaved reps): 1.915-1.927 ms per launch at 1 against
// 1.928-1.938 at 0 and 1.931-1.943 at 2
#ifndef GS_PAIR_RHO_PRIO
#define GS_PAIR_RHO_PRIO 1
#endif

// The arguments k_sweep_pair's sweep loop reads, fetched where they are used: scalar loads from the
// kernel-argument segment through an opaque pointer (the loads a use does not need fold away).  Read
// from the by-value parameter they were loaded once, held in SGPRs across the draw -- spilled into VGPR
// lanes there -- and brought back at every sweep with a v_readlane_b32 each, a VALU issue slot: 16 at
// the head of the rho step alone.  GS_PAIR_ARGS_RELOAD = 0 reads the parameter (A/B builds).
#ifndef GS_PAIR_ARGS_RELOAD
#define GS_PAIR_ARGS_RELOAD 1
#endif
struct PairLoopArgs {
  int64_t it0;
  double rhomin, rhomax;
  double *x_rec, *b_rec;
  int32_t* fail_count;
  gs_key key;
  int psr_base;
};
__device__ __forceinline__ PairLoopArgs pair_loop_args(const SweepArgs& A) {
  if constexpr (GS_PAIR_ARGS_RELOAD != 0) {
    // (SweepArgs is the kernel's only parameter: it sits at the start of the segment)
    auto* k = (const __attribute__((address_space(4))) SweepArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return {k->it0, k->rhomin, k->rhomax, k->x_rec, k->b_rec, k->fail_count, {k->key.k0, k->key.k1}, k->psr_base};
  } else {
    return {A.it0, A.rhomin, A.rhomax, A.x_rec, A.b_rec, A.fail_count, A.key, A.psr_base};
  }
}

template <int WPB>
__global__ __launch_bounds__(64 * WPB, 2) void k_sweep_pair(SweepArgs A) {
  extern __shared__ double lds[];
  constexpr int NF = 60, NFR = 30;
  const int wave = gs_wave_id(), lane = threadIdx.x & 63;
  constexpr int CPB = 2 * WPB;
  const int nb = (A.n_chain + CPB - 1) / CPB;
  const int p = blockIdx.x / nb;
  const int cA = (blockIdx.x % nb) * CPB + 2 * wave;  // chains cA, cA + 1 (n_chain is even)
  const int nM = __builtin_amdgcn_readfirstlane(A.nm[p]);
  stage_model_tiled(lds, A.model + (int64_t)p * A.mstride, NF, A.NMX, nM);
  const int64_t mlds = model_tiled_doubles(NF, A.NMX);
  if (cA >= A.n_chain) return;
  int NMXe = A.NMX;
  const ModelTiled M = model_tiled_view_psr<true>(lds, NF, A.NMX, nM, NMXe);
  const int64_t n_sys = (int64_t)A.n_psr * A.n_chain;
  const bool act = lane < NF, actm = lane < nM;
  const int kf = act ? (lane >> 1) : 0;
  const int fi = act ? A.fidx[p * NF + lane] : 0;
  const int mi = actm ? A.midx[p * A.NMX + lane] : 0;
  double* wl = lds + mlds + (int64_t)wave * GS_PAIR_SCR;
  double* const scr[2] = {wl + SweepPairLds::scr0, wl + SweepPairLds::scr1};
  double* bsave = wl + SweepPairLds::bsave;
  double* zmslot = wl + SweepPairLds::zm;
  double* xpark = wl + SweepPairLds::xpark;
  double* pfslot = wl + SweepPairLds::pf;  // written in this draw's tail
  // the slot holds the normals of the draw that comes next (wave-uniform).  Not at a launch's first draw,
  // nor after a sweep whose draw was skipped (both gates shut): those generate their normals inline
  bool pfv = false;

  const double irhomin = 1.0 / A.rhomin, irhomax = 1.0 / A.rhomax;
  const int64_t xr_step = n_sys * NFR;
  const int64_t br_step = (A.brec_nc == 0 ? n_sys : (int64_t)A.n_psr * A.brec_nc) * A.ldb;
  const int S = A.n_sweeps;
  int64_t sys[2];
  long long gchain[2];
  double x[2], bF[2], bM[2];
  int fail[2] = {0, 0};
  // record targets: per-lane 32/64-bit offsets from the uniform record bases (-1: this lane records
  // nothing), advanced by one sweep's rows per iteration
  int xro[2], bFo[2], bMo[2];
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const int c = cA + ch;
    sys[ch] = (int64_t)p * A.n_chain + c;
    gchain[ch] = A.chain_base + c;
    x[ch] = act ? A.x_state[sys[ch] * NFR + kf] : 0.0;
    bF[ch] = act ? A.b_state[sys[ch] * A.ldb + fi] : 0.0;
    bM[ch] = actm ? A.b_state[sys[ch] * A.ldb + mi] : 0.0;
    xro[ch] = (A.x_rec && act && !(lane & 1)) ? (int)(sys[ch] * NFR + kf) : -1;
    const bool brec = A.b_rec && (A.brec_nc == 0 || c < A.brec_nc);
    const int64_t brow0 = A.brec_nc == 0 ? sys[ch] : (int64_t)p * A.brec_nc + c;
    bFo[ch] = (brec && act) ? (int)(brow0 * A.ldb + fi) : -1;
    bMo[ch] = (brec && actm) ? (int)(brow0 * A.ldb + mi) : -1;
  }
#pragma unroll 1
  for (int sw = 0; sw < S; ++sw) {
    const PairLoopArgs Ah = pair_loop_args(A);
    const long long ii = Ah.it0 + sw;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {  // record-before-update (pulsar_gibbs.py:658-659)
      if (xro[ch] >= 0) Ah.x_rec[sw * xr_step + xro[ch]] = x[ch];
      if (bFo[ch] >= 0) Ah.b_rec[sw * br_step + bFo[ch]] = bF[ch];
      if (bMo[ch] >= 0) Ah.b_rec[sw * br_step + bMo[ch]] = bM[ch];
    }
#pragma unroll 1
    for (int pass = (ii == 0) ? 0 : 1; pass < 2; ++pass) {
      int ev = GS_EV_B0;
      double phinv[2] = {0.0, 0.0};
      bool draw[2] = {true, true};
      if (pass == 1) {
        if constexpr (GS_PAIR_RHO_PRIO > 0) __builtin_amdgcn_s_setprio(GS_PAIR_RHO_PRIO);
        {
          // rho|b analytic (pulsar_gibbs.py:208-216, 236), as sweep_freespec_body, for both chains in
          // one pass: lane 32 h + k computes frequency k of chain h (the one-chain layout has each
          // frequency on two lanes), same operations and Philox counter per (chain, k)
          const int h = lane >> 5, k = lane & 31;
          const bool am = k < NFR;
          double tau2[2];
#pragma unroll
          for (int ch = 0; ch < 2; ++ch) {
            const double partner = __shfl_xor(bF[ch], 1);
            const double be = (lane & 1) ? partner : bF[ch], bo = (lane & 1) ? bF[ch] : partner;
            tau2[ch] = gs_add_rn(gs_mul_rn(be, be), gs_mul_rn(bo, bo)) / 2;
          }
          const int src = am ? 2 * k : 0;
          const double ta = gtile::bcast_lane_bp(tau2[0], src), tb = gtile::bcast_lane_bp(tau2[1], src);
          const double tau = h ? tb : ta;
          double U, u2;
          // (kc opaque: the first Philox round's products of the lane, invariant over the sweeps, were
          // hoisted out of the sweep loop, spilled across the draw and reloaded here)
          int kc = k;
          uint32_t cz = (uint32_t)(h ? gchain[1] : gchain[0]);  // the counter's chain word
          asm volatile("" : "+v"(kc), "+v"(cz));
          const PairLoopArgs Ar = pair_loop_args(A);
          gs_uniform2(gs_counter(kc, ii, cz, p + Ar.psr_base, GS_EV_RHO), pair_key(Ar.key), U, u2);
          // (1 - exp(arg) is exactly 1 where the law skips the exp, so its one ballot over both chains
          // draws the same values as a ballot per chain)
          const RhoDraw rd = rho_given_b(tau, U, Ar.rhomin, Ar.rhomax, irhomin, irhomax, am);
          const double xnew = rd.xnew, phm = rd.phinv;
          // gate: all(xnew != x_old[-1])  (pulsar_gibbs.py:697), per chain
          const double xl0 = rdlane(x[0], NF - 1), xl1 = rdlane(x[1], NF - 1);
          const unsigned long long same = __ballot(am && (xnew == (h ? xl1 : xl0)));
          draw[0] = (same & 0xffffffffull) == 0ull;
          draw[1] = (same >> 32) == 0ull;
          // back to the one-chain layout: lane l of chain ch holds frequency l >> 1
#pragma unroll
          for (int ch = 0; ch < 2; ++ch) {
            const int from = 32 * ch + (act ? (lane >> 1) : 0);
            const double xv = gtile::bcast_lane_bp(xnew, from), pv = gtile::bcast_lane_bp(phm, from);
            x[ch] = act ? xv : 0.0;
            phinv[ch] = act ? pv : 0.0;
          }
        }
        if constexpr (GS_PAIR_RHO_PRIO > 0) __builtin_amdgcn_s_setprio(GS_BASE_PRIO);
        if (!draw[0] && !draw[1]) {
          pfv = false;  // the slot's normals were this sweep's
          break;
        }
        ev = GS_EV_B;
      }
      double zF[2], zM[2];
      const PairLoopArgs Ad = pair_loop_args(A);
      if (pfv) {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) pair_prefetch_read(pfslot, ch, lane, zF[ch], zM[ch]);
      } else {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
          gs_normal2(gs_counter(lane, ii, gchain[ch], p + Ad.psr_base, ev), pair_key(Ad.key), zF[ch], zM[ch]);
      }
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {
        if (pass == 0) phinv[ch] = act ? 1.0 / pow(10.0, 2.0 * x[ch]) : 0.0;  // first draw from xs
        // the previous b waits in the wave's save slot (a failed or shut draw keeps it)
        bsave[SweepPairLds::B * ch + lane] = bF[ch];
        bsave[SweepPairLds::B * ch + SweepPairLds::ROW + lane] = bM[ch];
        xpark[SweepPairLds::ROW * ch + lane] = x[ch];
      }
      int f[2];
      // the draw that follows is GS_EV_B of this sweep (after pass 0) or of the next: same counters,
      // functions and bits as the inline path.  (The last sweep's prefetch is generated and dropped: a
      // uniform branch around it would cut the draw's tail into separate scheduling regions.)
      const PairPrefetch pf = {Ad.key, (uint32_t)(ii + pass), {(uint32_t)gchain[0], (uint32_t)gchain[1]},
                               p + Ad.psr_base, GS_EV_B, pfslot};
      bdraw_tile_pair60<true, true>(M, NMXe, nM, lane, phinv, zF, zM, bF, bM, scr, zmslot, f, pf);
      pfv = true;
      gtile::lds_fence();
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {
        x[ch] = xpark[SweepPairLds::ROW * ch + lane];
        const bool keep = !draw[ch] || f[ch];
        if (keep) {
          gtile::lds_fence();
          bF[ch] = bsave[SweepPairLds::B * ch + lane];
          bM[ch] = bsave[SweepPairLds::B * ch + SweepPairLds::ROW + lane];
        }
        if (draw[ch] && f[ch]) {
          if (!fail[ch]) fail[ch] = f[ch];
          int32_t* const fc = pair_loop_args(A).fail_count;
          if (fc && lane == 0) fc[sys[ch]] += 1;
        }
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    if (act && !(lane & 1)) A.x_state[sys[ch] * NFR + kf] = x[ch];
    if (act) A.b_state[sys[ch] * A.ldb + fi] = bF[ch];
    if (actm) A.b_state[sys[ch] * A.ldb + mi] = bM[ch];
    if (A.info && lane == 0) A.info[sys[ch]] = fail[ch];
  }
}

// ------------------------------------------------------------ rho|b analytic
__global__ void k_rho_analytic(RhoArgs A) {
  const int64_t n_sys = (int64_t)A.n_psr * A.n_chain;
  const int NFR = A.NF / 2;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_sys * NFR) return;
  const int64_t sys = t / NFR;
  const int k = (int)(t % NFR);
  const int p = (int)(sys / A.n_chain), c = (int)(sys % A.n_chain);
  const double bs = A.b[sys * A.ldb + A.fidx[p * A.NF + 2 * k]];
  const double bc = A.b[sys * A.ldb + A.fidx[p * A.NF + 2 * k + 1]];
  const double tau = gs_add_rn(gs_mul_rn(bs, bs), gs_mul_rn(bc, bc)) / 2;  // numpy's rounding
  double U;
  if (A.u) {
    U = A.u[sys * NFR + k];
  } else {
    double u2;
    gs_uniform2(gs_counter(k, gs_sweep(A.sweep, A.sweep_dev), A.chain_base + c, p + A.psr_base, GS_EV_RHO), A.key, U, u2);
  }
  const double hi = 1 - exp((tau / A.rhomax) - (tau / A.rhomin));
  const double eta = 0.0 + hi * U;
  const double rho = tau / ((tau / A.rhomax) - log(1 - eta));
  A.x[sys * A.ldx + k] = 0.5 * log10(rho);
}

#ifdef GS_PHASE_PROF
extern "C" int gs_debug_phase_cycles(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gs_phase_cyc), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(gs_phase_cyc), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// The fused sweep's tile variant: the fixed block of the staged model tiled (NMX <= 16) or row-major.
template <int WPB>
int dispatch_nf_sweep_tile(int NF, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
  const bool fx = model_tiled_fix(a.NMX);
  return dispatch_nf(NF, [&](auto nfc, auto ntc) {
    constexpr int NFC = decltype(nfc)::value, NTC = decltype(ntc)::value;
    return fx ? launch_lds(k_sweep_freespec<NFC, NTC, WPB, 3>, grid, 64 * WPB, lds, s, a)
              : launch_lds(k_sweep_freespec_rm<NFC, NTC, WPB, 3>, grid, 64 * WPB, lds, s, a);
  });
}
// Every variant (the one-chain-per-wave shape).  The lane-row variants read the row-major block, not the
// tiled one, so k_sweep_freespec serves them whatever NMX.
template <int WPB>
int dispatch_nf_sweep(int NF, int bc, dim3 grid, size_t lds, hipStream_t s, const SweepArgs& a) {
  if (bc == GS_BCAST_TILE) return dispatch_nf_sweep_tile<WPB>(NF, grid, lds, s, a);
  return dispatch_nf(NF, [&](auto nfc, auto) {
    constexpr int NFC = decltype(nfc)::value;
    GS_LANE_ROW_CASES(k_sweep_freespec)
    return dispatch_nf_sweep_tile<WPB>(NF, grid, lds, s, a);  // NF at run time: the tile variant
  });
}

// Workgroup shape of the tile-variant sweep (GS_OPT_SWEEP_SCHED 0: this cost model).  In units
// of one full round R (3 waves on each SIMD for the launch's sweeps; measured on MI355X, NF = 60,
// r03n/r03q): 4-wave workgroups take floor(q/3) R + g(q mod 3) with q = waves per SIMD and a
// part-filled last round of 1 / 2 waves per SIMD costing g = 0.46 / 0.74 R (latency-bound); the
// 12-wave hand-off workgroups (4/3 chains per wave) take ceil(workgroups / CUs) x 4/3 R whatever
// the last round's fill.  4096 chains: 1.46 R vs 1.33 R (2.232 vs 2.072 ms); 3072: 1 R vs 1.33 R;
// configs[2] (45 x 256): 3.74 R vs 4 R.
// rounds R of the launch in the two one-chain shapes: 4-wave workgroups, 12-wave hand-off workgroups
struct OneChainRounds {
  double w4, w12;
};
static OneChainRounds one_chain_rounds(const SweepArgs& a) {
  const double ncu = device_cus();
  const double q = (double)a.n_psr * a.n_chain / (4.0 * ncu);
  const double k = std::floor(q / 3.0), r = q - 3.0 * k;
  const double g = r <= 0.0 ? 0.0 : r <= 1.0 ? 0.46 * r : r <= 2.0 ? 0.46 + 0.28 * (r - 1.0) : 0.74 + 0.26 * (r - 2.0);
  const double wg = (double)a.n_psr * ((a.n_chain + 15) / 16);
  return {k + g, std::ceil(wg / ncu) * (4.0 / 3.0)};
}
static bool sweep_handoff_wins(const SweepArgs& a) {
  if (a.sched) return a.sched == 1;
  const OneChainRounds one = one_chain_rounds(a);
  return one.w12 < 0.97 * one.w4;
}
// Two chains per wave (k_sweep_pair) against the one-chain shapes, in the same unit R.  Its waves run
// 2 per SIMD: a full round (8 waves per CU, 16 chains) takes P = 1.27 R and a last round of at most one
// wave per SIMD 0.70 P (r06l, 1 GPU: 4096 chains 1.965 ms = P, 8192 3.905 ms, 2048 and 1024 chains
// 1.37-1.38 ms; R = 1.55 ms from the 4096-chain one-chain / hand-off times above).  4096 chains: 1.27 R
// vs 1.33 R (hand-off); 8192: 2.54 R vs 2.67 R; 6144: 2.16 R vs 2 R; 2048: 0.89 R vs 0.74 R.
static bool sweep_pair_wins(const SweepArgs& a) {
  if (a.sched) return a.sched == 3;
  const double ncu = device_cus();
  const OneChainRounds oc = one_chain_rounds(a);
  const double one = std::min(oc.w4, oc.w12);
  const double w = (double)a.n_psr * (a.n_chain / 2) / (4.0 * ncu);  // pair waves per SIMD
  const double kp = std::floor(w / 2.0), rp = w - 2.0 * kp;
  const double pair = 1.27 * (kp + (rp <= 0.0 ? 0.0 : rp <= 1.0 ? 0.70 : 1.0));
  return pair < 0.97 * one;
}
}  // namespace

int launch_sweep_freespec(hipStream_t s, const SweepArgs& a, int* shape) {
  const bool fixed = a.NF == 20 || a.NF == 40 || a.NF == 60;
  const bool tiled = !fixed || a.bcast == GS_BCAST_TILE;
  const size_t mlds = tiled ? (size_t)model_tiled_doubles(a.NF, a.NMX) : (size_t)a.mstride;
  // two chains per wave (k_sweep_pair): NF = 60 on the tiled block with a tiled fixed part, device
  // Philox (no injected draws), an even chain count
  const bool pair_ok = a.NF == 60 && tiled && model_tiled_fix(a.NMX) && !a.z0_inj && !a.z_inj && !a.u_inj &&
                       (a.n_chain % 2) == 0 && !a.dbg_handoff;
  if (pair_ok && sweep_pair_wins(a)) {
    constexpr int WPB = GS_PAIR_WPB;
    const size_t lds = (mlds + (size_t)WPB * GS_PAIR_SCR) * sizeof(double);
    // two workgroups per CU (the kernel's 2 waves per SIMD) must fit the CU's 160 KB
    if (lds <= device_lds_optin() && 2 * lds <= 160 * 1024) {
      const int nb = (a.n_chain + 2 * WPB - 1) / (2 * WPB);
      if (lds > 65536 && set_lds(k_sweep_pair<WPB>, lds)) return 2;
      hipLaunchKernelGGL((k_sweep_pair<WPB>), dim3((unsigned)(a.n_psr * nb)), dim3(64 * WPB), lds, s, a);
      *shape = 3;
      return 0;
    }
  }
  // the 12-wave hand-off shape holds 12 waves' scratch, save and park slots beside the model
  // block: at large NF x NMX (e.g. NF = 60, NMX = 64: 168 KB) it does not fit, and the 4-wave
  // shape (~102 KB there) runs instead, whatever the cost model or GS_OPT_SWEEP_SCHED say
  constexpr int HW = SweepLds::HANDOFF_WPB;
  const size_t lds12 = sweep_lds_bytes((int64_t)mlds, a.NF, GS_BCAST_TILE, HW);
  if (tiled && lds12 <= device_lds_optin() && sweep_handoff_wins(a)) {
    const int nb = (a.n_chain + 15) / 16;
    dim3 grid((unsigned)(a.n_psr * nb));
    *shape = 1;
    return dispatch_nf_sweep_tile<HW>(a.NF, grid, lds12, s, a);
  }
  const int nb = (a.n_chain + GS_SWEEP_WPB - 1) / GS_SWEEP_WPB;
  dim3 grid((unsigned)(a.n_psr * nb));
  // (a run-time NF takes the tile variant whatever a.bcast says)
  const size_t lds = sweep_lds_bytes((int64_t)mlds, a.NF, fixed ? a.bcast : GS_BCAST_TILE, GS_SWEEP_WPB);
  *shape = 2;
  return dispatch_nf_sweep<GS_SWEEP_WPB>(a.NF, a.bcast, grid, lds, s, a);
}

int launch_rho_analytic(hipStream_t s, const RhoArgs& a) {
  const int64_t n = (int64_t)a.n_psr * a.n_chain * (a.NF / 2);
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_rho_analytic, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return 0;
}
