// The marginalised likelihood (k_lnlike_marg) and the PTA hyper-parameter Metropolis block on it
// (k_hyper_mh): the tile factorisation in likelihood mode (gibbs_tile.h, LNL = 1), gfx950, fp64.
#include "gibbs_bdraw.h"

namespace {

// ------------------------------------------------------------ marginalised likelihood
//  get_lnlikelihood_fullmarg pulsar_gibbs.py:569-610, phiinv-dependent part:
//   lnl = 1/2 (d^T Sigma^-1 d - log det Sigma) + 1/2 sum_F log phiinv_F
// with the prefix: d^T Sigma^-1 d = |e|^2 + |y|^2, log det Sigma = 2 sum log diag L_M +
// log det S; |y|^2 and log det S come out of the augmented tile factorisation.  The
// model constants -1/2 (log det N + r^T N^-1 r) - 1/2 sum_M log phi_M are the caller's.
// A shared model block is staged once per workgroup for GS_BDRAW_LOOP chain groups (as k_bdraw):
// staging it for every WPB chains cost more than the factorisations (0.61 ms per configs[3]-shaped
// launch, 92k systems; r04).
template <int NFC, int NTC, int WPB>
__device__ __forceinline__ void lnlike_item(const LnlArgs& A, const double* mb, int p, int c, double* scr, int lane) {
  const int NF = NFC ? NFC : A.NF;
  const int64_t sys = (int64_t)p * A.n_chain + c;
  const ModelLds M = model_view(mb, NF, A.NMX);
  const double phinv = lane < NF ? A.phiinv_F[sys * NF + lane] : 1.0;
  double yy = 0.0, ldS = 0.0;
  // (bdraw_tile_nf and lnl_phi_sum written out: called here they reorder the scheduling of 7 of the 8
  // k_lnlike_marg instantiations -- same registers, other code -- so this copy stays until a change of
  // this kernel's code is wanted anyway)
  int fail;
  if constexpr (NFC == 0)
    fail = bdraw_tile_n<NTC, true>(M, A.NMX, A.nm[p], lane, phinv, 0.0, 0.0, yy, ldS, scr, NF);
  else
    fail = bdraw_tile<NFC, true>(M, A.NMX, A.nm[p], lane, phinv, 0.0, 0.0, yy, ldS, scr);
  double lph = lane < NF ? gs_log_lnl(phinv) : 0.0;  // phinv > 0 (lnl_terms)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lph += __shfl_xor(lph, o);
  const int64_t ao = model_aux_offset(NF, A.NMX);
  const double lm = mb[ao], ee = mb[ao + 1];
  if (lane == 0) {
    A.lnl[sys] = GS_LNL_VALUE(fail, ee, lm, yy, ldS, lph);
    if (A.info) A.info[sys] = fail;
  }
}

template <int NFC, int NTC, int WPB>
__global__ __launch_bounds__(64 * WPB, 2) void k_lnlike_marg(LnlArgs A) {
  extern __shared__ double lds[];
  const int wave = gs_wave_id(), lane = threadIdx.x & 63;
  const int nb = (A.n_chain + WPB - 1) / WPB;
  const bool in_lds = !A.model_per_sys && !A.model_global;
  double* scr = lds + (in_lds ? A.mstride : 0) + wave * gs_tile_scr(NFC ? NFC : A.NF);
  if (!in_lds) {
    const int p = blockIdx.x / nb;
    const int c = (blockIdx.x % nb) * WPB + wave;
    if (c >= A.n_chain || (A.skip && A.skip[c])) return;
    const int64_t sys = (int64_t)p * A.n_chain + c;
    lnlike_item<NFC, NTC, WPB>(A, A.model + (A.model_per_sys ? sys : (int64_t)p) * A.mstride, p, c, scr, lane);
    return;
  }
  const int nbl = (nb + GS_BDRAW_LOOP - 1) / GS_BDRAW_LOOP;
  const int p = blockIdx.x / nbl;
  const int g0 = (blockIdx.x % nbl) * GS_BDRAW_LOOP;
  constexpr int PER = GS_BDRAW_LOOP * WPB;  // chains per workgroup
  __shared__ int sel[PER];
  if (A.skip) {
    // gs_lnlike_marg_gated: workgroup j of pulsar p takes the chains of rank [PER j, PER j + PER)
    // among those with skip[c] == 0 (a block-wide ballot scan of skip), so the model is staged only
    // by workgroups with work and every wave of them draws.  Workgroups past the count return.
    __shared__ int wcnt[WPB];
    __shared__ int base_s;
    const int want0 = (blockIdx.x % nbl) * PER;
    if (threadIdx.x < PER) sel[threadIdx.x] = -1;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (int c0 = 0; c0 < A.n_chain; c0 += 64 * WPB) {
      const int c = c0 + (int)threadIdx.x;
      const bool todo = c < A.n_chain && A.skip[c] == 0;
      const unsigned long long m = __ballot(todo);
      if (lane == 0) wcnt[wave] = __popcll(m);
      __syncthreads();
      int rank = base_s;
      for (int w = 0; w < wave; ++w) rank += wcnt[w];
      rank += __popcll(m & ((1ull << lane) - 1ull));
      if (todo && rank >= want0 && rank < want0 + PER) sel[rank - want0] = c;
      __syncthreads();
      if (threadIdx.x == 0)
        for (int w = 0; w < WPB; ++w) base_s += wcnt[w];
      __syncthreads();
      if (base_s >= want0 + PER) break;
    }
    if (sel[0] < 0) return;
  }
  stage_model(lds, A.model + (int64_t)p * A.mstride, A.mstride);
#pragma unroll 1
  for (int r = 0; r < GS_BDRAW_LOOP; ++r) {
    const int c = A.skip ? sel[r * WPB + wave] : (g0 + r) * WPB + wave;
    if (c < 0 || c >= A.n_chain) break;
    lnlike_item<NFC, NTC, WPB>(A, lds, p, c, scr, lane);
  }
}

// ------------------------------------------------------------ PTA red hyper-parameter MH
// PTABlockGibbs.update_hyper_params with redsample='mh' (pta_gibbs.py:278-340), the reference's
// default: `nsteps` single-parameter Metropolis steps per chain on the summed marginalised
// likelihood get_lnlikelihood (:577-621).  A step moves one red parameter of ONE pulsar p, so
// only lnL_p changes: diff = lnL_p(q) - lnL_p(x) (the reference's full sums (lnlike1 + lnprior1)
// - (lnlike0 + lnprior0) differ from it only by rounding: the other pulsars' terms and the
// uniform prior constants cancel), and a proposal outside its prior box is rejected without a
// likelihood (the reference evaluates it first and can die in cho_factor on the overflowed phi).
// One wavefront per chain (one per workgroup), the chain's x row and lnL_p of every pulsar in LDS,
// the pulsar's model block read from global memory (all blocks ~2 MB: L2-resident), the
// likelihood from the augmented tile factorisation of gs_lnlike_marg (same arithmetic, so
// lnl_p seeded by gs_lnlike_marg and the in-kernel values agree exactly).
// Proposal (pta_gibbs.py:322-328): scale = choice(sizes, p), par = choice(hind), q[par] +=
// randn * (0.05 len(hind)) * scale; accept if diff > log(rand).  Philox event GS_EV_HYPER,
// slots 3 s .. 3 s + 2 of step s: (u_scale, u_par), (Box-Muller pair), (u_acc, -).
// (Two waves per chain, split by pulsar parity, were measured slower on the sweep: HISTORY.md.)
template <int NFC, int NTC>
__global__ __launch_bounds__(64, 2) void k_hyper_mh(HyperMhArgs A) {
  extern __shared__ double lds[];
  const int NF = NFC ? NFC : A.NF;
  const int n_f = NF / 2;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x;
  double* xs = lds;              // the chain's x row
  double* Ls = lds + A.ldx;      // lnL_p of every pulsar at x
  // The proposals do not depend on the chain state: lane l draws step s0 + l's (scale, parameter,
  // normal, log u) for 64 steps at once into the chain's step table (3 Philox blocks per lane in
  // parallel instead of 3 wave-uniform blocks on the critical path of every step).
  double* stab = lds + ((A.ldx + A.n_psr + 1) & ~1);
  double* scr = stab + 4 * 64;
  double* xg = A.x + (int64_t)c * A.ldx;
  for (int i = threadIdx.x; i < A.ldx; i += 64) xs[i] = xg[i];
  for (int p = threadIdx.x; p < A.n_psr; p += 64) Ls[p] = A.lnl_p[(int64_t)p * A.n_chain + c];
  wave_lds_sync();
  const bool act = lane < NF;
  const int kf = act ? (lane >> 1) : 0;
  // the common spectrum is fixed during the block (only red parameters move)
  const double gw = act ? pow(10.0, 2.0 * xs[A.gw_col[kf]]) : 0.0;
  const double sig = 0.05 * A.n_h;  // sigmas = 0.05 * len(hind)
  const long long chain = A.chain_base + c;
  const long long sw = gs_sweep(A.sweep, A.sweep_dev);
  int nacc = 0;
  for (int s0 = 0; s0 < A.nsteps; s0 += 64) {
    const int ns = min(64, A.nsteps - s0);
    if (lane < ns) {
      const int st = s0 + lane;
      double sc, z, u;
      int j;
      if (A.inj) {
        const double* q = A.inj + ((int64_t)st * A.n_chain + c) * 4;
        sc = q[0];
        j = min(max((int)q[1], 0), A.n_h - 1);  // the host validates; never index out of range
        z = q[2];
        u = q[3];
      } else {
        double u1, u2, v1, v2, u4;
        gs_uniform2(gs_counter(3u * st, sw, chain, 0, GS_EV_HYPER), A.key, u1, u2);
        gs_normal2(gs_counter(3u * st + 1, sw, chain, 0, GS_EV_HYPER), A.key, v1, v2);
        gs_uniform2(gs_counter(3u * st + 2, sw, chain, 0, GS_EV_HYPER), A.key, u, u4);
        sc = gs_mh_scale(u1);
        j = min((int)(u2 * A.n_h), A.n_h - 1);
        z = v1;
      }
      stab[4 * lane] = sc;
      stab[4 * lane + 1] = (double)j;
      stab[4 * lane + 2] = z;
      stab[4 * lane + 3] = log(u);
    }
    wave_lds_sync();
    for (int i = 0; i < ns; ++i) {
      const int st = s0 + i;
      const int j = __builtin_amdgcn_readfirstlane((int)stab[4 * i + 1]);
      const int col = A.hcol[j], p = A.hpsr[j];
      if (p < 0) continue;  // a pulsar of another rank (pulsar-sharded run): its steps are applied there
      const double sc = stab[4 * i], z = stab[4 * i + 2], lu = stab[4 * i + 3];
      // q[par] += randn * sigmas * scale, rounded as numpy does (no fma contraction)
      const double xq = gs_add_rn(xs[col], gs_mul_rn(gs_mul_rn(z, sig), sc));
      bool accepted = false;
      if (xq >= A.hlo[j] && xq <= A.hhi[j]) {  // uniform prior: -inf outside (:298, :624-628)
        double red;
        if (A.red_kind == 0) {  // free spectrum: phi_red = 10^(2 rho_red)
          const int rc = A.red_col[p * n_f + kf];
          red = pow(10.0, 2.0 * (rc == col ? xq : xs[rc]));
        } else {                // power law: log phi_red = (a log10_A + c) + g gamma
          const int ca = A.pl_col[2 * p], cg = A.pl_col[2 * p + 1];
          const double la = ca == col ? xq : xs[ca], ga = cg == col ? xq : xs[cg];
          const double* L = A.lnphi + (int64_t)p * 3 * n_f;
          red = exp(gs_add_rn(gs_add_rn(gs_mul_rn(L[n_f + kf], la), L[kf]), gs_mul_rn(L[2 * n_f + kf], ga)));
        }
        const double phinv = act ? 1.0 / (gw + red) : 1.0;
        const double* mb = A.model + (int64_t)p * A.mstride;
        const ModelLds M = model_view(mb, NF, A.NMX);
        double yy = 0.0, ldS = 0.0;
        const int fail =
            bdraw_tile_nf<NFC, NTC, 1, false>(M, A.NMX, A.nm[p], lane, phinv, 0.0, 0.0, yy, ldS, scr, NF);
        const double lph = lnl_phi_sum(act, phinv);  // as gs_lnlike_marg (bit-identical seeds)
        const int64_t ao = model_aux_offset(NF, A.NMX);
        const double L1 = GS_LNL_VALUE(fail, mb[ao + 1], mb[ao], yy, ldS, lph);
        const double diff = L1 - Ls[p];
        if (diff > lu) {
          accepted = true;
          ++nacc;
          if (lane == 0) {
            xs[col] = xq;
            Ls[p] = L1;
          }
        }
        wave_lds_sync();
      }
      if (A.q_rec && lane == 0) {
        double* qr = A.q_rec + ((int64_t)st * A.n_chain + c) * 3;
        qr[0] = (double)j;
        qr[1] = xq;
        qr[2] = accepted ? 1.0 : 0.0;
      }
    }
    wave_lds_sync();  // the next 64 steps rewrite the table
  }
  for (int i = threadIdx.x; i < A.ldx; i += 64) xg[i] = xs[i];
  for (int p = threadIdx.x; p < A.n_psr; p += 64) A.lnl_p[(int64_t)p * A.n_chain + c] = Ls[p];
  if (A.n_acc && threadIdx.x == 0) A.n_acc[c] = nacc;
}

}  // namespace

int launch_lnlike_marg(hipStream_t s, const LnlArgs& a) {
  constexpr int WPB = GS_SWEEP_WPB;
  const int nb = (a.n_chain + WPB - 1) / WPB;
  const bool in_lds = !a.model_per_sys && !a.model_global;
  dim3 grid((unsigned)(a.n_psr * (in_lds ? (nb + GS_BDRAW_LOOP - 1) / GS_BDRAW_LOOP : nb)));
  const size_t lds = ((size_t)(a.model_per_sys || a.model_global ? 0 : a.mstride) + gs_tile_scr(a.NF) * WPB) *
                     sizeof(double);
  // (a shared model block staged in LDS is above 64 KB at e.g. NF = 60 with NMX > 31)
  return dispatch_nf(a.NF, [&](auto nfc, auto ntc) {
    return launch_lds(k_lnlike_marg<decltype(nfc)::value, decltype(ntc)::value, WPB>, grid, 64 * WPB, lds, s, a);
  });
}

int launch_hyper_mh(hipStream_t s, const HyperMhArgs& a) {
  if (a.n_chain == 0) return 0;
  // x row, lnL_p, the 64-step proposal table, the wave's tile scratch
  const size_t lds = ((size_t)((a.ldx + a.n_psr + 1) & ~1) + 4 * 64 + gs_tile_scr(a.NF)) * sizeof(double);
  dim3 grid((unsigned)a.n_chain);
  return dispatch_nf(a.NF, [&](auto nfc, auto ntc) {
    return launch_lds(k_hyper_mh<decltype(nfc)::value, decltype(ntc)::value>, grid, 64, lds, s, a);
  });
}
