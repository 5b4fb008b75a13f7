// Pooled autocovariance of the recorded chains on the device (gs_chain_acf_block,
// gs_chain_acf_reduce, include/pulsar_gibbs.h): the estimator of diagnostics.pooled_iat truncated at
// max_lag = L, for a block of rows of n_group x n_chain chains (the record blocks of the
// single-pulsar samplers: a group is a pulsar).  Values are taken about the fixed mid[j]
// (d = v - mid) and the chains' own means are removed at reduction time:
//   sum_t (d_t - m)(d_{t+k} - m) = P_k - m (2 s1 - F_k - E_k) + (n - k) m^2,   m = s1 / n,
// P_k the lagged product sum, F_k / E_k the sums of the chain's first / last k values.
// Every result is reproducible: no floating-point atomics, and every sum runs in an order fixed
// by the shapes and the call sequence.
//
// The opaque state (doubles; all zeros = empty), T = n_group * n_chain * n_param flat entries
// e = (g * n_chain + c) * n_param + j:
//   [0]              n, the post-burn rows taken so far (int64 bits); [1..7] unused
//   s1   [T]         sum of d
//   head [L][T]      the first L post-burn values (row u of the chain at head[u])
//   tail [L][T]      a ring of the last L values (row u at tail[u % L])
//   part [W][JT][L + 1]   workgroup w's own sum of P over its chains, per parameter lane and lag
// (lanes run along e in every array that a wave reads or writes).
#include "gibbs_internal.h"

namespace {

constexpr int AC_EW = 32;        // entry lanes of a workgroup: (chain lane, parameter lane)
constexpr int AC_NLG = 8;        // lag groups of a workgroup: thread = (entry lane, lag group)
constexpr int AC_THREADS = AC_EW * AC_NLG;
constexpr int AC_ROWS = 240;     // LDS rows of 32 doubles: 60 KB, two workgroups per CU
constexpr int AC_HDR = 8;        // doubles in front of s1
constexpr int AC_LD = 8;         // independent loads a thread keeps in flight
// workgroups the plan aims at: two per CU of an MI355X, so that a workgroup's partial (read and
// written once per call) stays small beside the rows it reads
constexpr int AC_WGS = 512;

}  // namespace

AcfPlan acf_plan(int n_group, int n_chain, int n_param, int max_lag) {
  AcfPlan p;
  int jt = 1;
  while (jt < n_param && jt < AC_EW) jt *= 2;
  p.jt = jt;
  p.ct = AC_EW / jt;
  p.njt = (n_param + jt - 1) / jt;
  const int64_t passes = ((int64_t)n_chain + p.ct - 1) / p.ct;          // per (group, parameter tile)
  const int64_t tiles = (int64_t)n_group * p.njt;
  int64_t per = tiles > 0 ? (passes * tiles + AC_WGS - 1) / AC_WGS : 1;  // passes per workgroup
  per = per < 1 ? 1 : per;
  p.cs = per * p.ct;                                                     // chains per workgroup
  p.ns = p.cs > 0 ? ((int64_t)n_chain + p.cs - 1) / p.cs : 0;            // workgroups per tile
  p.T = (int64_t)n_group * n_chain * n_param;
  p.off_s1 = AC_HDR;
  p.off_head = p.off_s1 + p.T;
  p.off_tail = p.off_head + (int64_t)max_lag * p.T;
  p.off_part = p.off_tail + (int64_t)max_lag * p.T;
  p.size = p.off_part + tiles * p.ns * jt * (int64_t)(max_lag + 1);
  return p;
}

namespace {

// first row of the block at or above burn (the rows below burn are a prefix: the sweep index
// rises with r) -- gs_chain_summary_block's rule
__device__ __forceinline__ int acf_first_row(const AcfArgs& A) {
  const long long sw0 = gs_sweep(A.sweep, A.sweep_dev);
  long long first = (long long)A.burn - sw0;
  first = first < 0 ? 0 : first;
  return first < A.n_rows ? (int)first : A.n_rows;
}

// grid (groups x parameter tiles x chain strips), 256 threads = 32 entry lanes x 8 lag groups.
// A workgroup owns the chains [strip * cs, (strip + 1) * cs) of one group and one tile of jt
// parameters, ct = 32 / jt chains per pass.  Per pass and tile of rows it stages the d values of
// its 32 entries in LDS, rows q (relative to the block's first post-burn row; q < 0 from the
// state's ring, zero before the chain's first row): the window [t0 - klo - KT, t0 + RT) -- for
// klo > 0 the window of earlier members [t0 - klo - KT, t0 + RT - klo - 1) and the rows
// [t0, t0 + RT) apart.  Thread (entry, lag group lg) holds the sums of lags kb + 1 .. kb + KL,
// kb = klo + lg * KL, in registers with the last KL earlier members beside them, and walks t
// upwards: two LDS reads per KL (+ 1) fmas.  Lag 0 rides with every thread (used from lag group 0
// of the first lag tile).  The sums run on over the workgroup's passes; then the chain lanes of a
// parameter are added in ascending order and the result goes onto the workgroup's partial.
template <int KL>
__global__ __launch_bounds__(AC_THREADS) void k_chain_acf_block(AcfArgs A) {
  constexpr int KT = KL * AC_NLG;
  __shared__ double sh[AC_ROWS * AC_EW];
  const AcfPlan& P = A.plan;
  const int tid = threadIdx.x, el = tid & (AC_EW - 1), lg = tid >> 5;
  const int L = A.max_lag, np = A.n_param, C = A.n_chain;
  const int r0 = acf_first_row(A);
  const int nb = A.n_rows - r0;
  if (nb == 0) return;  // whole block below burn (uniform: before any barrier)
  const int64_t n_prev = *(const int64_t*)A.state;

  const int64_t wg = blockIdx.x;
  const int64_t tile = wg / P.ns, strip = wg - tile * P.ns;
  const int g = (int)(tile / P.njt), jtile = (int)(tile - (int64_t)g * P.njt);
  const int jl = el & (P.jt - 1), cl = el / P.jt;
  const int j = jtile * P.jt + jl;
  const bool jok = j < np;
  const double mid = jok ? A.mid[j] : 0.0;
  const int64_t c_lo = strip * P.cs;
  const int64_t c_hi = c_lo + P.cs < C ? c_lo + P.cs : (int64_t)C;
  const double* tail = A.state + P.off_tail;
  double* part = A.state + P.off_part + wg * P.jt * (int64_t)(L + 1);
  // rows of a tile: one lag tile keeps the rows inside its window, more keep them apart
  const int RT = L <= KT ? AC_ROWS - KT : (AC_ROWS - KT) / 2 / KL * KL;
  const int step = AC_NLG % L;  // a thread's ring slot from one of its rows to the next

  for (int klo = 0; klo < L; klo += KT) {
    const int kb = klo + lg * KL;
    const bool active = kb < L;
    const int arow = klo == 0 ? KT : RT + KT;      // LDS row of t = t0
    const int nwin = klo == 0 ? RT + KT : RT + KT - 1;
    double acc[KL], acc0 = 0.0;
#pragma unroll
    for (int i = 0; i < KL; ++i) acc[i] = 0.0;

    for (int64_t c0 = c_lo; c0 < c_hi; c0 += P.ct) {
      const int64_t c = c0 + cl;
      const bool eok = jok && c < c_hi;
      const int64_t e = ((int64_t)g * C + c) * np + j;
      for (int t0 = 0; t0 < nb; t0 += RT) {
        __syncthreads();
        {
          // row r of the window is q = t0 - klo - KT + r; its ring slot advances with r.  AC_LD
          // loads in flight: every lane loads from a valid address (mid where it has no value)
          // and the value is chosen afterwards
          long long q = (long long)t0 - klo - KT + lg;
          int slot = (int)((((n_prev + q) % L) + L) % L);
          for (int r = lg; r < nwin; r += AC_NLG * AC_LD) {
            double v[AC_LD];
            int kind[AC_LD];  // 1: a row of the block, 2: a row of the ring, 0: none
#pragma unroll
            for (int u = 0; u < AC_LD; ++u) {
              const long long qu = q + u * AC_NLG;
              const bool in = eok && r + u * AC_NLG < nwin && qu < nb;
              kind[u] = in && qu >= 0 ? 1 : (in && n_prev + qu >= 0 ? 2 : 0);
              const double* p = kind[u] == 1 ? A.x + (int64_t)(r0 + qu) * A.row_stride + e
                                             : (kind[u] == 2 ? tail + (int64_t)slot * P.T + e : A.mid);
              v[u] = *p;
              slot += step;
              slot = slot >= L ? slot - L : slot;
            }
#pragma unroll
            for (int u = 0; u < AC_LD; ++u)
              if (r + u * AC_NLG < nwin)
                sh[(r + u * AC_NLG) * AC_EW + el] = kind[u] == 1 ? v[u] - mid : (kind[u] == 2 ? v[u] : 0.0);
            q += AC_NLG * AC_LD;
          }
        }
        if (klo != 0) {
          for (int r = lg; r < RT; r += AC_NLG) {
            const int q = t0 + r;
            sh[(arow + r) * AC_EW + el] =
                eok && q < nb ? A.x[(int64_t)(r0 + q) * A.row_stride + e] - mid : 0.0;
          }
        }
        __syncthreads();
        if (!active) continue;
        const int tend = nb - t0 < RT ? nb - t0 : RT;
        // LDS row of the newest earlier member at t = t0: q = t0 - kb - 1
        const double* wp = sh + (KT - 1 - lg * KL) * AC_EW + el;
        const double* vp = sh + arow * AC_EW + el;
        double w[KL];
        w[0] = 0.0;
#pragma unroll
        for (int s = 1; s < KL; ++s) w[s] = wp[(s - KL) * AC_EW];
        for (int tb = 0; tb < tend; tb += KL) {
#pragma unroll
          for (int s = 0; s < KL; ++s) {
            if (tb + s >= tend) break;
            w[s] = wp[(tb + s) * AC_EW];
            const double v = vp[(tb + s) * AC_EW];
            acc0 = fma(v, v, acc0);
#pragma unroll
            for (int i = 0; i < KL; ++i) acc[i] = fma(w[(s - i + KL) % KL], v, acc[i]);
          }
        }
      }
    }

    // the chain lanes of each parameter lane, in ascending order, onto the workgroup's partial
    __syncthreads();
    if (lg == 0) sh[el] = acc0;
#pragma unroll
    for (int i = 0; i < KL; ++i) sh[(1 + lg * KL + i) * AC_EW + el] = acc[i];
    __syncthreads();
    for (int idx = tid; idx < P.jt * (KT + 1); idx += AC_THREADS) {
      const int j2 = idx / (KT + 1), kk = idx - j2 * (KT + 1);
      const int k = kk == 0 ? 0 : klo + kk;
      if ((kk == 0 && klo != 0) || k > L) continue;
      double sum = sh[kk * AC_EW + j2];
      for (int c2 = 1; c2 < P.ct; ++c2) sum += sh[kk * AC_EW + c2 * P.jt + j2];
      part[(int64_t)j2 * (L + 1) + k] += sum;
    }
  }
}

// one thread per flat entry, after k_chain_acf_block has read the ring: s1 in ascending r, the
// head rows that are still empty, and the block's last L rows into the ring
__global__ __launch_bounds__(256) void k_chain_acf_update(AcfArgs A) {
  const AcfPlan& P = A.plan;
  const int r0 = acf_first_row(A);
  const int nb = A.n_rows - r0;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (nb == 0 || e >= P.T) return;
  const int L = A.max_lag;
  const int64_t n_prev = *(const int64_t*)A.state;
  const double mid = A.mid[e % A.n_param];
  double* s1 = A.state + P.off_s1;
  double* head = A.state + P.off_head;
  double* tail = A.state + P.off_tail;
  double a = s1[e];
  int64_t slot = n_prev % L;
  const double* xe = A.x + (int64_t)r0 * A.row_stride + e;
  auto take = [&](int q, double v) {
    const double d = v - mid;
    a = a + d;
    if (n_prev + q < L) head[(n_prev + q) * P.T + e] = d;
    if (q >= nb - L) tail[slot * P.T + e] = d;
    slot = slot + 1 == L ? 0 : slot + 1;
  };
  int q = 0;
  for (; q + AC_LD <= nb; q += AC_LD) {
    double v[AC_LD];
#pragma unroll
    for (int u = 0; u < AC_LD; ++u) v[u] = xe[(int64_t)(q + u) * A.row_stride];
#pragma unroll
    for (int u = 0; u < AC_LD; ++u) take(q + u, v[u]);
  }
  for (; q < nb; ++q) take(q, xe[(int64_t)q * A.row_stride]);
  s1[e] = a;
}

__global__ void k_chain_acf_count(AcfArgs A) {
  *(int64_t*)A.state += A.n_rows - acf_first_row(A);
}

__global__ void k_chain_acf_count_out(AcfArgs A, int64_t* n_out) { n_out[0] = *(const int64_t*)A.state; }

// ---- gs_chain_acf_reduce
constexpr int AR_THREADS = 256;
constexpr int AR_LD = 8;  // independent loads a thread keeps in flight

// grid (n_group * L): block (g, k), k = 1 .. L, writes D_k[j] = sum_c m_c (head_c[k - 1] + the
// chain's k-th value from the end) into acov[g][j][k] for every j -- the growth of sum_c m_c
// (F_k + E_k) from lag k - 1 to k (0 for k >= n).  Threads (chain lane, parameter lane): lanes
// along the parameters of a chain, the chains of a thread in ascending order, then the chain
// lanes in ascending order.
__global__ __launch_bounds__(AR_THREADS) void k_chain_acf_edges(AcfArgs A, double* acov) {
  __shared__ double red[AR_THREADS];
  const AcfPlan& P = A.plan;
  const int L = A.max_lag, np = A.n_param, C = A.n_chain;
  const int g = blockIdx.x / L, k = blockIdx.x - g * L + 1;
  const int64_t n = *(const int64_t*)A.state;
  const int tid = threadIdx.x;
  const int jt = np < AR_THREADS ? np : AR_THREADS, nc = AR_THREADS / jt;
  const int jl = tid % jt, cl = tid / jt;
  const double* s1 = A.state + P.off_s1;
  const double* head = A.state + P.off_head + (int64_t)(k - 1) * P.T;
  const double* tail = A.state + P.off_tail + (k < n ? ((n - k) % L) * P.T : 0);
  const double nd = (double)n;
  for (int j0 = 0; j0 < np; j0 += jt) {
    const int j = j0 + jl;
    double a = 0.0;
    if (k < n && cl < nc && j < np) {
      for (int c = cl; c < C; c += nc * AR_LD) {
        double s[AR_LD], h[AR_LD], t[AR_LD];
#pragma unroll
        for (int u = 0; u < AR_LD; ++u) {
          const int cu = c + u * nc < C ? c + u * nc : c;  // a valid chain; dropped below
          const int64_t e = ((int64_t)g * C + cu) * np + j;
          s[u] = s1[e];
          h[u] = head[e];
          t[u] = tail[e];
        }
#pragma unroll
        for (int u = 0; u < AR_LD; ++u)
          if (c + u * nc < C) a = fma(s[u] / nd, h[u] + t[u], a);
      }
    }
    red[tid] = a;
    __syncthreads();
    if (cl == 0 && j < np) {
      double sum = red[jl];
      for (int c2 = 1; c2 < nc; ++c2) sum += red[c2 * jt + jl];
      acov[((int64_t)g * np + j) * (L + 1) + k] = sum;
    }
    __syncthreads();
  }
}

// grid (n_group * n_param): block (g, j) turns its row of acov, which holds D_1 .. D_L, into the
// pooled autocovariance: the prefix sums of D (thread 0, ascending k), S_a = sum_c m_c s1_c and
// S_b = sum_c m_c^2 (a thread's chains, then the threads, ascending), the partials of the
// workgroups in ascending order, and
//   acov_k = (sum_w P_k - 2 S_a + sum_{i <= k} D_i + (n - k) S_b) / (C n)   for k < n,
// the bare sum of P_k for k >= n: exactly 0, or NaN where a non-finite value came in.
__global__ __launch_bounds__(AR_THREADS) void k_chain_acf_finish(AcfArgs A, double* acov, int64_t* n_out) {
  extern __shared__ double dp[];  // [L + 1] prefix sums, [2 * AR_THREADS] reduction
  const AcfPlan& P = A.plan;
  const int L = A.max_lag, np = A.n_param, C = A.n_chain;
  const int g = blockIdx.x / np, j = blockIdx.x - g * np;
  const int tid = threadIdx.x;
  const int64_t n = *(const int64_t*)A.state;
  if (blockIdx.x == 0 && tid == 0) n_out[0] = n;
  double* row = acov + ((int64_t)g * np + j) * (L + 1);
  double* ra = dp + L + 1;
  double* rb = ra + AR_THREADS;
  const double nd = (double)n;
  const double* s1 = A.state + P.off_s1;
  double sa = 0.0, sb = 0.0;
  if (n > 0) {
    for (int c = tid; c < C; c += AR_THREADS) {
      const double s = s1[((int64_t)g * C + c) * np + j], m = s / nd;
      sa = fma(m, s, sa);
      sb = fma(m, m, sb);
    }
  }
  ra[tid] = sa;
  rb[tid] = sb;
  for (int k = tid; k <= L; k += AR_THREADS) dp[k] = k == 0 ? 0.0 : row[k];
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k <= L; ++k) dp[k] = dp[k - 1] + dp[k];
    for (int i = 1; i < AR_THREADS; ++i) {
      sa += ra[i];
      sb += rb[i];
    }
    ra[0] = sa;
    rb[0] = sb;
  }
  __syncthreads();
  sa = ra[0];
  sb = rb[0];
  const int jtile = j / P.jt, jl = j - jtile * P.jt;
  const double* part = A.state + P.off_part + (((int64_t)g * P.njt + jtile) * P.ns * P.jt + jl) * (int64_t)(L + 1);
  const int64_t wstep = (int64_t)P.jt * (L + 1);
  const double cn = (double)C * nd;
  for (int k = tid; k <= L; k += AR_THREADS) {
    double p = 0.0;
    for (int64_t w = 0; w < P.ns; w += AR_LD) {
      double v[AR_LD];
#pragma unroll
      for (int u = 0; u < AR_LD; ++u) v[u] = part[(w + u < P.ns ? w + u : w) * wstep + k];
#pragma unroll
      for (int u = 0; u < AR_LD; ++u)
        if (w + u < P.ns) p += v[u];
    }
    row[k] = k < n && C > 0 ? (p - 2.0 * sa + dp[k] + (double)(n - k) * sb) / cn : p;
  }
}

}  // namespace

int launch_chain_acf_block(hipStream_t s, AcfArgs a) {
  const AcfPlan& p = a.plan;
  if (p.T == 0 || a.n_rows == 0) return 0;
  const int64_t wgs = (int64_t)a.n_group * p.njt * p.ns;
  if (a.max_lag <= 64)
    hipLaunchKernelGGL(k_chain_acf_block<8>, dim3((unsigned)wgs), dim3(AC_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(k_chain_acf_block<16>, dim3((unsigned)wgs), dim3(AC_THREADS), 0, s, a);
  hipLaunchKernelGGL(k_chain_acf_update, dim3((unsigned)((p.T + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_chain_acf_count, dim3(1), dim3(1), 0, s, a);
  return 0;
}

int launch_chain_acf_reduce(hipStream_t s, AcfArgs a, double* acov, int64_t* n) {
  if (a.n_group == 0) {
    hipLaunchKernelGGL(k_chain_acf_count_out, dim3(1), dim3(1), 0, s, a, n);
    return 0;
  }
  hipLaunchKernelGGL(k_chain_acf_edges, dim3((unsigned)a.n_group * (unsigned)a.max_lag), dim3(AR_THREADS), 0, s, a,
                     acov);
  const size_t lds = (size_t)(a.max_lag + 1 + 2 * AR_THREADS) * sizeof(double);
  hipLaunchKernelGGL(k_chain_acf_finish, dim3((unsigned)a.n_group * (unsigned)a.n_param), dim3(AR_THREADS), lds, s,
                     a, acov, n);
  return 0;
}
