// Pooled first and second moments of the recorded coefficients b on the device
// (gs_coef_moments_block, gs_coef_moments_reduce, include/pulsar_gibbs.h): for a block of rows of
// n_group x n_chain chains (the b record blocks of the single-pulsar samplers: a group is a
// pulsar with m[g] <= ldb coefficients) the sums S1[i] = sum d_i and S2[i][k] = sum d_i d_k over
// every post-burn (row, chain) sample, d = v - shift[g], as an fp64-MFMA rank-K update: 4 samples
// (consecutive chains of a row) x 16 columns per v_mfma_f64_16x16x4_f64 operand.
// Every result is reproducible: no floating-point atomics, and every sum runs in an order fixed
// by the shapes and the call sequence.
//
// The opaque state (doubles; all zeros = empty):
//   n     [n_group]         samples taken (post-burn rows x chains, int64 bits), padded to 8
//   shift [n_group][ldb]    chain 0's values in the group's first post-burn row
//   diag  [n_group][nsb][ns][15 x 256 + 80]   workgroup (set of 5 column blocks, chain strip)'s own
//         sums: the lower-triangle 16 x 16 tiles (I, J <= I) of its set, tile I (I + 1) / 2 + J, an
//         element as the MFMA leaves it (register s of lane l at s * 64 + l: row (l >> 4) + 4 s,
//         column l & 15), then S1 of the set's 80 columns
//   off   [n_group][noff][ns][25 x 256]       the same for a pair of different sets (SI > SJ): all
//         25 tiles, tile I * 5 + J
#include "gibbs_internal.h"

namespace {

constexpr int BM_SB = 5;                      // column blocks of a set: 15 accumulators of 8 VGPRs
constexpr int BM_THREADS = 256;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr int BM_TD = BM_SB * (BM_SB + 1) / 2;  // tiles of a set against itself
constexpr int BM_TO = BM_SB * BM_SB;            // tiles of a pair of different sets
constexpr int BM_S1 = BM_SB * 16;
constexpr int64_t BM_PD = BM_TD * 256 + BM_S1;  // doubles of a workgroup's partial
constexpr int64_t BM_PO = BM_TO * 256;
// workgroups the plan aims at: two per CU of an MI355X, so that the partials (read and written
// once per call) stay small beside the rows
constexpr int BM_WGS = 512;
constexpr int BM_LD = 8;                      // independent loads a reducing thread keeps in flight

typedef double bm_d4_t __attribute__((ext_vector_type(4)));

}  // namespace

BmomPlan bmom_plan(int n_group, int n_chain, int ldb) {
  BmomPlan p;
  p.nt = (ldb + 15) / 16;
  p.nsb = (p.nt + BM_SB - 1) / BM_SB;
  p.noff = p.nsb * (p.nsb - 1) / 2;
  const int64_t passes = ((int64_t)n_chain + 3) / 4;                     // steps of a row per group
  const int64_t tiles = (int64_t)n_group * (p.nsb + p.noff);
  int64_t per = tiles > 0 ? (passes * tiles + BM_WGS - 1) / BM_WGS : 1;  // steps of a row per workgroup
  per = per < 1 ? 1 : per;
  p.cs = per * 4;
  p.ns = ((int64_t)n_chain + p.cs - 1) / p.cs;
  p.off_shift = ((int64_t)n_group + 7) / 8 * 8;
  p.off_diag = p.off_shift + (int64_t)n_group * ldb;
  p.off_off = p.off_diag + (int64_t)n_group * p.nsb * p.ns * BM_PD;
  p.size = p.off_off + (int64_t)n_group * p.noff * p.ns * BM_PO;
  return p;
}

namespace {

// first row of the block at or above burn -- gs_chain_summary_block's rule (acf_first_row)
__device__ __forceinline__ int bmom_first_row(const BmomArgs& A) {
  const long long sw0 = gs_sweep(A.sweep, A.sweep_dev);
  long long first = (long long)A.burn - sw0;
  first = first < 0 ? 0 : first;
  return first < A.n_rows ? (int)first : A.n_rows;
}

__device__ __forceinline__ int bmom_m(const BmomArgs& A, int g) {
  const int m = A.m[g];
  return m < 1 ? 1 : (m > A.ldb ? A.ldb : m);
}

// grid (n_group), ahead of the product kernel: an empty group that gets a post-burn row takes
// chain 0's values of that row as its shift; then the group's sample count
__global__ __launch_bounds__(128) void k_coef_moments_shift(BmomArgs A) {
  const int r0 = bmom_first_row(A);
  const int nb = A.n_rows - r0;
  if (nb == 0) return;
  const int g = blockIdx.x, m = bmom_m(A, g);
  int64_t* np = (int64_t*)A.state + g;
  const int64_t n = *np;
  if (n == 0) {
    double* shift = A.state + A.plan.off_shift + (int64_t)g * A.ldb;
    const double* row = A.b + (int64_t)r0 * A.row_stride + (int64_t)g * A.n_chain * A.ldb;
    for (int i = threadIdx.x; i < A.ldb; i += blockDim.x) shift[i] = i < m ? row[i] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) *np = n + (int64_t)nb * A.n_chain;
}

// grid (groups x pairs of sets x chain strips), 4 waves.  A workgroup owns the chains
// [strip * cs, (strip + 1) * cs) of one group and the tiles of one pair of sets of 5 column blocks
// (DIAG: a set against itself, lower triangle).  A step is 4 consecutive chains of one row: lane l
// loads v[chain k0 + (l >> 4)][column 16 I + (l & 15)] for each column block I of its sets -- 16
// contiguous doubles of 4 chains -- and d = v - shift (0 past the strip and for columns >= m,
// chosen after the subtraction) is the A operand of the tiles of block row I and the B operand of
// those of block column I.  The waves take the steps w, w + 4, ... (rows ascending, then chains),
// the loads of the next steps in flight under the MFMAs; then the waves are added in ascending order in
// LDS and the result goes onto the workgroup's partial.
template <bool DIAG>
__global__ __launch_bounds__(BM_THREADS, DIAG ? 2 : 1) void k_coef_moments_block(BmomArgs A) {
  constexpr int NTL = DIAG ? BM_TD : BM_TO;
  __shared__ double sh[NTL * 256 + (DIAG ? BM_WAVES * BM_SB * 64 : 0)];
  const BmomPlan& P = A.plan;
  const int r0 = bmom_first_row(A);
  const int nb = A.n_rows - r0;
  if (nb == 0) return;  // whole block below burn (uniform: before any barrier)
  const int64_t wg = blockIdx.x;
  const int64_t tile = wg / P.ns, strip = wg - tile * P.ns;
  int g, si, sj;
  if (DIAG) {
    g = (int)(tile / P.nsb);
    si = sj = (int)(tile - (int64_t)g * P.nsb);
  } else {
    g = (int)(tile / P.noff);
    const int so = (int)(tile - (int64_t)g * P.noff);  // si (si - 1) / 2 + sj, sj < si
    si = 1;
    while ((si + 1) * si / 2 <= so) ++si;
    sj = so - si * (si - 1) / 2;
  }
  const int C = A.n_chain, ldb = A.ldb, m = bmom_m(A, g);
  const int tid = threadIdx.x, l = tid & 63, w = gs_wave_id(), kq = l >> 4, ci = l & 15;
  const int nI = min(BM_SB, P.nt - si * BM_SB), nJ = DIAG ? nI : min(BM_SB, P.nt - sj * BM_SB);
  const double* shift = A.state + P.off_shift + (int64_t)g * ldb;

  // a lane's column of each block: column 0 (always a coefficient) where it has none
  int colA[BM_SB], colB[BM_SB];
  double shA[BM_SB], shB[BM_SB];
  bool okA[BM_SB], okB[BM_SB];
#pragma unroll
  for (int u = 0; u < BM_SB; ++u) {
    const int ca = (si * BM_SB + u) * 16 + ci, cb = (sj * BM_SB + u) * 16 + ci;
    okA[u] = u < nI && ca < m;
    okB[u] = u < nJ && cb < m;
    colA[u] = okA[u] ? ca : 0;
    colB[u] = okB[u] ? cb : 0;
    shA[u] = okA[u] ? shift[ca] : 0.0;
    shB[u] = okB[u] ? shift[cb] : 0.0;
  }

  const int64_t c_lo = strip * P.cs;
  const int64_t c_hi = c_lo + P.cs < C ? c_lo + P.cs : (int64_t)C;
  const int nq = (int)((c_hi - c_lo + 3) / 4);  // steps of a row
  const int64_t nsteps = (int64_t)nb * nq;
  const double* base = A.b + (int64_t)r0 * A.row_stride + (int64_t)g * C * ldb;

  bm_d4_t acc[NTL];
  double s1[BM_SB];
#pragma unroll
  for (int t = 0; t < NTL; ++t) acc[t] = bm_d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int u = 0; u < BM_SB; ++u) s1[u] = 0.0;

  // every lane loads from a valid address (its strip's first chain past the strip's end) and the
  // value is chosen afterwards
  auto load = [&](int r, int q, double (&va)[BM_SB], double (&vb)[BM_SB], bool& ok) {
    const int64_t c = c_lo + (int64_t)q * 4 + kq;
    ok = c < c_hi;
    const double* p = base + (int64_t)r * A.row_stride + (ok ? c : c_lo) * ldb;
#pragma unroll
    for (int u = 0; u < BM_SB; ++u) {
      if (u < nI) va[u] = p[colA[u]];
      if (!DIAG && u < nJ) vb[u] = p[colB[u]];
    }
  };

  // a ring of PF steps in flight: a step's 15 products take about 1000 cycles, a load from HBM
  // several times that.  (lr, lq) is the load cursor, PF steps of this wave ahead of the products.
  constexpr int PF = DIAG ? 4 : 2;
  double va[PF][BM_SB], vb[PF][BM_SB];
  bool ok[PF];
  int64_t ls = w;
  int lr = (int)(ls / nq), lq = (int)(ls - (int64_t)lr * nq);
  auto fill = [&](int p) {
    if (ls < nsteps) load(lr, lq, va[p], vb[p], ok[p]);
    ls += BM_WAVES;
    lq += BM_WAVES;
    while (lq >= nq) {
      lq -= nq;
      ++lr;
    }
  };
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    ok[p] = false;
#pragma unroll
    for (int u = 0; u < BM_SB; ++u) va[p][u] = vb[p][u] = 0.0;
    fill(p);
  }
  for (int64_t step = w; step < nsteps; step += BM_WAVES * PF) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      if (step + BM_WAVES * p >= nsteps) break;
      double da[BM_SB], db[BM_SB];
#pragma unroll
      for (int u = 0; u < BM_SB; ++u) {
        da[u] = ok[p] && okA[u] ? va[p][u] - shA[u] : 0.0;
        db[u] = ok[p] && okB[u] ? vb[p][u] - shB[u] : 0.0;
        if (DIAG) s1[u] += da[u];
      }
      fill(p);
#pragma unroll
      for (int i = 0; i < BM_SB; ++i) {
#pragma unroll
        for (int j = 0; j < BM_SB; ++j) {
          if (i >= nI) continue;
          if (DIAG) {
            if (j <= i) {
              const int t = i * (i + 1) / 2 + j;
              acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[i], da[j], acc[t], 0, 0, 0);
            }
          } else if (j < nJ) {
            acc[i * BM_SB + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[i], db[j], acc[i * BM_SB + j], 0, 0, 0);
          }
        }
      }
    }
  }

  // the waves in ascending order, then onto the workgroup's partial
  for (int w2 = 0; w2 < BM_WAVES; ++w2) {
    if (w == w2) {
#pragma unroll
      for (int t = 0; t < NTL; ++t) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          double* e = sh + t * 256 + s * 64 + l;
          *e = w2 == 0 ? acc[t][s] : *e + acc[t][s];
        }
      }
      if (DIAG) {
#pragma unroll
        for (int u = 0; u < BM_SB; ++u) sh[NTL * 256 + (w * BM_SB + u) * 64 + l] = s1[u];
      }
    }
    __syncthreads();
  }
  double* part = DIAG ? A.state + P.off_diag + wg * BM_PD : A.state + P.off_off + wg * BM_PO;
  for (int t = 0; t < NTL; ++t) {
    const bool used = DIAG ? t < nI * (nI + 1) / 2 : (t / BM_SB < nI && t % BM_SB < nJ);
    if (used) part[t * 256 + tid] += sh[t * 256 + tid];
  }
  if (DIAG && tid < nI * 16) {
    // column tid of the set: the waves, and in a wave the 4 samples of a step, in ascending order
    const int u = tid >> 4, c = tid & 15;
    double sum = 0.0;
    for (int w2 = 0; w2 < BM_WAVES; ++w2)
      for (int k = 0; k < 4; ++k) sum += sh[NTL * 256 + (w2 * BM_SB + u) * 64 + k * 16 + c];
    part[BM_TD * 256 + tid] += sum;
  }
}

// the partials of ns workgroups, `stride` apart, in ascending order
__device__ __forceinline__ double bmom_sum(const double* p, int64_t stride, int64_t ns) {
  double a = 0.0;
  for (int64_t w = 0; w < ns; w += BM_LD) {
    double v[BM_LD];
#pragma unroll
    for (int u = 0; u < BM_LD; ++u) v[u] = p[(w + u < ns ? w + u : w) * stride];
#pragma unroll
    for (int u = 0; u < BM_LD; ++u)
      if (w + u < ns) a += v[u];
  }
  return a;
}

// grid (n_group * ldb): block (g, i) writes row i of cov left of and on the diagonal and its
// mirror image, column i above the diagonal, from the lower-triangle element (i, k <= i) of the
// partials; block (g, 0) also n, shift and mean.  Every block sums S1 of all columns (it needs
// S1[k] beside S1[i], and a non-finite S1 anywhere makes the whole group NaN).  The state is read only.
__global__ __launch_bounds__(256) void k_coef_moments_reduce(BmomArgs A, int64_t* n_out, double* shift_out,
                                                             double* mean, double* cov) {
  __shared__ double s1s[512];
  const BmomPlan& P = A.plan;
  const int ldb = A.ldb, tid = threadIdx.x;
  const int g = blockIdx.x / ldb, i = blockIdx.x - g * ldb;
  const int m = bmom_m(A, g);
  const int64_t n = ((const int64_t*)A.state)[g];
  const double nd = (double)n;
  const double* shift = A.state + P.off_shift + (int64_t)g * ldb;
  const double* diag = A.state + P.off_diag + (int64_t)g * P.nsb * P.ns * BM_PD;
  const double* off = A.state + P.off_off + (int64_t)g * P.noff * P.ns * BM_PO;
  int bad = 0;
  for (int k = tid; k < ldb; k += 256) {
    double s = 0.0;
    if (k < m) {
      const int K = k >> 4, sk = K / BM_SB, u = K - sk * BM_SB;
      s = bmom_sum(diag + (int64_t)sk * P.ns * BM_PD + BM_TD * 256 + u * 16 + (k & 15), BM_PD, P.ns);
      bad |= !isfinite(s);
    }
    s1s[k] = s;
  }
  bad = __syncthreads_or(bad);
  const bool nan_out = n == 0 || bad;
  const double nan = __builtin_nan("");
  if (i == 0) {
    if (tid == 0) n_out[g] = n;
    for (int k = tid; k < ldb; k += 256) {
      shift_out[(int64_t)g * ldb + k] = k < m ? shift[k] : 0.0;
      mean[(int64_t)g * ldb + k] = k < m ? (nan_out ? nan : shift[k] + s1s[k] / nd) : 0.0;
    }
  }
  double* cg = cov + (int64_t)g * ldb * ldb;
  const int I = i >> 4, si = I / BM_SB, ui = I - si * BM_SB, ri = i & 15;
  const int erow = (ri >> 2) * 64 + (ri & 3) * 16;  // row ri of a tile: register ri / 4, lanes (ri % 4) * 16 ..
  for (int k = tid; k <= i; k += 256) {
    double v = 0.0;
    if (i < m) {  // k <= i < m
      if (nan_out) {
        v = nan;
      } else {
        const int J = k >> 4, sj = J / BM_SB, uj = J - sj * BM_SB;
        const double* p = si == sj
            ? diag + (int64_t)si * P.ns * BM_PD + (ui * (ui + 1) / 2 + uj) * 256
            : off + (int64_t)(si * (si - 1) / 2 + sj) * P.ns * BM_PO + (ui * BM_SB + uj) * 256;
        const double s2 = bmom_sum(p + erow + (k & 15), si == sj ? BM_PD : BM_PO, P.ns);
        v = s2 / nd - (s1s[i] / nd) * (s1s[k] / nd);
      }
    }
    cg[(int64_t)i * ldb + k] = v;
    cg[(int64_t)k * ldb + i] = v;
  }
}

}  // namespace

int launch_coef_moments_block(hipStream_t s, BmomArgs a) {
  const BmomPlan& p = a.plan;
  if (a.n_group == 0 || a.n_chain == 0 || a.n_rows == 0) return 0;
  hipLaunchKernelGGL(k_coef_moments_shift, dim3((unsigned)a.n_group), dim3(128), 0, s, a);
  hipLaunchKernelGGL(k_coef_moments_block<true>, dim3((unsigned)((int64_t)a.n_group * p.nsb * p.ns)),
                     dim3(BM_THREADS), 0, s, a);
  if (p.noff > 0)
    hipLaunchKernelGGL(k_coef_moments_block<false>, dim3((unsigned)((int64_t)a.n_group * p.noff * p.ns)),
                       dim3(BM_THREADS), 0, s, a);
  return 0;
}

int launch_coef_moments_reduce(hipStream_t s, BmomArgs a, int64_t* n, double* shift, double* mean, double* cov) {
  if (a.n_group == 0) return 0;
  hipLaunchKernelGGL(k_coef_moments_reduce, dim3((unsigned)a.n_group * (unsigned)a.ldb), dim3(256), 0, s, a, n,
                     shift, mean, cov);
  return 0;
}
