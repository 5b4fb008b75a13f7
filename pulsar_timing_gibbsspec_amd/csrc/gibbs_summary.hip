// Posterior summaries accumulated on the device (gs_chain_summary, include/pulsar_gibbs.h):
// per (chain, parameter) centred moments and per parameter a histogram over all chains, from a
// block of recorded states.  Every result is reproducible: the moments of one (c, j) are summed
// by one thread in row order, the histogram is integer counts (LDS and global integer atomics).
// gs_chain_summary_block is the same for a block of rows of n_group x n_chain chains with one
// histogram per group (the record blocks of the single-pulsar samplers: a group is a pulsar), its
// lanes along the flat (chain, parameter) index.
#include "gibbs_internal.h"

namespace {

constexpr int SM_TILE = 64;   // parameters per workgroup: one lane each
constexpr int SM_WAVES = 4;   // waves per workgroup; wave w takes the strip's chains w, w + 4, ...
constexpr int SM_U = 4;       // chains a thread keeps in flight (independent loads per row)
// workgroups the launcher aims at when it cuts the chains into strips (A/B: make variant-one
// FILE=gibbs_summary EXTRA=-DGS_SUMMARY_WGS=...).  One per CU measured best on MI355X: us per
// launch at 64 bins for 64 / 128 / 192 / 256 / 512 / 1024 / 2048 workgroups, 2048 chains x 1380
// parameters 55.6 / 33.0 / 27.7 / 27.8 / 28.8 / 31.6 / 38.6, x 120 parameters 10.7 / 10.0 / 10.6 /
// 11.4 / 14.5 / 16.8 / 16.9 (profiles/sample_stream/SUMMARY.md)
#ifndef GS_SUMMARY_WGS
#define GS_SUMMARY_WGS 256
#endif

// LDS word of (parameter lane jl, bin k).  Rows of 64 lanes, each row rotated by its bin: the
// counting phase has lanes along jl (one bank per lane when the bins agree), the flush has lanes
// along k (bank (jl + k) % 64: again one per lane).
__device__ __forceinline__ int sm_word(int k, int jl) { return k * SM_TILE + ((jl + k) & (SM_TILE - 1)); }

// grid (ceil(n_param / 64), strips of `strip` chains), 256 threads.  Thread (w, lane) owns
// (c, j0 + lane) for its chains c: it loads s1 / s2, adds the rows in ascending r and stores them
// (512-byte wave accesses of x, s1, s2), and counts every value into the workgroup's LDS table
// [n_bins][64] of 32-bit words; the table's non-zero words then go to counts with 64-bit integer
// atomics (lanes along k: contiguous runs of one parameter's bins).
__global__ __launch_bounds__(64 * SM_WAVES) void k_chain_summary(SummaryArgs A) {
  extern __shared__ unsigned int sm_tab[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nb = A.n_bins;
  const int j0 = blockIdx.x * SM_TILE;
  const int j = j0 + lane;
  const bool jok = j < A.n_param;
  // rows below burn are a prefix of the block (the sweep index rises with r)
  const long long sw0 = gs_sweep(A.sweep, A.sweep_dev);
  long long first = (long long)A.burn - sw0;
  first = first < 0 ? 0 : first;
  const int r0 = first < A.n_rows ? (int)first : A.n_rows;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) A.n_acc[0] += A.n_rows - r0;
  if (r0 == A.n_rows) return;  // whole block below burn (uniform: before any barrier)

  for (int i = tid; i < nb * SM_TILE; i += 64 * SM_WAVES) sm_tab[i] = 0u;
  __syncthreads();

  const double lo = jok ? A.lo[j] : 0.0, hi = jok ? A.hi[j] : 0.0;
  const double scale = jok ? A.scale[j] : 0.0, mid = jok ? A.mid[j] : 0.0;
  const int64_t c_lo = (int64_t)blockIdx.y * A.strip;
  const int64_t c_hi = c_lo + A.strip < A.n_chain ? c_lo + A.strip : (int64_t)A.n_chain;
  unsigned int n_out = 0;
  if (jok) {
    for (int64_t cb = c_lo + w; cb < c_hi; cb += SM_WAVES * SM_U) {
      double a1[SM_U], a2[SM_U];
      int64_t e[SM_U];
      bool ok[SM_U];
#pragma unroll
      for (int u = 0; u < SM_U; ++u) {
        const int64_t c = cb + (int64_t)u * SM_WAVES;
        ok[u] = c < c_hi;
        e[u] = c * A.n_param + j;
        a1[u] = ok[u] ? A.s1[e[u]] : 0.0;
        a2[u] = ok[u] ? A.s2[e[u]] : 0.0;
      }
      for (int r = r0; r < A.n_rows; ++r) {
        const double* xr = A.x + (int64_t)r * A.row_stride;
        double v[SM_U];
#pragma unroll
        for (int u = 0; u < SM_U; ++u) v[u] = ok[u] ? xr[e[u]] : 0.0;
#pragma unroll
        for (int u = 0; u < SM_U; ++u) {
          if (!ok[u]) continue;
          const double d = v[u] - mid;
          a1[u] = a1[u] + d;
          a2[u] = a2[u] + d * d;  // may contract to an fma
          if (v[u] >= lo && v[u] <= hi) {  // false for NaN
            // exactly subtract, multiply, floor: the bin numpy's floor((v - lo) * scale) gives
            int k = (int)floor((v[u] - lo) * scale);
            k = k < nb - 1 ? k : nb - 1;
            k = k > 0 ? k : 0;  // a non-finite scale (hi == lo) must not leave the table
            atomicAdd(&sm_tab[sm_word(k, lane)], 1u);
          } else {
            ++n_out;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < SM_U; ++u) {
        if (ok[u]) {
          A.s1[e[u]] = a1[u];
          A.s2[e[u]] = a2[u];
        }
      }
    }
    if (n_out) atomicAdd((unsigned long long*)&A.outside[j], (unsigned long long)n_out);
  }
  __syncthreads();
  for (int i = tid; i < nb * SM_TILE; i += 64 * SM_WAVES) {
    const int jl = i / nb, k = i - jl * nb;
    const unsigned int n = sm_tab[sm_word(k, jl)];
    if (n && j0 + jl < A.n_param)
      atomicAdd((unsigned long long*)&A.counts[(int64_t)(j0 + jl) * nb + k], (unsigned long long)n);
  }
}

// ---- gs_chain_summary_block: a block of rows of n_group x n_chain chains, one histogram per group
constexpr int SB_ROWS = 8;  // rows a thread keeps in flight (independent loads)
// threads per workgroup = (c, j) entries per workgroup (A/B: make variant-one FILE=gibbs_summary
// EXTRA=-DGS_SUMMARY_BLOCK_THREADS=...).  Fewer, wider workgroups flush fewer tables; narrower ones
// spread a group over more CUs.
#ifndef GS_SUMMARY_BLOCK_THREADS
#define GS_SUMMARY_BLOCK_THREADS 512
#endif
constexpr int SB_MAX_BLOCKS = 1 << 22;  // workgroups per launch (blocks x threads stays below 2^32)

// LDS table of one group: row j = parameter j's n_bins bins, then its `outside` word, in rows of
// sb_ld = (n_bins + 1) | 1 words (n_bins + 1, or n_bins + 2 with one unused word when n_bins is
// odd).  The odd row length puts word k of neighbouring parameters on neighbouring banks: a
// wave's lanes run along j (two or three lanes per parameter at n_param = 30), and with an even
// length such as 64 every parameter's bin k would sit on bank k % 32.
__host__ __device__ __forceinline__ int sb_ld(int nb) { return (nb + 1) | 1; }

// grid (groups of this launch x strips), up to GS_SUMMARY_BLOCK_THREADS threads.  Lanes run along
// the flat entry index e = c * n_param + j of one group: thread e loads s1 / s2, adds the rows in ascending r (SB_ROWS
// loads in flight, every wave access contiguous) and stores them, and counts every value with one
// LDS atomic into the group's table; the table's non-zero words then go to counts / outside with
// 64-bit integer atomics, once per launch.
__global__ __launch_bounds__(GS_SUMMARY_BLOCK_THREADS) void k_chain_summary_block(SummaryBlockArgs B) {
  extern __shared__ unsigned int sb_tab[];
  const SummaryArgs& A = B.s;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nb = A.n_bins, ld = sb_ld(nb), np = A.n_param;
  const int g = B.g0 + (int)(blockIdx.x / (unsigned)B.strips);
  const int64_t strip_id = blockIdx.x % (unsigned)B.strips;
  // rows below burn are a prefix of the block (the sweep index rises with r)
  const long long sw0 = gs_sweep(A.sweep, A.sweep_dev);
  long long first = (long long)A.burn - sw0;
  first = first < 0 ? 0 : first;
  const int r0 = first < A.n_rows ? (int)first : A.n_rows;
  if (blockIdx.x == 0 && B.g0 == 0 && tid == 0) A.n_acc[0] += A.n_rows - r0;
  if (r0 == A.n_rows) return;  // whole block below burn (uniform: before any barrier)

  for (int i = tid; i < np * ld; i += nt) sb_tab[i] = 0u;
  __syncthreads();

  const int64_t E = (int64_t)A.n_chain * np;  // entries of a group
  const int64_t e_lo = strip_id * B.strip;
  const int64_t e_hi = e_lo + B.strip < E ? e_lo + B.strip : E;
  const double* xg = A.x + (int64_t)g * E;
  double* s1g = A.s1 + (int64_t)g * E;
  double* s2g = A.s2 + (int64_t)g * E;
  for (int64_t e = e_lo + tid; e < e_hi; e += nt) {
    const int j = (int)(e % np);
    const double lo = A.lo[j], hi = A.hi[j], scale = A.scale[j], mid = A.mid[j];
    unsigned int* row = sb_tab + j * ld;
    const double* xe = xg + e;
    double a1 = s1g[e], a2 = s2g[e];
    auto take = [&](double v) {
      const double d = v - mid;
      a1 = a1 + d;
      a2 = a2 + d * d;  // may contract to an fma
      // exactly subtract, multiply, floor: the bin numpy's floor((v - lo) * scale) gives
      int k = (int)floor((v - lo) * scale);
      k = k < nb - 1 ? k : nb - 1;
      k = k > 0 ? k : 0;  // a non-finite scale (hi == lo) must not leave the table
      k = (v >= lo && v <= hi) ? k : nb;  // false for NaN: the row's `outside` word
      atomicAdd(&row[k], 1u);
    };
    int r = r0;
    for (; r + SB_ROWS <= A.n_rows; r += SB_ROWS) {
      double v[SB_ROWS];
#pragma unroll
      for (int u = 0; u < SB_ROWS; ++u) v[u] = xe[(int64_t)(r + u) * A.row_stride];
#pragma unroll
      for (int u = 0; u < SB_ROWS; ++u) take(v[u]);
    }
    for (; r < A.n_rows; ++r) take(xe[(int64_t)r * A.row_stride]);
    s1g[e] = a1;
    s2g[e] = a2;
  }
  __syncthreads();
  int64_t* cg = A.counts + (int64_t)g * np * nb;
  int64_t* og = A.outside + (int64_t)g * np;
  for (int i = tid; i < np * (nb + 1); i += nt) {
    const int j = i / (nb + 1), k = i - j * (nb + 1);
    const unsigned int n = sb_tab[j * ld + k];
    if (n) atomicAdd((unsigned long long*)(k < nb ? &cg[(int64_t)j * nb + k] : &og[j]), (unsigned long long)n);
  }
}

// the fallback's launches of k_chain_summary each add the rows they took to n_acc: take back all
// but one group's
__global__ void k_summary_nacc_once(SummaryArgs A, int n_group) {
  const long long sw0 = gs_sweep(A.sweep, A.sweep_dev);
  long long first = (long long)A.burn - sw0;
  first = first < 0 ? 0 : first;
  const int r0 = first < A.n_rows ? (int)first : A.n_rows;
  A.n_acc[0] -= (int64_t)(n_group - 1) * (A.n_rows - r0);
}

}  // namespace

int launch_chain_summary_block(hipStream_t s, SummaryBlockArgs b) {
  SummaryArgs& a = b.s;
  if (b.n_group == 0 || a.n_chain == 0 || a.n_rows == 0) return 0;
  const int64_t E = (int64_t)a.n_chain * a.n_param;
  const size_t lds = (size_t)a.n_param * sb_ld(a.n_bins) * sizeof(unsigned int);
  if (lds > 65536) {
    // the group's table does not fit 64 KB of LDS: the tiled kernel, one launch per group
    for (int g = 0; g < b.n_group; ++g) {
      SummaryArgs ag = a;
      ag.x = a.x + g * E;
      ag.s1 = a.s1 + g * E;
      ag.s2 = a.s2 + g * E;
      ag.counts = a.counts + (int64_t)g * a.n_param * a.n_bins;
      ag.outside = a.outside + (int64_t)g * a.n_param;
      launch_chain_summary(s, ag);
    }
    if (b.n_group > 1) hipLaunchKernelGGL(k_summary_nacc_once, dim3(1), dim3(1), 0, s, a, b.n_group);
    return 0;
  }
  int64_t threads = (E + 63) / 64 * 64;
  threads = threads < GS_SUMMARY_BLOCK_THREADS ? threads : GS_SUMMARY_BLOCK_THREADS;
  // one entry per thread, unless that would take more strips than a launch has workgroups
  int64_t batches = ((E + threads - 1) / threads + SB_MAX_BLOCKS - 1) / SB_MAX_BLOCKS;
  b.strip = threads * batches;
  b.strips = (int)((E + b.strip - 1) / b.strip);
  const int per_launch = SB_MAX_BLOCKS / b.strips;  // groups per launch, >= 1
  for (b.g0 = 0; b.g0 < b.n_group; b.g0 += per_launch) {
    const int ng = b.n_group - b.g0 < per_launch ? b.n_group - b.g0 : per_launch;
    hipLaunchKernelGGL(k_chain_summary_block, dim3((unsigned)ng * (unsigned)b.strips), dim3((unsigned)threads), lds,
                       s, b);
  }
  return 0;
}

int launch_chain_summary(hipStream_t s, SummaryArgs a) {
  if (a.n_chain == 0 || a.n_rows == 0) return 0;
  const int tiles = (a.n_param + SM_TILE - 1) / SM_TILE;
  // chains per workgroup: about GS_SUMMARY_WGS workgroups, at least one chain per wave; fewer
  // strips mean fewer zeroings and flushes of the table and fewer atomics
  int64_t strip = ((int64_t)a.n_chain * tiles + GS_SUMMARY_WGS - 1) / GS_SUMMARY_WGS;
  strip = strip < SM_WAVES ? SM_WAVES : strip;
  const int64_t fit = ((int64_t)a.n_chain + 65534) / 65535;  // gridDim.y <= 65535
  strip = strip < fit ? fit : strip;
  strip = (strip + SM_WAVES - 1) / SM_WAVES * SM_WAVES;
  a.strip = (int)strip;
  const unsigned strips = (unsigned)((a.n_chain + strip - 1) / strip);
  const size_t lds = (size_t)a.n_bins * SM_TILE * sizeof(unsigned int);  // <= 64 KB at n_bins = 256
  hipLaunchKernelGGL(k_chain_summary, dim3((unsigned)tiles, strips), dim3(64 * SM_WAVES), lds, s, a);
  return 0;
}
