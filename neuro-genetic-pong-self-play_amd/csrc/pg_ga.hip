// pg_ga.hip -- the genetic algorithm's device steps and their C entry points
// (include/pong_ga.h; DESIGN.md "GA").
//
//   u01, rng_key, rng_u01     the counter-based draws (tests/_ga_draws.py restates them)
//   k_select, k_select_ranked DEAP selTournament (pg_ga_select_tournament*)
//   k_vary<WT>                varAnd(cxBlend, mutGaussian), one wave per pair (pg_ga_vary)
//   k_mark_pairs, k_list_pairs  the pairs a pg_ga_vary call writes
//   k_schedule                evaluate()'s opponent schedule (pg_ga_schedule)
//   k_gather_rows<WT>, k_row_hash<WT>   pg_gather_rows, pg_row_hash
// Compiled with pong_ga.hip's scheduler flag (pong_amd/build.py SOURCE_FLAGS),
// under which these kernels were tuned and measured.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_device.hpp"
#include "pg_fail.hpp"

namespace pg {

// ================================================================ GA =====
// Counter-based uniform double in [0,1): splitmix64 of (seed, generation,
// stream, a, b).  DEAP draws from Python's Mersenne Twister; the device GA
// matches its distributions, not its stream (DESIGN.md "GA").
__device__ __forceinline__ double u01(uint64_t seed, uint64_t gen, uint64_t stream, uint64_t a,
                                      uint64_t b) {
  uint64_t k = splitmix64(seed + 0x9E3779B97F4A7C15ull * (gen + 1));
  k = splitmix64(k ^ (stream * 0xD6E8FEB86659FD93ull + a));
  k = splitmix64(k ^ b);
  return (double)(k >> 11) * 0x1.0p-53;
}

// tools.selTournament: for each pick, tournsize aspirants drawn with
// replacement (selRandom = random.choice), the first maximum wins (max()).
__global__ void k_select(pg_select_args a) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.k) return;
  int best = -1;
  double bf = 0.0;
  for (int t = 0; t < a.tournsize; ++t) {
    const int idx = (int)(u01(a.seed, a.generation, 1, (uint64_t)j, (uint64_t)t) * (double)a.n_pop);
    const double f = a.fitness[idx];
    if (best < 0 || f > bf) {
      best = idx;
      bf = f;
    }
  }
  a.chosen[j] = best;
}

// selTournament by rank sampling (see pong_ga.h): P(winner rank <= r) = ((r+1)/n)^t.
__global__ void k_select_ranked(pg_select_args a, const double *sorted, const int32_t *order) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.k) return;
  const int n = a.n_pop;
  const double v = u01(a.seed, a.generation, 8, (uint64_t)j, 0);
  int r = (int)((double)n * exp(log(v) / (double)a.tournsize));
  r = r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
  const double f = sorted[r];
  int lo = 0, hi = n;  // tie group [first, last) of value f
  int a0 = 0, b0 = r;
  while (a0 < b0) { const int m = (a0 + b0) >> 1; if (sorted[m] < f) a0 = m + 1; else b0 = m; }
  lo = a0;
  a0 = r; b0 = n;
  while (a0 < b0) { const int m = (a0 + b0) >> 1; if (sorted[m] <= f) a0 = m + 1; else b0 = m; }
  hi = a0;
  const int pick = lo + (int)(u01(a.seed, a.generation, 9, (uint64_t)j, 0) * (double)(hi - lo));
  a.chosen[j] = order[pick < hi ? pick : hi - 1];
}

// algorithms.varAnd: clone the chosen parents, cxBlend consecutive pairs
// (i-1, i) w.p. cxpb, then mutGaussian each individual w.p. mutpb.
//   cxBlend:     gamma = (1 + 2 alpha) U - alpha; x1' = (1-gamma) x1 + gamma x2; x2' = gamma x1 + (1-gamma) x2
//   mutGaussian: w.p. indpb per gene, x += N(mu, sigma)
// Counter-based randoms: a key per (generation, stream, pair or individual),
// then one splitmix64 per gene.  The two individuals of a pair share one
// Box-Muller draw (r cos t, r sin t), in f32 (the noise is added in f64).
__device__ __forceinline__ uint64_t rng_key(uint64_t seed, uint64_t gen, uint64_t stream, uint64_t a) {
  const uint64_t k = splitmix64(seed + 0x9E3779B97F4A7C15ull * (gen + 1));
  return splitmix64(k ^ (stream * 0xD6E8FEB86659FD93ull + a));
}
__device__ __forceinline__ double rng_u01(uint64_t key, uint64_t b) {
  return (double)(splitmix64(key ^ b) >> 11) * 0x1.0p-53;
}

// One wave per pair: the pair's draws (crossover, mutation, the keys of its
// per-gene streams) are wave-uniform scalar work done once, then the wave
// sweeps the genes 128 at a time (two coalesced 512-B pieces per parent row,
// all four loads issued before the arithmetic).
template <typename WT>
__device__ __forceinline__ void vary_pair(const pg_ga_args &a, int pair);

template <typename WT>
__global__ __launch_bounds__(256) void k_vary(pg_ga_args a) {
  const int wave = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (a.pair_list) {  // a compact list of the pairs to write (pong_ga.h): the grid strides over it
    const int count = __builtin_amdgcn_readfirstlane(*a.pair_count);
    const int waves = (int)gridDim.x * 4;
#pragma unroll 1
    for (int w = wave; w < count; w += waves) vary_pair<WT>(a, __builtin_amdgcn_readfirstlane(a.pair_list[w]));
    return;
  }
  vary_pair<WT>(a, wave);
}

template <typename WT>
__device__ __forceinline__ void vary_pair(const pg_ga_args &a, int pair) {
  const int pairs = (a.n + 1) / 2;
  if (pair >= pairs) return;
  const int lane = threadIdx.x & 63;
  const int i0 = 2 * pair, i1 = 2 * pair + 1;
  const bool has1 = i1 < a.n;
  const bool cx = has1 && rng_u01(rng_key(a.seed, a.generation, 2, (uint64_t)pair), 0) < a.cxpb;
  const bool mut0 = rng_u01(rng_key(a.seed, a.generation, 4, (uint64_t)i0), 0) < a.mutpb;
  const bool mut1 = has1 && rng_u01(rng_key(a.seed, a.generation, 4, (uint64_t)i1), 0) < a.mutpb;
  if (lane == 0) {
    a.invalid[i0] = (uint8_t)(cx || mut0);
    if (has1) a.invalid[i1] = (uint8_t)(cx || mut1);
  }
  if (!a.pair_list && a.pair_mask && !a.pair_mask[pair]) return;  // a pair this call does not write (pong_ga.h)
  const uint64_t k3 = rng_key(a.seed, a.generation, 3, (uint64_t)pair);
  const uint64_t k5 = rng_key(a.seed, a.generation, 5, (uint64_t)pair);
  const uint64_t k6 = rng_key(a.seed, a.generation, 6, (uint64_t)pair);
  const WT *p1 = (const WT *)a.parents + (long)a.chosen[i0] * a.stride;
  const WT *p2 = (const WT *)a.parents + (long)(has1 ? a.chosen[i1] : a.chosen[i0]) * a.stride;
  WT *o1 = (WT *)a.offspring + (long)i0 * a.stride;
  WT *o2 = (WT *)a.offspring + (long)i1 * a.stride;
  const auto one = [&](long gene, double x1, double x2) {
    if (cx) {
      const double u = rng_u01(k3, (uint64_t)gene);
      const double gamma = __dadd_rn(__dmul_rn(1.0 + 2.0 * a.alpha, u), -a.alpha);
      const double y1 = __dadd_rn(__dmul_rn(1.0 - gamma, x1), __dmul_rn(gamma, x2));
      const double y2 = __dadd_rn(__dmul_rn(gamma, x1), __dmul_rn(1.0 - gamma, x2));
      x1 = y1;
      x2 = y2;
    }
    // one 64-bit draw decides both individuals' indpb hits (32 bits each),
    // one more feeds the shared Box-Muller pair (24 bits per uniform)
    const uint64_t hb = splitmix64(k5 ^ (uint64_t)gene);
    const bool h0 = mut0 && (double)(uint32_t)hb * 0x1.0p-32 < a.indpb;
    const bool h1 = mut1 && (double)(uint32_t)(hb >> 32) * 0x1.0p-32 < a.indpb;
    if (h0 || h1) {
      const uint64_t nb = splitmix64(k6 ^ (uint64_t)gene);
      const float u1 = 1.0f - (float)(nb >> 40) * 0x1.0p-24f;  // (0, 1]
      const float u2 = (float)((nb >> 8) & 0xFFFFFFu) * 0x1.0p-24f;
      const float r = sqrtf(-2.0f * logf(u1));
      float sn, cs;
      sincosf(6.2831853f * u2, &sn, &cs);
      if (h0) x1 = __dadd_rn(x1, __dadd_rn(a.mu, __dmul_rn(a.sigma, (double)(r * cs))));
      if (h1) x2 = __dadd_rn(x2, __dadd_rn(a.mu, __dmul_rn(a.sigma, (double)(r * sn))));
    }
    o1[gene] = (WT)x1;
    if (has1) o2[gene] = (WT)x2;
  };
  // kVaryChunk 128-gene pieces of both parents requested before any arithmetic
  // (a [6,64,3] genome, 454 genes, is one chunk): more loads in flight per wave
  constexpr int kVaryChunk = 4;
  for (long g0 = 0; g0 < a.genes; g0 += 128 * kVaryChunk) {
    double x[kVaryChunk][2][2];
#pragma unroll
    for (int c = 0; c < kVaryChunk; ++c) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const long g = g0 + c * 128 + h * 64 + lane;
        const bool v = g < a.genes;
        x[c][h][0] = v ? (double)p1[g] : 0.0;
        x[c][h][1] = v && has1 ? (double)p2[g] : 0.0;
      }
    }
#pragma unroll
    for (int c = 0; c < kVaryChunk; ++c) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const long g = g0 + c * 128 + h * 64 + lane;
        if (g < a.genes) one(g, x[c][h][0], x[c][h][1]);
      }
    }
  }
}

__global__ void k_mark_pairs(uint8_t *mask, int n_pairs, const int32_t *rows, int n_rows, int skip_lo, int skip_hi,
                             const uint8_t *exclude) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const int r = rows[i];
  if (r < 0 || r >= 2 * n_pairs) return;
  const int j = r >> 1;
  if ((j < skip_lo || j >= skip_hi) && !(exclude && exclude[j])) mask[j] = 1;
}

// pg_ga_list_pairs: the marked pairs appended to a list (order irrelevant).
__global__ void k_list_pairs(const uint8_t *mask, int n_pairs, int32_t *list, int32_t *count) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n_pairs && mask[j]) list[atomicAdd(count, 1)] = j;
}

// Opponent schedule of evaluate() (main.py:28-66) for rows [0, n).
__global__ void k_schedule(pg_schedule_args a) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (long)a.n * a.n_games) return;
  const long i = w / a.n_games;
  const int g = (int)(w % a.n_games);
  const long row = a.rows ? (long)a.rows[i] : a.row_offset + i;
  int kind = kOppHard, opp = 0;
  double mult = 1.0;
  if (a.mode == PG_SCHED_SELFPLAY) {
    if (a.n_hof > 0) {
      kind = kOppNN;
      const int K = a.hof_slices > 1 && a.n_hof >= a.hof_slices ? a.hof_slices : 1;
      if (K == 1) {
        opp = (int)((row * a.n_games + g) % a.n_hof);
      } else {  // the block's interleaved slice of the hall (pong_ga.h)
        const int b = (int)((row / a.block_rows) % K);
        const long m = (a.n_hof - b + K - 1) / K;
        const int k = (int)((row * a.n_games + g) % m);
        opp = a.slice_local ? k : k * K + b;
      }
    }
  } else if (g < 3) {
    kind = g == 0 ? kOppHard : (g == 1 ? kOppRomCpu : kOppScore);
    // right_score_multiplier is 1 until the first pick (main.py:32)
  } else if (a.n_hof > 0) {
    kind = kOppNN;
    opp = (int)(u01(a.seed, a.generation, 10, (uint64_t)row, (uint64_t)g) * (double)a.n_hof);
    opp = opp < a.n_hof ? opp : a.n_hof - 1;
    mult = a.hof_fitness[opp];
  }
  a.kind[w] = kind;
  a.opp[w] = opp;
  a.mult[w] = mult;
}

// pg_gather_rows: one workgroup per destination row.
template <typename WT>
__global__ __launch_bounds__(256) void k_gather_rows(WT *dst, int64_t dst_stride, const WT *old_rows, int64_t old_stride,
                                                     const WT *rows, int64_t rows_stride, const int64_t *index,
                                                     const int32_t *src, int n_old, int64_t genes) {
  const int j = blockIdx.x;
  const int s = src[j];
  const WT *from = s < n_old ? old_rows + (long)s * old_stride
                             : rows + (index ? index[s - n_old] : (long)(s - n_old)) * rows_stride;
  WT *to = dst + (long)j * dst_stride;
  for (int64_t g = threadIdx.x; g < genes; g += 256) to[g] = from[g];
}

// 64-bit content hash of each row: an order-independent sum of mixed
// (index, bit pattern) terms, so the block reduction order cannot matter.
template <typename WT>
__global__ __launch_bounds__(256) void k_row_hash(const WT *rows, int64_t stride, const int32_t *index, int n,
                                                  int64_t genes, uint64_t *out) {
  __shared__ uint64_t part[4];
  const int r = blockIdx.x;
  if (r >= n) return;
  const WT *row = rows + (long)(index ? index[r] : r) * stride;
  uint64_t h = 0;
  for (int64_t j = threadIdx.x; j < genes; j += 256) {
    uint64_t bits;
    if constexpr (sizeof(WT) == 8) {
      const double v = row[j];
      bits = v == 0.0 ? 0ull : (uint64_t)__double_as_longlong(v);
    } else {
      const float v = row[j];
      bits = v == 0.0f ? 0ull : (uint64_t)__float_as_uint(v);
    }
    h += splitmix64(bits ^ ((uint64_t)j * 0x9E3779B97F4A7C15ull));
  }
  for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) out[r] = splitmix64(part[0] + part[1] + part[2] + part[3] + (uint64_t)genes);
}

}  // namespace pg

using namespace pg;

extern "C" {

int32_t pg_ga_select_tournament(const pg_select_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  if (a->k < 0 || a->n_pop < 1 || a->tournsize < 1 || !a->fitness || !a->chosen)
    return fail(PG_ERR_INVALID, "selTournament needs k >= 0, n_pop >= 1, tournsize >= 1 and buffers");
  if (a->k == 0) return PG_OK;
  hipLaunchKernelGGL(k_select, dim3((a->k + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_ga_select_tournament_ranked(const pg_select_args *a, const double *sorted_fitness,
                                       const int32_t *order, void *stream) {
  if (!a || !sorted_fitness || !order) return fail(PG_ERR_INVALID, "args/sorted_fitness/order is NULL");
  if (a->k < 0 || a->n_pop < 1 || a->tournsize < 1 || !a->chosen)
    return fail(PG_ERR_INVALID, "selTournament needs k >= 0, n_pop >= 1, tournsize >= 1 and buffers");
  if (a->k == 0) return PG_OK;
  hipLaunchKernelGGL(k_select_ranked, dim3((a->k + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a,
                     sorted_fitness, order);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_ga_vary(const pg_ga_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  if (a->n < 0 || a->genes < 1 || a->stride < a->genes || !a->parents || !a->chosen || !a->offspring ||
      !a->invalid || (a->dtype != PG_F32 && a->dtype != PG_F64))
    return fail(PG_ERR_INVALID, "varAnd: bad sizes or NULL buffers");
  if (a->n == 0) return PG_OK;
  const int pairs = (a->n + 1) / 2;
  if (a->pair_list && (!a->pair_count || a->pair_cap < 0)) return fail(PG_ERR_INVALID, "varAnd: pair_list needs pair_count and pair_cap >= 0");
  // list mode: the grid strides over the listed pairs, so pair_cap (an upper
  // bound of the count, which the device holds) only sizes the grid
  constexpr int kListWaves = 8192;
  int waves = a->pair_list ? (a->pair_cap < pairs ? a->pair_cap : pairs) : pairs;
  if (a->pair_list && waves > kListWaves) waves = kListWaves;
  if (waves == 0) return PG_OK;
  const dim3 grid((unsigned)((waves + 3) / 4));  // one wave per pair
  if (a->dtype == PG_F64)
    hipLaunchKernelGGL(k_vary<double>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(k_vary<float>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_ga_list_pairs(const uint8_t *mask, int32_t n_pairs, int32_t *list, int32_t *count, void *stream) {
  if (n_pairs < 0 || !count || (n_pairs && (!mask || !list))) return fail(PG_ERR_INVALID, "list_pairs: bad sizes or NULL buffers");
  PG_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), (hipStream_t)stream));
  if (n_pairs == 0) return PG_OK;
  hipLaunchKernelGGL(k_list_pairs, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask,
                     n_pairs, list, count);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_ga_mark_pairs(uint8_t *mask, int32_t n_pairs, const int32_t *rows, int32_t n_rows, int32_t skip_lo,
                         int32_t skip_hi, const uint8_t *exclude, void *stream) {
  if (n_pairs < 0 || n_rows < 0 || (n_rows && (!mask || !rows)))
    return fail(PG_ERR_INVALID, "mark_pairs: bad sizes or NULL buffers");
  if (n_rows == 0) return PG_OK;
  hipLaunchKernelGGL(k_mark_pairs, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask,
                     n_pairs, rows, n_rows, skip_lo, skip_hi, exclude);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_ga_schedule(const pg_schedule_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  if (a->n < 0 || a->n_games < 1 || a->n_hof < 0 || a->row_offset < 0 ||
      (a->mode != PG_SCHED_REFERENCE && a->mode != PG_SCHED_SELFPLAY))
    return fail(PG_ERR_INVALID, "schedule: bad sizes or mode");
  if (a->n == 0) return PG_OK;
  if (!a->kind || !a->opp || !a->mult || (a->mode == PG_SCHED_REFERENCE && a->n_hof > 0 && !a->hof_fitness))
    return fail(PG_ERR_INVALID, "schedule: NULL output or hof_fitness");
  const long total = (long)a->n * a->n_games;
  if (a->hof_slices > 1 && a->block_rows < 1) return fail(PG_ERR_INVALID, "schedule: hof_slices > 1 needs block_rows >= 1");
  hipLaunchKernelGGL(k_schedule, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_gather_rows(void *dst, int64_t dst_stride, const void *old_rows, int64_t old_stride, const void *rows,
                       int64_t rows_stride, const int64_t *index, const int32_t *src, int32_t n_old, int32_t n,
                       int64_t genes, int32_t dtype, void *stream) {
  if (n < 0 || n_old < 0 || genes < 1 || (dtype != PG_F32 && dtype != PG_F64) ||
      (n > 0 && (!dst || !src || (n_old > 0 && !old_rows) || dst_stride < genes || old_stride < genes ||
                 rows_stride < genes)))
    return fail(PG_ERR_INVALID, "gather_rows: bad sizes, dtype or NULL buffers");
  if (n == 0) return PG_OK;
  if (dtype == PG_F64)
    hipLaunchKernelGGL(k_gather_rows<double>, dim3(n), dim3(256), 0, (hipStream_t)stream, (double *)dst, dst_stride,
                       (const double *)old_rows, old_stride, (const double *)rows, rows_stride, index, src, n_old,
                       genes);
  else
    hipLaunchKernelGGL(k_gather_rows<float>, dim3(n), dim3(256), 0, (hipStream_t)stream, (float *)dst, dst_stride,
                       (const float *)old_rows, old_stride, (const float *)rows, rows_stride, index, src, n_old,
                       genes);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_row_hash(const void *rows, int64_t stride, const int32_t *index, int32_t n, int64_t genes,
                    int32_t dtype, uint64_t *hash, void *stream) {
  if (n < 0 || genes < 0 || (n > 0 && (!rows || !hash || stride < genes)) || (dtype != PG_F32 && dtype != PG_F64))
    return fail(PG_ERR_INVALID, "row_hash: bad sizes, dtype or NULL buffers");
  if (n == 0) return PG_OK;
  if (dtype == PG_F64)
    hipLaunchKernelGGL(k_row_hash<double>, dim3(n), dim3(256), 0, (hipStream_t)stream, (const double *)rows, stride,
                       index, n, genes, hash);
  else
    hipLaunchKernelGGL(k_row_hash<float>, dim3(n), dim3(256), 0, (hipStream_t)stream, (const float *)rows, stride,
                       index, n, genes, hash);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

}  // extern "C"
