// pg_relu2.hpp -- device code of k_relu2 (pg_relu2.hip): the certified f32
// forward of a [6, H1 <= 64, H2 <= 64, 2..4] ReLU network with bias
// (activation_function = ReLU, numpy_nn.py:6-9, 26) held by a half-group of LN
// lanes, and its f64 re-decision in numpy's order.  The bound's arithmetic and
// its derivation are in pg_relu2_bound.h (it also compiles for the host).
//
// Lane hl of a half-group holds layer-1 units hl U1 .. hl U1 + U1 - 1 (7
// weights each), layer-2 units hl U2 .. hl U2 + U2 - 1 (a whole row of W2 each:
// LN U1 weights and the bias) and those units' O output weights, all as f32 in
// VGPRs for the whole game.  Padding units and padding inputs have zero
// weights: max(0, 0) = 0 times 0 contributes exactly 0.  Each frame the lanes
// write their layer-1 activations to the half-group's LDS row (an all-gather:
// LN U1 floats), every lane reads them all back for its layer-2 rows, and the
// outputs are summed over the lanes as k_relu's are.
//
// The decision is k_relu's (pg_relu.hpp): with |z^_o - z64_o| <= e and t1 >= t2
// the two largest z^, the index is 0 if t1 <= -e, that of t1 if t1 > e and
// t1 - t2 > 2e, and is otherwise recomputed in f64 from the genes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_cascade.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_relu.hpp"
#include "pg_relu2_bound.h"

namespace pg {

constexpr int kRelu2MaxH = PG_RELU2_MAX_H;
// the instances: lanes per network and units per lane (both layers) by the
// wider hidden layer -- 16 x 16 on 4 lanes (8 games a wave), 32 x 32 on 16
// (2 games), 64 x 64 on 32 (1 game)
__host__ __device__ constexpr int relu2_lanes(int H1, int H2) {
  return (H1 > H2 ? H1 : H2) <= 16 ? 4 : ((H1 > H2 ? H1 : H2) <= 32 ? 16 : 32);
}
__host__ __device__ constexpr int relu2_units(int LN) { return LN == 4 ? 4 : 2; }

template <int LN, int U1, int U2, int O>
struct Relu2Net {
  float w1[U1][7];        // layer-1 unit hl U1 + u: 6 input weights + bias weight
  float w2[U2][LN * U1];  // layer-2 unit hl U2 + v: its weight of every (padded) layer-1 unit
  float b2[U2];
  float w3[U2][O];        // output weights of that unit
  float c[O];             // output biases
  float e;                // |z^_o - z64_o| <= e for every output (pg_relu2_bound.h); inf: always f64
};

// LDS of one half-group: the f32 all-gather row, and the f64 path's
// activations (also the load's A_j): LN U1 + LN U2 hidden + O outputs
template <int LN, int U1, int U2>
struct alignas(16) Relu2Lds {
  float h[LN * U1];
  double d[LN * U1 + LN * U2 + 4];
};

// value of lane (hl = 0) of this lane's half-group
template <int LN>
__device__ __forceinline__ int half_broadcast(int v) {
  return __shfl(v, (int)(threadIdx.x & 63 & ~(LN - 1)), 64);
}

// This lane's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last) as
// f32, and the network's bound from the f64 genes.  H1 <= LN U1, H2 <= LN U2
// (host-checked).
template <int LN, int U1, int U2, int O, typename WT>
__device__ __forceinline__ void relu2_load(Relu2Net<LN, U1, U2, O> &n, const WT *__restrict__ g, int H1, int H2,
                                           Relu2Lds<LN, U1, U2> &lds, int hl) {
  static_assert(LN * U1 <= PG_RELU2_MAX_H && LN * U2 <= PG_RELU2_MAX_H, "pg_relu2_bound_genome, the LDS rows");
  static_assert(1 + LN * U1 <= PG_RELU2_CHAIN2, "pg_relu2_bound.h's layer-2 chain");
  static_assert(1 + U2 + relu_log2(LN) + 1 <= PG_RELU2_CHAIN3, "pg_relu2_bound.h's layer-3 chain");
  static_assert(O <= PG_RELU_MAX_OUT, "pg_relu2_sums");
  // hl made opaque: the unit offsets and masks below would otherwise be hoisted out
  // of the game loop as loop-invariant VGPRs kept live across every frame
  asm volatile("" : "+v"(hl));
  asm volatile("" : "+s"(H1), "+s"(H2));  // (the same for the 64 padding tests j < H1: scalar masks otherwise)
  const long off2 = (long)H1 * 7, off3 = off2 + (long)H2 * (H1 + 1);
  double asum = 0.0;
#pragma unroll
  for (int u = 0; u < U1; ++u) {
    const int j = hl * U1 + u;
    const bool ok = j < H1;
    const WT *row = g + (long)(ok ? j : 0) * 7;  // padding units load a valid row and are zeroed
    double w[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const WT raw = row[i];
      w[i] = ok ? (double)raw : 0.0;
      relu_set(n.w1[u][i], (float)w[i]);
    }
    const double a = pg_relu2_unit1(w);
    lds.d[j] = a;
    asum += a;
    __builtin_amdgcn_sched_barrier(0);  // one unit's loads in flight at a time (see relu_load)
  }
  asum = half_sum_f64<LN>(asum);
  wave_lds_sync();
  pg_relu2_sums s;
  pg_relu2_sums_init(&s);
#pragma unroll
  for (int v = 0; v < U2; ++v) {
    const int k = hl * U2 + v;
    const bool ok = k < H2;
    const WT *row = g + off2 + (long)(ok ? k : 0) * (H1 + 1);
    double b = 0.0, wsum = 0.0;
#pragma unroll
    for (int j = 0; j < LN * U1; ++j) {
      const bool okj = ok && j < H1;
      const WT raw = row[j < H1 ? j : 0];
      const double w = okj ? (double)raw : 0.0;
      relu_set(n.w2[v][j], (float)w);
      b += fabs(w) * (j < H1 ? lds.d[j] : 0.0);
      wsum += fabs(w);
      if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
    const WT rawb = row[H1];
    const double bias = ok ? (double)rawb : 0.0;
    relu_set(n.b2[v], (float)bias);
    b += fabs(bias);
    double w3[O];
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const WT raw = g[off3 + (long)o * (H2 + 1) + (ok ? k : 0)];
      w3[o] = ok ? (double)raw : 0.0;
      relu_set(n.w3[v][o], (float)w3[o]);
    }
    pg_relu2_sums_unit2(&s, b, wsum, w3, O);
    __builtin_amdgcn_sched_barrier(0);
  }
  double c[O];
#pragma unroll
  for (int o = 0; o < O; ++o) {
    c[o] = (double)g[off3 + (long)o * (H2 + 1) + H2];
    relu_set(n.c[o], (float)c[o]);
    s.S[o] = half_sum_f64<LN>(s.S[o]);
    s.T[o] = half_sum_f64<LN>(s.T[o]);
    s.W3[o] = half_sum_f64<LN>(s.W3[o]);
  }
  s.B = half_sum_f64<LN>(s.B);
  s.W2 = half_sum_f64<LN>(s.W2);
  // one lane's bound for the whole half-group: every lane certifies under the same e
  const float e = pg_relu2_bound_finish(&s, asum, c, O);
  relu_set(n.e, __int_as_float(half_broadcast<LN>(__float_as_int(e))));
  wave_lds_sync();  // the A_j are read: lds.d is free for the f64 path
}

// The f32 output pre-activations z^ on the doubled-centroid features k, with
// the chain lengths pg_relu2_bound.h bounds; every lane of the half-group
// gets them.
template <int LN, int U1, int U2, int O>
__device__ __forceinline__ void relu2_z32(const Relu2Net<LN, U1, U2, O> &n, const int k[6], float *hrow, int hl,
                                          float z[O]) {
  static_assert(U1 == 2 || U1 == 4, "the vector store below");
  float x[6], h1[U1];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat32(k[i]);
#pragma unroll
  for (int u = 0; u < U1; ++u) {
    float a = n.w1[u][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) a = fmaf(n.w1[u][i], x[i], a);
    h1[u] = fmaxf(a, 0.f);
  }
  wave_lds_sync();  // the row's readers of the frame before are done
  if constexpr (U1 == 2) *(float2 *)(hrow + hl * U1) = make_float2(h1[0], h1[1]);
  else *(float4 *)(hrow + hl * U1) = make_float4(h1[0], h1[1], h1[2], h1[3]);
  wave_lds_sync();
  float a2[U2];
#pragma unroll
  for (int v = 0; v < U2; ++v) a2[v] = n.b2[v];
#pragma unroll
  for (int j = 0; j < LN * U1; j += 4) {
    const float4 h = *(const float4 *)(hrow + j);
#pragma unroll
    for (int v = 0; v < U2; ++v) {
      a2[v] = fmaf(n.w2[v][j], h.x, a2[v]);
      a2[v] = fmaf(n.w2[v][j + 1], h.y, a2[v]);
      a2[v] = fmaf(n.w2[v][j + 2], h.z, a2[v]);
      a2[v] = fmaf(n.w2[v][j + 3], h.w, a2[v]);
    }
  }
  float acc[O];
#pragma unroll
  for (int o = 0; o < O; ++o) acc[o] = 0.f;
#pragma unroll
  for (int v = 0; v < U2; ++v) {
    const float h2 = fmaxf(a2[v], 0.f);
#pragma unroll
    for (int o = 0; o < O; ++o) acc[o] = fmaf(n.w3[v][o], h2, acc[o]);
  }
#pragma unroll
  for (int o = 0; o < O; ++o) z[o] = group_sum<LN>(acc[o]) + n.c[o];
}

// The f64 forward of one pass by the LN lanes of a half-group, as
// forward_f64_wave runs it (NeuralNetwork.run numpy_nn.py:120-137 in np.dot's
// order, blas_dot over [inputs..., 1] per unit): each layer's units strided
// over the lanes into LDS, lane o < O sums output o, every lane takes the
// argmax.  d: the half-group's Relu2Lds::d.
template <int LN, int U1, int U2, int O, typename WT>
__device__ PG_SLOW_INLINE int relu2_f64_half(const WT *__restrict__ g, int H1, int H2, const int k[6], double *d,
                                             int hl) {
  static_assert(O <= LN, "lane o sums output o");
  asm volatile("" : "+v"(hl));  // (as in relu2_load: nothing of this cold path is hoisted into the frame loop)
  double *d1 = d, *d2 = d + LN * U1, *out = d + LN * U1 + LN * U2;
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat64(k[i]);
#pragma unroll 1
  for (int j = hl; j < H1 && j < LN * U1; j += LN) {
    const WT *row = g + (long)j * 7;
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < 6 ? x[i] : 1.0; }, 7,
                              blas_kind(j, H1));
    d1[j] = relu_f64(z);
  }
  wave_lds_sync();
  const int H1c = H1 < LN * U1 ? H1 : LN * U1, H2c = H2 < LN * U2 ? H2 : LN * U2;
  const WT *w2 = g + (long)H1 * 7;
#pragma unroll 1
  for (int j = hl; j < H2c; j += LN) {
    const WT *row = w2 + (long)j * (H1 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H1c ? d1[i] : 1.0; },
                              H1c + 1, blas_kind(j, H2));
    d2[j] = relu_f64(z);
  }
  wave_lds_sync();
  if (hl < O) {
    const WT *row = w2 + (long)H2 * (H1 + 1) + (long)hl * (H2 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H2c ? d2[i] : 1.0; },
                              H2c + 1, blas_kind(hl, O));
    out[hl] = relu_f64(z);
  }
  wave_lds_sync();
  int best = 0;  // np.argmax: the first NaN if any, else the first maximum
#pragma unroll
  for (int o = 1; o < O; ++o)
    if (!__builtin_isnan(out[best]) && (__builtin_isnan(out[o]) || out[o] > out[best])) best = o;
  wave_lds_sync();
  return best;
}

// One decision of a half-group: z^ (returned in z), the certificate as lane 0
// of the half-group takes it (every lane acts on that one index), else the f64
// forward (slow = 1).  live = false (the idle left half of a game against a
// scripted opponent): index 0, never the f64 path.
template <int LN, int U1, int U2, int O, typename WT>
__device__ __forceinline__ int relu2_decide(const Relu2Net<LN, U1, U2, O> &n, const WT *__restrict__ g, int H1, int H2,
                                            const int k[6], bool live, Relu2Lds<LN, U1, U2> &lds, int hl, float z[O],
                                            int &slow) {
  relu2_z32<LN, U1, U2, O>(n, k, lds.h, hl, z);
  int idx = half_broadcast<LN>(relu_certify<O>(z, n.e));
  const bool need = live && idx < 0;
  slow = need ? 1 : 0;
  if (PG_ANY(need) && need) idx = relu2_f64_half<LN, U1, U2, O, WT>(g, H1, H2, k, lds.d, hl);
  return idx < 0 ? 0 : idx;
}

// pg_relu2_decide's parameters (k_relu2_decide)
struct Relu2DecideParams {
  const void *genomes;
  const int32_t *gidx;
  const int32_t *k;
  int32_t *index;
  int32_t *stage;
  float *z32;
  float *bound;
  int64_t gstride;
  int n, H1, H2;
};

}  // namespace pg
