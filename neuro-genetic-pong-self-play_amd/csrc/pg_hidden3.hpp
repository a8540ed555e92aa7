// pg_hidden3.hpp -- device code of k_relu3 (pg_relu3.hip): the certified f32
// forward of a [6, H1 <= 32, H2 <= 32, H3 <= 32, 2..4] ReLU network with bias
// (activation_function = ReLU, numpy_nn.py:6-9, 26) held by a half-group of LN
// lanes, its decision and its f64 re-decision in numpy's order: k_relu2's idiom
// (pg_hidden2.hpp) one layer deeper.  The bound's arithmetic and its derivation
// are in pg_relu3_bound.h (it also compiles for the host).  hidden3_z32 and
// hidden3_f64_half are templates on the activation (ACT, a pg_activation, as
// pg_hidden2.hpp's are): k_sig3 (pg_sig3.hpp) runs them with the sigmoid on this
// layout, under a load and a bound of its own.
//
// Lane hl of a half-group holds layer-1 units 2 hl, 2 hl + 1 (7 weights each),
// layer-2 units 2 hl, 2 hl + 1 (a whole row of W2 each: 2 LN weights and the
// bias), layer-3 units 2 hl, 2 hl + 1 (a whole row of W3 each, the same) and
// those units' O output weights, all as f32 in VGPRs for the whole game.  Each
// frame the lanes write their layer-1 activations to the half-group's first
// LDS row (an all-gather: 2 LN floats), every lane reads them all back for its
// layer-2 rows, the layer-2 activations go through the second row in the same
// way, and the outputs are summed over the lanes as k_relu's are.
//
// Padding.  A padding unit (j >= H1, k >= H2 or l >= H3) and a padding input
// have zero weights: max(0, 0) = 0 times 0 contributes exactly 0.
//
// The decision is k_relu's (pg_relu.hpp): with |z^_o - z64_o| <= e and t1 >= t2
// the two largest z^, the index is 0 if t1 <= -e, that of t1 if t1 > e and
// t1 - t2 > 2e, and is otherwise recomputed in f64 from the genes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_certgame.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_hidden2.hpp"  // half_broadcast
#include "pg_relu.hpp"
#include "pg_relu3_bound.h"

namespace pg {

constexpr int kHidden3MaxH = 32;
constexpr int kHidden3Units = 2;  // units of each hidden layer per lane
static_assert(PG_RELU3_MAX_H == kHidden3MaxH, "the bound's arrays");
// the instances: lanes per network by the widest hidden layer -- 16 units on
// 8 lanes (4 games a wave), 32 on 16 (2 games)
__host__ __device__ constexpr int hidden3_lanes(int H1, int H2, int H3) {
  return (H1 > H2 ? (H1 > H3 ? H1 : H3) : (H2 > H3 ? H2 : H3)) <= 16 ? 8 : 16;
}

// the hidden sizes of a network (k_relu3's own: CertDims, which the other
// families' kernels are compiled with, has two)
struct Hidden3Dims {
  int H1, H2, H3;
};

// pg_relu3_decide's parameters: the families' and the third width
struct Hidden3DecideParams : CertDecideParams {
  int H3;
};

template <int LN, int U, int O>
struct Hidden3Net {
  float w1[U][7];       // layer-1 unit hl U + u: 6 input weights + bias weight
  float w2[U][LN * U];  // layer-2 unit hl U + v: its weight of every (padded) layer-1 unit
  float b2[U];
  float w3[U][LN * U];  // layer-3 unit hl U + v: its weight of every (padded) layer-2 unit
  float b3[U];
  float w4[U][O];       // output weights of that layer-3 unit
  float c[O];           // output biases
  float e;              // |z^_o - z64_o| <= e for every output (pg_relu3_bound.h); inf: always f64
};

// LDS of one half-group: the two f32 all-gather rows, and the f64 path's
// activations (also the load's A_j, B_k and V2_k): 3 LN U hidden + O outputs
template <int LN, int U>
struct alignas(16) Hidden3Lds {
  float h1[LN * U];
  float h2[LN * U];
  double d[3 * LN * U + 4];
};

// This lane's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [H3, H2 + 1], W4 [O, H3 + 1], bias
// columns last) as f32 -- exact zeros for every padding unit's row and column
// -- and the network's bound from the f64 genes.  H1, H2, H3 <= LN U
// (host-checked).
template <int LN, int U, int O, typename WT>
__device__ __forceinline__ void hidden3_load(Hidden3Net<LN, U, O> &n, const WT *__restrict__ g, int H1, int H2, int H3,
                                             Hidden3Lds<LN, U> &lds, int hl) {
  static_assert(LN * U <= PG_RELU3_MAX_H, "pg_relu3_bound_genome, the LDS rows, the underflow term's unit counts");
  static_assert(PG_RELU3_CHAIN1 == 1 + 2 + 6, "the bound's layer-1 chain: gene, feat32, hidden3_z32's 6 fmas");
  static_assert(1 + LN * U <= PG_RELU3_CHAIN2, "the bound's layer-2 chain");
  static_assert(1 + LN * U <= PG_RELU3_CHAIN3, "the bound's layer-3 chain");
  static_assert(1 + U + relu_log2(LN) + 1 <= PG_RELU3_CHAIN4, "the bound's layer-4 chain");
  static_assert(O <= PG_RELU_MAX_OUT, "the bound's sums");
  // hl and the widths made opaque: the unit offsets and masks below would otherwise be
  // hoisted out of the game loop as loop-invariant registers kept live across every frame
  asm volatile("" : "+v"(hl));
  asm volatile("" : "+s"(H1), "+s"(H2), "+s"(H3));
  constexpr int N = LN * U;
  const long off2 = (long)H1 * 7, off3 = off2 + (long)H2 * (H1 + 1), off4 = off3 + (long)H3 * (H2 + 1);
  double *dA = lds.d, *dB = lds.d + N, *dV = lds.d + 2 * N;
  double asum = 0.0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = hl * U + u;
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
    dA[j] = a;
    asum += a;
    __builtin_amdgcn_sched_barrier(0);  // one unit's loads in flight at a time (see relu_load)
  }
  asum = half_sum_f64<LN>(asum);
  wave_lds_sync();
  pg_relu3_sums s;
  pg_relu3_sums_init(&s);
#pragma unroll
  for (int v = 0; v < U; ++v) {
    const int k = hl * U + v;
    const bool ok = k < H2;
    const WT *row = g + off2 + (long)(ok ? k : 0) * (H1 + 1);
    double p = 0.0, wsum = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool okj = ok && j < H1;
      const WT raw = row[j < H1 ? j : 0];
      const double w = okj ? (double)raw : 0.0;  // a padding unit's outgoing weight: exactly zero
      relu_set(n.w2[v][j], (float)w);
      p += fabs(w) * (j < H1 ? dA[j] : 0.0);
      wsum += fabs(w);
      if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
    const WT rawb = row[H1];
    const double bias = ok ? (double)rawb : 0.0;
    relu_set(n.b2[v], (float)bias);
    const double b = p + fabs(bias);
    dB[k] = b;  // (a padding unit: 0, and 0)
    dV[k] = wsum;
    pg_relu3_sums_unit2(&s, b, wsum);
    __builtin_amdgcn_sched_barrier(0);
  }
  wave_lds_sync();
#pragma unroll
  for (int v = 0; v < U; ++v) {
    const int l = hl * U + v;
    const bool ok = l < H3;
    const WT *row = g + off3 + (long)(ok ? l : 0) * (H2 + 1);
    double cl = 0.0, t = 0.0, wsum = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool okk = ok && k < H2;
      const WT raw = row[k < H2 ? k : 0];
      const double w = okk ? (double)raw : 0.0;
      relu_set(n.w3[v][k], (float)w);
      cl += fabs(w) * (k < H2 ? dB[k] : 0.0);
      t += fabs(w) * (k < H2 ? dV[k] : 0.0);
      wsum += fabs(w);
      if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
    const WT rawb = row[H2];
    const double bias = ok ? (double)rawb : 0.0;
    relu_set(n.b3[v], (float)bias);
    double w4[O];
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const WT raw = g[off4 + (long)o * (H3 + 1) + (ok ? l : 0)];
      w4[o] = ok ? (double)raw : 0.0;  // (the same for a padding layer-3 unit)
      relu_set(n.w4[v][o], (float)w4[o]);
    }
    pg_relu3_sums_unit3(&s, cl + fabs(bias), t, wsum, w4, O);
    __builtin_amdgcn_sched_barrier(0);
  }
  double c[O];
#pragma unroll
  for (int o = 0; o < O; ++o) {
    c[o] = (double)g[off4 + (long)o * (H3 + 1) + H3];
    relu_set(n.c[o], (float)c[o]);
    s.S[o] = half_sum_f64<LN>(s.S[o]);
    s.Q[o] = half_sum_f64<LN>(s.Q[o]);
    s.R[o] = half_sum_f64<LN>(s.R[o]);
    s.W4[o] = half_sum_f64<LN>(s.W4[o]);
  }
  s.B = half_sum_f64<LN>(s.B);
  s.C = half_sum_f64<LN>(s.C);
  s.W2 = half_sum_f64<LN>(s.W2);
  s.W3 = half_sum_f64<LN>(s.W3);
  // one lane's bound for the whole half-group: every lane certifies under the same e
  const float e = __int_as_float(half_broadcast<LN>(__float_as_int(pg_relu3_bound_finish(&s, asum, c, O))));
  relu_set(n.e, e);
  wave_lds_sync();  // the B_k and V2_k are read: lds.d is free for the f64 path
}

// The f32 output pre-activations z^ on the doubled-centroid features k, with
// the chain lengths pg_relu3_bound.h and pg_sig3_bound.h bound (under the
// sigmoid a padding unit's activation is 0.5, met by zero weights only); every lane of the half-group gets
// the bitwise-identical values (group_sum).
template <int ACT, int LN, int U, int O>
__device__ __forceinline__ void hidden3_z32(const Hidden3Net<LN, U, O> &n, const int k[6], float *row1, float *row2,
                                            int hl, float z[O]) {
  static_assert(U == 2, "the vector stores below");
  float x[6], h1[U];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat32(k[i]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float a = n.w1[u][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) a = fmaf(n.w1[u][i], x[i], a);
    h1[u] = hidden2_act32<ACT>(a);
  }
  wave_lds_sync();  // both rows' readers of the frame before are done
  *(float2 *)(row1 + hl * U) = make_float2(h1[0], h1[1]);
  wave_lds_sync();
  float a2[U];
#pragma unroll
  for (int v = 0; v < U; ++v) a2[v] = n.b2[v];
#pragma unroll
  for (int j = 0; j < LN * U; j += 4) {
    const float4 h = *(const float4 *)(row1 + j);
#pragma unroll
    for (int v = 0; v < U; ++v) {
      a2[v] = fmaf(n.w2[v][j], h.x, a2[v]);
      a2[v] = fmaf(n.w2[v][j + 1], h.y, a2[v]);
      a2[v] = fmaf(n.w2[v][j + 2], h.z, a2[v]);
      a2[v] = fmaf(n.w2[v][j + 3], h.w, a2[v]);
    }
  }
  *(float2 *)(row2 + hl * U) = make_float2(hidden2_act32<ACT>(a2[0]), hidden2_act32<ACT>(a2[1]));
  wave_lds_sync();
  float a3[U];
#pragma unroll
  for (int v = 0; v < U; ++v) a3[v] = n.b3[v];
#pragma unroll
  for (int j = 0; j < LN * U; j += 4) {
    const float4 h = *(const float4 *)(row2 + j);
#pragma unroll
    for (int v = 0; v < U; ++v) {
      a3[v] = fmaf(n.w3[v][j], h.x, a3[v]);
      a3[v] = fmaf(n.w3[v][j + 1], h.y, a3[v]);
      a3[v] = fmaf(n.w3[v][j + 2], h.z, a3[v]);
      a3[v] = fmaf(n.w3[v][j + 3], h.w, a3[v]);
    }
  }
  float acc[O];
#pragma unroll
  for (int o = 0; o < O; ++o) acc[o] = 0.f;
#pragma unroll
  for (int v = 0; v < U; ++v) {
    const float h3 = hidden2_act32<ACT>(a3[v]);
#pragma unroll
    for (int o = 0; o < O; ++o) acc[o] = fmaf(n.w4[v][o], h3, acc[o]);
  }
#pragma unroll
  for (int o = 0; o < O; ++o) z[o] = group_sum<LN>(acc[o]) + n.c[o];
}

// The f64 forward of one pass by the LN lanes of a half-group, as
// forward_f64_wave runs it (NeuralNetwork.run numpy_nn.py:120-137 in np.dot's
// order, blas_dot over [inputs..., 1] per unit): each layer's units strided
// over the lanes into LDS, lane o < O sums output o, every lane takes the
// argmax.  d: the half-group's Hidden3Lds::d.
template <int ACT, int LN, int U, int O, typename WT>
__device__ PG_SLOW_INLINE int hidden3_f64_half(const WT *__restrict__ g, int H1, int H2, int H3, const int k[6],
                                               double *d, int hl) {
  static_assert(O <= LN, "lane o sums output o");
  asm volatile("" : "+v"(hl));  // (as in hidden3_load: nothing of this cold path is hoisted into the frame loop)
  constexpr int N = LN * U;
  double *d1 = d, *d2 = d + N, *d3 = d + 2 * N, *out = d + 3 * N;
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat64(k[i]);
  const int H1c = H1 < N ? H1 : N, H2c = H2 < N ? H2 : N, H3c = H3 < N ? H3 : N;
#pragma unroll 1
  for (int j = hl; j < H1c; j += LN) {
    const WT *row = g + (long)j * 7;
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < 6 ? x[i] : 1.0; }, 7,
                              blas_kind(j, H1));
    d1[j] = hidden2_act64<ACT>(z);
  }
  wave_lds_sync();
  const WT *w2 = g + (long)H1 * 7;
#pragma unroll 1
  for (int j = hl; j < H2c; j += LN) {
    const WT *row = w2 + (long)j * (H1 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H1c ? d1[i] : 1.0; },
                              H1c + 1, blas_kind(j, H2));
    d2[j] = hidden2_act64<ACT>(z);
  }
  wave_lds_sync();
  const WT *w3 = w2 + (long)H2 * (H1 + 1);
#pragma unroll 1
  for (int j = hl; j < H3c; j += LN) {
    const WT *row = w3 + (long)j * (H2 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H2c ? d2[i] : 1.0; },
                              H2c + 1, blas_kind(j, H3));
    d3[j] = hidden2_act64<ACT>(z);
  }
  wave_lds_sync();
  if (hl < O) {
    const WT *row = w3 + (long)H3 * (H2 + 1) + (long)hl * (H3 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H3c ? d3[i] : 1.0; },
                              H3c + 1, blas_kind(hl, O));
    out[hl] = hidden2_act64<ACT>(z);
  }
  wave_lds_sync();
  int best = 0;  // np.argmax: the first NaN if any, else the first maximum
#pragma unroll
  for (int o = 1; o < O; ++o)
    if (!__builtin_isnan(out[best]) && (__builtin_isnan(out[o]) || out[o] > out[best])) best = o;
  wave_lds_sync();
  return best;
}

// k_relu3's policy (pg_certgame.hpp).  Dims and dims: the hidden sizes as this
// family takes them from a launch's parameters.  decide: one decision of a
// half-group, z^ returned in z.  live = false (the idle left half of a game
// against a scripted opponent): index 0, stage 0, never the f64 path.
template <int LN_, int U, int O_, typename WT_>
struct Relu3Policy {
  static constexpr int LN = LN_, O = O_, kF64Stage = 1;
  using WT = WT_;
  using Net = Hidden3Net<LN, U, O>;
  using Lds = Hidden3Lds<LN, U>;
  using Dims = Hidden3Dims;
  static __device__ __forceinline__ Dims dims(const EvalParams &p) { return {p.nodes[1], p.nodes[2], p.nodes[3]}; }
  static __device__ __forceinline__ Dims dims(const Hidden3DecideParams &p) { return {p.H1, p.H2, p.H3}; }
  static __device__ __forceinline__ void load(Net &net, const WT *g, const Dims &dims, Lds &lds, int hl) {
    hidden3_load<LN, U, O, WT>(net, g, dims.H1, dims.H2, dims.H3, lds, hl);
  }
  // the certificate as lane 0 of the half-group takes it (every lane acts on
  // that one index), else the f64 forward (stage 1)
  static __device__ __forceinline__ int decide(const Net &n, const WT *__restrict__ g, const Dims &dims, const int k[6],
                                               bool live, Lds &lds, int hl, float z[O], int &stage) {
    hidden3_z32<PG_ACT_RELU, LN, U, O>(n, k, lds.h1, lds.h2, hl, z);
    int idx = half_broadcast<LN>(relu_certify<O>(z, n.e));
    const bool need = live && idx < 0;
    stage = need ? 1 : 0;
    if (PG_ANY(need) && need) idx = hidden3_f64_half<PG_ACT_RELU, LN, U, O, WT>(g, dims.H1, dims.H2, dims.H3, k, lds.d, hl);
    return idx < 0 ? 0 : idx;
  }
};

// ------------------------------------------------------------ host side ----
// the instances: LN = hidden3_lanes(H1, H2, H3) lanes per network, kHidden3Units units of each layer per lane
#define PG_HIDDEN3_DISPATCH(KERNEL, LN, O, f64, grid, s, p)                          \
  do {                                                                               \
    if (LN == 8) PG_CERT_DISPATCH(KERNEL, 8, (kHidden3Units), O, f64, grid, s, p);   \
    else PG_CERT_DISPATCH(KERNEL, 16, (kHidden3Units), O, f64, grid, s, p);          \
  } while (0)

static_assert(8 * kHidden3Units >= 16 && 16 * kHidden3Units >= kHidden3MaxH,
              "hidden3_lanes' thresholds: a layout for every width in scope");

// What Relu3Family (pg_relu3.hip) and Sig3Family (pg_sig3.hip) share of a
// family's description (pg_family.hpp); each adds its kernel, its activation,
// its messages and the launches of its kernels.
struct Hidden3Family {
  static constexpr bool kModifiers = true, kScopeOnEntry = true;
  using DecideParams = Hidden3DecideParams;
  // the shapes [6, 2..32, 2..32, 2..32, 2..4]
  static bool shape_ok(int n_nodes, const int32_t *nodes) {
    if (n_nodes != 5 || nodes[0] != 6 || nodes[4] < 2 || nodes[4] > 4) return false;
    for (int i = 1; i <= 3; ++i)
      if (nodes[i] < 2 || nodes[i] > kHidden3MaxH) return false;
    return true;
  }
  static long genes(const int32_t *nd) {
    return (long)nd[1] * 7 + (long)nd[2] * (nd[1] + 1) + (long)nd[3] * (nd[2] + 1) + (long)nd[4] * (nd[3] + 1);
  }
  static int lanes(const int32_t *nd) { return hidden3_lanes(nd[1], nd[2], nd[3]); }
  static int game_grid(const EvalParams &p) { return cert_game_grid(p, lanes(p.nodes)); }
  static int decide_grid(const pg_relu_decide_args *a) { return cert_decide_grid(a->n, lanes(a->net.nodes)); }
  static DecideParams decide_params(const pg_relu_decide_args *a) {
    DecideParams p;
    static_cast<CertDecideParams &>(p) = cert_decide_params(a, a->net.nodes[1], a->net.nodes[2]);
    p.H3 = a->net.nodes[3];
    return p;
  }
};

}  // namespace pg
