// pg_sig2.hpp -- device code of k_sig2 (pg_sig2.hip): the certified f32
// forward of a [6, H1 <= 64, H2 <= 64, 2..4] sigmoid network with bias
// (activation_function = sigmoid, numpy_nn.py:22-26) held by a half-group of
// LN lanes, its decision cascade and its f64 re-decision in numpy's order.
// The bound's arithmetic and its derivation are in pg_sig2_bound.h (it also
// compiles for the host).
//
// The layout is k_relu2's (pg_relu2.hpp: Relu2Net, Relu2Lds, relu2_lanes /
// relu2_units): lane hl of a half-group holds layer-1 units hl U1 .. hl U1 +
// U1 - 1, layer-2 units hl U2 .. hl U2 + U2 - 1 (a whole row of W2 each) and
// those units' O output weights as f32 in VGPRs for the whole game; layer 1's
// activations are all-gathered through the half-group's LDS row each frame.
// The activations are sigmoid_f32 (pg_cascade.hpp) of both hidden layers.
//
// Padding.  A padding unit (j >= H1 or k >= H2) has zero incoming weights and
// so the activation sigmoid_f32(0) = 0.5, not 0 as under ReLU.  Correctness
// rests on its OUTGOING weights being exactly zero: sig2_load writes 0.0f for
// every weight of a padding row and for every column j >= H1 of W2, and
// fma(0, 0.5, a) = a leaves every sum and its error bound untouched.
//
// The decision is k_service's cascade on the output pre-activations z^ with
// |z^_o - znp_o| <= e (numpy's f64 pre-activations): certify_c under the
// game's make_cert(e); for an undecided half-group tight_gap_move, then
// plateau_f32; then the f64 forward from the genes in np.dot's order with the
// correctly rounded sigmoid_f64 in all three layers and np.argmax's rule.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_cascade.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_relu.hpp"
#include "pg_relu2.hpp"
#include "pg_sig2_bound.h"

namespace pg {

constexpr int kSig2MaxH = PG_SIG2_MAX_H;

// k_relu2's weights and bound, and certify_c's constants of that bound
template <int LN, int U1, int U2, int O>
struct Sig2Net {
  Relu2Net<LN, U1, U2, O> n;
  Cert ct;
};

// This lane's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last) as
// f32 -- exact zeros for every padding unit's row and column, see above -- and
// the network's bound from the f64 genes.  H1 <= LN U1, H2 <= LN U2
// (host-checked).
template <int LN, int U1, int U2, int O, typename WT>
__device__ __forceinline__ void sig2_load(Sig2Net<LN, U1, U2, O> &sn, const WT *__restrict__ g, int H1, int H2,
                                          Relu2Lds<LN, U1, U2> &lds, int hl) {
  static_assert(LN * U1 <= PG_SIG2_MAX_H && LN * U2 <= PG_SIG2_MAX_H,
                "pg_sig2_bound_genome, the LDS rows, the underflow term's unit counts");
  static_assert(PG_SIG2_CHAIN1 == 1 + 2 + 6, "pg_sig2_bound.h's layer-1 chain: gene, feat32, sig2_z32's 6 fmas");
  static_assert(1 + LN * U1 <= PG_SIG2_CHAIN2, "pg_sig2_bound.h's layer-2 chain");
  static_assert(1 + U2 + relu_log2(LN) + 1 <= PG_SIG2_CHAIN3, "pg_sig2_bound.h's layer-3 chain");
  static_assert(O <= PG_SIG2_MAX_OUT, "pg_sig2_sums");
  Relu2Net<LN, U1, U2, O> &n = sn.n;
  // (hl, H1, H2 made opaque: see relu2_load)
  asm volatile("" : "+v"(hl));
  asm volatile("" : "+s"(H1), "+s"(H2));
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
    const double a = pg_sig2_unit1(w);
    lds.d[j] = a;
    asum += a;
    __builtin_amdgcn_sched_barrier(0);  // one unit's loads in flight at a time (see relu_load)
  }
  asum = half_sum_f64<LN>(asum);
  wave_lds_sync();
  pg_sig2_sums s;
  pg_sig2_sums_init(&s);
#pragma unroll
  for (int v = 0; v < U2; ++v) {
    const int k = hl * U2 + v;
    const bool ok = k < H2;
    const WT *row = g + off2 + (long)(ok ? k : 0) * (H1 + 1);
    double p = 0.0, wsum = 0.0;
#pragma unroll
    for (int j = 0; j < LN * U1; ++j) {
      const bool okj = ok && j < H1;
      const WT raw = row[j < H1 ? j : 0];
      const double w = okj ? (double)raw : 0.0;  // a padding unit's outgoing weight: exactly zero
      relu_set(n.w2[v][j], (float)w);
      p += fabs(w) * (j < H1 ? lds.d[j] : 0.0);
      wsum += fabs(w);
      if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
    const WT rawb = row[H1];
    const double bias = ok ? (double)rawb : 0.0;
    relu_set(n.b2[v], (float)bias);
    double w3[O];
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const WT raw = g[off3 + (long)o * (H2 + 1) + (ok ? k : 0)];
      w3[o] = ok ? (double)raw : 0.0;  // (the same for a padding layer-2 unit)
      relu_set(n.w3[v][o], (float)w3[o]);
    }
    pg_sig2_sums_unit2(&s, p, wsum, bias, w3, O);
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
  s.P = half_sum_f64<LN>(s.P);
  // one lane's bound for the whole half-group: every lane certifies under the same e
  const float e = __int_as_float(half_broadcast<LN>(__float_as_int(pg_sig2_bound_finish(&s, asum, c, O))));
  const Cert ct = make_cert(e);
  relu_set(n.e, e);
  relu_set(sn.ct.tlo, ct.tlo);
  relu_set(sn.ct.thi, ct.thi);
  relu_set(sn.ct.lowz, ct.lowz);
  relu_set(sn.ct.e2, ct.e2);
  relu_set(sn.ct.ee, ct.ee);
  wave_lds_sync();  // the A_j are read: lds.d is free for the f64 path
}

// The f32 output pre-activations z^ on the doubled-centroid features k, with
// the chain lengths pg_sig2_bound.h bounds; every lane of the half-group gets
// the bitwise-identical values (group_sum).
template <int LN, int U1, int U2, int O>
__device__ __forceinline__ void sig2_z32(const Relu2Net<LN, U1, U2, O> &n, const int k[6], float *hrow, int hl,
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
    h1[u] = sigmoid_f32(a);  // (a padding unit: 0.5, met by zero weights only)
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
    const float h2 = sigmoid_f32(a2[v]);
#pragma unroll
    for (int o = 0; o < O; ++o) acc[o] = fmaf(n.w3[v][o], h2, acc[o]);
  }
#pragma unroll
  for (int o = 0; o < O; ++o) z[o] = group_sum<LN>(acc[o]) + n.c[o];
}

// The f64 forward of one pass by the LN lanes of a half-group
// (NeuralNetwork.run numpy_nn.py:120-137 in np.dot's order, blas_dot over
// [inputs..., 1] per unit; relu2_f64_half's structure): each layer's units
// strided over the lanes into LDS with numpy's sigmoid (sigmoid_f64: np.e **
// -z correctly rounded), lane o < O sums output o, every lane takes the
// argmax.  d: the half-group's Relu2Lds::d.
template <int LN, int U1, int U2, int O, typename WT>
__device__ PG_SLOW_INLINE int sig2_f64_half(const WT *__restrict__ g, int H1, int H2, const int k[6], double *d,
                                            int hl) {
  static_assert(O <= LN, "lane o sums output o");
  asm volatile("" : "+v"(hl));  // (nothing of this cold path is hoisted into the frame loop)
  double *d1 = d, *d2 = d + LN * U1, *out = d + LN * U1 + LN * U2;
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat64(k[i]);
#pragma unroll 1
  for (int j = hl; j < H1 && j < LN * U1; j += LN) {
    const WT *row = g + (long)j * 7;
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < 6 ? x[i] : 1.0; }, 7,
                              blas_kind(j, H1));
    d1[j] = sigmoid_f64(z);
  }
  wave_lds_sync();
  const int H1c = H1 < LN * U1 ? H1 : LN * U1, H2c = H2 < LN * U2 ? H2 : LN * U2;
  const WT *w2 = g + (long)H1 * 7;
#pragma unroll 1
  for (int j = hl; j < H2c; j += LN) {
    const WT *row = w2 + (long)j * (H1 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H1c ? d1[i] : 1.0; },
                              H1c + 1, blas_kind(j, H2));
    d2[j] = sigmoid_f64(z);
  }
  wave_lds_sync();
  if (hl < O) {
    const WT *row = w2 + (long)H2 * (H1 + 1) + (long)hl * (H2 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H2c ? d2[i] : 1.0; },
                              H2c + 1, blas_kind(hl, O));
    out[hl] = sigmoid_f64(z);
  }
  wave_lds_sync();
  int best = 0;  // np.argmax: the first NaN if any, else the first maximum
#pragma unroll
  for (int o = 1; o < O; ++o)
    if (!__builtin_isnan(out[best]) && (__builtin_isnan(out[o]) || out[o] > out[best])) best = o;
  wave_lds_sync();
  return best;
}

// the first maximum of z: the output every rule of the cascade proves or rejects
template <int O>
__device__ __forceinline__ int sig2_first_max(const float z[O]) {
  int w = 0;
  float top = z[0];
#pragma unroll
  for (int o = 1; o < O; ++o) {
    const bool gt = z[o] > top;
    w = gt ? o : w;
    top = gt ? z[o] : top;
  }
  return w;
}

// One decision of a half-group: z^ (returned in z) and the cascade.  stage: 0
// certify_c (lane 0 of the half-group decides, every lane acts on that one
// index), 1 tight_gap_move, 2 plateau_f32, 3 the f64 forward.  live = false
// (the idle left half of a game against a scripted opponent): index 0, stage 0.
template <int LN, int U1, int U2, int O, typename WT>
__device__ __forceinline__ int sig2_decide(const Sig2Net<LN, U1, U2, O> &sn, const WT *__restrict__ g, int H1, int H2,
                                           const int k[6], bool live, Relu2Lds<LN, U1, U2> &lds, int hl, float z[O],
                                           int &stage) {
  sig2_z32<LN, U1, U2, O>(sn.n, k, lds.h, hl, z);
  int idx = half_broadcast<LN>(certify_c<O>(z, sn.ct));
  const bool need = live && idx < 0;  // uniform over the half-group
  stage = 0;
  if (PG_ANY(need) && need) {
    // the in-register rules (pg_cascade.hpp): tight_gap_move proves the f32 winner
    // (it returns that output's move; the index is the first maximum it took)
    int r = tight_gap_move<O>(z, sn.n.e, sn.ct) != -1 ? sig2_first_max<O>(z) : -1;
    stage = 1;
    if (r < 0) {
      r = plateau_f32<O>(z, sn.n.e);
      stage = 2;
    }
    r = half_broadcast<LN>(r);
    stage = half_broadcast<LN>(stage);
    if (r < 0) {
      r = sig2_f64_half<LN, U1, U2, O, WT>(g, H1, H2, k, lds.d, hl);
      stage = 3;
    }
    idx = r;
  }
  return idx < 0 ? 0 : idx;
}

// pg_sig2_decide's parameters (k_sig2_decide) are k_relu2_decide's: Relu2DecideParams

}  // namespace pg
