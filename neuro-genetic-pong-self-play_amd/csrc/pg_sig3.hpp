// pg_sig3.hpp -- device code of k_sig3 (pg_sig3.hip): the certified f32 forward
// of a [6, H1 <= 32, H2 <= 32, H3 <= 32, 2..4] sigmoid network with bias (the
// reference's default activation, numpy_nn.py:22-26) held by a half-group of LN
// lanes, its decision cascade and its f64 re-decision in numpy's order:
// k_relu3's layout (pg_hidden3.hpp: Hidden3Net, Hidden3Lds, the two LDS
// all-gather rows) with k_sig2's sigmoid, bound idiom and cascade
// (pg_hidden2.hpp, pg_cascade.hpp).  The bound's arithmetic and its derivation
// are in pg_sig3_bound.h (it also compiles for the host).
//
// The f32 chain and the f64 forward are pg_hidden3.hpp's, instantiated with the
// sigmoid (hidden3_z32<PG_ACT_SIGMOID>, hidden3_f64_half<PG_ACT_SIGMOID>:
// sigmoid_f64, numpy's np.e ** -z correctly rounded, in all four layers);
// sharing them changes no k_relu3 instance.  The load stands
// apart: this bound takes other sums of the weights than pg_relu3_bound.h's.
//
// Padding.  A padding unit (j >= H1, k >= H2 or l >= H3) and a padding input
// have zero weights.  A padding unit's activation is sigmoid_f32(0) = 0.5, not
// 0: correctness rests on its OUTGOING weights being exactly zero.  sig3_load
// writes 0.0f for every weight of a padding row, for every column j >= H1 of
// W2, every column k >= H2 of W3 and the W4 weights of every l >= H3, and
// fma(0, 0.5, a) = a leaves every sum and its error bound untouched.
//
// The decision is k_sig2's cascade on the output pre-activations z^ with
// |z^_o - znp_o| <= e (numpy's f64 pre-activations): certify_c under the
// game's make_cert(e); for an undecided half-group tight_gap_move, then
// plateau_f32; then the f64 forward from the genes in np.dot's order with the
// correctly rounded sigmoid_f64 in all four layers and np.argmax's rule.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_cascade.hpp"
#include "pg_certgame.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_hidden2.hpp"  // half_broadcast, sig2_first_max
#include "pg_hidden3.hpp"  // the layout: Hidden3Net, Hidden3Lds, Hidden3Dims, hidden3_lanes, PG_HIDDEN3_DISPATCH
#include "pg_relu.hpp"
#include "pg_sig3_bound.h"

namespace pg {

static_assert(PG_SIG3_MAX_H == kHidden3MaxH, "the bound's arrays");

// k_sig3's: the weights and bound, and certify_c's constants of that bound
template <int LN, int U, int O>
struct Sig3Net : Hidden3Net<LN, U, O> {
  Cert ct;
};

// This lane's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [H3, H2 + 1], W4 [O, H3 + 1], bias
// columns last) as f32 -- exact zeros for every padding unit's row and column,
// see above -- and the network's bound from the f64 genes.  H1, H2, H3 <= LN U
// (host-checked).
template <int LN, int U, int O, typename WT>
__device__ __forceinline__ void sig3_load(Sig3Net<LN, U, O> &n, const WT *__restrict__ g, int H1, int H2, int H3,
                                          Hidden3Lds<LN, U> &lds, int hl) {
  static_assert(LN * U <= PG_SIG3_MAX_H, "pg_sig3_bound_genome, the LDS rows, the underflow term's unit counts");
  static_assert(PG_SIG3_CHAIN1 == 1 + 2 + 6, "the bound's layer-1 chain: gene, feat32, hidden3_z32's 6 fmas");
  static_assert(1 + LN * U <= PG_SIG3_CHAIN2, "the bound's layer-2 chain");
  static_assert(1 + LN * U <= PG_SIG3_CHAIN3, "the bound's layer-3 chain");
  static_assert(1 + U + relu_log2(LN) + 1 <= PG_SIG3_CHAIN4, "the bound's layer-4 chain");
  static_assert(2 * LN * U + (LN - 1) + 2 <= PG_SIG3_UNDER_C, "the underflow term's count of layer-4 operations");
  static_assert(O <= PG_SIG2_MAX_OUT, "the bound's sums");
  // hl and the widths made opaque: the unit offsets and masks below would otherwise be
  // hoisted out of the game loop as loop-invariant registers kept live across every frame
  asm volatile("" : "+v"(hl));
  asm volatile("" : "+s"(H1), "+s"(H2), "+s"(H3));
  constexpr int N = LN * U;
  const long off2 = (long)H1 * 7, off3 = off2 + (long)H2 * (H1 + 1), off4 = off3 + (long)H3 * (H2 + 1);
  double *dA = lds.d, *dX = lds.d + N, *dV = lds.d + 2 * N;
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
    const double a = pg_sig2_unit1(w);
    dA[j] = a;
    asum += a;
    __builtin_amdgcn_sched_barrier(0);  // one unit's loads in flight at a time (see relu_load)
  }
  asum = half_sum_f64<LN>(asum);
  wave_lds_sync();
  pg_sig3_sums s;
  pg_sig3_sums_init(&s);
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
      // a padding unit's outgoing weight: exactly zero (its activation is 0.5, and fma(0, 0.5, a) = a)
      const double w = okj ? (double)raw : 0.0;
      relu_set(n.w2[v][j], (float)w);
      p += fabs(w) * (j < H1 ? dA[j] : 0.0);
      wsum += fabs(w);
      if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
    }
    const WT rawb = row[H1];
    const double bias = ok ? (double)rawb : 0.0;
    relu_set(n.b2[v], (float)bias);
    // (a padding unit: p = w = bias = 0; its Q2_k / 4 + 4.5 + c3 is met by zero W3 weights only)
    dX[k] = pg_sig3_sums_unit2(&s, p, wsum, bias);
    dV[k] = wsum;
    __builtin_amdgcn_sched_barrier(0);
  }
  wave_lds_sync();
#pragma unroll
  for (int v = 0; v < U; ++v) {
    const int l = hl * U + v;
    const bool ok = l < H3;
    const WT *row = g + off3 + (long)(ok ? l : 0) * (H2 + 1);
    double x = 0.0, t = 0.0, wsum = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool okk = ok && k < H2;
      const WT raw = row[k < H2 ? k : 0];
      const double w = okk ? (double)raw : 0.0;  // (the same: zero for a padding layer-2 unit's column)
      relu_set(n.w3[v][k], (float)w);
      x += fabs(w) * (k < H2 ? dX[k] : 0.0);
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
    pg_sig3_sums_unit3(&s, x, t, wsum, bias, w4, O);
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
  s.P = half_sum_f64<LN>(s.P);
  s.Q3 = half_sum_f64<LN>(s.Q3);
  // one lane's bound for the whole half-group: every lane certifies under the same e
  const float e = __int_as_float(half_broadcast<LN>(__float_as_int(pg_sig3_bound_finish(&s, asum, c, O))));
  const Cert ct = make_cert(e);
  relu_set(n.e, e);
  relu_set(n.ct.tlo, ct.tlo);
  relu_set(n.ct.thi, ct.thi);
  relu_set(n.ct.lowz, ct.lowz);
  relu_set(n.ct.e2, ct.e2);
  relu_set(n.ct.ee, ct.ee);
  wave_lds_sync();  // the Q2_k's and V2_k are read: lds.d is free for the f64 path
}

// k_sig3's policy (pg_certgame.hpp): Sig2Policy's cascade on Relu3Policy's
// layout and dims.  live = false (the idle left half of a game against a
// scripted opponent): index 0, stage 0, never the f64 path.
template <int LN_, int U, int O_, typename WT_>
struct Sig3Policy {
  static constexpr int LN = LN_, O = O_, kF64Stage = 3;
  using WT = WT_;
  using Net = Sig3Net<LN, U, O>;
  using Lds = Hidden3Lds<LN, U>;
  using Dims = Hidden3Dims;
  static __device__ __forceinline__ Dims dims(const EvalParams &p) { return {p.nodes[1], p.nodes[2], p.nodes[3]}; }
  static __device__ __forceinline__ Dims dims(const Hidden3DecideParams &p) { return {p.H1, p.H2, p.H3}; }
  static __device__ __forceinline__ void load(Net &net, const WT *g, const Dims &dims, Lds &lds, int hl) {
    sig3_load<LN, U, O, WT>(net, g, dims.H1, dims.H2, dims.H3, lds, hl);
  }
  // the cascade.  stage: 0 certify_c (lane 0 of the half-group decides, every
  // lane acts on that one index), 1 tight_gap_move, 2 plateau_f32, 3 the f64 forward
  static __device__ __forceinline__ int decide(const Net &n, const WT *__restrict__ g, const Dims &dims, const int k[6],
                                               bool live, Lds &lds, int hl, float z[O], int &stage) {
    hidden3_z32<PG_ACT_SIGMOID, LN, U, O>(n, k, lds.h1, lds.h2, hl, z);
    int idx = half_broadcast<LN>(certify_c<O>(z, n.ct));
    const bool need = live && idx < 0;  // uniform over the half-group
    stage = 0;
    if (PG_ANY(need) && need) {
      // the in-register rules (pg_cascade.hpp): tight_gap_move proves the f32 winner
      // (it returns that output's move; the index is the first maximum it took)
      int r = tight_gap_move<O>(z, n.e, n.ct) != -1 ? sig2_first_max<O>(z) : -1;
      stage = 1;
      if (r < 0) {
        r = plateau_f32<O>(z, n.e);
        stage = 2;
      }
      r = half_broadcast<LN>(r);
      stage = half_broadcast<LN>(stage);
      if (r < 0) {
        r = hidden3_f64_half<PG_ACT_SIGMOID, LN, U, O, WT>(g, dims.H1, dims.H2, dims.H3, k, lds.d, hl);
        stage = 3;
      }
      idx = r;
    }
    return idx < 0 ? 0 : idx;
  }
};

}  // namespace pg
