// pg_block2.hpp -- the block-per-game layout of k_relu2_block
// (pg_relu2_block.hip) and k_sig2_block (pg_sig2_block.hip): the certified f32
// forward of a [6, H1 <= 128, H2 <= 128, 2..4] network with bias held by a
// 256-thread block, with ReLU or the sigmoid in both hidden layers, its f64
// re-decision in numpy's order, and the two families' shared host side.
// DESIGN.md 4.2k, 4.2l.  pg_hidden2.hpp is the same for the lane layout.
// The two kernels' own bodies -- the game loop and the decide pass -- stand in
// each family's file: moved into a device function that both call, they
// compile to other code for all 12 k_relu2_block symbols.
//
// Layout.  Threads 0..127 (waves 0-1) hold the right paddle's network (the
// genome), threads 128..255 (waves 2-3) the left paddle's (a hall-of-fame row;
// idle against the scripted opponents and the ROM CPU: they skip the forward
// and only keep the barriers).  Thread hl = tid & 127 of a network holds, as
// f32 in VGPRs for the whole game, layer-1 unit hl (7 weights), layer-2 unit hl
// (its whole W2 row: 128 padded weights and the bias) and that unit's O output
// weights.  A padding unit (hl >= H1 or hl >= H2) and a padding column
// (j >= H1) have exact zero weights (block_load); what that means for each
// activation is in the family's file.  Every thread steps the same Pong state
// (pg_device.hpp); thread 0 writes the results and the trace.
//
// A frame.  feat32; the 6-fma chain of unit hl onto its bias weight; the
// activation; it goes to the network's LDS row; barrier A; 32 float4 broadcast
// reads of the row with 128 fmas onto the layer-2 bias, in ascending j; the
// activation; the O products W3_o,hl h2_hl, each summed over the wave's 64 lanes
// by group_sum<64> (six butterfly steps, every lane the same total) and written
// by the wave's lane 0 to LDS; barrier B; every thread then forms both
// networks' z^_o = (wave 0's sum + wave 1's sum) + b3_o -- in that order --
// from LDS, and takes both decisions itself under the networks' bounds, also
// in LDS: all 256 threads hold the same two action codes with no further
// exchange.  That is the order the bound headers' block chain lengths bound and
// tests/_relu2_model.py and tests/_sig2_block_model.py restate.
//
// A family F describes what differs between the two kernels below their
// decision, which each kernel's body states itself:
//   kActivation      PG_ACT_RELU or PG_ACT_SIGMOID: both hidden layers' (and
//                    the f64 path's outputs') activation
//   Sums, init, unit1, kOther   the bound header's sums over a thread's
//                    layer-2 unit and the field that is the header's own
//                    beside B (block_load itself calls the header's unit2 and
//                    finish under its block layout, by kActivation)
//   Lds              the block's __shared__ struct: the fields below and what
//                    publish writes beside e
//   publish(lds, net, e)   the hl == 0 thread's: the network's bound, and the
//                    constants the decide step takes from it, into LDS
//
// Barriers.  Every __syncthreads() is reached under conditions formed from
// block-uniform values only, each passed through readfirstlane so that the
// branch is a scalar one: the game index thread 0 broadcast through LDS, the
// shared game state (vis, the end of the game), the decisions every thread
// read from LDS (the families' need masks).  block_load, block_z32 and
// block_f64 are entered by the whole block; inside them only work without a
// barrier is under a per-network (wave-uniform) or per-thread condition.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_cascade.hpp"
#include "pg_certgame.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_hidden2.hpp"
#include "pg_relu.hpp"

namespace pg {

constexpr int kBlockH = 128;  // threads per network, padded units per hidden layer
static_assert(PG_RELU2_BLOCK_MAX_H == kBlockH && PG_SIG2_BLOCK_MAX_H == kBlockH, "one layout for both families");
// z^_o = (group_sum<64>(w3 h2) of wave 0 + that of wave 1) + b3_o
constexpr int kBlockChain1 = 1 + 2 + 6;        // gene, feat32, block_z32's 6 fmas
constexpr int kBlockChain2 = 1 + kBlockH;      // gene, one fma per padded unit
constexpr int kBlockChain3 = 1 + 1 + relu_log2(64) + 1 + 1;  // gene, product, group_sum<64>'s steps, the two waves, the bias

template <int O>
struct BlockNet {
  float w1[7];        // layer-1 unit hl: 6 input weights + bias weight
  float w2[kBlockH];  // layer-2 unit hl: its weight of every (padded) layer-1 unit
  float b2;
  float w3[O];        // output weights of that unit
};

// The fields every family's Lds has.  n: 0 the right paddle's network, 1 the left paddle's.
//   float h[2][kBlockH]            the f32 all-gather rows
//   float part[4][4]               [wave][o]: the wave's sum of the O products
//   float c[2][4]                  [n][o]: output biases
//   float e[2]                     [n]: |z^_o - z64_o| <= e (the bound header); inf: always f64
//   int game                       the game thread 0 took
//   double d[2][2 * kBlockH + 4]   [n]: the f64 path's activations (layer 1, layer 2, outputs); the load's A_j
//   double red[4][3 * 4 + 3]       [wave]: the load's sums of the bound

// This thread's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last) as f32
// -- exact zeros for every padding unit's row and column -- and the network's
// bound and output biases into LDS, from the f64 genes.  Entered by the whole
// block; live (wave-uniform): this thread's network plays.  H1, H2 <= kBlockH
// (host-checked).
template <class F, int O, typename WT>
__device__ __forceinline__ void block_load(BlockNet<O> &n, const WT *__restrict__ g, int H1, int H2,
                                           typename F::Lds &lds, int wv, int hl, bool live) {
  static_assert(O <= PG_RELU_MAX_OUT && O <= PG_SIG2_MAX_OUT, "the bound's sums");
  // hl, H1 and H2 made opaque, as in hidden2_load: the unit offsets and the 128 padding tests j < H1
  // would otherwise be hoisted out of the game loop and kept live across every frame
  asm volatile("" : "+v"(hl));
  asm volatile("" : "+s"(H1), "+s"(H2));
  const int net = wv >> 1;
  const long off2 = (long)H1 * 7, off3 = off2 + (long)H2 * (H1 + 1);
  double asum = 0.0;
  if (live) {
    const bool ok = hl < H1;
    const WT *row = g + (long)(ok ? hl : 0) * 7;  // padding units load a valid row and are zeroed
    double w[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const WT raw = row[i];
      w[i] = ok ? (double)raw : 0.0;
      n.w1[i] = (float)w[i];
    }
    asum = F::unit1(w);
    lds.d[net][hl] = asum;
  }
  __syncthreads();  // the A_j of both networks
  typename F::Sums s;
  F::init(s);
  if (live) {
    const bool ok = hl < H2;
    const WT *row = g + off2 + (long)(ok ? hl : 0) * (H1 + 1);
    double p = 0.0, wsum = 0.0;
#pragma unroll
    for (int j = 0; j < kBlockH; ++j) {
      const bool inj = j < H1;
      const WT raw = row[inj ? j : 0];
      const double w = (ok && inj) ? (double)raw : 0.0;  // a padding unit's outgoing weight: exactly zero
      n.w2[j] = (float)w;
      p += fabs(w) * lds.d[net][j];  // (a padding unit j >= H1 wrote A_j = 0)
      wsum += fabs(w);
      if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // eight loads in flight at a time: not the kernel's register budget
    }
    const WT rawb = row[H1];
    const double bias = ok ? (double)rawb : 0.0;
    n.b2 = (float)bias;
    double w3[O];
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const WT raw = g[off3 + (long)o * (H2 + 1) + (ok ? hl : 0)];
      w3[o] = ok ? (double)raw : 0.0;  // (the same for a padding layer-2 unit)
      n.w3[o] = (float)w3[o];
    }
    // (the bound headers' unit2 and finish are called from here, not through F: one more level of
    // inlining around their loops over o changes the code of all six k_relu2_block instances)
    if constexpr (F::kActivation == PG_ACT_RELU) pg_relu2_sums_unit2(&s, p + fabs(bias), wsum, w3, O);
    else pg_sig2_sums_unit2_l(pg_sig2_layout_block(), &s, p, wsum, bias, w3, O);
  }
  // the sums over the network's 128 threads: over each wave, then its two waves in order (sums of
  // non-negative f64 terms: any order is within 2^-40, the bound headers)
  double v[3 * O + 3];
#pragma unroll
  for (int o = 0; o < O; ++o) {
    v[3 * o] = s.S[o];
    v[3 * o + 1] = s.T[o];
    v[3 * o + 2] = s.W3[o];
  }
  v[3 * O] = s.B;
  v[3 * O + 1] = s.*F::kOther;
  v[3 * O + 2] = asum;
#pragma unroll
  for (int i = 0; i < 3 * O + 3; ++i) {
    v[i] = half_sum_f64<64>(v[i]);
    if ((threadIdx.x & 63) == 0) lds.red[wv][i] = v[i];
  }
  __syncthreads();
  if (hl == 0) {  // one thread per network: its bound and output biases, for every thread of the block
    float e = __builtin_inff();
    float cf[O];
#pragma unroll
    for (int o = 0; o < O; ++o) cf[o] = 0.f;
    if (live) {
      const double *r0 = lds.red[2 * net], *r1 = lds.red[2 * net + 1];
      typename F::Sums t;
      F::init(t);
      double c[O];
#pragma unroll
      for (int o = 0; o < O; ++o) {
        t.S[o] = r0[3 * o] + r1[3 * o];
        t.T[o] = r0[3 * o + 1] + r1[3 * o + 1];
        t.W3[o] = r0[3 * o + 2] + r1[3 * o + 2];
        c[o] = (double)g[off3 + (long)o * (H2 + 1) + H2];
        cf[o] = (float)c[o];
      }
      t.B = r0[3 * O] + r1[3 * O];
      t.*F::kOther = r0[3 * O + 1] + r1[3 * O + 1];
      if constexpr (F::kActivation == PG_ACT_RELU)
        e = pg_relu2_bound_finish(pg_relu2_layout_block(), &t, r0[3 * O + 2] + r1[3 * O + 2], c, O);
      else e = pg_sig2_bound_finish_l(pg_sig2_layout_block(), &t, r0[3 * O + 2] + r1[3 * O + 2], c, O);
    }
    F::publish(lds, net, e);
#pragma unroll
    for (int o = 0; o < O; ++o) lds.c[net][o] = cf[o];
  }
  __syncthreads();  // e and c are in place; the A_j are read: lds.d is free for the f64 path
}

// One frame's f32 chain of the live networks on the doubled-centroid features
// k (this thread's network's), up to the waves' sums in lds.part.  Entered by
// the whole block.
template <class F, int O>
__device__ __forceinline__ void block_z32(const BlockNet<O> &n, const int k[6], typename F::Lds &lds, int wv, int hl,
                                          bool live) {
  const int net = wv >> 1;
  if (live) {
    float a = n.w1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) a = fmaf(n.w1[i], feat32(k[i]), a);
    lds.h[net][hl] = hidden2_act32<F::kActivation>(a);
  }
  __syncthreads();  // barrier A: the rows
  if (live) {
    float a2 = n.b2;
    const float *hrow = lds.h[net];
    // eight float4 reads in flight, then their 32 fmas: left to the scheduler, every read but the
    // first four is waited for on its own (28 exposed LDS latencies a frame)
    constexpr int kBatch = 8;
#pragma unroll
    for (int j0 = 0; j0 < kBlockH; j0 += 4 * kBatch) {
      float4 h[kBatch];
#pragma unroll
      for (int b = 0; b < kBatch; ++b) h[b] = *(const float4 *)(hrow + j0 + 4 * b);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int b = 0; b < kBatch; ++b) {
        const int j = j0 + 4 * b;
        a2 = fmaf(n.w2[j], h[b].x, a2);
        a2 = fmaf(n.w2[j + 1], h[b].y, a2);
        a2 = fmaf(n.w2[j + 2], h[b].z, a2);
        a2 = fmaf(n.w2[j + 3], h[b].w, a2);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const float h2 = hidden2_act32<F::kActivation>(a2);
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const float t = group_sum<64>(n.w3[o] * h2);
      if ((threadIdx.x & 63) == 0) lds.part[wv][o] = t;
    }
  }
  __syncthreads();  // barrier B: the waves' sums
}

// network n's z^ from the waves' sums
template <int O, class Lds>
__device__ __forceinline__ void block_z_out(const Lds &lds, int n, float z[O]) {
#pragma unroll
  for (int o = 0; o < O; ++o) z[o] = (lds.part[2 * n][o] + lds.part[2 * n + 1][o]) + lds.c[n][o];
}

// The f64 forward of one pass for the networks of need (bit n: network n), as
// forward_f64_wave runs it (NeuralNetwork.run numpy_nn.py:120-137 in np.dot's
// order, blas_dot over [inputs..., 1] per unit): one unit per thread,
// activations through LDS, every thread takes the argmax of each network of
// need into idx[n].  Entered by the whole block; g, k: this thread's network's.
template <class F, int O, typename WT>
__device__ PG_SLOW_INLINE void block_f64(const WT *__restrict__ g, int H1, int H2, const int k[6], typename F::Lds &lds,
                                         int wv, int hl, int need, int idx[2]) {
  asm volatile("" : "+v"(hl));  // (as in block_load: nothing of this cold path is hoisted into the frame loop)
  const int net = wv >> 1;
  const bool mine = (need >> net) & 1;  // wave-uniform
  double *d1 = lds.d[net], *d2 = d1 + kBlockH, *out = d2 + kBlockH;
  const WT *w2 = g + (long)H1 * 7;
  if (mine && hl < H1) {
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = feat64(k[i]);
    const WT *row = g + (long)hl * 7;
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < 6 ? x[i] : 1.0; }, 7,
                              blas_kind(hl, H1));
    d1[hl] = hidden2_act64<F::kActivation>(z);
  }
  __syncthreads();
  if (mine && hl < H2) {
    const WT *row = w2 + (long)hl * (H1 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H1 ? d1[i] : 1.0; },
                              H1 + 1, blas_kind(hl, H2));
    d2[hl] = hidden2_act64<F::kActivation>(z);
  }
  __syncthreads();
  if (mine && hl < O) {
    const WT *row = w2 + (long)H2 * (H1 + 1) + (long)hl * (H2 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H2 ? d2[i] : 1.0; },
                              H2 + 1, blas_kind(hl, O));
    out[hl] = hidden2_act64<F::kActivation>(z);
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    if ((need >> n) & 1) {
      const double *o_n = lds.d[n] + 2 * kBlockH;
      int best = 0;  // np.argmax: the first NaN if any, else the first maximum
#pragma unroll
      for (int o = 1; o < O; ++o)
        if (!__builtin_isnan(o_n[best]) && (__builtin_isnan(o_n[o]) || o_n[o] > o_n[best])) best = o;
      idx[n] = best;
    }
  }
}

// ------------------------------------------------------------ host side ----
#define PG_BLOCK_DISPATCH(KERNEL, O, f64, grid, s, p)                                         \
  do {                                                                                        \
    if (O == 2) {                                                                             \
      if (f64) hipLaunchKernelGGL((KERNEL<2, double>), dim3(grid), dim3(256), 0, s, p);       \
      else hipLaunchKernelGGL((KERNEL<2, float>), dim3(grid), dim3(256), 0, s, p);            \
    } else if (O == 3) {                                                                      \
      if (f64) hipLaunchKernelGGL((KERNEL<3, double>), dim3(grid), dim3(256), 0, s, p);       \
      else hipLaunchKernelGGL((KERNEL<3, float>), dim3(grid), dim3(256), 0, s, p);            \
    } else {                                                                                  \
      if (f64) hipLaunchKernelGGL((KERNEL<4, double>), dim3(grid), dim3(256), 0, s, p);       \
      else hipLaunchKernelGGL((KERNEL<4, float>), dim3(grid), dim3(256), 0, s, p);            \
    }                                                                                         \
  } while (0)

// a persistent grid: two blocks per CU, at most one per game or pass
inline int block2_grid(int n) {
  const int cap = num_cus() * 2;
  return n < cap ? n : cap;
}

// What Relu2BlockFamily (pg_relu2_block.hip) and Sig2BlockFamily
// (pg_sig2_block.hip) share of a family's description (pg_family.hpp); each
// adds its kernel, its activation, its messages and the launches of its
// kernels.  No modifier bits: every frame is stepped, a block plays both paddles.
struct Block2Family {
  static constexpr bool kModifiers = false, kScopeOnEntry = true;
  using DecideParams = CertDecideParams;
  // the shapes [6, 2..128, 2..128, 2..4]
  static bool shape_ok(int n_nodes, const int32_t *nodes) {
    return n_nodes == 4 && nodes[0] == 6 && nodes[1] >= 2 && nodes[1] <= kBlockH && nodes[2] >= 2 &&
           nodes[2] <= kBlockH && nodes[3] >= 2 && nodes[3] <= 4;
  }
  static long genes(const int32_t *nd) { return (long)nd[1] * 7 + (long)nd[2] * (nd[1] + 1) + (long)nd[3] * (nd[2] + 1); }
  static int game_grid(const EvalParams &p) { return block2_grid(p.total); }
  static int decide_grid(const pg_relu_decide_args *a) { return block2_grid(a->n); }
  static DecideParams decide_params(const pg_relu_decide_args *a) {
    return cert_decide_params(a, a->net.nodes[1], a->net.nodes[2]);
  }
};

}  // namespace pg
