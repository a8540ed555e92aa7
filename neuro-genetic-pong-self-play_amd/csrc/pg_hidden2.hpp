// pg_hidden2.hpp -- device code of k_relu2 (pg_relu2.hip) and k_sig2
// (pg_sig2.hip): the certified f32 forward of a [6, H1 <= 64, H2 <= 64, 2..4]
// network with bias held by a half-group of LN lanes, with ReLU
// (activation_function = ReLU, numpy_nn.py:6-9, 26) or the sigmoid
// (numpy_nn.py:22-26) in both hidden layers, its decision and its f64
// re-decision in numpy's order; and the two families' shared host side.  The
// bounds' arithmetic and their derivations are in pg_relu2_bound.h (under its
// lane layout here; k_relu2_block, pg_relu2_block.hip, is its block layout) and
// pg_sig2_bound.h (they also compile for the host).
//
// Lane hl of a half-group holds layer-1 units hl U1 .. hl U1 + U1 - 1 (7
// weights each), layer-2 units hl U2 .. hl U2 + U2 - 1 (a whole row of W2 each:
// LN U1 weights and the bias) and those units' O output weights, all as f32 in
// VGPRs for the whole game.  Each frame the lanes write their layer-1
// activations to the half-group's LDS row (an all-gather: LN U1 floats), every
// lane reads them all back for its layer-2 rows, and the outputs are summed
// over the lanes as k_relu's are.
//
// Padding.  A padding unit (j >= H1 or k >= H2) and a padding input have zero
// weights.  Under ReLU max(0, 0) = 0 times 0 contributes exactly 0.  Under the
// sigmoid a padding unit's activation is sigmoid_f32(0) = 0.5, not 0:
// correctness rests on its OUTGOING weights being exactly zero.  hidden2_load
// writes 0.0f for every weight of a padding row and for every column j >= H1
// of W2, and fma(0, 0.5, a) = a leaves every sum and its error bound untouched.
//
// The decisions.  ReLU: k_relu's (pg_relu.hpp): with |z^_o - z64_o| <= e and
// t1 >= t2 the two largest z^, the index is 0 if t1 <= -e, that of t1 if
// t1 > e and t1 - t2 > 2e, and is otherwise recomputed in f64 from the genes.
// Sigmoid: k_service's cascade on the output pre-activations z^ with
// |z^_o - znp_o| <= e (numpy's f64 pre-activations): certify_c under the
// game's make_cert(e); for an undecided half-group tight_gap_move, then
// plateau_f32; then the f64 forward from the genes in np.dot's order with the
// correctly rounded sigmoid_f64 in all three layers and np.argmax's rule.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_cascade.hpp"
#include "pg_certgame.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_relu.hpp"
#include "pg_relu2_bound.h"
#include "pg_sig2_bound.h"

namespace pg {

constexpr int kHidden2MaxH = 64;
static_assert(PG_RELU2_MAX_H == kHidden2MaxH && PG_SIG2_MAX_H == kHidden2MaxH, "one layout for both families");
// the instances: lanes per network and units per lane (both layers) by the
// wider hidden layer -- 16 x 16 on 4 lanes (8 games a wave), 32 x 32 on 16
// (2 games), 64 x 64 on 32 (1 game)
__host__ __device__ constexpr int hidden2_lanes(int H1, int H2) {
  return (H1 > H2 ? H1 : H2) <= 16 ? 4 : ((H1 > H2 ? H1 : H2) <= 32 ? 16 : 32);
}
__host__ __device__ constexpr int hidden2_units(int LN) { return LN == 4 ? 4 : 2; }

template <int LN, int U1, int U2, int O>
struct Hidden2Net {
  float w1[U1][7];        // layer-1 unit hl U1 + u: 6 input weights + bias weight
  float w2[U2][LN * U1];  // layer-2 unit hl U2 + v: its weight of every (padded) layer-1 unit
  float b2[U2];
  float w3[U2][O];        // output weights of that unit
  float c[O];             // output biases
  float e;                // |z^_o - z64_o| <= e for every output (pg_*2_bound.h); inf: always f64
};

// k_sig2's: the weights and bound, and certify_c's constants of that bound
template <int LN, int U1, int U2, int O>
struct Sig2Net : Hidden2Net<LN, U1, U2, O> {
  Cert ct;
};

// LDS of one half-group: the f32 all-gather row, and the f64 path's
// activations (also the load's A_j): LN U1 + LN U2 hidden + O outputs
template <int LN, int U1, int U2>
struct alignas(16) Hidden2Lds {
  float h[LN * U1];
  double d[LN * U1 + LN * U2 + 4];
};

// value of lane (hl = 0) of this lane's half-group
template <int LN>
__device__ __forceinline__ int half_broadcast(int v) {
  return __shfl(v, (int)(threadIdx.x & 63 & ~(LN - 1)), 64);
}

// The activation of both hidden layers (and of the f64 path's outputs), a
// compile-time choice as k_wide's is (ACT, a pg_activation).
template <int ACT>
__device__ __forceinline__ float hidden2_act32(float a) {
  if constexpr (ACT == PG_ACT_RELU) return fmaxf(a, 0.f);
  else return sigmoid_f32(a);  // (a padding unit: 0.5, met by zero weights only)
}
template <int ACT>
__device__ __forceinline__ double hidden2_act64(double z) {
  if constexpr (ACT == PG_ACT_RELU) return relu_f64(z);
  else return sigmoid_f64(z);  // numpy's: np.e ** -z correctly rounded
}

// What hidden2_load needs of a bound header: its sums over a lane's layer-2
// units (p = sum_j |W2_kj| A_j and w = sum_j |W2_kj| of a row), the half-group
// reduction of the fields that are its own (S, T and W3 are common), and the
// network's constants of the finished bound.  (O is a template parameter of
// unit2 and finish: as an argument it is no constant while the header's
// functions are inlined into these, and their loops over o come out otherwise.)
struct Relu2Bound {
  using Sums = pg_relu2_sums;
  static constexpr int kMaxH = PG_RELU2_MAX_H, kMaxOut = PG_RELU_MAX_OUT;
  static constexpr int kChain1 = PG_RELU2_CHAIN1, kChain2 = PG_RELU2_CHAIN2, kChain3 = PG_RELU2_CHAIN3;
  static __device__ __forceinline__ void init(Sums &s) { pg_relu2_sums_init(&s); }
  static __device__ __forceinline__ double unit1(const double w[7]) { return pg_relu2_unit1(w); }
  template <int O>
  static __device__ __forceinline__ void unit2(Sums &s, double p, double w, double bias, const double *w3) {
    pg_relu2_sums_unit2(&s, p + fabs(bias), w, w3, O);
  }
  template <int LN>
  static __device__ __forceinline__ void reduce(Sums &s) {
    s.B = half_sum_f64<LN>(s.B);
    s.W2 = half_sum_f64<LN>(s.W2);
  }
  template <int O>
  static __device__ __forceinline__ float finish(const Sums &s, double asum, const double *c) {
    return pg_relu2_bound_finish(pg_relu2_layout_lanes(), &s, asum, c, O);
  }
  template <class Net>
  static __device__ __forceinline__ void set(Net &n, float e) {
    relu_set(n.e, e);
  }
};

struct Sig2Bound {
  using Sums = pg_sig2_sums;
  static constexpr int kMaxH = PG_SIG2_MAX_H, kMaxOut = PG_SIG2_MAX_OUT;
  static constexpr int kChain1 = PG_SIG2_CHAIN1, kChain2 = PG_SIG2_CHAIN2, kChain3 = PG_SIG2_CHAIN3;
  static __device__ __forceinline__ void init(Sums &s) { pg_sig2_sums_init(&s); }
  static __device__ __forceinline__ double unit1(const double w[7]) { return pg_sig2_unit1(w); }
  template <int O>
  static __device__ __forceinline__ void unit2(Sums &s, double p, double w, double bias, const double *w3) {
    pg_sig2_sums_unit2_l(pg_sig2_layout_lanes(), &s, p, w, bias, w3, O);
  }
  template <int LN>
  static __device__ __forceinline__ void reduce(Sums &s) {
    s.B = half_sum_f64<LN>(s.B);
    s.P = half_sum_f64<LN>(s.P);
  }
  template <int O>
  static __device__ __forceinline__ float finish(const Sums &s, double asum, const double *c) {
    return pg_sig2_bound_finish_l(pg_sig2_layout_lanes(), &s, asum, c, O);
  }
  template <class Net>
  static __device__ __forceinline__ void set(Net &n, float e) {
    const Cert ct = make_cert(e);
    relu_set(n.e, e);
    relu_set(n.ct.tlo, ct.tlo);
    relu_set(n.ct.thi, ct.thi);
    relu_set(n.ct.lowz, ct.lowz);
    relu_set(n.ct.e2, ct.e2);
    relu_set(n.ct.ee, ct.ee);
  }
};

// This lane's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last) as
// f32 -- exact zeros for every padding unit's row and column, see above -- and
// the network's bound from the f64 genes.  H1 <= LN U1, H2 <= LN U2
// (host-checked).
template <class Bound, int LN, int U1, int U2, int O, typename WT, class Net>
__device__ __forceinline__ void hidden2_load(Net &n, const WT *__restrict__ g, int H1, int H2,
                                             Hidden2Lds<LN, U1, U2> &lds, int hl) {
  static_assert(LN * U1 <= Bound::kMaxH && LN * U2 <= Bound::kMaxH,
                "pg_*2_bound_genome, the LDS rows, the underflow term's unit counts");
  static_assert(Bound::kChain1 == 1 + 2 + 6, "the bound's layer-1 chain: gene, feat32, hidden2_z32's 6 fmas");
  static_assert(1 + LN * U1 <= Bound::kChain2, "the bound's layer-2 chain");
  static_assert(1 + U2 + relu_log2(LN) + 1 <= Bound::kChain3, "the bound's layer-3 chain");
  static_assert(O <= Bound::kMaxOut, "the bound's sums");
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
    const double a = Bound::unit1(w);
    lds.d[j] = a;
    asum += a;
    __builtin_amdgcn_sched_barrier(0);  // one unit's loads in flight at a time (see relu_load)
  }
  asum = half_sum_f64<LN>(asum);
  wave_lds_sync();
  typename Bound::Sums s;
  Bound::init(s);
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
    Bound::template unit2<O>(s, p, wsum, bias, w3);
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
  Bound::template reduce<LN>(s);
  // one lane's bound for the whole half-group: every lane certifies under the same e
  const float e = __int_as_float(half_broadcast<LN>(__float_as_int(Bound::template finish<O>(s, asum, c))));
  Bound::set(n, e);
  wave_lds_sync();  // the A_j are read: lds.d is free for the f64 path
}

// The f32 output pre-activations z^ on the doubled-centroid features k, with
// the chain lengths the bound headers bound; every lane of the half-group gets
// the bitwise-identical values (group_sum).
template <int ACT, int LN, int U1, int U2, int O>
__device__ __forceinline__ void hidden2_z32(const Hidden2Net<LN, U1, U2, O> &n, const int k[6], float *hrow, int hl,
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
    h1[u] = hidden2_act32<ACT>(a);
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
    const float h2 = hidden2_act32<ACT>(a2[v]);
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
// argmax.  d: the half-group's Hidden2Lds::d.
template <int ACT, int LN, int U1, int U2, int O, typename WT>
__device__ PG_SLOW_INLINE int hidden2_f64_half(const WT *__restrict__ g, int H1, int H2, const int k[6], double *d,
                                               int hl) {
  static_assert(O <= LN, "lane o sums output o");
  asm volatile("" : "+v"(hl));  // (as in hidden2_load: nothing of this cold path is hoisted into the frame loop)
  double *d1 = d, *d2 = d + LN * U1, *out = d + LN * U1 + LN * U2;
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat64(k[i]);
#pragma unroll 1
  for (int j = hl; j < H1 && j < LN * U1; j += LN) {
    const WT *row = g + (long)j * 7;
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < 6 ? x[i] : 1.0; }, 7,
                              blas_kind(j, H1));
    d1[j] = hidden2_act64<ACT>(z);
  }
  wave_lds_sync();
  const int H1c = H1 < LN * U1 ? H1 : LN * U1, H2c = H2 < LN * U2 ? H2 : LN * U2;
  const WT *w2 = g + (long)H1 * 7;
#pragma unroll 1
  for (int j = hl; j < H2c; j += LN) {
    const WT *row = w2 + (long)j * (H1 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H1c ? d1[i] : 1.0; },
                              H1c + 1, blas_kind(j, H2));
    d2[j] = hidden2_act64<ACT>(z);
  }
  wave_lds_sync();
  if (hl < O) {
    const WT *row = w2 + (long)H2 * (H1 + 1) + (long)hl * (H2 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H2c ? d2[i] : 1.0; },
                              H2c + 1, blas_kind(hl, O));
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

// The policies of k_relu2 and k_sig2 (pg_certgame.hpp).  decide: one decision
// of a half-group, z^ returned in z.  live = false (the idle left half of a
// game against a scripted opponent): index 0, stage 0, never the f64 path.
template <int LN_, int U1, int U2, int O_, typename WT_>
struct Relu2Policy {
  static constexpr int LN = LN_, O = O_, kF64Stage = 1;
  using WT = WT_;
  using Net = Hidden2Net<LN, U1, U2, O>;
  using Lds = Hidden2Lds<LN, U1, U2>;
  static __device__ __forceinline__ void load(Net &net, const WT *g, const CertDims &dims, Lds &lds, int hl) {
    hidden2_load<Relu2Bound, LN, U1, U2, O, WT>(net, g, dims.H1, dims.H2, lds, hl);
  }
  // the certificate as lane 0 of the half-group takes it (every lane acts on
  // that one index), else the f64 forward (stage 1)
  static __device__ __forceinline__ int decide(const Net &n, const WT *__restrict__ g, const CertDims &dims,
                                               const int k[6], bool live, Lds &lds, int hl, float z[O], int &stage) {
    hidden2_z32<PG_ACT_RELU, LN, U1, U2, O>(n, k, lds.h, hl, z);
    int idx = half_broadcast<LN>(relu_certify<O>(z, n.e));
    const bool need = live && idx < 0;
    stage = need ? 1 : 0;
    if (PG_ANY(need) && need) idx = hidden2_f64_half<PG_ACT_RELU, LN, U1, U2, O, WT>(g, dims.H1, dims.H2, k, lds.d, hl);
    return idx < 0 ? 0 : idx;
  }
};

template <int LN_, int U1, int U2, int O_, typename WT_>
struct Sig2Policy {
  static constexpr int LN = LN_, O = O_, kF64Stage = 3;
  using WT = WT_;
  using Net = Sig2Net<LN, U1, U2, O>;
  using Lds = Hidden2Lds<LN, U1, U2>;
  static __device__ __forceinline__ void load(Net &net, const WT *g, const CertDims &dims, Lds &lds, int hl) {
    hidden2_load<Sig2Bound, LN, U1, U2, O, WT>(net, g, dims.H1, dims.H2, lds, hl);
  }
  // the cascade.  stage: 0 certify_c (lane 0 of the half-group decides, every
  // lane acts on that one index), 1 tight_gap_move, 2 plateau_f32, 3 the f64 forward
  static __device__ __forceinline__ int decide(const Net &n, const WT *__restrict__ g, const CertDims &dims,
                                               const int k[6], bool live, Lds &lds, int hl, float z[O], int &stage) {
    hidden2_z32<PG_ACT_SIGMOID, LN, U1, U2, O>(n, k, lds.h, hl, z);
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
        r = hidden2_f64_half<PG_ACT_SIGMOID, LN, U1, U2, O, WT>(g, dims.H1, dims.H2, k, lds.d, hl);
        stage = 3;
      }
      idx = r;
    }
    return idx < 0 ? 0 : idx;
  }
};

// ------------------------------------------------------------ host side ----
// the instances: LN = hidden2_lanes(H1, H2) lanes per network, hidden2_units(LN) units of each layer per lane
#define PG_HIDDEN2_DISPATCH(KERNEL, LN, O, f64, grid, s, p)                                                    \
  do {                                                                                                         \
    if (LN == 4) PG_CERT_DISPATCH(KERNEL, 4, (hidden2_units(4), hidden2_units(4)), O, f64, grid, s, p);        \
    else if (LN == 16) PG_CERT_DISPATCH(KERNEL, 16, (hidden2_units(16), hidden2_units(16)), O, f64, grid, s, p); \
    else PG_CERT_DISPATCH(KERNEL, 32, (hidden2_units(32), hidden2_units(32)), O, f64, grid, s, p);             \
  } while (0)

static_assert(4 * hidden2_units(4) >= 16 && 16 * hidden2_units(16) >= 32 && 32 * hidden2_units(32) >= kHidden2MaxH,
              "hidden2_lanes' thresholds: a layout for every H1, H2 in scope");

// What Relu2Family (pg_relu2.hip) and Sig2Family (pg_sig2.hip) share of a
// family's description (pg_family.hpp); each adds its kernel, its activation,
// its messages and the launches of its kernels.
struct Hidden2Family {
  static constexpr bool kModifiers = true, kScopeOnEntry = true;
  using DecideParams = CertDecideParams;
  // the shapes [6, 2..64, 2..64, 2..4]
  static bool shape_ok(int n_nodes, const int32_t *nodes) {
    return n_nodes == 4 && nodes[0] == 6 && nodes[1] >= 2 && nodes[1] <= kHidden2MaxH && nodes[2] >= 2 &&
           nodes[2] <= kHidden2MaxH && nodes[3] >= 2 && nodes[3] <= 4;
  }
  static long genes(const int32_t *nd) { return (long)nd[1] * 7 + (long)nd[2] * (nd[1] + 1) + (long)nd[3] * (nd[2] + 1); }
  static int lanes(const int32_t *nd) { return hidden2_lanes(nd[1], nd[2]); }
  static int game_grid(const EvalParams &p) { return cert_game_grid(p, lanes(p.nodes)); }
  static int decide_grid(const pg_relu_decide_args *a) { return cert_decide_grid(a->n, lanes(a->net.nodes)); }
  static DecideParams decide_params(const pg_relu_decide_args *a) {
    return cert_decide_params(a, a->net.nodes[1], a->net.nodes[2]);
  }
};

}  // namespace pg
