// pg_relu.hpp -- device code of k_relu (pg_relu.hip): the certified f32 forward
// of a [6, H <= 256, 2..4] ReLU network with bias (activation_function = ReLU,
// numpy_nn.py:6-9, 26) held by a half-group of LN lanes, U hidden units per
// lane, and its f64 re-decision in numpy's order.  The bound's arithmetic and
// its derivation are in pg_relu_bound.h (it also compiles for the host).
//
// A ReLU network needs no transcendental and its f32 error propagates
// linearly, so one static bound per network decides: with z^ the f32 output
// pre-activations, |z^_o - z64_o| <= e for numpy's f64 z64, and t1 >= t2 the
// two largest z^ (ties to the lower index), np.argmax(max(0, z64)) is
//   0            if t1 <= -e          (every activation is 0: the first maximum)
//   index of t1  if t1 > e and t1 - t2 > 2e   (it alone is the largest, and > 0)
// and is otherwise recomputed in f64 from the genes.  Both tests are exact in
// f32: the first two compare stored values, and fl(t1 - t2) > 2e implies
// t1 - t2 > 2e (rounding is monotone and 2e is a float).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_cascade.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_relu_bound.h"

namespace pg {

constexpr int kReluUnits = 16;   // hidden units per lane: 16 (7 + O) + O weights in VGPRs
constexpr int kReluMaxH = 256;
// lanes per network: the fewest that hold H units (padding units have zero
// weights: max(0, 0) = 0 times 0 contributes exactly 0)
__host__ __device__ constexpr int relu_lanes(int H) { return H <= 64 ? 4 : (H <= 128 ? 8 : 16); }
__host__ __device__ constexpr int relu_log2(int n) { return n <= 1 ? 0 : 1 + relu_log2(n >> 1); }

template <int U, int O>
struct ReluNet {
  float w1[U][7];  // hidden unit j = hl + LN * u: 6 input weights + bias weight
  float w2[U][O];  // output weights of that unit
  float c[O];      // output biases
  float e;         // |z^_o - z64_o| <= e for every output (pg_relu_bound.h); inf: always f64
};

// np.maximum(0.0, z) (numpy_nn.py:6-9): NaN propagates, -0.0 and every z <= 0 give 0
__device__ __forceinline__ double relu_f64(double z) { return !(z <= 0.0) ? z : 0.0; }

// dst = v written in place.  The game loop replaces a group's network inside a
// divergent branch; as a plain assignment the old and the new value of each of
// the ~160 weights are distinct registers until the branch joins (the old one
// is live for the lanes that keep their game), which doubled the kernel's
// VGPRs.  Tying the result to the old register makes the update in place.
__device__ __forceinline__ void relu_set(float &dst, float v) { asm("v_mov_b32 %0, %1" : "+v"(dst) : "v"(v)); }

// sum over the LN lanes of an aligned half-group (cold: once per game)
template <int LN>
__device__ __forceinline__ double half_sum_f64(double v) {
#pragma unroll
  for (int m = 1; m < LN; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// This lane's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H, 7], then W2 [O, H + 1], bias column last) as f32, and the
// network's bound from the f64 genes.  H <= LN * U (host-checked).
template <int LN, int U, int O, typename WT>
__device__ __forceinline__ void relu_load(ReluNet<U, O> &n, const WT *__restrict__ g, int H, int hl) {
  static_assert(1 + U + relu_log2(LN) + 1 <= PG_RELU_CHAIN_MAX, "pg_relu_bound.h's output-layer chain");
  static_assert(O <= PG_RELU_MAX_OUT, "pg_relu_sums");
  // hl made opaque: the unit offsets and masks below would otherwise be hoisted out
  // of the game loop as ~100 loop-invariant VGPRs kept live across every frame
  asm volatile("" : "+v"(hl));
  const long off2 = (long)H * 7;
  pg_relu_sums s;
  pg_relu_sums_init(&s);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = hl + LN * u;
    const bool ok = j < H;
    const int jj = ok ? j : 0;  // padding units load a valid row and are zeroed (see load_net)
    WT raw[7 + O];
#pragma unroll
    for (int i = 0; i < 7; ++i) raw[i] = g[(long)jj * 7 + i];
#pragma unroll
    for (int o = 0; o < O; ++o) raw[7 + o] = g[off2 + (long)o * (H + 1) + jj];
    const double m = ok ? 1.0 : 0.0;  // (inf or NaN times 0 is NaN: the bound then reads inf)
    double w1[7], w2[O];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      w1[i] = (double)raw[i] * m;
      relu_set(n.w1[u][i], (float)w1[i]);
    }
#pragma unroll
    for (int o = 0; o < O; ++o) {
      w2[o] = (double)raw[7 + o] * m;
      relu_set(n.w2[u][o], (float)w2[o]);
    }
    pg_relu_sums_unit(&s, w1, w2, O);
    __builtin_amdgcn_sched_barrier(0);  // one unit's loads in flight at a time: this cold spot must not set the kernel's register budget
  }
  double c[O];
#pragma unroll
  for (int o = 0; o < O; ++o) {
    c[o] = (double)g[off2 + (long)o * (H + 1) + H];
    relu_set(n.c[o], (float)c[o]);
    s.S[o] = half_sum_f64<LN>(s.S[o]);
    s.W2[o] = half_sum_f64<LN>(s.W2[o]);
  }
  s.A = half_sum_f64<LN>(s.A);
  relu_set(n.e, pg_relu_bound_finish(&s, c, O, LN * U));
}

// The f32 output pre-activations z^ on the doubled-centroid features k, in the
// operation order pg_relu_bound.h bounds; every lane of the half-group gets them.
template <int LN, int U, int O>
__device__ __forceinline__ void relu_z32(const ReluNet<U, O> &n, const int k[6], float z[O]) {
  float x[6], acc[O];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat32(k[i]);
#pragma unroll
  for (int o = 0; o < O; ++o) acc[o] = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float a = n.w1[u][6];
#pragma unroll
    for (int i = 0; i < 6; ++i) a = fmaf(n.w1[u][i], x[i], a);
    const float h = fmaxf(a, 0.f);
#pragma unroll
    for (int o = 0; o < O; ++o) acc[o] = fmaf(n.w2[u][o], h, acc[o]);
  }
#pragma unroll
  for (int o = 0; o < O; ++o) z[o] = group_sum<LN>(acc[o]) + n.c[o];
}

// The certificate (see the header of this file): the proven index, or -1.
template <int O>
__device__ __forceinline__ int relu_certify(const float z[O], float e) {
  int i1 = 0;
  float t1 = z[0], t2 = -__builtin_inff();
#pragma unroll
  for (int o = 1; o < O; ++o) {
    const bool up = z[o] > t1;  // a tie keeps the lower index
    t2 = up ? t1 : fmaxf(t2, z[o]);
    i1 = up ? o : i1;
    t1 = up ? z[o] : t1;
  }
  if (!(e < __builtin_inff())) return -1;  // z^ may be inf or NaN then: never decided here
  if (t1 <= -e) return 0;
  return (t1 > e && t1 - t2 > 2.f * e) ? i1 : -1;
}

// The f64 forward of one pass by the LN lanes of a half-group, as
// forward_f64_wave runs it (NeuralNetwork.run numpy_nn.py:120-137 in np.dot's
// order, blas_dot over [inputs..., 1] per unit): hidden units strided over the
// lanes into LDS, lane o < O sums output o, every lane takes the argmax.
// lds: this half-group's LN * U + O doubles; H <= LN * U.
template <int LN, int U, int O, typename WT>
__device__ PG_SLOW_INLINE int relu_f64_half(const WT *__restrict__ g, int H, const int k[6], double *lds, int hl) {
  static_assert(O <= LN, "lane o sums output o");
  asm volatile("" : "+v"(hl));  // (as in relu_load: nothing of this cold path is hoisted into the frame loop)
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = feat64(k[i]);
#pragma unroll 1
  for (int j = hl; j < H && j < LN * U; j += LN) {
    const WT *row = g + (long)j * 7;
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < 6 ? x[i] : 1.0; }, 7,
                              blas_kind(j, H));
    lds[j] = relu_f64(z);
  }
  wave_lds_sync();
  double *out = lds + LN * U;
  if (hl < O) {
    const WT *row = g + (long)H * 7 + (long)hl * (H + 1);
    const int Hc = H < LN * U ? H : LN * U;
    const double z = blas_dot([&](int j) { return (double)row[j]; }, [&](int j) { return j < Hc ? lds[j] : 1.0; },
                              Hc + 1, blas_kind(hl, O));
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

// One decision of a half-group: z^ (returned in z), the certificate, else the
// f64 forward (slow = 1).  live = false (the idle left half of a game against a
// scripted opponent): index 0, never the f64 path.
template <int LN, int U, int O, typename WT>
__device__ __forceinline__ int relu_decide(const ReluNet<U, O> &n, const WT *__restrict__ g, int H, const int k[6],
                                           bool live, double *lds, int hl, float z[O], int &slow) {
  relu_z32<LN, U, O>(n, k, z);
  int idx = relu_certify<O>(z, n.e);
  const bool need = live && idx < 0;
  slow = need ? 1 : 0;
  if (PG_ANY(need) && need) idx = relu_f64_half<LN, U, O, WT>(g, H, k, lds, hl);
  return idx < 0 ? 0 : idx;
}

}  // namespace pg
