/* pg_relu2_bound.h -- the static f32 error bound of the two-hidden-layer ReLU
 * certificate, for both layouts that hold such a network: k_relu2's lanes of a
 * wave (pg_hidden2.hpp) and k_relu2_block's 256-thread block
 * (pg_relu2_block.hip).  In plain C so that it compiles for the device and for
 * the host alike (tests/test_relu2_host.py runs it under gcc).
 *
 * The network [6, H1, H2, O] with bias, inputs x_i = k_i / 320 in [0, 1]:
 *   z1_j = sum_i W1_ji x_i + b1_j,   h1_j = max(0, z1_j)
 *   z2_k = sum_j W2_kj h1_j + b2_k,  h2_k = max(0, z2_k)
 *   z_o  = sum_k W3_ok h2_k + b3_o.
 * The derivation does not depend on the order of any sum: if every term of a
 * computed dot product passes through at most c roundings (factors 1 + d,
 * |d| <= u = 2^-24), the result is sum_i t_i (1 + theta_i) with |theta_i| <=
 * gamma_c = c u / (1 - c u), so it differs from the exact sum by at most
 * gamma_c sum_i |t_i|, whatever the order.  A layout enters only through its
 * three chain lengths c1, c2, c3 (the roundings a term of layer 1, 2, 3 passes
 * through) and one count of operations for the underflow, pg_relu2_layout
 * below; the two layouts' tables follow the derivation.
 *
 * With  A_j = sum_i |W1_ji| + |b1_j|           (>= |z1_j|, as x_i <= 1)
 *       B_k = sum_j |W2_kj| A_j + |b2_k|       (>= |z2_k|)
 *       S_o = sum_k |W3_ok| B_k + |b3_o|
 * and ReLU exact and 1-Lipschitz:
 *   |h1^_j - h1_j| <= gamma_c1 A_j
 *   |z2^_k - z2_k| <= sum_j |W2_kj| (gamma_c1 A_j (1 + gamma_c2) + gamma_c2 A_j) + gamma_c2 |b2_k|
 *                  <= gamma_(c1+c2) B_k      (gamma_a + gamma_b + gamma_a gamma_b <= gamma_(a+b))
 *   |z^_o - z_o|   <= sum_k |W3_ok| (gamma_(c1+c2) B_k (1 + gamma_c3) + gamma_c3 B_k) + gamma_c3 |b3_o|
 *                  <= gamma_(c1+c2+c3) S_o.
 * numpy's own f64 result differs from the exact z_o by its three np.dot calls'
 * and the features' roundings: < 2^-40 S_o, i.e. < 2^-16 u S_o.  The bound kept:
 *   e = (K u max_o S_o + underflow) (1 + 2^-20),   K = c1 + c2 + c3 + 2:
 * two u of slack for gamma_c - c u with c = c1 + c2 + c3 (= c^2 u^2 / (1 - c u):
 * < 10^-3 u for c = 85, < 2 10^-3 u for c = 148), the f64 part and the f64
 * rounding of S_o itself (sums of non-negative terms: relative error below
 * 2^-40 whatever the order, the lanes' partial sums and the host's serial loop
 * alike), and 2^-20 for the conversion of e to f32.
 * Underflow.  The above holds for normal results.  Every operation whose
 * result is subnormal or flushed to zero adds at most eta = 2^-126:
 *   a layer-1 unit: 7 gene conversions and 6 fmas, <= 13 eta (1 + u) in h1^_j;
 *   a layer-2 unit: those through |W2^_kj| (<= 14 eta sum_j |W2_kj|), a flushed
 *     W2 gene times its h1^_j (<= eta (1 + gamma_c1) A_j + ... <= 2 eta A_j
 *     each), the bias conversion and the c2 - 1 fmas, each error then carried
 *     through at most c2 - 1 more roundings (c2 eta (1 + gamma_c2) < (c2 + 1) eta):
 *     E2_k <= eta (14 sum_j |W2_kj| + 2 sum_j A_j + c2 + 2);
 *   an output: E2_k through |W3^_ok| (a factor 1 + u: 15, c2 + 3), a flushed W3
 *     gene times its h2^_k (<= 2 eta B_k), and the operations of the layer-3
 *     sum: the <= 11 of one term's chain, with the bias conversion and the bias
 *     addition, under a constant 16; and, where one output is summed from many
 *     threads' terms, every further operation that feeds it (sum_ops):
 *   underflow = eta (15 max_o T_o + (2 sum_j A_j + c2 + 3) max_o sum_k |W3_ok| + 2 sum_k B_k + 16 + sum_ops),
 *     T_o = sum_k |W3_ok| sum_j |W2_kj|.
 * (A feature k_i * fl32(1/320) is 0 or >= 2^-9: never subnormal.)
 * Overflow.  With sum_j A_j, sum_kj |W2_kj|, sum_k B_k, sum_k |W3_ok|, T_o and
 * S_o all <= PG_RELU_CAP = 1e25 (sums of absolute values: NaN and inf
 * propagate into them and fail the test) every gene converts to a finite f32
 * and no intermediate exceeds B_k or S_o times (1 + gamma) < FLT_MAX, so z^ is
 * finite.  Otherwise e = inf: the certificate never decides and the f64 path
 * (numpy's semantics, NaN rule included) does.
 *
 * The lane layout (k_relu2; H1, H2 <= PG_RELU2_MAX_H = 64):
 *   layer 1  PG_RELU2_CHAIN1 = 9:   1 (gene to f32) + 2 (the feature
 *            fl32(k * fl32(1 / 320)), feat32) + 6 fused multiply-adds
 *   layer 2  PG_RELU2_CHAIN2 = 65:  1 (gene) + one fused multiply-add per
 *            (padded) layer-1 unit, <= 64, onto the bias
 *   layer 3  PG_RELU2_CHAIN3 = 11:  1 (gene) + a lane's <= 4 units + the sum
 *            over <= 32 lanes (5 steps) + the bias
 * (pg_hidden2.hpp asserts that every instantiated layout stays within them).
 *   gamma_9 A_j, gamma_74 B_k, gamma_85 S_o;  K = PG_RELU2_K = 9 + 65 + 11 + 2 = 87;
 *   E2_k <= eta (14 sum_j |W2_kj| + 2 sum_j A_j + 67): the bias conversion and
 *   64 fmas; sum_ops = 0: the <= 11 operations of the layer-3 chain are all
 *   that an output's term meets, within the 16:
 *   underflow = eta (15 max_o T_o + (2 sum_j A_j + 68) max_o sum_k |W3_ok| + 2 sum_k B_k + 16).
 *
 * The block layout (k_relu2_block; H1, H2 <= PG_RELU2_BLOCK_MAX_H = 128):
 *   layer 1  PG_RELU2_BLOCK_CHAIN1 = 9:    1 (gene to f32) + 2 (the feature,
 *            feat32) + 6 fused multiply-adds
 *   layer 2  PG_RELU2_BLOCK_CHAIN2 = 129:  1 (gene) + one fused multiply-add
 *            per (padded) layer-1 unit, 128, onto the bias
 *   layer 3  PG_RELU2_BLOCK_CHAIN3 = 10:   1 (gene) + 1 (a thread's one
 *            product W3_ok h2_k) + 6 (the sum over the wave's 64 lanes) + 1 (the
 *            network's two waves) + 1 (the bias)
 * (pg_relu2_block.hip asserts its reduction against CHAIN3.)
 *   gamma_9 A_j, gamma_(9 + 129) B_k = gamma_138 B_k, gamma_(138 + 10) S_o =
 *   gamma_148 S_o;  K = PG_RELU2_BLOCK_K = 9 + 129 + 10 + 2 = 150;
 *   E2_k <= eta (14 sum_j |W2_kj| + 2 sum_j A_j + 131): the bias conversion and
 *   128 fmas, each error then carried through at most 128 more roundings
 *   (129 eta (1 + gamma_129) < 130 eta); through |W3^_ok|: 15, 132;
 *   sum_ops = 128 + 127: every operation of the layer-3 sum, all of which feed
 *   the one output: the 128 threads' products W3^_ok h2^_k (128 eta), the 127
 *   additions of the tree over the two waves (126 in the waves, 1 across them:
 *   127 eta -- with denormals on, as the kernels are compiled, an f32 addition
 *   is exact in the subnormal range and loses nothing; they are budgeted so
 *   that the bound also holds were results flushed), and the bias conversion
 *   and the bias addition, under the 16 kept from the lane layout:
 *   underflow = eta (15 max_o T_o + (2 sum_j A_j + 132) max_o sum_k |W3_ok| + 2 sum_k B_k + 128 + 127 + 16).
 */
#ifndef PG_RELU2_BOUND_H
#define PG_RELU2_BOUND_H

#include <math.h>

#include "pg_relu_bound.h" /* PG_HD, PG_RELU_CAP, PG_RELU_MAX_OUT */

#define PG_RELU2_MAX_H 64
#define PG_RELU2_CHAIN1 9  /* gene + feature (2) + 6 fmas */
#define PG_RELU2_CHAIN2 65 /* gene + <= 64 fmas */
#define PG_RELU2_CHAIN3 11 /* gene + <= 4 fmas + <= 5 lane-sum steps + bias */
#define PG_RELU2_K ((double)(PG_RELU2_CHAIN1 + PG_RELU2_CHAIN2 + PG_RELU2_CHAIN3 + 2))

#define PG_RELU2_BLOCK_MAX_H 128
#define PG_RELU2_BLOCK_CHAIN1 9   /* gene + feature (2) + 6 fmas */
#define PG_RELU2_BLOCK_CHAIN2 129 /* gene + 128 fmas */
#define PG_RELU2_BLOCK_CHAIN3 10  /* gene + product + 6 lane-sum steps + the two waves + bias */
#define PG_RELU2_BLOCK_K \
  ((double)(PG_RELU2_BLOCK_CHAIN1 + PG_RELU2_BLOCK_CHAIN2 + PG_RELU2_BLOCK_CHAIN3 + 2))

/* What the bound needs of a layout.  Its instances come by value from the two
 * functions below, so that every field is a constant where finish is inlined. */
typedef struct pg_relu2_layout {
  int chain1, chain2, chain3; /* roundings a term of layer 1, 2, 3 passes through */
  int sum_ops;                /* operations of the layer-3 sum that feed one output beyond a term's own chain */
  int max_h;                  /* units per hidden layer: what pg_relu2_bound_genome accepts */
} pg_relu2_layout;

PG_HD pg_relu2_layout pg_relu2_layout_lanes(void) {
  pg_relu2_layout l = {PG_RELU2_CHAIN1, PG_RELU2_CHAIN2, PG_RELU2_CHAIN3, 0, PG_RELU2_MAX_H};
  return l;
}

PG_HD pg_relu2_layout pg_relu2_layout_block(void) { /* 128 products + 127 additions of the tree */
  pg_relu2_layout l = {PG_RELU2_BLOCK_CHAIN1, PG_RELU2_BLOCK_CHAIN2, PG_RELU2_BLOCK_CHAIN3,
                       PG_RELU2_BLOCK_MAX_H + (PG_RELU2_BLOCK_MAX_H - 1), PG_RELU2_BLOCK_MAX_H};
  return l;
}

/* Sums over (a share of) the layer-2 units; shares add field by field. */
typedef struct pg_relu2_sums {
  double S[PG_RELU_MAX_OUT];  /* sum_k |W3_ok| B_k */
  double T[PG_RELU_MAX_OUT];  /* sum_k |W3_ok| sum_j |W2_kj| */
  double W3[PG_RELU_MAX_OUT]; /* sum_k |W3_ok| */
  double B;                   /* sum_k B_k */
  double W2;                  /* sum_kj |W2_kj| */
} pg_relu2_sums;

PG_HD void pg_relu2_sums_init(pg_relu2_sums *s) {
  for (int o = 0; o < PG_RELU_MAX_OUT; ++o) s->S[o] = s->T[o] = s->W3[o] = 0.0;
  s->B = s->W2 = 0.0;
}

/* A_j of one layer-1 unit: its 6 input weights and its bias weight. */
PG_HD double pg_relu2_unit1(const double w1[7]) {
  double a = 0.0;
  for (int i = 0; i < 7; ++i) a += fabs(w1[i]);
  return a;
}

/* One layer-2 unit: b = B_k and w = sum_j |W2_kj| of its row, w3 its O output weights. */
PG_HD void pg_relu2_sums_unit2(pg_relu2_sums *s, double b, double w, const double *w3, int O) {
  for (int o = 0; o < O; ++o) {
    s->S[o] += fabs(w3[o]) * b;
    s->T[o] += fabs(w3[o]) * w;
    s->W3[o] += fabs(w3[o]);
  }
  s->B += b;
  s->W2 += w;
}

/* The bound of layout l from the sums over all layer-2 units, asum = sum_j A_j and the output biases c. */
PG_HD float pg_relu2_bound_finish(pg_relu2_layout l, const pg_relu2_sums *s, double asum, const double *c, int O) {
  double smax = 0.0, tmax = 0.0, w3max = 0.0;
  int ok = asum <= PG_RELU_CAP && s->B <= PG_RELU_CAP && s->W2 <= PG_RELU_CAP; /* false for NaN */
  for (int o = 0; o < O; ++o) {
    const double so = s->S[o] + fabs(c[o]);
    ok = ok && so <= PG_RELU_CAP && s->T[o] <= PG_RELU_CAP && s->W3[o] <= PG_RELU_CAP;
    smax = so > smax ? so : smax;
    tmax = s->T[o] > tmax ? s->T[o] : tmax;
    w3max = s->W3[o] > w3max ? s->W3[o] : w3max;
  }
  if (!ok) return (float)INFINITY;
  const double u = 0x1.0p-24, eta = 0x1.0p-126;
  const double K = (double)(l.chain1 + l.chain2 + l.chain3 + 2);
  const double under =
      eta * (15.0 * tmax + (2.0 * asum + (double)(l.chain2 + 3)) * w3max + 2.0 * s->B + (double)(16 + l.sum_ops));
  return (float)((K * u * smax + under) * (1.0 + 0x1.0p-20));
}

/* The whole bound of one genome (numpy_nn.py:52-69 layout with bias: W1
 * [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last), serially:
 * what a test or a host tool calls; k_relu2's lanes and k_relu2_block's threads
 * run the same functions on their shares.  A network wider than the layout
 * holds (H1 or H2 > l.max_h) has no bound: inf. */
PG_HD float pg_relu2_bound_genome(pg_relu2_layout l, const double *g, int H1, int H2, int O) {
  double A[PG_RELU2_BLOCK_MAX_H], asum = 0.0, c[PG_RELU_MAX_OUT]; /* the larger layout's */
  if (H1 > l.max_h || H2 > l.max_h || l.max_h > PG_RELU2_BLOCK_MAX_H) return (float)INFINITY;
  const double *w2 = g + (long)H1 * 7, *w3 = w2 + (long)H2 * (H1 + 1);
  pg_relu2_sums s;
  pg_relu2_sums_init(&s);
  for (int j = 0; j < H1; ++j) {
    A[j] = pg_relu2_unit1(g + (long)j * 7);
    asum += A[j];
  }
  for (int k = 0; k < H2; ++k) {
    const double *row = w2 + (long)k * (H1 + 1);
    double b = 0.0, w = 0.0, v[PG_RELU_MAX_OUT];
    for (int j = 0; j < H1; ++j) {
      b += fabs(row[j]) * A[j];
      w += fabs(row[j]);
    }
    b += fabs(row[H1]);
    for (int o = 0; o < O; ++o) v[o] = w3[(long)o * (H2 + 1) + k];
    pg_relu2_sums_unit2(&s, b, w, v, O);
  }
  for (int o = 0; o < O; ++o) c[o] = w3[(long)o * (H2 + 1) + H2];
  return pg_relu2_bound_finish(l, &s, asum, c, O);
}

#endif /* PG_RELU2_BOUND_H */
