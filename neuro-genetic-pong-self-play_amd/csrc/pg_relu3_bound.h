/* pg_relu3_bound.h -- the static f32 error bound of the three-hidden-layer ReLU
 * certificate (k_relu3, pg_hidden3.hpp): pg_relu2_bound.h's derivation one
 * layer further.  In plain C so that it compiles for the device and for the
 * host alike (tests/test_relu3_host.py runs it under gcc).
 *
 * The network [6, H1, H2, H3, O] with bias, inputs x_i = k_i / 320 in [0, 1]:
 *   z1_j = sum_i W1_ji x_i + b1_j,   h1_j = max(0, z1_j)
 *   z2_k = sum_j W2_kj h1_j + b2_k,  h2_k = max(0, z2_k)
 *   z3_l = sum_k W3_lk h2_k + b3_l,  h3_l = max(0, z3_l)
 *   z_o  = sum_l W4_ol h3_l + b4_o.
 * As there, no step depends on the order of a sum: a computed dot product whose
 * terms pass through at most c roundings (factors 1 + d, |d| <= u = 2^-24)
 * differs from the exact one by at most gamma_c sum_i |t_i|, gamma_c =
 * c u / (1 - c u).  With
 *       A_j = sum_i |W1_ji| + |b1_j|           (>= |z1_j|, as x_i <= 1)
 *       B_k = sum_j |W2_kj| A_j + |b2_k|       (>= |z2_k|)
 *       C_l = sum_k |W3_lk| B_k + |b3_l|       (>= |z3_l|)
 *       S_o = sum_l |W4_ol| C_l + |b4_o|
 * and ReLU exact and 1-Lipschitz, pg_relu2_bound.h gives
 *   |h1^_j - h1_j| <= gamma_c1 A_j,   |h2^_k - h2_k| <= gamma_(c1+c2) B_k,
 * and the same step twice more (gamma_a + gamma_b + gamma_a gamma_b <= gamma_(a+b)):
 *   |z3^_l - z3_l| <= sum_k |W3_lk| (gamma_(c1+c2) B_k (1 + gamma_c3) + gamma_c3 B_k) + gamma_c3 |b3_l|
 *                  <= gamma_(c1+c2+c3) C_l
 *   |z^_o - z_o|   <= sum_l |W4_ol| (gamma_(c1+c2+c3) C_l (1 + gamma_c4) + gamma_c4 C_l) + gamma_c4 |b4_o|
 *                  <= gamma_(c1+c2+c3+c4) S_o.
 * numpy's own f64 result differs from the exact z_o by its four np.dot calls'
 * and the features' roundings: < 2^-40 S_o, i.e. < 2^-16 u S_o.  The bound kept:
 *   e = (K u max_o S_o + underflow) (1 + 2^-20),   K = c1 + c2 + c3 + c4 + 2:
 * two u of slack for gamma_c - c u with c = c1 + c2 + c3 + c4 = 83 (c^2 u^2 /
 * (1 - c u) < 10^-3 u), the f64 part and the f64 rounding of S_o itself (sums
 * of non-negative terms: relative error below 2^-40 whatever the order), and
 * 2^-20 for the conversion of e to f32.
 *
 * The chain lengths (k_relu3's two layouts, LN = 8 or 16 lanes with two units
 * of each layer per lane; pg_hidden3.hpp asserts that both stay within them):
 *   layer 1  PG_RELU3_CHAIN1 = 9:   1 (gene to f32) + 2 (the feature
 *            fl32(k * fl32(1 / 320)), feat32) + 6 fused multiply-adds
 *   layer 2  PG_RELU3_CHAIN2 = 33:  1 (gene) + one fused multiply-add per
 *            (padded) layer-1 unit, <= 32, onto the bias
 *   layer 3  PG_RELU3_CHAIN3 = 33:  the same over the (padded) layer-2 units
 *   layer 4  PG_RELU3_CHAIN4 = 8:   1 (gene) + a lane's 2 units + the sum over
 *            <= 16 lanes (4 steps) + the bias
 *   K = PG_RELU3_K = 9 + 33 + 33 + 8 + 2 = 85.
 *
 * Underflow.  The above holds for normal results.  Every operation whose
 * result is subnormal or flushed to zero adds at most eta = 2^-126.  As in
 * pg_relu2_bound.h, with V2_k = sum_j |W2_kj| and V3_l = sum_k |W3_lk|:
 *   a layer-1 unit: 7 gene conversions and 6 fmas, <= 13 eta (1 + u) in h1^_j;
 *   a layer-2 unit: E2_k <= eta (14 V2_k + 2 sum_j A_j + c2 + 2);
 *   a layer-3 unit: E2_k through |W3^_lk| (a factor 1 + u: 15, and 3 sum_j A_j
 *     + c2 + 3, the 3 for 2 (1 + u)^2 whatever the sum's size), a flushed W3 gene
 *     times its h2^_k (<= 2 eta B_k each), the bias conversion and the c3 - 1
 *     fmas, each error then carried through at most c3 - 1 more roundings:
 *     E3_l <= eta (15 T3_l + (3 sum_j A_j + c2 + 3) V3_l + 2 sum_k B_k + c3 + 2),
 *     T3_l = sum_k |W3_lk| V2_k;
 *   an output: E3_l through |W4^_ol| (a factor 1 + u again: 16, c2 + 4, 3 sum_k
 *     B_k + c3 + 3), a flushed W4 gene times its h3^_l (<= 2 eta C_l), and the
 *     <= 8 operations of the layer-4 chain with the bias conversion, under the
 *     same constant 16:
 *   underflow = eta (16 max_o Q_o + (3 sum_j A_j + c2 + 4) max_o R_o
 *                    + (3 sum_k B_k + c3 + 3) max_o sum_l |W4_ol| + 2 sum_l C_l + 16),
 *     Q_o = sum_l |W4_ol| T3_l,  R_o = sum_l |W4_ol| V3_l.
 * (A feature k_i * fl32(1/320) is 0 or >= 2^-9: never subnormal.)
 * Overflow.  With sum_j A_j, sum_k B_k, sum_l C_l, sum_kj |W2_kj|, sum_lk
 * |W3_lk|, sum_l |W4_ol|, Q_o, R_o and S_o all <= PG_RELU_CAP = 1e25 (sums of
 * absolute values: NaN and inf propagate into them and fail the test) every
 * gene converts to a finite f32 and no intermediate exceeds B_k, C_l or S_o
 * times (1 + gamma) < FLT_MAX, so z^ is finite.  Otherwise e = inf: the
 * certificate never decides and the f64 path (numpy's semantics, NaN rule
 * included) does.
 */
#ifndef PG_RELU3_BOUND_H
#define PG_RELU3_BOUND_H

#include <math.h>

#include "pg_relu2_bound.h" /* pg_relu2_unit1; pg_relu_bound.h's PG_HD, PG_RELU_CAP, PG_RELU_MAX_OUT */

#define PG_RELU3_MAX_H 32
#define PG_RELU3_CHAIN1 9  /* gene + feature (2) + 6 fmas */
#define PG_RELU3_CHAIN2 33 /* gene + <= 32 fmas */
#define PG_RELU3_CHAIN3 33 /* gene + <= 32 fmas */
#define PG_RELU3_CHAIN4 8  /* gene + 2 fmas + <= 4 lane-sum steps + bias */
#define PG_RELU3_K ((double)(PG_RELU3_CHAIN1 + PG_RELU3_CHAIN2 + PG_RELU3_CHAIN3 + PG_RELU3_CHAIN4 + 2))

/* Sums over (a share of) the layer-3 units and, for B and W2, of the layer-2 units; shares add field by field. */
typedef struct pg_relu3_sums {
  double S[PG_RELU_MAX_OUT];  /* sum_l |W4_ol| C_l */
  double Q[PG_RELU_MAX_OUT];  /* sum_l |W4_ol| T3_l */
  double R[PG_RELU_MAX_OUT];  /* sum_l |W4_ol| V3_l */
  double W4[PG_RELU_MAX_OUT]; /* sum_l |W4_ol| */
  double B, C;                /* sum_k B_k, sum_l C_l */
  double W2, W3;              /* sum_kj |W2_kj|, sum_lk |W3_lk| */
} pg_relu3_sums;

PG_HD void pg_relu3_sums_init(pg_relu3_sums *s) {
  for (int o = 0; o < PG_RELU_MAX_OUT; ++o) s->S[o] = s->Q[o] = s->R[o] = s->W4[o] = 0.0;
  s->B = s->C = s->W2 = s->W3 = 0.0;
}

/* One layer-2 unit: b = B_k and v = V2_k of its row. */
PG_HD void pg_relu3_sums_unit2(pg_relu3_sums *s, double b, double v) {
  s->B += b;
  s->W2 += v;
}

/* One layer-3 unit: c = C_l, t = T3_l and v = V3_l of its row, w4 its O output weights. */
PG_HD void pg_relu3_sums_unit3(pg_relu3_sums *s, double c, double t, double v, const double *w4, int O) {
  for (int o = 0; o < O; ++o) {
    s->S[o] += fabs(w4[o]) * c;
    s->Q[o] += fabs(w4[o]) * t;
    s->R[o] += fabs(w4[o]) * v;
    s->W4[o] += fabs(w4[o]);
  }
  s->C += c;
  s->W3 += v;
}

/* The bound from the sums over all units, asum = sum_j A_j and the output biases c. */
PG_HD float pg_relu3_bound_finish(const pg_relu3_sums *s, double asum, const double *c, int O) {
  double smax = 0.0, qmax = 0.0, rmax = 0.0, w4max = 0.0;
  int ok = asum <= PG_RELU_CAP && s->B <= PG_RELU_CAP && s->C <= PG_RELU_CAP && s->W2 <= PG_RELU_CAP &&
           s->W3 <= PG_RELU_CAP; /* false for NaN */
  for (int o = 0; o < O; ++o) {
    const double so = s->S[o] + fabs(c[o]);
    ok = ok && so <= PG_RELU_CAP && s->Q[o] <= PG_RELU_CAP && s->R[o] <= PG_RELU_CAP && s->W4[o] <= PG_RELU_CAP;
    smax = so > smax ? so : smax;
    qmax = s->Q[o] > qmax ? s->Q[o] : qmax;
    rmax = s->R[o] > rmax ? s->R[o] : rmax;
    w4max = s->W4[o] > w4max ? s->W4[o] : w4max;
  }
  if (!ok) return (float)INFINITY;
  const double u = 0x1.0p-24, eta = 0x1.0p-126;
  const double under = eta * (16.0 * qmax + (3.0 * asum + (double)(PG_RELU3_CHAIN2 + 4)) * rmax +
                              (3.0 * s->B + (double)(PG_RELU3_CHAIN3 + 3)) * w4max + 2.0 * s->C + 16.0);
  return (float)((PG_RELU3_K * u * smax + under) * (1.0 + 0x1.0p-20));
}

/* The whole bound of one genome (numpy_nn.py:52-69 layout with bias: W1
 * [H1, 7], W2 [H2, H1 + 1], W3 [H3, H2 + 1], W4 [O, H3 + 1], bias columns
 * last), serially: what a test or a host tool calls; k_relu3's lanes run the
 * same functions on their shares.  A network wider than the layouts hold has
 * no bound: inf. */
PG_HD float pg_relu3_bound_genome(const double *g, int H1, int H2, int H3, int O) {
  double A[PG_RELU3_MAX_H], B[PG_RELU3_MAX_H], V2[PG_RELU3_MAX_H], asum = 0.0, c[PG_RELU_MAX_OUT];
  if (H1 > PG_RELU3_MAX_H || H2 > PG_RELU3_MAX_H || H3 > PG_RELU3_MAX_H) return (float)INFINITY;
  const double *w2 = g + (long)H1 * 7, *w3 = w2 + (long)H2 * (H1 + 1), *w4 = w3 + (long)H3 * (H2 + 1);
  pg_relu3_sums s;
  pg_relu3_sums_init(&s);
  for (int j = 0; j < H1; ++j) {
    A[j] = pg_relu2_unit1(g + (long)j * 7);
    asum += A[j];
  }
  for (int k = 0; k < H2; ++k) {
    const double *row = w2 + (long)k * (H1 + 1);
    double b = 0.0, v = 0.0;
    for (int j = 0; j < H1; ++j) {
      b += fabs(row[j]) * A[j];
      v += fabs(row[j]);
    }
    B[k] = b + fabs(row[H1]);
    V2[k] = v;
    pg_relu3_sums_unit2(&s, B[k], v);
  }
  for (int l = 0; l < H3; ++l) {
    const double *row = w3 + (long)l * (H2 + 1);
    double cl = 0.0, t = 0.0, v = 0.0, x[PG_RELU_MAX_OUT];
    for (int k = 0; k < H2; ++k) {
      cl += fabs(row[k]) * B[k];
      t += fabs(row[k]) * V2[k];
      v += fabs(row[k]);
    }
    cl += fabs(row[H2]);
    for (int o = 0; o < O; ++o) x[o] = w4[(long)o * (H3 + 1) + l];
    pg_relu3_sums_unit3(&s, cl, t, v, x, O);
  }
  for (int o = 0; o < O; ++o) c[o] = w4[(long)o * (H3 + 1) + H3];
  return pg_relu3_bound_finish(&s, asum, c, O);
}

#endif /* PG_RELU3_BOUND_H */
