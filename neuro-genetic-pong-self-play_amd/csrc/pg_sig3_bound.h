/* pg_sig3_bound.h -- the static f32 error bound of the three-hidden-layer
 * sigmoid certificate (k_sig3, pg_sig3.hpp): pg_sig2_bound.h's derivation one
 * layer further, on k_relu3's layout (pg_hidden3.hpp).  In plain C so that it
 * compiles for the device and for the host alike (tests/test_sig3_host.py runs
 * it under gcc).
 *
 * The network [6, H1, H2, H3, O] with bias, inputs x_i = k_i / 320 in [0, 1],
 * s(z) = 1 / (1 + e^-z):
 *   z1_j = sum_i W1_ji x_i + b1_j,   h1_j = s(z1_j)
 *   z2_k = sum_j W2_kj h1_j + b2_k,  h2_k = s(z2_k)
 *   z3_l = sum_k W3_lk h2_k + b3_l,  h3_l = s(z3_l)
 *   z_o  = sum_l W4_ol h3_l + b4_o.
 * e bounds |z^_o - znp_o|: z^ k_sig3's f32 output pre-activation, znp the f64
 * pre-activation numpy computes (the argument of its last sigmoid), which is
 * what certify_c / tight_gap_move / plateau_f32 (pg_cascade.hpp) ask for.
 *
 * Sums.  As in pg_sig2_bound.h no step depends on the order of a sum: if every
 * term of a computed dot product passes through at most c roundings (factors
 * 1 + d, |d| <= u = 2^-24), the result differs from the exact sum by at most
 * gamma_c sum_i |t_i|, gamma_c = c u / (1 - c u), whatever the order.  The
 * chain lengths are k_relu3's (the layout is the same: LN = 8 or 16 lanes with
 * two units of each layer per lane; pg_sig3.hpp asserts that both layouts stay
 * within them):
 *   layer 1  PG_SIG3_CHAIN1 = 9:   1 (gene to f32) + 2 (the feature
 *            fl32(k * fl32(1 / 320)), feat32) + 6 fused multiply-adds
 *   layer 2  PG_SIG3_CHAIN2 = 33:  1 (gene) + one fused multiply-add per
 *            (padded) layer-1 unit, <= 32, onto the bias
 *   layer 3  PG_SIG3_CHAIN3 = 33:  the same over the (padded) layer-2 units
 *   layer 4  PG_SIG3_CHAIN4 = 8:   1 (gene) + a lane's 2 units + the sum over
 *            <= 16 lanes (4 steps) + the bias
 * Sigmoid.  sigmoid_f32 is allowed PG_SIG2_SIG = 4.5 u of absolute error of its
 * own at every argument (pg_sig2_bound.h counts it: 3.84 u); its slope is
 * <= 1/4, its value and the computed one lie in [0, 1].
 *
 * With  A_j = sum_i |W1_ji| + |b1_j|           (>= |z1_j|, as x_i <= 1)
 *       P_k = sum_j |W2_kj| A_j
 *       B_k = sum_j |W2_kj| + |b2_k|           (>= |z2_k|, as |h1_j| <= 1)
 * and c1..c4 the chain lengths:
 *   |z1^_j - z1_j| <= gamma_c1 A_j
 *   |h1^_j - h1_j| <= gamma_c1 A_j / 4 + 4.5 u
 *   |z2^_k - z2_k| <= sum_j |W2_kj| ((gamma_c1 A_j / 4 + 4.5 u)(1 + gamma_c2) + gamma_c2) + gamma_c2 |b2_k|
 *                  <= u Q2_k (1 + 2^-17),   Q2_k = (c1 / 4) P_k + (4.5 + c2) B_k
 *   |h2^_k - h2_k| <= u (Q2_k / 4) (1 + 2^-17) + 4.5 u
 *   |z3^_l - z3_l| <= sum_k |W3_lk| ((u (Q2_k / 4)(1 + 2^-17) + 4.5 u)(1 + gamma_c3) + gamma_c3) + gamma_c3 |b3_l|
 *                  <= u Q3_l (1 + 2^-16),   Q3_l = sum_k |W3_lk| (Q2_k / 4 + 4.5 + c3) + c3 |b3_l|
 *   |h3^_l - h3_l| <= u (Q3_l / 4) (1 + 2^-16) + 4.5 u
 *   |z^_o - z_o|   <= sum_l |W4_ol| ((u (Q3_l / 4)(1 + 2^-16) + 4.5 u)(1 + gamma_c4) + gamma_c4) + gamma_c4 |b4_o|
 *                  <= u S_o (1 + 2^-15),   S_o = sum_l |W4_ol| (Q3_l / 4 + 4.5 + c4) + c4 |b4_o|
 * (the gamma_c3 and gamma_c4 terms multiply a computed activation, which is in
 * [0, 1]).  The second-order factors, counted for this depth: gamma_c = c u (1
 * + c u / (1 - c u)) with c u <= 33 x 2^-24 < 2^-18.9, so gamma_9 <= 9 u (1 +
 * 2^-20.8), gamma_33 <= 33 u (1 + 2^-18.9) and 1 + gamma_33 <= 1 + 2^-18.9:
 *   layer 2: (1 + 2^-20.8)(1 + 2^-18.9) < 1 + 2^-18.5 <= 1 + 2^-17;
 *   layer 3: (1 + 2^-17)(1 + 2^-18.9) < 1 + 2^-16.6 <= 1 + 2^-16, and the
 *            gamma_33 terms' own 1 + 2^-18.9 is below it;
 *   layer 4: (1 + 2^-16)(1 + gamma_8) < 1 + 2^-15.9 <= 1 + 2^-15.
 * One more layer than pg_sig2_bound.h costs one more such product; with the
 * chains half as long each factor is one binade smaller than there (2^-16,
 * 2^-15, 2^-14 for two layers), and the last, 2^-15, is 32 times inside 2^-10.
 * A padding unit has activation s(0) = 0.5, not 0: its outgoing weights are
 * exactly zero, fma(0, 0.5, a) = a, so it adds nothing to a sum or to its error.
 * numpy's own f64 values differ from the exact ones by the same recurrence with
 * 2^-53 for u and constants of the same size (np.dot over <= 33 terms, the
 * features' roundings, np.e ** -z within an ulp or two, np.e for e): less than
 * 2^-25 of the above.  The bound kept:
 *   e = (u max_o S_o + underflow) (1 + 2^-10):
 * the 2^-10 covers the 2^-15 above, the f64 part, the f64 rounding of the sums
 * themselves (non-negative terms: relative error below 2^-40 whatever the
 * order, the lanes' partial sums and the host's serial loop alike), the
 * conversion of e to f32 and the f32 roundings of make_cert's forms of e.
 *
 * Underflow.  The above holds for normal results.  Every operation whose
 * result is subnormal or flushed to zero adds at most eta = 2^-126.  Line by
 * line for this layout (<= 32 padded units a layer), every line in full, with
 * V2_k = sum_j |W2_kj|, V3_l = sum_k |W3_lk|, T3_l = sum_k |W3_lk| V2_k:
 *   a layer-1 unit: 7 gene conversions and 6 fmas, <= 13 eta (1 + u) in z1^_j,
 *     a quarter of it in h1^_j, plus the sigmoid's product, v_exp_f32 and
 *     v_rcp_f32 (<= 6 eta): 13 / 4 + 6 = 9.25, <= 10 eta in h1^_j with the
 *     factors 1 + u of the next line;
 *   a layer-2 unit: those through |W2^_kj| (10 eta V2_k), a flushed W2 gene
 *     times its h1^_j <= 1 (<= 32 of them), the bias conversion and 32 fmas,
 *     each error then carried through at most 32 more roundings (65 eta (1 +
 *     gamma_33) < 66 eta): <= eta (10 V2_k + 66) in z2^_k, so, with the
 *     sigmoid's own <= 6 eta, <= eta (2.5 V2_k + 22.5) in h2^_k;
 *   a layer-3 unit: those through |W3^_lk| (a factor 1 + u: 3 T3_l + 23 V3_l),
 *     a flushed W3 gene times its h2^_k <= 1 (<= 32 of them), the bias
 *     conversion and 32 fmas, carried as above (< 66 eta): <= eta (3 T3_l + 23
 *     V3_l + 66) in z3^_l, so <= eta (0.75 T3_l + 5.75 V3_l + 22.5) in h3^_l;
 *   an output: that through |W4^_ol| (a factor 1 + u: Q_o + 6 R_o + 23 sum_l
 *     |W4_ol|, Q_o = sum_l |W4_ol| T3_l, R_o = sum_l |W4_ol| V3_l); a flushed W4
 *     gene times its h3^_l <= 1 (<= 32 of them); and every operation of the
 *     layer-4 sum, all of which feed the one output: the <= 16 lanes' two fmas
 *     each (32 eta), the 15 additions of the lane tree (exact in the subnormal
 *     range with denormals on, as the kernels are compiled, and budgeted so that
 *     the bound also holds were results flushed), the bias conversion and the
 *     bias addition (2 eta): 32 + 32 + 15 + 2 = 81 <= 96:
 *   underflow = eta (max_o Q_o + 6 max_o R_o + 23 max_o sum_l |W4_ol| + 96).
 * (A feature k_i * fl32(1/320) is 0 or >= 2^-9: never subnormal.  Where
 * v_exp_f32 overflows or flushes, the sigmoid's result is 0 or 1 and the true
 * value within 2^-126 of it: one of its 6 eta.)
 * Overflow.  With sum_j A_j, sum_k P_k, sum_k B_k, sum_l Q3_l (which is >= 33
 * sum_l (V3_l + |b3_l|)), Q_o, R_o, sum_l |W4_ol| and S_o all <= PG_SIG2_CAP =
 * 1e25 (sums of absolute values: NaN and inf propagate into them and fail the
 * test) every gene converts to a finite f32, every pre-activation is at most
 * A_j, B_k, V3_l + |b3_l| or sum_l |W4_ol| + |b4_o| times (1 + gamma) <
 * FLT_MAX / 2 (so a * -log2 e is finite too), every activation is in [0, 1] and
 * z^ is finite.  Otherwise e = inf: the certificate and the in-register rules
 * then never decide and the f64 path (numpy's semantics, NaN rule included)
 * does.
 */
#ifndef PG_SIG3_BOUND_H
#define PG_SIG3_BOUND_H

#include <math.h>

#include "pg_sig2_bound.h" /* PG_HD, PG_SIG2_SIG, PG_SIG2_SLOPE, PG_SIG2_CAP, PG_SIG2_MAX_OUT, pg_sig2_unit1 */

#define PG_SIG3_MAX_H 32
#define PG_SIG3_CHAIN1 9  /* gene + feature (2) + 6 fmas */
#define PG_SIG3_CHAIN2 33 /* gene + <= 32 fmas */
#define PG_SIG3_CHAIN3 33 /* gene + <= 32 fmas */
#define PG_SIG3_CHAIN4 8  /* gene + 2 fmas + <= 4 lane-sum steps + bias */
/* underflow = eta (UNDER_Q max_o Q_o + UNDER_R max_o R_o + UNDER_W4 max_o sum_l |W4_ol| + UNDER_C) */
#define PG_SIG3_UNDER_Q 1.0
#define PG_SIG3_UNDER_R 6.0
#define PG_SIG3_UNDER_W4 23.0
#define PG_SIG3_UNDER_C 96.0

/* Sums over (a share of) the layer-3 units and, for B and P, of the layer-2 units; shares add field by field. */
typedef struct pg_sig3_sums {
  double S[PG_SIG2_MAX_OUT];  /* sum_l |W4_ol| (Q3_l / 4 + 4.5 + c4) */
  double Q[PG_SIG2_MAX_OUT];  /* sum_l |W4_ol| T3_l */
  double R[PG_SIG2_MAX_OUT];  /* sum_l |W4_ol| V3_l */
  double W4[PG_SIG2_MAX_OUT]; /* sum_l |W4_ol| */
  double B, P;                /* sum_k B_k, sum_k P_k */
  double Q3;                  /* sum_l Q3_l */
} pg_sig3_sums;

PG_HD void pg_sig3_sums_init(pg_sig3_sums *s) {
  for (int o = 0; o < PG_SIG2_MAX_OUT; ++o) s->S[o] = s->Q[o] = s->R[o] = s->W4[o] = 0.0;
  s->B = s->P = s->Q3 = 0.0;
}

/* One layer-2 unit: p = P_k and w = V2_k of its row, bias its bias weight.  Returns Q2_k / 4 + 4.5 + c3, the
 * unit's weight in a layer-3 unit's Q3_l. */
PG_HD double pg_sig3_sums_unit2(pg_sig3_sums *s, double p, double w, double bias) {
  const double b = w + fabs(bias);
  const double q2 = (PG_SIG2_SLOPE * PG_SIG3_CHAIN1) * p + (PG_SIG2_SIG + PG_SIG3_CHAIN2) * b;
  s->B += b;
  s->P += p;
  return PG_SIG2_SLOPE * q2 + (PG_SIG2_SIG + PG_SIG3_CHAIN3);
}

/* One layer-3 unit: x = sum_k |W3_lk| (Q2_k / 4 + 4.5 + c3), t = T3_l and v = V3_l of its row, bias its bias
 * weight, w4 its O output weights. */
PG_HD void pg_sig3_sums_unit3(pg_sig3_sums *s, double x, double t, double v, double bias, const double *w4, int O) {
  const double q3 = x + PG_SIG3_CHAIN3 * fabs(bias);
  const double y = PG_SIG2_SLOPE * q3 + (PG_SIG2_SIG + PG_SIG3_CHAIN4);
  for (int o = 0; o < O; ++o) {
    s->S[o] += fabs(w4[o]) * y;
    s->Q[o] += fabs(w4[o]) * t;
    s->R[o] += fabs(w4[o]) * v;
    s->W4[o] += fabs(w4[o]);
  }
  s->Q3 += q3;
}

/* The bound from the sums over all units, asum = sum_j A_j and the output biases c. */
PG_HD float pg_sig3_bound_finish(const pg_sig3_sums *s, double asum, const double *c, int O) {
  double smax = 0.0, qmax = 0.0, rmax = 0.0, w4max = 0.0;
  int ok = asum <= PG_SIG2_CAP && s->B <= PG_SIG2_CAP && s->P <= PG_SIG2_CAP && s->Q3 <= PG_SIG2_CAP; /* false for NaN */
  for (int o = 0; o < O; ++o) {
    const double so = s->S[o] + PG_SIG3_CHAIN4 * fabs(c[o]);
    ok = ok && so <= PG_SIG2_CAP && s->Q[o] <= PG_SIG2_CAP && s->R[o] <= PG_SIG2_CAP && s->W4[o] <= PG_SIG2_CAP;
    smax = so > smax ? so : smax;
    qmax = s->Q[o] > qmax ? s->Q[o] : qmax;
    rmax = s->R[o] > rmax ? s->R[o] : rmax;
    w4max = s->W4[o] > w4max ? s->W4[o] : w4max;
  }
  if (!ok) return (float)INFINITY;
  const double u = 0x1.0p-24, eta = 0x1.0p-126;
  const double under = eta * (PG_SIG3_UNDER_Q * qmax + PG_SIG3_UNDER_R * rmax + PG_SIG3_UNDER_W4 * w4max + PG_SIG3_UNDER_C);
  return (float)((u * smax + under) * (1.0 + 0x1.0p-10));
}

/* The whole bound of one genome (numpy_nn.py:52-69 layout with bias: W1
 * [H1, 7], W2 [H2, H1 + 1], W3 [H3, H2 + 1], W4 [O, H3 + 1], bias columns
 * last), serially: what a test or a host tool calls; k_sig3's lanes run the
 * same functions on their shares.  A network wider than the layouts hold has
 * no bound: inf. */
PG_HD float pg_sig3_bound_genome(const double *g, int H1, int H2, int H3, int O) {
  double A[PG_SIG3_MAX_H], X2[PG_SIG3_MAX_H], V2[PG_SIG3_MAX_H], asum = 0.0, c[PG_SIG2_MAX_OUT];
  if (H1 > PG_SIG3_MAX_H || H2 > PG_SIG3_MAX_H || H3 > PG_SIG3_MAX_H) return (float)INFINITY;
  const double *w2 = g + (long)H1 * 7, *w3 = w2 + (long)H2 * (H1 + 1), *w4 = w3 + (long)H3 * (H2 + 1);
  pg_sig3_sums s;
  pg_sig3_sums_init(&s);
  for (int j = 0; j < H1; ++j) {
    A[j] = pg_sig2_unit1(g + (long)j * 7);
    asum += A[j];
  }
  for (int k = 0; k < H2; ++k) {
    const double *row = w2 + (long)k * (H1 + 1);
    double p = 0.0, v = 0.0;
    for (int j = 0; j < H1; ++j) {
      p += fabs(row[j]) * A[j];
      v += fabs(row[j]);
    }
    X2[k] = pg_sig3_sums_unit2(&s, p, v, row[H1]);
    V2[k] = v;
  }
  for (int l = 0; l < H3; ++l) {
    const double *row = w3 + (long)l * (H2 + 1);
    double x = 0.0, t = 0.0, v = 0.0, y[PG_SIG2_MAX_OUT];
    for (int k = 0; k < H2; ++k) {
      x += fabs(row[k]) * X2[k];
      t += fabs(row[k]) * V2[k];
      v += fabs(row[k]);
    }
    for (int o = 0; o < O; ++o) y[o] = w4[(long)o * (H3 + 1) + l];
    pg_sig3_sums_unit3(&s, x, t, v, row[H2], y, O);
  }
  for (int o = 0; o < O; ++o) c[o] = w4[(long)o * (H3 + 1) + H3];
  return pg_sig3_bound_finish(&s, asum, c, O);
}

#endif /* PG_SIG3_BOUND_H */
