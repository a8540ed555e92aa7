/* pg_sig2_bound.h -- the static f32 error bound of k_sig2's certificate
 * (pg_hidden2.hpp), in plain C so that it compiles for the device and for the
 * host alike (tests/test_sig2_host.py runs it under gcc).
 *
 * The network [6, H1, H2, O] with bias, inputs x_i = k_i / 320 in [0, 1],
 * s(z) = 1 / (1 + e^-z):
 *   z1_j = sum_i W1_ji x_i + b1_j,   h1_j = s(z1_j)
 *   z2_k = sum_j W2_kj h1_j + b2_k,  h2_k = s(z2_k)
 *   z_o  = sum_k W3_ok h2_k + b3_o.
 * e bounds |z^_o - znp_o|: z^ k_sig2's f32 output pre-activation, znp the f64
 * pre-activation numpy computes (the argument of its last sigmoid), which is
 * what certify / tight_gap_move / plateau_f32 (pg_cascade.hpp) ask for.
 *
 * Sums.  The derivation does not depend on the order of any sum: if every
 * term of a computed dot product passes through at most c roundings (factors
 * 1 + d, |d| <= u = 2^-24), the result differs from the exact sum by at most
 * gamma_c sum_i |t_i|, gamma_c = c u / (1 - c u), whatever the order.  The
 * chain lengths are k_relu2's (the layout is the same; pg_hidden2.hpp asserts that
 * every instantiated layout stays within them):
 *   layer 1  PG_SIG2_CHAIN1 = 9:   1 (gene to f32) + 2 (the feature
 *            fl32(k * fl32(1 / 320)), feat32) + 6 fused multiply-adds
 *   layer 2  PG_SIG2_CHAIN2 = 65:  1 (gene) + one fused multiply-add per
 *            (padded) layer-1 unit, <= 64, onto the bias
 *   layer 3  PG_SIG2_CHAIN3 = 11:  1 (gene) + a lane's <= 4 units + the sum
 *            over <= 32 lanes (5 steps) + the bias
 * Sigmoid.  sigmoid_f32(a) = v_rcp_f32(1 + v_exp_f32(a * -log2 e)) is allowed
 * PG_SIG2_SIG = 4.5 u of absolute error of its own at every a, the allowance of
 * load_net (pg_cascade.hpp): the product's rounding moves the result by at most
 * 1.5 u |a| s (1 - s) <= 0.34 u, v_exp_f32 (1 ulp = 2 u relative on q = e^-a,
 * q / (1 + q)^2 <= 1/4) by 0.5 u, the add by u and v_rcp_f32 (1 ulp) by 2 u: 3.84 u.
 * Where v_exp_f32 overflows or flushes, the result is 0 or 1 and the true value
 * within 2^-126 of it (the underflow term below).  The sigmoid's slope is <= 1/4
 * and its value in [0, 1]; the computed one is in [0, 1] as well.
 *
 * With  A_j = sum_i |W1_ji| + |b1_j|           (>= |z1_j|, as x_i <= 1)
 *       P_k = sum_j |W2_kj| A_j
 *       B_k = sum_j |W2_kj| + |b2_k|           (>= |z2_k|, as |h1_j| <= 1)
 *   |z1^_j - z1_j| <= gamma_9 A_j
 *   |h1^_j - h1_j| <= gamma_9 A_j / 4 + 4.5 u
 *   |z2^_k - z2_k| <= sum_j |W2_kj| ((gamma_9 A_j / 4 + 4.5 u)(1 + gamma_65) + gamma_65) + gamma_65 |b2_k|
 *                  <= u Q_k (1 + 2^-16),   Q_k = (9 / 4) P_k + (4.5 + 65) B_k
 *   |h2^_k - h2_k| <= u Q_k (1 + 2^-16) / 4 + 4.5 u
 *   |z^_o - z_o|   <= sum_k |W3_ok| ((u Q_k / 4 + 4.5 u)(1 + 2^-15) + gamma_11) + gamma_11 |b3_o|
 *                  <= u S_o (1 + 2^-14),   S_o = sum_k |W3_ok| (Q_k / 4 + 4.5 + 11) + 11 |b3_o|.
 * A padding unit has activation s(0) = 0.5, not 0: its outgoing weights are
 * exactly zero, fma(0, 0.5, a) = a, so it adds nothing to a sum or to its error.
 * numpy's own f64 values differ from the exact ones by the same recurrence with
 * 2^-53 for u and constants of the same size (np.dot over <= 65 terms, the
 * features' roundings, np.e ** -z within an ulp, np.e for e: <= 0.23 x 2^-53
 * on s): less than 2^-25 of the above.  The bound kept:
 *   e = (u max_o S_o + underflow) (1 + 2^-10):
 * the 2^-10 covers the 2^-14 above, the f64 part, the f64 rounding of the sums
 * themselves (non-negative terms: relative error below 2^-40 whatever the
 * order, the lanes' partial sums and the host's serial loop alike), the
 * conversion of e to f32 and the f32 roundings of make_cert's forms of e.
 * Underflow.  The above holds for normal results.  Every operation whose
 * result is subnormal or flushed to zero adds at most eta = 2^-126:
 *   a layer-1 unit: 7 gene conversions and 6 fmas, <= 13 eta (1 + u) in z1^_j,
 *     a quarter of it in h1^_j, plus the sigmoid's product, v_exp_f32 and
 *     v_rcp_f32: <= 6 eta in h1^_j;
 *   a layer-2 unit: those through |W2^_kj|, a flushed W2 gene times its h1^_j
 *     <= 1, the bias conversion and <= 64 fmas: <= eta (7 sum_j |W2_kj| + 130)
 *     in z2^_k, so <= eta (1.75 sum_j |W2_kj| + 35) in h2^_k;
 *   an output: that through |W3^_ok|, a flushed W3 gene times its h2^_k <= 1
 *     (<= 64 of them), the <= 11 operations of the layer-3 chain and the bias:
 *   underflow = eta (2 max_o T_o + 36 max_o sum_k |W3_ok| + 80),
 *     T_o = sum_k |W3_ok| sum_j |W2_kj|.
 * (A feature k_i * fl32(1/320) is 0 or >= 2^-9: never subnormal.)
 * Overflow.  With sum_j A_j, sum_k P_k, sum_k B_k, sum_k |W3_ok|, T_o and S_o
 * all <= PG_SIG2_CAP = 1e25 (sums of absolute values: NaN and inf propagate
 * into them and fail the test) every gene converts to a finite f32, every
 * pre-activation is at most A_j, B_k or sum_k |W3_ok| + |b3_o| times
 * (1 + gamma) < FLT_MAX / 2 (so a * -log2 e is finite too), every activation is
 * in [0, 1] and z^ is finite.  Otherwise e = inf: the certificate and the
 * in-register rules then never decide and the f64 path (numpy's semantics, NaN
 * rule included) does.
 */
#ifndef PG_SIG2_BOUND_H
#define PG_SIG2_BOUND_H

#include <math.h>

#ifndef PG_HD
#if defined(__HIPCC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD static inline
#endif
#endif

#define PG_SIG2_MAX_H 64
#define PG_SIG2_MAX_OUT 4
#define PG_SIG2_CHAIN1 9   /* gene + feature (2) + 6 fmas */
#define PG_SIG2_CHAIN2 65  /* gene + <= 64 fmas */
#define PG_SIG2_CHAIN3 11  /* gene + <= 4 fmas + <= 5 lane-sum steps + bias */
#define PG_SIG2_SIG 4.5    /* sigmoid_f32's own absolute error, in u (load_net's allowance) */
#define PG_SIG2_SLOPE 0.25 /* the sigmoid's largest slope */
#define PG_SIG2_CAP 1e25

/* Sums over (a share of) the layer-2 units; shares add field by field. */
typedef struct pg_sig2_sums {
  double S[PG_SIG2_MAX_OUT];  /* sum_k |W3_ok| (Q_k / 4 + 4.5 + 11) */
  double T[PG_SIG2_MAX_OUT];  /* sum_k |W3_ok| sum_j |W2_kj| */
  double W3[PG_SIG2_MAX_OUT]; /* sum_k |W3_ok| */
  double B;                   /* sum_k B_k */
  double P;                   /* sum_k P_k */
} pg_sig2_sums;

PG_HD void pg_sig2_sums_init(pg_sig2_sums *s) {
  for (int o = 0; o < PG_SIG2_MAX_OUT; ++o) s->S[o] = s->T[o] = s->W3[o] = 0.0;
  s->B = s->P = 0.0;
}

/* A_j of one layer-1 unit: its 6 input weights and its bias weight. */
PG_HD double pg_sig2_unit1(const double w1[7]) {
  double a = 0.0;
  for (int i = 0; i < 7; ++i) a += fabs(w1[i]);
  return a;
}

/* One layer-2 unit: p = P_k and w = sum_j |W2_kj| of its row, bias its bias weight, w3 its O output weights. */
PG_HD void pg_sig2_sums_unit2(pg_sig2_sums *s, double p, double w, double bias, const double *w3, int O) {
  const double b = w + fabs(bias);
  const double q = (PG_SIG2_SLOPE * PG_SIG2_CHAIN1) * p + (PG_SIG2_SIG + PG_SIG2_CHAIN2) * b;
  const double t = PG_SIG2_SLOPE * q + (PG_SIG2_SIG + PG_SIG2_CHAIN3);
  for (int o = 0; o < O; ++o) {
    s->S[o] += fabs(w3[o]) * t;
    s->T[o] += fabs(w3[o]) * w;
    s->W3[o] += fabs(w3[o]);
  }
  s->B += b;
  s->P += p;
}

/* The bound from the sums over all layer-2 units, asum = sum_j A_j and the output biases c. */
PG_HD float pg_sig2_bound_finish(const pg_sig2_sums *s, double asum, const double *c, int O) {
  double smax = 0.0, tmax = 0.0, w3max = 0.0;
  int ok = asum <= PG_SIG2_CAP && s->B <= PG_SIG2_CAP && s->P <= PG_SIG2_CAP; /* false for NaN */
  for (int o = 0; o < O; ++o) {
    const double so = s->S[o] + PG_SIG2_CHAIN3 * fabs(c[o]);
    ok = ok && so <= PG_SIG2_CAP && s->T[o] <= PG_SIG2_CAP && s->W3[o] <= PG_SIG2_CAP;
    smax = so > smax ? so : smax;
    tmax = s->T[o] > tmax ? s->T[o] : tmax;
    w3max = s->W3[o] > w3max ? s->W3[o] : w3max;
  }
  if (!ok) return (float)INFINITY;
  const double u = 0x1.0p-24, eta = 0x1.0p-126;
  const double under = eta * (2.0 * tmax + 36.0 * w3max + 80.0);
  return (float)((u * smax + under) * (1.0 + 0x1.0p-10));
}

/* The whole bound of one genome (numpy_nn.py:52-69 layout with bias: W1
 * [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last), serially:
 * what a test or a host tool calls; k_sig2's lanes run the same functions on
 * their shares.  H1 <= PG_SIG2_MAX_H. */
PG_HD float pg_sig2_bound_genome(const double *g, int H1, int H2, int O) {
  double A[PG_SIG2_MAX_H], asum = 0.0, c[PG_SIG2_MAX_OUT];
  const double *w2 = g + (long)H1 * 7, *w3 = w2 + (long)H2 * (H1 + 1);
  pg_sig2_sums s;
  pg_sig2_sums_init(&s);
  for (int j = 0; j < H1; ++j) {
    A[j] = pg_sig2_unit1(g + (long)j * 7);
    asum += A[j];
  }
  for (int k = 0; k < H2; ++k) {
    const double *row = w2 + (long)k * (H1 + 1);
    double p = 0.0, w = 0.0, v[PG_SIG2_MAX_OUT];
    for (int j = 0; j < H1; ++j) {
      p += fabs(row[j]) * A[j];
      w += fabs(row[j]);
    }
    for (int o = 0; o < O; ++o) v[o] = w3[(long)o * (H2 + 1) + k];
    pg_sig2_sums_unit2(&s, p, w, row[H1], v, O);
  }
  for (int o = 0; o < O; ++o) c[o] = w3[(long)o * (H2 + 1) + H2];
  return pg_sig2_bound_finish(&s, asum, c, O);
}

#endif /* PG_SIG2_BOUND_H */
