/* pg_relu_bound.h -- the static f32 error bound of k_relu's certificate
 * (pg_relu.hpp), in plain C so that it compiles for the device and for the
 * host alike (tests/test_relu_host.py runs it under gcc).
 *
 * The network: z1_j = sum_i W1_ji x_i + b1_j, h_j = max(0, z1_j),
 * z_o = sum_j W2_oj h_j + b2_o, inputs x_i = k_i / 320 in [0, 1] (doubled
 * centroids k_i in [0, 320], utils.py:139-153).  k_relu evaluates it in f32 in
 * this order (u = 2^-24, gamma_n = n u / (1 - n u)):
 *
 *   w^ = fl32(w)                              1 rounding per gene
 *   x^_i = fl32(k_i * fl32(1 / 320))          2 roundings (feat32; k_i is exact)
 *   z1^_j = fma(w^_5, x^_5, ... fma(w^_0, x^_0, b1^_j))   6 fused roundings
 *   h^_j = max(0, z1^_j)                      exact, 1-Lipschitz
 *   a lane's partial sum over its U units u = 0..U-1 from 0:
 *       acc_o = fma(w2^_oj, h^_j, acc_o)      <= U roundings
 *   the sum over the LN lanes of the half-group (group_sum)  log2 LN roundings
 *   z^_o = that + b2^_o                       1 rounding
 *
 * Hidden layer.  Every term of z1^_j carries at most 1 (gene) + 2 (feature)
 * + 6 (fma) = 9 factors (1 + d), |d| <= u, so with
 *   A_j = sum_i |W1_ji| + |b1_j|   (>= sum_i |W1_ji| x_i + |b1_j|, x_i <= 1)
 *   |z1^_j - z1_j| <= gamma_9 A_j,  |h^_j - h_j| <= gamma_9 A_j,  |h^_j| <= (1 + gamma_9) A_j.
 * Output layer.  Term j carries 1 (gene) + U (fma) + log2 LN + 1 <= 22
 * factors for U = 16, LN <= 16, the bias term 2:
 *   |z^_o - z_o| <= sum_j |W2_oj| (gamma_9 A_j (1 + gamma_22) + gamma_22 (1 + gamma_9) A_j) + gamma_2 |b2_o|
 *               <= (31 u + O(u^2)) S_o,   S_o = sum_j |W2_oj| A_j + |b2_o|.
 * numpy's own f64 result differs from the exact z_o by the roundings of its
 * two np.dot calls and of the features (k / 2) / 160: <= gamma64_(H + 20) S_o
 * < 2^-44 S_o for H <= 256, i.e. < 2^-20 u S_o.  The bound kept is
 *   e = (33 u max_o S_o + underflow) (1 + 2^-20):
 * two u of slack over the 31 above for the O(u^2) terms, the f64 part and the
 * f64 rounding of S_o itself (a sum of <= 8 H + 1 non-negative terms,
 * relative error <= gamma64_(8 H + 1) whatever the order: the lanes' partial
 * sums and the host's serial loop both stay inside), and 2^-20 for the final
 * conversion of e to f32.
 * Underflow.  The analysis above holds for normal results.  Every operation
 * whose result is subnormal (rounded with absolute error <= 2^-150, or flushed
 * to zero: <= 2^-126) adds at most eta = 2^-126: per hidden unit 7 gene
 * conversions and 6 fmas, passed on with factors x_i <= 1 and |W2_oj| (<= 13
 * eta sum_j |W2_oj| (1 + u)); a flushed W2 gene times its h_j (<= eta (1 +
 * gamma_9) sum_j A_j); the U fmas per lane, log2 LN adds, the bias conversion and the
 * bias add of the output (<= (units + 6) eta):
 *   underflow = eta (16 max_o sum_j |W2_oj| + 2 sum_j A_j + units + 16).
 * (A feature k_i * fl32(1/320) is 0 or >= 2^-9: never subnormal.)
 * Overflow.  With sum_j A_j, sum_j |W2_oj| and S_o all <= 1e25 (sums of
 * absolute values: NaN and inf propagate into them and fail the test) every
 * gene converts to a finite f32 and no intermediate exceeds S_o (1 + gamma)
 * < FLT_MAX, so z^ is finite and the certificate needs no NaN test.  Otherwise
 * e = inf: the certificate then never decides and the f64 path (numpy's
 * semantics, NaN rule included) does.
 */
#ifndef PG_RELU_BOUND_H
#define PG_RELU_BOUND_H

#include <math.h>

#ifndef PG_HD
#if defined(__HIPCC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD static inline
#endif
#endif

#define PG_RELU_MAX_OUT 4
#define PG_RELU_K 33.0          /* e = PG_RELU_K u max_o S_o + ... (see above) */
#define PG_RELU_CHAIN_MAX 22    /* 1 + U + log2 LN + 1 the derivation allows */
#define PG_RELU_CAP 1e25

/* Sums over (a share of) the hidden units; shares add field by field. */
typedef struct pg_relu_sums {
  double S[PG_RELU_MAX_OUT];   /* sum_j |W2_oj| A_j */
  double W2[PG_RELU_MAX_OUT];  /* sum_j |W2_oj| */
  double A;                    /* sum_j A_j */
} pg_relu_sums;

PG_HD void pg_relu_sums_init(pg_relu_sums *s) {
  for (int o = 0; o < PG_RELU_MAX_OUT; ++o) s->S[o] = s->W2[o] = 0.0;
  s->A = 0.0;
}

/* One hidden unit: its 6 input weights and bias weight w1, its O output weights w2. */
PG_HD void pg_relu_sums_unit(pg_relu_sums *s, const double w1[7], const double *w2, int O) {
  double a = 0.0;
  for (int i = 0; i < 7; ++i) a += fabs(w1[i]);
  for (int o = 0; o < O; ++o) {
    s->S[o] += fabs(w2[o]) * a;
    s->W2[o] += fabs(w2[o]);
  }
  s->A += a;
}

/* The bound from the sums over all hidden units, the output biases c and the
 * number of (padded) hidden units a half-group evaluates. */
PG_HD float pg_relu_bound_finish(const pg_relu_sums *s, const double *c, int O, int units) {
  double smax = 0.0, w2max = 0.0;
  int ok = s->A <= PG_RELU_CAP;  /* false for NaN */
  for (int o = 0; o < O; ++o) {
    const double so = s->S[o] + fabs(c[o]);
    ok = ok && so <= PG_RELU_CAP && s->W2[o] <= PG_RELU_CAP;
    smax = so > smax ? so : smax;
    w2max = s->W2[o] > w2max ? s->W2[o] : w2max;
  }
  if (!ok) return (float)INFINITY;
  const double u = 0x1.0p-24, eta = 0x1.0p-126;
  const double under = eta * (16.0 * w2max + 2.0 * s->A + (double)units + 16.0);
  return (float)((PG_RELU_K * u * smax + under) * (1.0 + 0x1.0p-20));
}

/* The whole bound of one genome (numpy_nn.py:52-69 layout with bias: W1
 * [H, 7] then W2 [O, H + 1], bias column last), serially: what a test or a
 * host tool calls; k_relu's lanes run the same three functions on their shares. */
PG_HD float pg_relu_bound_genome(const double *g, int H, int O, int units) {
  pg_relu_sums s;
  pg_relu_sums_init(&s);
  const double *v = g + (long)H * 7;
  double c[PG_RELU_MAX_OUT];
  for (int j = 0; j < H; ++j) {
    double w2[PG_RELU_MAX_OUT];
    for (int o = 0; o < O; ++o) w2[o] = v[(long)o * (H + 1) + j];
    pg_relu_sums_unit(&s, g + (long)j * 7, w2, O);
  }
  for (int o = 0; o < O; ++o) c[o] = v[(long)o * (H + 1) + H];
  return pg_relu_bound_finish(&s, c, O, units);
}

#endif /* PG_RELU_BOUND_H */
