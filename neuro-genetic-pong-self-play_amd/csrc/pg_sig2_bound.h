/* pg_sig2_bound.h -- the static f32 error bound of the two-hidden-layer
 * sigmoid certificate, for both layouts that hold such a network: k_sig2's
 * lanes of a wave (pg_hidden2.hpp) and k_sig2_block's 256-thread block
 * (pg_sig2_block.hip, pg_block2.hpp).  In plain C so that it compiles for the
 * device and for the host alike (tests/test_sig2_host.py and
 * tests/test_sig2_block_host.py run it under gcc).  A layout enters through
 * its three chain lengths and the constants of its underflow term,
 * pg_sig2_layout below: the derivation is written out for the lane layout,
 * and the block layout's lines follow it.
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
 *
 * The block layout (k_sig2_block; H1, H2 <= PG_SIG2_BLOCK_MAX_H = 128).  The
 * derivation above with the chain lengths c1, c2, c3 for 9, 65, 11:
 *   layer 1  PG_SIG2_BLOCK_CHAIN1 = 9:    1 (gene to f32) + 2 (the feature,
 *            feat32) + 6 fused multiply-adds
 *   layer 2  PG_SIG2_BLOCK_CHAIN2 = 129:  1 (gene) + one fused multiply-add
 *            per (padded) layer-1 unit, 128, onto the bias
 *   layer 3  PG_SIG2_BLOCK_CHAIN3 = 10:   1 (gene) + 1 (a thread's one
 *            product W3_ok h2_k) + 6 (the sum over the wave's 64 lanes) + 1 (the
 *            network's two waves) + 1 (the bias)
 * (pg_sig2_block.hip asserts them against its code.)
 *   Q_k = (9 / 4) P_k + (4.5 + 129) B_k,
 *   S_o = sum_k |W3_ok| (Q_k / 4 + 4.5 + 10) + 10 |b3_o|;
 * the second-order terms grow with gamma_129 < 2^-16.9 and stay inside the
 * 2^-16, 2^-15 and 2^-14 factors of the lines above, so inside the 2^-10.
 * Underflow, line by line for 128 padded units:
 *   a layer-1 unit: as above, <= 13 eta (1 + u) in z1^_j, a quarter of it in
 *     h1^_j, plus the sigmoid's <= 6 eta: 13 / 4 + 6 = 9.25 <= 10 eta in h1^_j;
 *   a layer-2 unit: those through |W2^_kj| (10 eta sum_j |W2_kj|), a flushed W2
 *     gene times its h1^_j <= 1 (<= 128 of them), the bias conversion and 128
 *     fmas, each error then carried through at most 128 more roundings
 *     (257 eta (1 + gamma_129) < 258 eta): <= eta (10 sum_j |W2_kj| + 258) in
 *     z2^_k, so, with the sigmoid's own <= 6 eta, <= eta (2.5 sum_j |W2_kj| +
 *     70.5) in h2^_k;
 *   an output: that through |W3^_ok| (a factor 1 + u): 3 T_o + 72 sum_k |W3_ok|;
 *     a flushed W3 gene times its h2^_k <= 1 (<= 128 of them); and every
 *     operation of the layer-3 sum, all of which feed the one output
 *     (pg_relu2_bound.h's treatment of this layout): the 128 threads' products
 *     (128 eta), the 127 additions of the tree over the two waves (127 eta;
 *     exact in the subnormal range with denormals on, as the kernels are
 *     compiled, and budgeted so that the bound also holds were results
 *     flushed), the bias conversion and the bias addition (2 eta):
 *     128 + 128 + 127 + 2 = 385 <= 400:
 *   underflow = eta (3 max_o T_o + 72 max_o sum_k |W3_ok| + 400).
 * (The lane layout's lines take a layer-1 unit's share of h1^_j as 7 eta and a
 * layer-2 unit's constant as 35 where the counts above, taken in full, give
 * 9.25 and 130 / 4 + 6 = 38.5: the sigmoid's 6 is a count of three operations
 * of which at most one can flush at a given argument.  Its constants are kept
 * as they were measured and tested; the block layout's take every line in
 * full.)
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

#define PG_SIG2_BLOCK_MAX_H 128
#define PG_SIG2_BLOCK_CHAIN1 9   /* gene + feature (2) + 6 fmas */
#define PG_SIG2_BLOCK_CHAIN2 129 /* gene + 128 fmas */
#define PG_SIG2_BLOCK_CHAIN3 10  /* gene + product + 6 lane-sum steps + the two waves + bias */

/* What the bound needs of a layout.  Its instances come by value from the two
 * functions below, so that every field is a constant where the functions are
 * inlined. */
typedef struct pg_sig2_layout {
  int chain1, chain2, chain3; /* roundings a term of layer 1, 2, 3 passes through */
  int max_h;                  /* units per hidden layer: what pg_sig2_bound_genome_l accepts */
  double under_t, under_w3, under_c; /* underflow = eta (under_t max_o T_o + under_w3 max_o sum_k |W3_ok| + under_c) */
} pg_sig2_layout;

PG_HD pg_sig2_layout pg_sig2_layout_lanes(void) {
  pg_sig2_layout l = {PG_SIG2_CHAIN1, PG_SIG2_CHAIN2, PG_SIG2_CHAIN3, PG_SIG2_MAX_H, 2.0, 36.0, 80.0};
  return l;
}

PG_HD pg_sig2_layout pg_sig2_layout_block(void) {
  pg_sig2_layout l = {PG_SIG2_BLOCK_CHAIN1, PG_SIG2_BLOCK_CHAIN2, PG_SIG2_BLOCK_CHAIN3, PG_SIG2_BLOCK_MAX_H,
                      3.0, 72.0, 400.0};
  return l;
}

/* Sums over (a share of) the layer-2 units; shares add field by field. */
typedef struct pg_sig2_sums {
  double S[PG_SIG2_MAX_OUT];  /* sum_k |W3_ok| (Q_k / 4 + 4.5 + c3) */
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

/* One layer-2 unit under layout l: p = P_k and w = sum_j |W2_kj| of its row, bias its bias weight, w3 its O
 * output weights. */
PG_HD void pg_sig2_sums_unit2_l(pg_sig2_layout l, pg_sig2_sums *s, double p, double w, double bias, const double *w3,
                                int O) {
  const double b = w + fabs(bias);
  const double q = (PG_SIG2_SLOPE * l.chain1) * p + (PG_SIG2_SIG + l.chain2) * b;
  const double t = PG_SIG2_SLOPE * q + (PG_SIG2_SIG + l.chain3);
  for (int o = 0; o < O; ++o) {
    s->S[o] += fabs(w3[o]) * t;
    s->T[o] += fabs(w3[o]) * w;
    s->W3[o] += fabs(w3[o]);
  }
  s->B += b;
  s->P += p;
}

/* The bound of layout l from the sums over all layer-2 units, asum = sum_j A_j and the output biases c. */
PG_HD float pg_sig2_bound_finish_l(pg_sig2_layout l, const pg_sig2_sums *s, double asum, const double *c, int O) {
  double smax = 0.0, tmax = 0.0, w3max = 0.0;
  int ok = asum <= PG_SIG2_CAP && s->B <= PG_SIG2_CAP && s->P <= PG_SIG2_CAP; /* false for NaN */
  for (int o = 0; o < O; ++o) {
    const double so = s->S[o] + l.chain3 * fabs(c[o]);
    ok = ok && so <= PG_SIG2_CAP && s->T[o] <= PG_SIG2_CAP && s->W3[o] <= PG_SIG2_CAP;
    smax = so > smax ? so : smax;
    tmax = s->T[o] > tmax ? s->T[o] : tmax;
    w3max = s->W3[o] > w3max ? s->W3[o] : w3max;
  }
  if (!ok) return (float)INFINITY;
  const double u = 0x1.0p-24, eta = 0x1.0p-126;
  const double under = eta * (l.under_t * tmax + l.under_w3 * w3max + l.under_c);
  return (float)((u * smax + under) * (1.0 + 0x1.0p-10));
}

/* The whole bound of one genome under layout l (numpy_nn.py:52-69 layout with
 * bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last),
 * serially: what a test or a host tool calls; k_sig2's lanes and k_sig2_block's
 * threads run the same functions on their shares.  A network wider than the
 * layout holds (H1 or H2 > l.max_h) has no bound: inf. */
PG_HD float pg_sig2_bound_genome_l(pg_sig2_layout l, const double *g, int H1, int H2, int O) {
  double A[PG_SIG2_BLOCK_MAX_H], asum = 0.0, c[PG_SIG2_MAX_OUT]; /* the larger layout's */
  if (H1 > l.max_h || H2 > l.max_h || l.max_h > PG_SIG2_BLOCK_MAX_H) return (float)INFINITY;
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
    pg_sig2_sums_unit2_l(l, &s, p, w, row[H1], v, O);
  }
  for (int o = 0; o < O; ++o) c[o] = w3[(long)o * (H2 + 1) + H2];
  return pg_sig2_bound_finish_l(l, &s, asum, c, O);
}

/* The lane layout's, under their earlier names and signatures (k_sig2, pg_hidden2.hpp; H1 <= PG_SIG2_MAX_H). */
PG_HD void pg_sig2_sums_unit2(pg_sig2_sums *s, double p, double w, double bias, const double *w3, int O) {
  pg_sig2_sums_unit2_l(pg_sig2_layout_lanes(), s, p, w, bias, w3, O);
}

PG_HD float pg_sig2_bound_finish(const pg_sig2_sums *s, double asum, const double *c, int O) {
  return pg_sig2_bound_finish_l(pg_sig2_layout_lanes(), s, asum, c, O);
}

PG_HD float pg_sig2_bound_genome(const double *g, int H1, int H2, int O) {
  return pg_sig2_bound_genome_l(pg_sig2_layout_lanes(), g, H1, H2, O);
}

#endif /* PG_SIG2_BOUND_H */
