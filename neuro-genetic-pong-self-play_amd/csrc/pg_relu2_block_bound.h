/* pg_relu2_block_bound.h -- the static f32 error bound of k_relu2_block's
 * certificate (pg_relu2_block.hip), in plain C so that it compiles for the
 * device and for the host alike (tests/test_relu2_block_host.py runs it under
 * gcc).
 *
 * The network, the quantities A_j, B_k, S_o, T_o and the derivation are
 * pg_relu2_bound.h's: it does not depend on the order of any sum, only on the
 * number of roundings c a term of a computed dot product passes through
 * (gamma_c = c u / (1 - c u), u = 2^-24).  This layout's three chain lengths:
 *
 *   layer 1  PG_RELU2_BLOCK_CHAIN1 = 9:    1 (gene to f32) + 2 (the feature,
 *            feat32) + 6 fused multiply-adds
 *   layer 2  PG_RELU2_BLOCK_CHAIN2 = 129:  1 (gene) + one fused multiply-add
 *            per (padded) layer-1 unit, 128, onto the bias
 *   layer 3  PG_RELU2_BLOCK_CHAIN3 = 10:   1 (gene) + 1 (a thread's one
 *            product W3_ok h2_k) + 6 (the sum over the wave's 64 lanes) + 1 (the
 *            network's two waves) + 1 (the bias)
 * (pg_relu2_block.hip asserts its reduction against CHAIN3.)  So
 *   |h1^_j - h1_j| <= gamma_9 A_j
 *   |z2^_k - z2_k| <= gamma_(9 + 129) B_k = gamma_138 B_k
 *   |z^_o - z_o|   <= gamma_(138 + 10) S_o = gamma_148 S_o
 * and, with numpy's own f64 result within 2^-16 u S_o of the exact z_o,
 *   e = (K u max_o S_o + underflow) (1 + 2^-20),
 *   K = PG_RELU2_BLOCK_K = 9 + 129 + 10 + 2 = 150:
 * two u of slack for gamma_148 - 148 u (= 148^2 u^2 / (1 - 148 u) < 2 10^-3 u),
 * the f64 part and the f64 rounding of S_o itself, and 2^-20 for the
 * conversion of e to f32, as there.
 *
 * Underflow, eta = 2^-126 per operation whose result is subnormal or flushed:
 *   a layer-1 unit: 7 gene conversions and 6 fmas, <= 13 eta (1 + u) in h1^_j
 *     (unchanged);
 *   a layer-2 unit: those through |W2^_kj| (<= 14 eta sum_j |W2_kj|), a flushed
 *     W2 gene times its h1^_j (<= 2 eta A_j each), the bias conversion and
 *     128 fmas, each error then carried through at most 128 more roundings
 *     (129 eta (1 + gamma_129) < 130 eta):
 *     E2_k <= eta (14 sum_j |W2_kj| + 2 sum_j A_j + 131);
 *   an output: E2_k through |W3^_ok| (a factor 1 + u: 15, 132), a flushed W3
 *     gene times its h2^_k (<= 2 eta B_k), and every operation of the layer-3
 *     sum, all of which feed the one output: the 128 threads' products
 *     W3^_ok h2^_k (128 eta), the 127 additions of the tree over the two waves
 *     (126 in the waves, 1 across them: 127 eta -- with denormals on, as the
 *     kernels are compiled, an f32 addition is exact in the subnormal range and
 *     loses nothing; they are budgeted so that the bound also holds were
 *     results flushed), and the bias conversion and the bias addition, under
 *     the 16 kept from there:
 *   underflow = eta (15 max_o T_o + (2 sum_j A_j + 132) max_o sum_k |W3_ok| + 2 sum_k B_k + 128 + 127 + 16).
 * Overflow: PG_RELU_CAP on every sum, as there; otherwise e = inf and the f64
 * path (numpy's semantics, NaN rule included) decides every frame.
 */
#ifndef PG_RELU2_BLOCK_BOUND_H
#define PG_RELU2_BLOCK_BOUND_H

#include <math.h>

#include "pg_relu2_bound.h" /* pg_relu2_sums and its functions, PG_HD, PG_RELU_CAP, PG_RELU_MAX_OUT */

#define PG_RELU2_BLOCK_MAX_H 128
#define PG_RELU2_BLOCK_CHAIN1 9   /* gene + feature (2) + 6 fmas */
#define PG_RELU2_BLOCK_CHAIN2 129 /* gene + 128 fmas */
#define PG_RELU2_BLOCK_CHAIN3 10  /* gene + product + 6 lane-sum steps + the two waves + bias */
#define PG_RELU2_BLOCK_K \
  ((double)(PG_RELU2_BLOCK_CHAIN1 + PG_RELU2_BLOCK_CHAIN2 + PG_RELU2_BLOCK_CHAIN3 + 2))

/* The bound from the sums over all layer-2 units (pg_relu2_sums_unit2), asum = sum_j A_j and the output biases c. */
PG_HD float pg_relu2_block_bound_finish(const pg_relu2_sums *s, double asum, const double *c, int O) {
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
  const double under = eta * (15.0 * tmax + (2.0 * asum + 132.0) * w3max + 2.0 * s->B + 271.0);
  return (float)((PG_RELU2_BLOCK_K * u * smax + under) * (1.0 + 0x1.0p-20));
}

/* The whole bound of one genome (numpy_nn.py:52-69 layout with bias), serially:
 * what a test or a host tool calls; k_relu2_block's threads run the same
 * functions on their units.  H1 <= PG_RELU2_BLOCK_MAX_H. */
PG_HD float pg_relu2_block_bound_genome(const double *g, int H1, int H2, int O) {
  double A[PG_RELU2_BLOCK_MAX_H], asum = 0.0, c[PG_RELU_MAX_OUT];
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
  return pg_relu2_block_bound_finish(&s, asum, c, O);
}

#endif /* PG_RELU2_BLOCK_BOUND_H */
