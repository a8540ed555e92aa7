// pg_relu2.hip -- k_relu2: evaluate() (main.py:28-66) for [6, H1 <= 64,
// H2 <= 64, 2..4] ReLU networks with bias (two hidden layers; activation_function
// = ReLU, numpy_nn.py:6-9, 26), and pg_relu2_decide, its decision code on given
// inputs (include/pong_ga.h).
//
//   k_relu2<LN, U1, U2, O, WT>  the certified families' game loop
//                         (pg_certgame.hpp) with Relu2Policy (pg_hidden2.hpp):
//                         all three layers as f32 in VGPRs for the whole game,
//                         so HBM is touched once per game.  Each frame: the
//                         f32 chain (layer 1's activations all-gathered through
//                         the half-group's LDS row), the certificate under the
//                         network's static bound (pg_relu2_bound.h), and for the
//                         undecided half-groups the f64 forward in numpy's
//                         order from the genes.
// This file holds the family's kernels, its description (pg_family.hpp; what it
// shares with k_sig2's is pg_hidden2.hpp's Hidden2Family), its row of the family
// table and its C entry point.  Compiled a second time with -DPG_SOLO_UNIT
// (pong_amd/build.py) it holds k_relu2_solo and k_relu2_adv_solo
// (PG_KERNEL_SOLO) and nothing else, so this unit's kernels are what they were
// without them.  DESIGN.md 4.2d, 4.2g.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_certgame.hpp"
#include "pg_eval.hpp"
#include "pg_family.hpp"
#include "pg_hidden2.hpp"

namespace pg {

#ifdef PG_SOLO_UNIT
// k_relu2 and k_relu2_adv with a half-group per game against a scripted opponent
// (PG_KERNEL_SOLO; pg_certgame.hpp)
template <int LN, int U1, int U2, int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_relu2_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu2Policy<LN, U1, U2, O, WT>, false, true>(p);
}

template <int LN, int U1, int U2, int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_relu2_adv_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu2Policy<LN, U1, U2, O, WT>, true, true>(p);
}

void relu2_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p) {
  if (advance) PG_HIDDEN2_DISPATCH(k_relu2_adv_solo, LN, O, f64, grid, s, p);
  else PG_HIDDEN2_DISPATCH(k_relu2_solo, LN, O, f64, grid, s, p);
}

}  // namespace pg
#else
template <int LN, int U1, int U2, int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_relu2(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu2Policy<LN, U1, U2, O, WT>, false>(p);
}

// k_relu2 with the serve delays and periodic rallies advanced in closed form
// (PG_KERNEL_ADVANCE, untraced launches; pg_certgame.hpp)
template <int LN, int U1, int U2, int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_relu2_adv(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu2Policy<LN, U1, U2, O, WT>, true>(p);
}

template <int LN, int U1, int U2, int O, typename WT>
__global__ __launch_bounds__(256) void k_relu2_decide(CertDecideParams p) {
  constexpr int HPB = 256 / LN;
  for (long base = (long)blockIdx.x * HPB; base < p.n; base += (long)gridDim.x * HPB)
    cert_decide_pass<Relu2Policy<LN, U1, U2, O, WT>>(p, base);
}

struct Relu2Family : Hidden2Family {
  static constexpr int kKernel = PG_KERNEL_RELU2, kActivation = PG_ACT_RELU;
  static constexpr const char *kName = "relu2";
  static constexpr const char *kBadActivation = "activation sigmoid: the relu2 kernel evaluates PG_ACT_RELU networks only";
  static constexpr const char *kBadShape = "relu2 kernel needs NETWORK_SHAPE [6, 2..64, 2..64, 2..4] with bias";
  static constexpr const char *kNoBias = kBadShape;
  static constexpr const char *kDecideBadActivation =
      "pg_relu2_decide: activation=%d, the relu2 kernel decides PG_ACT_RELU networks only";
  static constexpr const char *kDecideBadShape =
      "pg_relu2_decide: the relu2 kernel's shapes [6, 2..64, 2..64, 2..4] with bias only";
  static constexpr const char *kDecideNoBias = kDecideBadShape;
  static void game(const EvalParams &p, bool f64, bool advance, bool solo, int grid, hipStream_t s) {
    const int LN = lanes(p.nodes), O = p.nodes[3];
    if (solo) relu2_solo_game(LN, O, f64, advance, grid, s, p);
    else if (advance) PG_HIDDEN2_DISPATCH(k_relu2_adv, LN, O, f64, grid, s, p);
    else PG_HIDDEN2_DISPATCH(k_relu2, LN, O, f64, grid, s, p);
  }
  static void decide(const int32_t *nodes, bool f64, int grid, hipStream_t s, const DecideParams &p) {
    PG_HIDDEN2_DISPATCH(k_relu2_decide, lanes(nodes), nodes[3], f64, grid, s, p);
  }
};

bool relu2_shape_ok(const pg_net &n) { return Relu2Family::shape_ok(n.n_nodes, n.nodes) && n.bias != 0; }

FamilyDesc relu2_family() { return family_desc<Relu2Family>(); }

}  // namespace pg

extern "C" int32_t pg_relu2_decide(const pg_relu_decide_args *a, void *stream) {
  return pg::family_decide<pg::Relu2Family>(a, stream);
}
#endif  // PG_SOLO_UNIT
