// pg_relu3.hip -- k_relu3: evaluate() (main.py:28-66) for [6, H1 <= 32,
// H2 <= 32, H3 <= 32, 2..4] ReLU networks with bias (three hidden layers;
// activation_function = ReLU, numpy_nn.py:6-9, 26), and pg_relu3_decide, its
// decision code on given inputs (include/pong_ga.h).
//
//   k_relu3<LN, U, O, WT>  the certified families' game loop (pg_certgame.hpp)
//                         with Relu3Policy (pg_hidden3.hpp): all four layers
//                         as f32 in VGPRs for the whole game, so HBM is touched
//                         once per game.  Each frame: the f32 chain (layer 1's
//                         and layer 2's activations all-gathered through the
//                         half-group's two LDS rows), the certificate under the
//                         network's static bound (pg_relu3_bound.h), and for the
//                         undecided half-groups the f64 forward in numpy's
//                         order from the genes.
// This file holds the family's kernels, its description (pg_family.hpp; what it
// shares with k_sig3's is pg_hidden3.hpp's Hidden3Family), its row of the family
// table and its C entry point.  Compiled a second time with -DPG_SOLO_UNIT
// (pong_amd/build.py) it holds k_relu3_solo and k_relu3_adv_solo
// (PG_KERNEL_SOLO) and nothing else, as pg_relu2.hip does.  DESIGN.md 4.2m.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_certgame.hpp"
#include "pg_eval.hpp"
#include "pg_family.hpp"
#include "pg_hidden3.hpp"

namespace pg {

// Blocks per CU the game kernels are compiled for: two.  The 16-lane layout's
// 158 weights per lane do not all stay in 256 VGPRs: at two blocks its kernels
// spill 11 to 66 VGPRs, nearly all in the load and the f64 path, one or two
// reloads on the frame's common path; at one block (PG_RELU3_BLOCKS16=1 in a
// variant build, tools/build_variant.py) they use 264 to 278 registers without
// any scratch access and measure 1.6 times slower at 65 536 genomes (106.7 ms
// against 66.9 ms at [6, 32, 32, 32, 3]), so two it is.
#ifndef PG_RELU3_BLOCKS16
#define PG_RELU3_BLOCKS16 2
#endif
__host__ __device__ constexpr int relu3_blocks(int LN) { return LN == 8 ? 2 : PG_RELU3_BLOCKS16; }

#ifdef PG_SOLO_UNIT
// k_relu3 and k_relu3_adv with a half-group per game against a scripted opponent
// (PG_KERNEL_SOLO; pg_certgame.hpp)
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, relu3_blocks(LN)) void k_relu3_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu3Policy<LN, U, O, WT>, false, true>(p);
}

template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, relu3_blocks(LN)) void k_relu3_adv_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu3Policy<LN, U, O, WT>, true, true>(p);
}

void relu3_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p) {
  if (advance) PG_HIDDEN3_DISPATCH(k_relu3_adv_solo, LN, O, f64, grid, s, p);
  else PG_HIDDEN3_DISPATCH(k_relu3_solo, LN, O, f64, grid, s, p);
}

}  // namespace pg
#else
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, relu3_blocks(LN)) void k_relu3(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu3Policy<LN, U, O, WT>, false>(p);
}

// k_relu3 with the serve delays and periodic rallies advanced in closed form
// (PG_KERNEL_ADVANCE, untraced launches; pg_certgame.hpp)
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, relu3_blocks(LN)) void k_relu3_adv(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Relu3Policy<LN, U, O, WT>, true>(p);
}

template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256) void k_relu3_decide(Hidden3DecideParams p) {
  constexpr int HPB = 256 / LN;
  for (long base = (long)blockIdx.x * HPB; base < p.n; base += (long)gridDim.x * HPB)
    cert_decide_pass<Relu3Policy<LN, U, O, WT>>(p, base);
}

struct Relu3Family : Hidden3Family {
  static constexpr int kKernel = PG_KERNEL_RELU3, kActivation = PG_ACT_RELU;
  static constexpr const char *kName = "relu3";
  static constexpr const char *kBadActivation = "activation sigmoid: the relu3 kernel evaluates PG_ACT_RELU networks only";
  static constexpr const char *kBadShape = "relu3 kernel needs NETWORK_SHAPE [6, 2..32, 2..32, 2..32, 2..4] with bias";
  static constexpr const char *kNoBias = kBadShape;
  static constexpr const char *kDecideBadActivation =
      "pg_relu3_decide: activation=%d, the relu3 kernel decides PG_ACT_RELU networks only";
  static constexpr const char *kDecideBadShape =
      "pg_relu3_decide: the relu3 kernel's shapes [6, 2..32, 2..32, 2..32, 2..4] with bias only";
  static constexpr const char *kDecideNoBias = kDecideBadShape;
  static void game(const EvalParams &p, bool f64, bool advance, bool solo, int grid, hipStream_t s) {
    const int LN = lanes(p.nodes), O = p.nodes[4];
    if (solo) relu3_solo_game(LN, O, f64, advance, grid, s, p);
    else if (advance) PG_HIDDEN3_DISPATCH(k_relu3_adv, LN, O, f64, grid, s, p);
    else PG_HIDDEN3_DISPATCH(k_relu3, LN, O, f64, grid, s, p);
  }
  static void decide(const int32_t *nodes, bool f64, int grid, hipStream_t s, const DecideParams &p) {
    PG_HIDDEN3_DISPATCH(k_relu3_decide, lanes(nodes), nodes[4], f64, grid, s, p);
  }
};

FamilyDesc relu3_family() { return family_desc<Relu3Family>(); }

}  // namespace pg

extern "C" int32_t pg_relu3_decide(const pg_relu_decide_args *a, void *stream) {
  return pg::family_decide<pg::Relu3Family>(a, stream);
}
#endif  // PG_SOLO_UNIT
