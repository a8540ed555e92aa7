// pg_sig3.hip -- k_sig3: evaluate() (main.py:28-66) for [6, H1 <= 32,
// H2 <= 32, H3 <= 32, 2..4] sigmoid networks with bias (three hidden layers; the
// reference's default activation, numpy_nn.py:22-26), and pg_sig3_decide, its
// decision code on given inputs (include/pong_ga.h).
//
//   k_sig3<LN, U, O, WT>  the certified families' game loop (pg_certgame.hpp)
//                         with Sig3Policy (pg_sig3.hpp): k_relu3's layout, all
//                         four layers as f32 in VGPRs for the whole game, so HBM
//                         is touched once per game.  Each frame: the f32 chain
//                         with sigmoid_f32 in the three hidden layers (layer 1's
//                         and layer 2's activations all-gathered through the
//                         half-group's two LDS rows), certify_c under the
//                         network's static bound (pg_sig3_bound.h), and for the
//                         undecided half-groups tight_gap_move, plateau_f32 and
//                         then the f64 forward in numpy's order from the genes.
//                         No lane records, no workspace beyond the base.
// This file holds the family's kernels, its description (pg_family.hpp; what it
// shares with k_relu3's is pg_hidden3.hpp's Hidden3Family), its row of the
// family table and its C entry point.  Compiled a second time with
// -DPG_SOLO_UNIT (pong_amd/build.py) it holds k_sig3_solo and k_sig3_adv_solo
// (PG_KERNEL_SOLO) and nothing else, as pg_relu3.hip does.  DESIGN.md 4.2n.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_certgame.hpp"
#include "pg_eval.hpp"
#include "pg_family.hpp"
#include "pg_sig3.hpp"

namespace pg {

// Blocks per CU the game kernels are compiled for (DESIGN.md 4.2n has the
// measurement): two for the 8-lane layout; for the 16-lane layout, whose 158
// weights and 5 certificate constants per lane do not all stay in 256 VGPRs at
// two blocks, PG_SIG3_BLOCKS16 (a variant build, tools/build_variant.py, takes
// the other value).
#ifndef PG_SIG3_BLOCKS16
#define PG_SIG3_BLOCKS16 2
#endif
__host__ __device__ constexpr int sig3_blocks(int LN) { return LN == 8 ? 2 : PG_SIG3_BLOCKS16; }

#ifdef PG_SOLO_UNIT
// k_sig3 and k_sig3_adv with a half-group per game against a scripted opponent
// (PG_KERNEL_SOLO; pg_certgame.hpp)
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, sig3_blocks(LN)) void k_sig3_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Sig3Policy<LN, U, O, WT>, false, true>(p);
}

template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, sig3_blocks(LN)) void k_sig3_adv_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Sig3Policy<LN, U, O, WT>, true, true>(p);
}

void sig3_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p) {
  if (advance) PG_HIDDEN3_DISPATCH(k_sig3_adv_solo, LN, O, f64, grid, s, p);
  else PG_HIDDEN3_DISPATCH(k_sig3_solo, LN, O, f64, grid, s, p);
}

}  // namespace pg
#else
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, sig3_blocks(LN)) void k_sig3(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Sig3Policy<LN, U, O, WT>, false>(p);
}

// k_sig3 with the serve delays and periodic rallies advanced in closed form
// (PG_KERNEL_ADVANCE, untraced launches; pg_certgame.hpp)
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, sig3_blocks(LN)) void k_sig3_adv(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 64, "other_half / group_broadcast layouts");
  cert_game<Sig3Policy<LN, U, O, WT>, true>(p);
}

template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256) void k_sig3_decide(Hidden3DecideParams p) {
  constexpr int HPB = 256 / LN;
  for (long base = (long)blockIdx.x * HPB; base < p.n; base += (long)gridDim.x * HPB)
    cert_decide_pass<Sig3Policy<LN, U, O, WT>>(p, base);
}

struct Sig3Family : Hidden3Family {
  static constexpr int kKernel = PG_KERNEL_SIG3, kActivation = PG_ACT_SIGMOID;
  static constexpr const char *kName = "sig3";
  static constexpr const char *kBadActivation =
      "activation relu: the sig3 kernel evaluates sigmoid networks only (use RELU3)";
  static constexpr const char *kBadShape = "sig3 kernel needs NETWORK_SHAPE [6, 2..32, 2..32, 2..32, 2..4]";
  static constexpr const char *kNoBias = "sig3 kernel needs a network with bias";
  static constexpr const char *kNoHorizon = "sig3 kernel: no fixed-horizon mode (horizon must be 0)";
  static constexpr const char *kNoHardLog = "sig3 kernel: no hard-case log (hard_log must be NULL)";
  static constexpr const char *kDecideBadActivation =
      "pg_sig3_decide: activation=%d, the sig3 kernel decides sigmoid networks only";
  static constexpr const char *kDecideBadShape =
      "pg_sig3_decide: the sig3 kernel's shapes [6, 2..32, 2..32, 2..32, 2..4] only";
  static constexpr const char *kDecideNoBias = "pg_sig3_decide: the sig3 kernel needs a network with bias";
  static void game(const EvalParams &p, bool f64, bool advance, bool solo, int grid, hipStream_t s) {
    const int LN = lanes(p.nodes), O = p.nodes[4];
    if (solo) sig3_solo_game(LN, O, f64, advance, grid, s, p);
    else if (advance) PG_HIDDEN3_DISPATCH(k_sig3_adv, LN, O, f64, grid, s, p);
    else PG_HIDDEN3_DISPATCH(k_sig3, LN, O, f64, grid, s, p);
  }
  static void decide(const int32_t *nodes, bool f64, int grid, hipStream_t s, const DecideParams &p) {
    PG_HIDDEN3_DISPATCH(k_sig3_decide, lanes(nodes), nodes[4], f64, grid, s, p);
  }
};

FamilyDesc sig3_family() { return family_desc<Sig3Family>(); }

}  // namespace pg

extern "C" int32_t pg_sig3_decide(const pg_relu_decide_args *a, void *stream) {
  return pg::family_decide<pg::Sig3Family>(a, stream);
}
#endif  // PG_SOLO_UNIT
