// pg_relu.hip -- k_relu: evaluate() (main.py:28-66) for [6, H <= 256, 2..4]
// ReLU networks with bias (activation_function = ReLU, numpy_nn.py:6-9, 26), and
// pg_relu_decide, its decision code on given inputs (include/pong_ga.h).
//
//   k_relu<LN, U, O, WT>  an aligned group of 2 LN lanes plays one game to its
//                         end, taking games from the p.work queue; lanes
//                         [0, LN) hold the right paddle's network (the genome),
//                         lanes [LN, 2 LN) the left paddle's (a hall-of-fame
//                         row; idle against the scripted opponents and the ROM
//                         CPU), U hidden units per lane as f32 in VGPRs for the
//                         whole game, so HBM is touched once per game.  Every
//                         lane of a group steps the same Pong state.  Each
//                         frame: the f32 chain, the certificate under the
//                         network's static bound (pg_relu.hpp), and for the
//                         undecided half-groups the f64 forward in numpy's order
//                         from the genes.  Every frame is stepped.
// The game loop and the decide pass are the certified families' shared ones
// (pg_certgame.hpp); this file holds k_relu's policy, its kernels, its
// description (pg_family.hpp), its row of the family table and its C entry
// point.  Compiled a second time with -DPG_SOLO_UNIT (pong_amd/build.py) it holds
// k_relu_solo and k_relu_adv_solo (PG_KERNEL_SOLO) and nothing else, so this
// unit's kernels are what they were without them.  DESIGN.md 4.2c, 4.2g, 4.2i.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_cascade.hpp"
#include "pg_certgame.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_family.hpp"
#include "pg_relu.hpp"

namespace pg {

// k_relu's policy (pg_certgame.hpp): U hidden units per lane, the half-group's
// LDS is its f64 forward's LN * U hidden + O outputs
template <int LN_, int U, int O_, typename WT_>
struct ReluPolicy {
  static constexpr int LN = LN_, O = O_, kF64Stage = 1;
  using WT = WT_;
  using Net = ReluNet<U, O>;
  struct Lds {
    double d[LN * U + 4];
  };
  static __device__ __forceinline__ void load(Net &net, const WT *g, const CertDims &dims, Lds &, int hl) {
    relu_load<LN, U, O, WT>(net, g, dims.H1, hl);
  }
  static __device__ __forceinline__ int decide(const Net &net, const WT *g, const CertDims &dims, const int k[6],
                                               bool live, Lds &lds, int hl, float z[O], int &stage) {
    return relu_decide<LN, U, O, WT>(net, g, dims.H1, k, live, lds.d, hl, z, stage);
  }
};

// the instances: LN = relu_lanes(H) lanes per network, kReluUnits units per lane
#define PG_RELU_DISPATCH(KERNEL, LN, O, f64, grid, s, p)                            \
  do {                                                                              \
    if (LN == 4) PG_CERT_DISPATCH(KERNEL, 4, (kReluUnits), O, f64, grid, s, p);     \
    else if (LN == 8) PG_CERT_DISPATCH(KERNEL, 8, (kReluUnits), O, f64, grid, s, p); \
    else PG_CERT_DISPATCH(KERNEL, 16, (kReluUnits), O, f64, grid, s, p);            \
  } while (0)

#ifdef PG_SOLO_UNIT
// k_relu and k_relu_adv with a half-group per game against a scripted opponent
// (PG_KERNEL_SOLO; pg_certgame.hpp)
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, O <= 3 ? 2 : 1) void k_relu_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 32, "other_half / group_broadcast layouts");
  cert_game<ReluPolicy<LN, U, O, WT>, false, true>(p);
}

template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, O <= 3 ? 2 : 1) void k_relu_adv_solo(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 32, "other_half / group_broadcast layouts");
  cert_game<ReluPolicy<LN, U, O, WT>, true, true>(p);
}

void relu_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p) {
  if (advance) PG_RELU_DISPATCH(k_relu_adv_solo, LN, O, f64, grid, s, p);
  else PG_RELU_DISPATCH(k_relu_solo, LN, O, f64, grid, s, p);
}

}  // namespace pg
#else
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, O <= 3 ? 2 : 1) void k_relu(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 32, "other_half / group_broadcast layouts");
  cert_game<ReluPolicy<LN, U, O, WT>, false>(p);
}

// k_relu with the serve delays and periodic rallies advanced in closed form
// (PG_KERNEL_ADVANCE, untraced launches; pg_certgame.hpp)
template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256, O <= 3 ? 2 : 1) void k_relu_adv(EvalParams p) {
  static_assert(2 * LN >= 8 && 2 * LN <= 32, "other_half / group_broadcast layouts");
  cert_game<ReluPolicy<LN, U, O, WT>, true>(p);
}

template <int LN, int U, int O, typename WT>
__global__ __launch_bounds__(256) void k_relu_decide(CertDecideParams p) {
  constexpr int HPB = 256 / LN;
  for (long base = (long)blockIdx.x * HPB; base < p.n; base += (long)gridDim.x * HPB)
    cert_decide_pass<ReluPolicy<LN, U, O, WT>>(p, base);
}

static_assert(relu_lanes(kReluMaxH) * kReluUnits >= kReluMaxH, "a layout for every H in scope");

// k_relu's description (pg_family.hpp).  The one family whose scope is asked at
// the launch, not on entry (pong_ga.hip's scope_on_entry says what that keeps).
struct ReluFamily {
  static constexpr int kKernel = PG_KERNEL_RELU, kActivation = PG_ACT_RELU;
  static constexpr bool kModifiers = true, kScopeOnEntry = false;
  static constexpr const char *kName = "relu";
  static constexpr const char *kBadActivation = "activation sigmoid: the relu kernel evaluates PG_ACT_RELU networks only";
  static constexpr const char *kBadShape = "relu kernel needs NETWORK_SHAPE [6, H<=256, 2..4] with bias";
  static constexpr const char *kNoBias = kBadShape;
  static constexpr const char *kDecideBadActivation =
      "pg_relu_decide: activation=%d, the relu kernel decides PG_ACT_RELU networks only";
  static constexpr const char *kDecideBadShape = "pg_relu_decide: the relu kernel's shapes [6, H<=256, 2..4] with bias only";
  static constexpr const char *kDecideNoBias = kDecideBadShape;
  using DecideParams = CertDecideParams;
  // the shapes [6, 1..256, 2..4]
  static bool shape_ok(int n_nodes, const int32_t *nodes) {
    return n_nodes == 3 && nodes[0] == 6 && nodes[1] >= 1 && nodes[1] <= kReluMaxH && nodes[2] >= 2 && nodes[2] <= 4;
  }
  static long genes(const int32_t *nd) { return (long)nd[1] * 7 + (long)nd[2] * (nd[1] + 1); }
  static int lanes(const int32_t *nd) { return relu_lanes(nd[1]); }
  static int game_grid(const EvalParams &p) { return cert_game_grid(p, lanes(p.nodes)); }
  static int decide_grid(const pg_relu_decide_args *a) { return cert_decide_grid(a->n, lanes(a->net.nodes)); }
  static DecideParams decide_params(const pg_relu_decide_args *a) { return cert_decide_params(a, a->net.nodes[1], 0); }
  static void game(const EvalParams &p, bool f64, bool advance, bool solo, int grid, hipStream_t s) {
    const int LN = lanes(p.nodes), O = p.nodes[2];
    if (solo) relu_solo_game(LN, O, f64, advance, grid, s, p);
    else if (advance) PG_RELU_DISPATCH(k_relu_adv, LN, O, f64, grid, s, p);
    else PG_RELU_DISPATCH(k_relu, LN, O, f64, grid, s, p);
  }
  static void decide(const int32_t *nodes, bool f64, int grid, hipStream_t s, const DecideParams &p) {
    PG_RELU_DISPATCH(k_relu_decide, lanes(nodes), nodes[2], f64, grid, s, p);
  }
};

bool relu_shape_ok(const pg_net &n) { return ReluFamily::shape_ok(n.n_nodes, n.nodes) && n.bias != 0; }

FamilyDesc relu_family() { return family_desc<ReluFamily>(); }

}  // namespace pg

extern "C" int32_t pg_relu_decide(const pg_relu_decide_args *a, void *stream) {
  return pg::family_decide<pg::ReluFamily>(a, stream);
}
#endif  // PG_SOLO_UNIT
