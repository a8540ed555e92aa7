// pg_eval.hpp -- what the evaluation kernels of libpong_ga.so share across
// translation units: EvalParams and the per-game helpers, and each unit's
// host interface to pg_eval_population.
//
//   pong_ga.hip          the C-ABI of the evaluation (pg_eval_population, pg_decide,
//                        pg_wide_decide), errors, k_fitness, k_service's bench instance
//                        and the kernels its generated code depends on
//                        (k_forward_resident, k_physics_* with pg_physics_*)
//   pg_service_more.hip  every other k_service instance
//   pg_service_solo.hip  k_service's solo instances (PG_KERNEL_SOLO on the bench layout)
//   pg_general.hip       the f64 path: k_general, pg_forward with k_forward_general
//   pg_wide.hip          k_wide: wide two-hidden-layer networks, weights streamed
//   the certified f32 families, seven units on pg_certgame.hpp (device) and pg_family.hpp (host):
//   pg_relu.hip          k_relu: one hidden ReLU layer (pg_relu.hpp)
//   pg_relu2.hip, pg_sig2.hip   k_relu2, k_sig2: two hidden ReLU / sigmoid layers (pg_hidden2.hpp)
//   pg_relu3.hip         k_relu3: three hidden ReLU layers (pg_hidden3.hpp)
//   pg_sig3.hip          k_sig3: the same for three hidden sigmoid layers (pg_sig3.hpp, on pg_hidden3.hpp's layout)
//   pg_relu2_block.hip   k_relu2_block: k_relu2's certificate (pg_relu2_bound.h, its block layout) with a block per
//                        game (widths up to 128)
//   pg_sig2_block.hip    k_sig2_block: k_sig2's certificate (pg_sig2_bound.h, its block layout) on the same layout;
//                        pg_block2.hpp is what the two block units share
//   pg_decide.hip        k_decide (pg_decide)
//   pg_ga.hip            selection, variation, schedule, row gather and hash
//   pg_gen.hip, pg_hof.hip, pg_pixels.hip    the generation's device steps, the
//                        hall of fame on the device, frames as pixels
//   pg_hof_scan.cpp      the hall-of-fame scans on the host (plain C++)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pong_ga.h"
#include "pg_device.hpp"
#include "pg_fail.hpp"

namespace pg {

// ------------------------------------------------------- kernel params ----
struct EvalParams {
  const void *genomes;
  const void *opponents;
  const int32_t *rows;  // optional [n_genomes]: block i of games plays genome row rows[i] (NULL: row i)
  const int32_t *n_active;  // optional device count: only blocks i < min(*n_active, n_genomes) are played
  const int32_t *kind;
  const int32_t *opp;
  const double *mult;
  double *rewards;
  int32_t *scores;
  int32_t *frames;
  double *total_frames;
  int32_t *status_game;  // [n*games] scratch: zero-division per game
  uint64_t *counters;
  uint8_t *trace;
  uint32_t *hard_log;    // optional [hard_cap][8] (pg_eval_args.hard_log)
  int hard_cap;
  unsigned int *work;    // dynamic game counter (workspace)
  int64_t gstride, ostride;
  uint64_t seed;
  int n_genomes, n_games, total, n_opponents;
  int trace_games, trace_cap;
  int nodes[PG_MAX_NODES];
  int n_nodes, bias, max_width;
  float *recs;         // split kernel: lane records (k_prep_records), [n_genomes + n_opponents][L/2][rec_floats]
  int horizon;         // pg_eval_args.horizon: fixed-horizon measurement mode (T frames per game slot), 0 = off
  int timeout_thresh;  // pg_eval_args.timeout_thresh: TIMEOUT_THRESH (kTimeoutThresh unless set)
  int win_score;       // pg_eval_args.win_score: WIN_SCORE (kWinScore unless set)
  int prep;            // pg_prep: which records k_prep_records writes; it also zeroes the work header and
                       // the counters when its launch precedes the games (PG_PREP_ALL / PG_PREP_REST)
  void *wide_scratch;  // k_wide: the blocks' tile-major W2 copies (workspace)
  int wide_w3_resident;  // k_wide: every network's W3 kept in LDS for the genome's games
  // k_wide probe (pg_wide_decide, n_games = 1): block i runs one frame of
  // genome i on the doubled centroids wide_probe_k[i][0..5] instead of a game
  const int32_t *wide_probe_k;
  int32_t *wide_probe_index;  // out [n_genomes] np.argmax
  double *wide_probe_act;     // optional out [n_genomes, nodes[3]]
  int activation;             // pg_net.activation (k_general reads it; launch_wide picks k_wide's instance by it)
};

// Genome blocks / games this launch plays (pg_eval_args.n_active).  Made
// wave-uniform explicitly: as a per-lane load result the loop bound of the
// game loops became a vector compare, which cost k_service 14 % (11.0 vs
// 12.7 ms per launch, tools/runs/r2_b6.sh).
__device__ inline int active_genomes(const EvalParams &p) {
  if (!p.n_active) return p.n_genomes;
  const int a = __builtin_amdgcn_readfirstlane(*p.n_active);
  return a < 0 ? 0 : (a < p.n_genomes ? a : p.n_genomes);
}
__device__ inline int active_total(const EvalParams &p) {
  return p.n_active ? active_genomes(p) * p.n_games : p.total;
}

// Genome row played by block i of games (pg_eval_args.genome_rows).
__device__ inline int genome_row(const EvalParams &p, int i) { return p.rows ? p.rows[i] : i; }

// Results of one finished game: perform_episode's return value and the
// bookkeeping around it (main.py:108-112, utils.py:104-109).
// (S: Pong or PongK; only the scores are read)
template <class S>
__device__ inline double episode_reward(const S &st, int total, double mult, int &zero_div) {
  zero_div = 0;
  if (st.s1 == st.s2) return 0.0;  // main.py:109-110
  const double tf = (double)total;
  if (tf == 0.0) {
    zero_div = 1;
    return __builtin_nan("");
  }
  // ((my - enemy) + my * mult) / (total_frames / 100.0), no contraction
  const double diff = (double)(st.s2 - st.s1);
  const double bonus = __dmul_rn((double)st.s2, mult);
  return __dadd_rn(diff, bonus) / (tf / 100.0);
}

template <class S>
__device__ inline void finish_game(const EvalParams &p, int w, const S &st, int frames, int total) {
  int zero_div;
  const double reward = episode_reward(st, total, p.mult[w], zero_div);
  p.rewards[w] = reward;
  p.scores[2 * w] = st.s1;
  p.scores[2 * w + 1] = st.s2;
  p.frames[w] = frames;
  p.total_frames[w] = (double)total;
  p.status_game[w] = zero_div;
}

// Features of utils.inference (utils.py:139-153) in f64 from doubled
// centroids k: value = (k / 2) / 160, exactly the reference's rounding.
__device__ inline double feat64(int k) { return __dmul_rn(0.5, (double)k) / 160.0; }
__device__ inline double feat64_flip(int k) { return (160.0 - __dmul_rn(0.5, (double)k)) / 160.0; }


// ---------------------------------------------- host side (pong_ga.hip) ----
int num_cus();
int32_t check_net(const pg_net &n, bool game);  // game: the game's 6 inputs required
int gene_count(const pg_net &n);                // -1: above 2^31 - 1
int max_width(const pg_net &n);
inline size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// the network's fields of a kernel's parameters (EvalParams, pg_general.hip's FwdParams)
template <class Params>
inline void set_net(Params &p, const pg_net &n) {
  for (int i = 0; i < n.n_nodes; ++i) p.nodes[i] = n.nodes[i];
  p.n_nodes = n.n_nodes;
  p.bias = n.bias ? 1 : 0;
  p.max_width = max_width(n);
  p.activation = n.activation;
}

// Append one hard-decision record (pg_eval_args.hard_log); counters[9] counts them all.
__device__ inline void log_hard_raw(uint32_t *hard_log, uint64_t *counters, int hard_cap, int row, int is_opp, int idx,
                                    int source, const int k[6]) {
  if (!hard_log || !counters) return;
  const unsigned long long r = atomicAdd((unsigned long long *)&counters[9], 1ull);
  if (r >= (unsigned long long)hard_cap) return;
  uint32_t *rec = hard_log + r * 8;
  rec[0] = (uint32_t)row;
  rec[1] = (uint32_t)(is_opp & 1) | ((uint32_t)(idx & 255) << 8) | ((uint32_t)(source & 255) << 16);
  for (int i = 0; i < 6; ++i) rec[2 + i] = (uint32_t)k[i];
}
__device__ inline void log_hard(const EvalParams &p, int row, int is_opp, int idx, int source, const int k[6]) {
  log_hard_raw(p.hard_log, p.counters, p.hard_cap, row, is_opp, idx, source, k);
}

// pg_decide's parameters (k_decide, pg_decide.hip: k_service's cascade on given inputs)
struct DecideParams {
  const void *genomes;
  const int32_t *gidx;
  const int32_t *k;
  int32_t *index;
  int32_t *stage;
  int64_t gstride;
  int n, H, b;
};
// k_decide for the split layout of L lanes per game (pg_decide.hip; its own
// translation unit, on the default machine scheduler: the iterative-ILP one
// pong_ga.hip uses for k_service crashes the register allocator on k_decide)
int32_t launch_decide(const DecideParams &p, int L, int O, bool f64, size_t lds, hipStream_t s);

// ------------------------------------------------- the kernel families ----
// Each family's unit exports its scope and its launch (the certified f32
// families: as a FamilyDesc).  A scope is the refusal, in the family's words, of
// a network or of arguments that the kernel does not evaluate (activation
// first, then shape, bias, precision, horizon, hard-case log, as far as the
// family has a rule of its own), or PG_OK.  It is the only place that states
// them: the launches take what pg_eval_population let through.  a.kernel is
// the pg_kernel alone, without modifier bits.

// the f64 kernel for any NETWORK_SHAPE (k_general, pg_general.hip)
int32_t launch_general(const EvalParams &p, int dtype, hipStream_t s);

// pg_forward's parameters (pg_general.hip) and its certified path for the split
// kernel's shapes, k_forward_resident (pong_ga.hip, which says why there)
struct FwdParams {
  const void *genomes;
  const int32_t *gidx;
  const double *x;
  int32_t *index;
  double *act;
  double *z_all, *h_all;  // optional [n, sum(nodes[1:])]: every layer's pre-activations / activations
  uint64_t *counters;
  int64_t gstride;
  int n;
  int nodes[PG_MAX_NODES];
  int n_nodes, bias, max_width, n_units, activation;
};
int32_t launch_forward_resident(const FwdParams &p, int dtype, hipStream_t s);

// [6, H <= 256, 2..4] sigmoid networks on k_service (SPLIT; pong_ga.hip, pg_service_more.hip)
bool resident_shape_ok(const pg_net &n);
int32_t split_scope(const pg_eval_args &a);
// the split launches that PG_KERNEL_SOLO (through PG_KERNEL_AUTO) plays on k_service's solo instances
// (pg_service_solo.hip); outside it the bit changes nothing on SPLIT
bool split_solo_scope(const pg_eval_args &a);

// [6, H1, H2, O] networks (two hidden layers, H1, H2 <= 512, O in 2..4) on the
// weight-streaming kernel k_wide (pg_wide.hip); launch_wide runs the sigmoid
// or the ReLU instance (PG_KERNEL_RELU_WIDE) by p.activation, and wide_scope
// is that of relu ? RELU_WIDE : WIDE.
bool wide_shape_ok(const pg_net &n, int n_games);
size_t wide_workspace_bytes(const pg_eval_args *a);
int32_t wide_scope(const pg_eval_args &a, bool relu);
int32_t launch_wide(const EvalParams &p, int dtype, void *scratch, hipStream_t s);

// The certified f32 families: certified precision, networks with bias, no
// workspace beyond the base.  Each unit states its family's host side once, as
// a description for pg_family.hpp's templates, and exports this descriptor of
// it; pong_ga.hip looks a pg_kernel up in one table of the seven.  (Exported
// as a host function that returns the constant: a const object of namespace
// scope would be emitted into the unit's code object as well.)
struct FamilyDesc {
  int kernel;      // its pg_kernel
  bool modifiers;  // it takes PG_KERNEL_ADVANCE and PG_KERNEL_SOLO (it has k_*_adv and k_*_solo instances)
  bool scope_on_entry;  // scope is asked on pg_eval_population's entry, even for an empty launch; else at the launch
  int32_t (*scope)(const pg_eval_args &a);
  // advance: the k_*_adv instances, unless the launch is traced; solo: the k_*_solo instances, traced or not
  int32_t (*launch)(const EvalParams &p, int dtype, bool advance, bool solo, hipStream_t s);
};
FamilyDesc relu_family();   // k_relu, [6, 1..256, 2..4] ReLU networks (pg_relu.hip)
FamilyDesc relu2_family();  // k_relu2, [6, 2..64, 2..64, 2..4] ReLU networks (pg_relu2.hip, pg_hidden2.hpp)
FamilyDesc sig2_family();   // k_sig2, the same shapes of sigmoid networks (pg_sig2.hip, pg_hidden2.hpp); like
                            // every sigmoid family no horizon, no hard-case log
// k_relu2_block and k_sig2_block: k_relu2's and k_sig2's certificates with a 256-thread block per game,
// [6, 2..128, 2..128, 2..4] (pg_relu2_block.hip, pg_sig2_block.hip, pg_block2.hpp); no horizon, no hard-case
// log, no modifier bits
FamilyDesc relu2_block_family(), sig2_block_family();
// k_relu3 and k_sig3: the same for three hidden layers, [6, 2..32, 2..32, 2..32, 2..4] (pg_relu3.hip on
// pg_hidden3.hpp; pg_sig3.hip on pg_sig3.hpp: k_sig2's certificate and cascade on k_relu3's layout)
FamilyDesc relu3_family(), sig3_family();

// AUTO's choice among them for a ReLU network (resolve_kernel): the families' shapes, with bias
bool relu_shape_ok(const pg_net &n);
bool relu2_shape_ok(const pg_net &n);

// the launches of the k_*_solo / k_*_adv_solo instances (PG_KERNEL_SOLO): each
// family's source compiled again as a unit of its own (-DPG_SOLO_UNIT)
void relu_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p);
void relu2_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p);
void sig2_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p);
void relu3_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p);
void sig3_solo_game(int LN, int O, bool f64, bool advance, int grid, hipStream_t s, const EvalParams &p);

}  // namespace pg
