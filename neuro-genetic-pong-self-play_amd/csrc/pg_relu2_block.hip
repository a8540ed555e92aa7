// pg_relu2_block.hip -- k_relu2_block: evaluate() (main.py:28-66) for [6, H1 <=
// 128, H2 <= 128, 2..4] ReLU networks with bias (two hidden layers;
// activation_function = ReLU, numpy_nn.py:6-9, 26), and pg_relu2_block_decide,
// its decision code on given inputs (include/pong_ga.h).  DESIGN.md 4.2k.
//
// k_relu2's design (pg_hidden2.hpp) one level up: the group that plays a game
// is a 256-thread block, not a slice of a wave.
//
// The block layout -- the per-thread network, the load, the f32 frame, the f64
// forward -- is pg_block2.hpp's, shared with k_sig2_block; this file is the
// ReLU family of it and the two kernels' bodies.
//
// Padding.  A padding unit (hl >= H1 or hl >= H2) and a padding column
// (j >= H1) have exact zero weights: max(0, 0) = 0 times 0 contributes exactly
// 0 to every sum and to the bound.
//
// The decision is k_relu2's (relu_certify, pg_relu.hpp): index 0 if t1 <= -e,
// the index of t1 if t1 > e and t1 - t2 > 2e, else the f64 forward from the
// genes in numpy's order (block_f64: blas_dot over [inputs..., 1] per unit, one
// unit per thread, activations through LDS, np.argmax's NaN rule -- the values
// are forward_f64_wave's).  The bound is pg_relu2_bound.h's under its block
// layout.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_block2.hpp"
#include "pg_family.hpp"
#include "pg_relu2_bound.h"

namespace pg {

static_assert(PG_RELU2_BLOCK_CHAIN1 == kBlockChain1, "the bound's layer-1 chain: gene, feat32, block_z32's 6 fmas");
static_assert(PG_RELU2_BLOCK_CHAIN2 == kBlockChain2, "the bound's layer-2 chain: gene, one fma per padded unit");
static_assert(PG_RELU2_BLOCK_CHAIN3 == kBlockChain3,
              "the bound's layer-3 chain: gene, product, group_sum<64>'s steps, the two waves, the bias");

struct Relu2Block {
  static constexpr int kActivation = PG_ACT_RELU;
  using Sums = pg_relu2_sums;
  // LDS of a block (pg_block2.hpp names the fields)
  struct alignas(16) Lds {
    float h[2][kBlockH];
    float part[4][4];
    float c[2][4];
    float e[2];
    int game;
    double d[2][2 * kBlockH + 4];
    double red[4][3 * PG_RELU_MAX_OUT + 3];
  };
  static __device__ __forceinline__ void init(Sums &s) { pg_relu2_sums_init(&s); }
  static __device__ __forceinline__ double unit1(const double w[7]) { return pg_relu2_unit1(w); }
  static constexpr double Sums::*kOther = &Sums::W2;
  static __device__ __forceinline__ void publish(Lds &lds, int net, float e) { lds.e[net] = e; }
};

// network n's z^ from the waves' sums, and its certificate (relu_certify): the proven index or -1
template <int O>
__device__ __forceinline__ int block_certify(const Relu2Block::Lds &lds, int n, float z[O]) {
  block_z_out<O>(lds, n, z);
  return relu_certify<O>(z, lds.e[n]);
}

// evaluate() (main.py:28-66): a persistent grid of blocks, each playing one
// game at a time to its end; thread 0 takes the next game from p.work (one
// atomic per game) and broadcasts it through LDS.  Every frame is stepped.
template <int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_relu2_block(EvalParams params) {
  const EvalParams p = params;  // (a copy of this function's own, as cert_game's)
  __shared__ Relu2Block::Lds lds;
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), net = wv >> 1, hl = tid & (kBlockH - 1);
  const WT *genomes = (const WT *)p.genomes;
  const WT *opponents = (const WT *)p.opponents;
  const int H1 = p.nodes[1], H2 = p.nodes[2];
  const unsigned int games_total = (unsigned int)active_total(p);
  // thread 0's are reported.  64-bit: a block's sum over its games (768 of a 65 536-genome launch) of up to
  // 21 points x timeout_thresh <= 2^20 frames each is not bounded by 2^32
  unsigned long long c_steps = 0, c_fwd = 0, c_f64 = 0;
  uint32_t c_games = 0;
  for (;;) {
    if (tid == 0) lds.game = (int)atomicAdd(p.work, 1u);
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane(lds.game);  // (rewritten only after block_load's barriers)
    if ((unsigned int)w >= games_total) break;
    const int i = w / p.n_games, gi = w % p.n_games;
    const int kind = p.kind[w];
    const WT *gr = genomes + (long)genome_row(p, i) * p.gstride;
    const WT *gl = (kind == kOppNN) ? opponents + (long)p.opp[w] * p.ostride : gr;
    const WT *g = net ? gl : gr;
    const bool live_l = kind == kOppNN;
    const bool live = net == 0 || live_l;  // this thread's network plays
    BlockNet<O> nw = {};
    block_load<Relu2Block, O, WT>(nw, g, H1, H2, lds, wv, hl, live);
    Pong st;
    st.reset(game_seed(p.seed, gi), kind == kOppRomCpu);
    int act_r = 0, act_l = 0, timeout = 0, total = 0, frames = 0;
    for (;;) {
      const int s1b = st.s1, s2b = st.s2;
      const int pvis = st.vis, pbx2 = 2 * st.bx + kBallW - 1, pby2 = 2 * st.by + kBallH - 1;
      st.step(act_r, act_l);
      frames += 1;
      const int vis = __builtin_amdgcn_readfirstlane(st.vis);
      const int bx2 = 2 * st.bx + kBallW - 1, by2 = 2 * st.by + kBallH - 1;
      const int lc2 = paddle_c2(st.lpy), rc2 = paddle_c2(st.rpy);
      int left = 0, right = 0;
      if (vis) {  // get_actions main.py:143-150
        const int lbx2 = pvis ? pbx2 : bx2, lby2 = pvis ? pby2 : by2;
        // utils.inference's features (utils.py:139-153) as doubled centroids: the left
        // paddle sees the field mirrored, (160 - x) / 160 = (320 - 2x) / 320 exactly
        int k[6];
        k[0] = net ? 320 - bx2 : bx2;
        k[1] = by2;
        k[2] = net ? 320 - lbx2 : lbx2;
        k[3] = lby2;
        k[4] = net ? lc2 : rc2;
        k[5] = net ? rc2 : lc2;
        block_z32<Relu2Block, O>(nw, k, lds, wv, hl, live);
        float z[O];
        int idx[2];
        idx[0] = block_certify<O>(lds, 0, z);
        idx[1] = live_l ? block_certify<O>(lds, 1, z) : 0;
        // the networks the certificate left undecided: the same value in every thread of the block
        const int need = __builtin_amdgcn_readfirstlane((idx[0] < 0 ? 1 : 0) | (idx[1] < 0 ? 2 : 0));
        if (__builtin_expect(need != 0, 0)) block_f64<Relu2Block, O, WT>(g, H1, H2, k, lds, wv, hl, need, idx);
        right = index_to_code(idx[0]);
        left = index_to_code(idx[1]);
        c_fwd += live_l ? 2 : 1;
        c_f64 += (need & 1) + (need >> 1);
        if (kind == kOppScore)
          left = (st.s1 <= st.s2) ? hardcoded(by2, lc2) : 0;
        else if (kind != kOppNN)
          left = hardcoded(by2, lc2);
      }
      act_l = clamp_action(lc2, left);
      act_r = clamp_action(rc2, right);
      if (p.trace && w < p.trace_games && frames <= p.trace_cap && tid == 0)
        p.trace[(long)w * p.trace_cap + frames - 1] = (uint8_t)(act_r | (act_l << 2) | (vis << 4));
      if (frames > 1) {  // calculate_timeout_and_frames main.py:128-135
        if (st.s1 == s1b && st.s2 == s2b) {
          timeout += 1;
        } else {
          total += timeout;
          timeout = 0;
        }
      }
      const bool end = st.s1 >= p.win_score || st.s2 >= p.win_score || st.done() || timeout > p.timeout_thresh;
      if (__builtin_amdgcn_readfirstlane(end ? 1 : 0)) break;
    }
    c_steps += frames;
    c_games += 1;
    if (tid == 0) finish_game(p, w, st, frames, total);
  }
  if (p.counters && tid == 0 && c_games) {
    atomicAdd((unsigned long long *)&p.counters[0], c_steps);
    atomicAdd((unsigned long long *)&p.counters[3], (unsigned long long)c_games);
    if (c_fwd) atomicAdd((unsigned long long *)&p.counters[1], c_fwd);
    if (c_f64) {  // [2] the f64 forwards, [4] the frames the f32 certificate left undecided: the same here
      atomicAdd((unsigned long long *)&p.counters[2], c_f64);
      atomicAdd((unsigned long long *)&p.counters[4], c_f64);
    }
  }
}

// pg_relu2_block_decide: the decision code of a k_relu2_block frame, one block
// per pass on the right paddle's threads (waves 2-3 keep the barriers only).
template <int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_relu2_block_decide(CertDecideParams p) {
  __shared__ Relu2Block::Lds lds;
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), net = wv >> 1, hl = tid & (kBlockH - 1);
  const WT *genomes = (const WT *)p.genomes;
  const bool live = net == 0;
  for (long t = blockIdx.x; t < p.n; t += gridDim.x) {
    const WT *g = genomes + (long)(p.gidx ? p.gidx[t] : t) * p.gstride;
    BlockNet<O> nw = {};
    block_load<Relu2Block, O, WT>(nw, g, p.H1, p.H2, lds, wv, hl, live);
    int k[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = p.k[t * 6 + i];
    block_z32<Relu2Block, O>(nw, k, lds, wv, hl, live);
    float z[O];
    int idx[2] = {block_certify<O>(lds, 0, z), 0};
    const int need = __builtin_amdgcn_readfirstlane(idx[0] < 0 ? 1 : 0);
    if (need) block_f64<Relu2Block, O, WT>(g, p.H1, p.H2, k, lds, wv, hl, need, idx);
    if (tid == 0) {
      p.index[t] = idx[0];
      if (p.stage) p.stage[t] = need;
      if (p.bound) p.bound[t] = lds.e[0];
      if (p.z32) {
#pragma unroll
        for (int o = 0; o < O; ++o) p.z32[t * O + o] = z[o];
      }
    }
  }
}

// ------------------------------------------------------------ host side ----
struct Relu2BlockFamily : Block2Family {
  static constexpr int kKernel = PG_KERNEL_RELU2_BLOCK, kActivation = PG_ACT_RELU;
  static constexpr const char *kName = "relu2_block";
  static constexpr const char *kBadActivation =
      "activation sigmoid: the relu2_block kernel evaluates PG_ACT_RELU networks only";
  static constexpr const char *kBadShape = "relu2_block kernel needs NETWORK_SHAPE [6, 2..128, 2..128, 2..4] with bias";
  static constexpr const char *kNoBias = kBadShape;
  static constexpr const char *kNoHorizon =
      "relu2_block kernel plays whole episodes: no fixed-horizon mode (horizon must be 0)";
  static constexpr const char *kNoHardLog = "relu2_block kernel keeps no hard-case log (hard_log must be NULL)";
  static constexpr const char *kDecideBadActivation =
      "pg_relu2_block_decide: activation=%d, the relu2_block kernel decides PG_ACT_RELU networks only";
  static constexpr const char *kDecideBadShape =
      "pg_relu2_block_decide: the relu2_block kernel's shapes [6, 2..128, 2..128, 2..4] with bias only";
  static constexpr const char *kDecideNoBias = kDecideBadShape;
  static void game(const EvalParams &p, bool f64, bool, bool, int grid, hipStream_t s) {
    PG_BLOCK_DISPATCH(k_relu2_block, p.nodes[3], f64, grid, s, p);
  }
  static void decide(const int32_t *nodes, bool f64, int grid, hipStream_t s, const DecideParams &p) {
    PG_BLOCK_DISPATCH(k_relu2_block_decide, nodes[3], f64, grid, s, p);
  }
};

FamilyDesc relu2_block_family() { return family_desc<Relu2BlockFamily>(); }

}  // namespace pg

extern "C" int32_t pg_relu2_block_decide(const pg_relu_decide_args *a, void *stream) {
  return pg::family_decide<pg::Relu2BlockFamily>(a, stream);
}
