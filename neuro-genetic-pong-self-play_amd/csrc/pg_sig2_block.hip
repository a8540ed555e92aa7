// pg_sig2_block.hip -- k_sig2_block: evaluate() (main.py:28-66) for [6, H1 <=
// 128, H2 <= 128, 2..4] sigmoid networks with bias (two hidden layers; the
// reference's default activation, numpy_nn.py:22-26), and pg_sig2_block_decide,
// its decision code on given inputs (include/pong_ga.h).  DESIGN.md 4.2l.
//
// k_sig2's certificate (pg_hidden2.hpp) on k_relu2_block's layout: the group
// that plays a game is a 256-thread block, not a slice of a wave.  The block
// layout -- the per-thread network, the load, the f32 frame, the f64 forward --
// is pg_block2.hpp's, shared with k_relu2_block; this file is the sigmoid
// family of it, the cascade and the two kernels' bodies.
//
// Padding.  A padding unit (hl >= H1 or hl >= H2) has activation
// sigmoid_f32(0) = 0.5, not 0: correctness rests on its OUTGOING weights being
// exactly zero.  block_load writes 0.0f for every W2 column j >= H1, for every
// weight of a padding layer-2 unit's row and for its W3 weights, so that
// fma(0, 0.5, a) = a and 0 * 0.5 = 0 leave every sum -- and group_sum<64>'s
// tree over the products -- and its error bound untouched.  The in-register
// rules (tight_gap_move, plateau_f32) see only z^ and e: nothing of a padding
// unit reaches them by another way.
//
// The decision is k_sig2's cascade on the output pre-activations z^ with
// |z^_o - znp_o| <= e (pg_sig2_bound.h under its block layout), in the order of
// Sig2Policy::decide, taken by every thread of the block from the same LDS
// words (the waves' sums, the output biases, e and make_cert(e)'s constants,
// which the hl == 0 thread of each network wrote once per game): stage 0
// certify_c for both networks; for a network left undecided stage 1
// tight_gap_move (it proves the f32 first maximum), then stage 2 plateau_f32,
// both in registers and without a barrier; what remains goes to stage 3, the
// block-wide f64 forward from the genes in np.dot's order with the correctly
// rounded sigmoid_f64 in all three layers and np.argmax's first-maximum /
// first-NaN rule (block_f64).  All 256 threads compute the same values, and
// the two need masks -- after stage 0 and after the in-register rules -- are
// passed through readfirstlane before they guard anything.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_block2.hpp"
#include "pg_family.hpp"
#include "pg_sig2_bound.h"

namespace pg {

static_assert(PG_SIG2_BLOCK_CHAIN1 == kBlockChain1, "the bound's layer-1 chain: gene, feat32, block_z32's 6 fmas");
static_assert(PG_SIG2_BLOCK_CHAIN2 == kBlockChain2, "the bound's layer-2 chain: gene, one fma per padded unit");
static_assert(PG_SIG2_BLOCK_CHAIN3 == kBlockChain3,
              "the bound's layer-3 chain: gene, product, group_sum<64>'s steps, the two waves, the bias");

struct Sig2Block {
  static constexpr int kActivation = PG_ACT_SIGMOID;
  using Sums = pg_sig2_sums;
  // LDS of a block (pg_block2.hpp names the fields); ct: certify_c's constants of e
  struct alignas(16) Lds {
    float h[2][kBlockH];
    float part[4][4];
    float c[2][4];
    float e[2];
    int game;
    Cert ct[2];
    double d[2][2 * kBlockH + 4];
    double red[4][3 * PG_SIG2_MAX_OUT + 3];
  };
  static __device__ __forceinline__ void init(Sums &s) { pg_sig2_sums_init(&s); }
  static __device__ __forceinline__ double unit1(const double w[7]) { return pg_sig2_unit1(w); }
  static constexpr double Sums::*kOther = &Sums::P;
  static __device__ __forceinline__ void publish(Lds &lds, int net, float e) {
    lds.e[net] = e;
    lds.ct[net] = make_cert(e);
  }
};

// The cascade of one frame for both networks, every thread of the block alike
// (Sig2Policy::decide's order, pg_hidden2.hpp).  idx[n]: network n's np.argmax
// index (live_l false: idx[1] = 0); z: network 0's z^; stage: network 0's
// (0 certify_c, 1 tight_gap_move, 2 plateau_f32, 3 the f64 forward).  und, f64:
// the networks stage 0 left undecided and those recomputed in f64 (bit n:
// network n), block-uniform values through readfirstlane: they guard
// block_f64's barriers.  Entered by the whole block.
template <int O, typename WT>
__device__ __forceinline__ void block_cascade(Sig2Block::Lds &lds, const WT *__restrict__ g, int H1, int H2,
                                              const int k[6], int wv, int hl, bool live_l, int idx[2], float z[O],
                                              int &und, int &f64, int &stage) {
  float zl[O];
  block_z_out<O>(lds, 0, z);
  idx[0] = certify_c<O>(z, lds.ct[0]);
  idx[1] = 0;
  if (live_l) {
    block_z_out<O>(lds, 1, zl);
    idx[1] = certify_c<O>(zl, lds.ct[1]);
  } else {
#pragma unroll
    for (int o = 0; o < O; ++o) zl[o] = 0.f;
  }
  und = __builtin_amdgcn_readfirstlane((idx[0] < 0 ? 1 : 0) | (idx[1] < 0 ? 2 : 0));
  f64 = 0;
  stage = 0;
  if (__builtin_expect(und != 0, 0)) {
    // the in-register rules (pg_cascade.hpp), no barrier among them: tight_gap_move proves the f32 winner
    // (it returns that output's move; the index is the first maximum it took), then plateau_f32
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if ((und >> n) & 1) {
        const float *zn = n ? zl : z;
        int r = tight_gap_move<O>(zn, lds.e[n], lds.ct[n]) != -1 ? sig2_first_max<O>(zn) : -1;
        int st = 1;
        if (r < 0) {
          r = plateau_f32<O>(zn, lds.e[n]);
          st = 2;
        }
        idx[n] = r;
        if (n == 0) stage = st;
      }
    }
    f64 = __builtin_amdgcn_readfirstlane((idx[0] < 0 ? 1 : 0) | (idx[1] < 0 ? 2 : 0));
    if (f64 != 0) {
      block_f64<Sig2Block, O, WT>(g, H1, H2, k, lds, wv, hl, f64, idx);
      if (f64 & 1) stage = 3;
    }
  }
}

// evaluate() (main.py:28-66): a persistent grid of blocks, each playing one
// game at a time to its end; thread 0 takes the next game from p.work (one
// atomic per game) and broadcasts it through LDS.  Every frame is stepped.
// (k_relu2_block's loop, pg_relu2_block.hip, with the cascade for its
// certificate and [4] counted apart from [2]; why it stands twice: DESIGN.md 4.2l.)
template <int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_sig2_block(EvalParams params) {
  const EvalParams p = params;  // (a copy of this function's own, as cert_game's)
  __shared__ Sig2Block::Lds lds;
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), net = wv >> 1, hl = tid & (kBlockH - 1);
  const WT *genomes = (const WT *)p.genomes;
  const WT *opponents = (const WT *)p.opponents;
  const int H1 = p.nodes[1], H2 = p.nodes[2];
  const unsigned int games_total = (unsigned int)active_total(p);
  // thread 0's are reported.  64-bit: a block's sum over its games (768 of a 65 536-genome launch) of up to
  // 21 points x timeout_thresh <= 2^20 frames each is not bounded by 2^32
  unsigned long long c_steps = 0, c_fwd = 0, c_und = 0, c_f64 = 0;
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
    block_load<Sig2Block, O, WT>(nw, g, H1, H2, lds, wv, hl, live);
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
        block_z32<Sig2Block, O>(nw, k, lds, wv, hl, live);
        float z[O];
        int idx[2], stage;
        // und, f64: the networks stage 0 left undecided and those recomputed in f64 (bit n: network n),
        // the same values in every thread of the block
        int und, f64;
        block_cascade<O, WT>(lds, g, H1, H2, k, wv, hl, live_l, idx, z, und, f64, stage);
        right = index_to_code(idx[0]);
        left = index_to_code(idx[1]);
        c_fwd += live_l ? 2 : 1;
        c_f64 += (f64 & 1) + (f64 >> 1);
        c_und += (und & 1) + (und >> 1);
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
    // [4] the forwards stage 0 left undecided, [2] the f64 forwards among them: [2] <= [4] <= [1]
    if (c_und) atomicAdd((unsigned long long *)&p.counters[4], c_und);
    if (c_f64) atomicAdd((unsigned long long *)&p.counters[2], c_f64);
  }
}

// pg_sig2_block_decide: the decision code of a k_sig2_block frame, one block
// per pass on the right paddle's threads (waves 2-3 keep the barriers only).
template <int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_sig2_block_decide(CertDecideParams p) {
  __shared__ Sig2Block::Lds lds;
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), net = wv >> 1, hl = tid & (kBlockH - 1);
  const WT *genomes = (const WT *)p.genomes;
  const bool live = net == 0;
  for (long t = blockIdx.x; t < p.n; t += gridDim.x) {
    const WT *g = genomes + (long)(p.gidx ? p.gidx[t] : t) * p.gstride;
    BlockNet<O> nw = {};
    block_load<Sig2Block, O, WT>(nw, g, p.H1, p.H2, lds, wv, hl, live);
    int k[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = p.k[t * 6 + i];
    block_z32<Sig2Block, O>(nw, k, lds, wv, hl, live);
    float z[O];
    int idx[2], und, f64, stage;
    block_cascade<O, WT>(lds, g, p.H1, p.H2, k, wv, hl, false, idx, z, und, f64, stage);
    if (tid == 0) {
      p.index[t] = idx[0];
      if (p.stage) p.stage[t] = stage;
      if (p.bound) p.bound[t] = lds.e[0];
      if (p.z32) {
#pragma unroll
        for (int o = 0; o < O; ++o) p.z32[t * O + o] = z[o];
      }
    }
  }
}

// ------------------------------------------------------------ host side ----
struct Sig2BlockFamily : Block2Family {
  static constexpr int kKernel = PG_KERNEL_SIG2_BLOCK, kActivation = PG_ACT_SIGMOID;
  static constexpr const char *kName = "sig2_block";
  static constexpr const char *kBadActivation =
      "activation relu: the sig2_block kernel evaluates sigmoid networks only (use RELU2_BLOCK)";
  static constexpr const char *kBadShape = "sig2_block kernel needs NETWORK_SHAPE [6, 2..128, 2..128, 2..4] with bias";
  static constexpr const char *kNoBias = kBadShape;
  static constexpr const char *kNoHorizon =
      "sig2_block kernel plays whole episodes: no fixed-horizon mode (horizon must be 0)";
  static constexpr const char *kNoHardLog = "sig2_block kernel keeps no hard-case log (hard_log must be NULL)";
  static constexpr const char *kDecideBadActivation =
      "pg_sig2_block_decide: activation=%d, the sig2_block kernel decides sigmoid networks only";
  static constexpr const char *kDecideBadShape =
      "pg_sig2_block_decide: the sig2_block kernel's shapes [6, 2..128, 2..128, 2..4] with bias only";
  static constexpr const char *kDecideNoBias = kDecideBadShape;
  static void game(const EvalParams &p, bool f64, bool, bool, int grid, hipStream_t s) {
    PG_BLOCK_DISPATCH(k_sig2_block, p.nodes[3], f64, grid, s, p);
  }
  static void decide(const int32_t *nodes, bool f64, int grid, hipStream_t s, const DecideParams &p) {
    PG_BLOCK_DISPATCH(k_sig2_block_decide, nodes[3], f64, grid, s, p);
  }
};

FamilyDesc sig2_block_family() { return family_desc<Sig2BlockFamily>(); }

}  // namespace pg

extern "C" int32_t pg_sig2_block_decide(const pg_relu_decide_args *a, void *stream) {
  return pg::family_decide<pg::Sig2BlockFamily>(a, stream);
}
