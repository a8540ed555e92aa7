// pg_relu2_block.hip -- k_relu2_block: evaluate() (main.py:28-66) for [6, H1 <=
// 128, H2 <= 128, 2..4] ReLU networks with bias (two hidden layers;
// activation_function = ReLU, numpy_nn.py:6-9, 26), and pg_relu2_block_decide,
// its decision code on given inputs (include/pong_ga.h).  DESIGN.md 4.2k.
//
// k_relu2's design (pg_hidden2.hpp) one level up: the group that plays a game
// is a 256-thread block, not a slice of a wave.
//
// Layout.  Threads 0..127 (waves 0-1) hold the right paddle's network (the
// genome), threads 128..255 (waves 2-3) the left paddle's (a hall-of-fame row;
// idle against the scripted opponents and the ROM CPU: they skip the forward
// and only keep the barriers).  Thread hl = tid & 127 of a network holds, as
// f32 in VGPRs for the whole game, layer-1 unit hl (7 weights), layer-2 unit hl
// (its whole W2 row: 128 padded weights and the bias) and that unit's O output
// weights.  A padding unit (hl >= H1 or hl >= H2) and a padding column
// (j >= H1) have exact zero weights: max(0, 0) = 0 times 0 contributes exactly
// 0 to every sum and to the bound.  Every thread steps the same Pong state
// (pg_device.hpp); thread 0 writes the results and the trace.
//
// A frame.  feat32; the 6-fma chain of unit hl onto its bias weight; max(0, .);
// the activation goes to the network's LDS row; barrier A; 32 float4 broadcast
// reads of the row with 128 fmas onto the layer-2 bias, in ascending j;
// max(0, .); the O products W3_o,hl h2_hl, each summed over the wave's 64 lanes
// by group_sum<64> (six butterfly steps, every lane the same total) and written
// by the wave's lane 0 to LDS; barrier B; every thread then forms both
// networks' z^_o = (wave 0's sum + wave 1's sum) + b3_o -- in that order --
// from LDS, and takes both decisions itself under the networks' bounds, also
// in LDS: all 256 threads hold the same two action codes with no further
// exchange.  That is the order pg_relu2_bound.h's block chain lengths bound and
// tests/_relu2_model.py restates.
//
// The decision is k_relu2's (relu_certify, pg_relu.hpp): index 0 if t1 <= -e,
// the index of t1 if t1 > e and t1 - t2 > 2e, else the f64 forward from the
// genes in numpy's order (block_f64: blas_dot over [inputs..., 1] per unit, one
// unit per thread, activations through LDS, np.argmax's NaN rule -- the values
// are forward_f64_wave's).
//
// Barriers.  Every __syncthreads() is reached under conditions formed from
// block-uniform values only, each passed through readfirstlane so that the
// branch is a scalar one: the game index thread 0 broadcast through LDS, the
// shared game state (vis, the end of the game), the decisions every thread
// read from LDS (need).  block_load, block_z32 and block_f64 are entered by the
// whole block; inside them only work without a barrier is under a per-network
// (wave-uniform) or per-thread condition.
#include <hip/hip_runtime.h>

#include "../../include/pong_ga.h"
#include "pg_cascade.hpp"
#include "pg_certgame.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_relu.hpp"
#include "pg_relu2_bound.h"

namespace pg {

constexpr int kBlockH = PG_RELU2_BLOCK_MAX_H;  // threads per network, padded units per hidden layer
static_assert(kBlockH == 128, "two waves per network, four per 256-thread block");
static_assert(PG_RELU2_BLOCK_CHAIN1 == 1 + 2 + 6, "the bound's layer-1 chain: gene, feat32, block_z32's 6 fmas");
static_assert(PG_RELU2_BLOCK_CHAIN2 == 1 + kBlockH, "the bound's layer-2 chain: gene, one fma per padded unit");
// z^_o = (group_sum<64>(w3 h2) of wave 0 + that of wave 1) + b3_o
static_assert(PG_RELU2_BLOCK_CHAIN3 == 1 + 1 + relu_log2(64) + 1 + 1,
              "the bound's layer-3 chain: gene, product, group_sum<64>'s steps, the two waves, the bias");

template <int O>
struct BlockNet {
  float w1[7];        // layer-1 unit hl: 6 input weights + bias weight
  float w2[kBlockH];  // layer-2 unit hl: its weight of every (padded) layer-1 unit
  float b2;
  float w3[O];        // output weights of that unit
};

// LDS of a block.  n: 0 the right paddle's network, 1 the left paddle's.
struct alignas(16) BlockLds {
  float h[2][kBlockH];            // the f32 all-gather rows
  float part[4][4];               // [wave][o]: the wave's sum of the O products
  float c[2][4];                  // [n][o]: output biases
  float e[2];                     // [n]: |z^_o - z64_o| <= e (pg_relu2_bound.h); inf: always f64
  int game;                       // the game thread 0 took
  double d[2][2 * kBlockH + 4];   // [n]: the f64 path's activations (layer 1, layer 2, outputs); the load's A_j
  double red[4][3 * PG_RELU_MAX_OUT + 3];  // [wave]: the load's sums of the bound
};

// This thread's share of the genome's weights (numpy_nn.py:52-69 layout with
// bias: W1 [H1, 7], W2 [H2, H1 + 1], W3 [O, H2 + 1], bias columns last) as f32
// -- exact zeros for every padding unit's row and column -- and the network's
// bound and output biases into LDS, from the f64 genes.  Entered by the whole
// block; live (wave-uniform): this thread's network plays.  H1, H2 <= kBlockH
// (host-checked).
template <int O, typename WT>
__device__ __forceinline__ void block_load(BlockNet<O> &n, const WT *__restrict__ g, int H1, int H2, BlockLds &lds,
                                           int wv, int hl, bool live) {
  static_assert(O <= PG_RELU_MAX_OUT, "the bound's sums");
  // hl, H1 and H2 made opaque, as in hidden2_load: the unit offsets and the 128 padding tests j < H1
  // would otherwise be hoisted out of the game loop and kept live across every frame
  asm volatile("" : "+v"(hl));
  asm volatile("" : "+s"(H1), "+s"(H2));
  const int net = wv >> 1;
  const long off2 = (long)H1 * 7, off3 = off2 + (long)H2 * (H1 + 1);
  double asum = 0.0;
  if (live) {
    const bool ok = hl < H1;
    const WT *row = g + (long)(ok ? hl : 0) * 7;  // padding units load a valid row and are zeroed
    double w[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const WT raw = row[i];
      w[i] = ok ? (double)raw : 0.0;
      n.w1[i] = (float)w[i];
    }
    asum = pg_relu2_unit1(w);
    lds.d[net][hl] = asum;
  }
  __syncthreads();  // the A_j of both networks
  pg_relu2_sums s;
  pg_relu2_sums_init(&s);
  if (live) {
    const bool ok = hl < H2;
    const WT *row = g + off2 + (long)(ok ? hl : 0) * (H1 + 1);
    double p = 0.0, wsum = 0.0;
#pragma unroll
    for (int j = 0; j < kBlockH; ++j) {
      const bool inj = j < H1;
      const WT raw = row[inj ? j : 0];
      const double w = (ok && inj) ? (double)raw : 0.0;  // a padding unit's outgoing weight: exactly zero
      n.w2[j] = (float)w;
      p += fabs(w) * lds.d[net][j];  // (a padding unit j >= H1 wrote A_j = 0)
      wsum += fabs(w);
      if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);  // eight loads in flight at a time: not the kernel's register budget
    }
    const WT rawb = row[H1];
    const double bias = ok ? (double)rawb : 0.0;
    n.b2 = (float)bias;
    double w3[O];
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const WT raw = g[off3 + (long)o * (H2 + 1) + (ok ? hl : 0)];
      w3[o] = ok ? (double)raw : 0.0;  // (the same for a padding layer-2 unit)
      n.w3[o] = (float)w3[o];
    }
    pg_relu2_sums_unit2(&s, p + fabs(bias), wsum, w3, O);
  }
  // the sums over the network's 128 threads: over each wave, then its two waves in order (sums of
  // non-negative f64 terms: any order is within 2^-40, pg_relu2_bound.h)
  double v[3 * O + 3];
#pragma unroll
  for (int o = 0; o < O; ++o) {
    v[3 * o] = s.S[o];
    v[3 * o + 1] = s.T[o];
    v[3 * o + 2] = s.W3[o];
  }
  v[3 * O] = s.B;
  v[3 * O + 1] = s.W2;
  v[3 * O + 2] = asum;
#pragma unroll
  for (int i = 0; i < 3 * O + 3; ++i) {
    v[i] = half_sum_f64<64>(v[i]);
    if ((threadIdx.x & 63) == 0) lds.red[wv][i] = v[i];
  }
  __syncthreads();
  if (hl == 0) {  // one thread per network: its bound and output biases, for every thread of the block
    float e = __builtin_inff();
    float cf[O];
#pragma unroll
    for (int o = 0; o < O; ++o) cf[o] = 0.f;
    if (live) {
      const double *r0 = lds.red[2 * net], *r1 = lds.red[2 * net + 1];
      pg_relu2_sums t;
      pg_relu2_sums_init(&t);
      double c[O];
#pragma unroll
      for (int o = 0; o < O; ++o) {
        t.S[o] = r0[3 * o] + r1[3 * o];
        t.T[o] = r0[3 * o + 1] + r1[3 * o + 1];
        t.W3[o] = r0[3 * o + 2] + r1[3 * o + 2];
        c[o] = (double)g[off3 + (long)o * (H2 + 1) + H2];
        cf[o] = (float)c[o];
      }
      t.B = r0[3 * O] + r1[3 * O];
      t.W2 = r0[3 * O + 1] + r1[3 * O + 1];
      e = pg_relu2_bound_finish(pg_relu2_layout_block(), &t, r0[3 * O + 2] + r1[3 * O + 2], c, O);
    }
    lds.e[net] = e;
#pragma unroll
    for (int o = 0; o < O; ++o) lds.c[net][o] = cf[o];
  }
  __syncthreads();  // e and c are in place; the A_j are read: lds.d is free for the f64 path
}

// One frame's f32 chain of the live networks on the doubled-centroid features
// k (this thread's network's), up to the waves' sums in lds.part.  Entered by
// the whole block.
template <int O>
__device__ __forceinline__ void block_z32(const BlockNet<O> &n, const int k[6], BlockLds &lds, int wv, int hl,
                                          bool live) {
  const int net = wv >> 1;
  if (live) {
    float a = n.w1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) a = fmaf(n.w1[i], feat32(k[i]), a);
    lds.h[net][hl] = fmaxf(a, 0.f);
  }
  __syncthreads();  // barrier A: the rows
  if (live) {
    float a2 = n.b2;
    const float *hrow = lds.h[net];
    // eight float4 reads in flight, then their 32 fmas: left to the scheduler, every read but the
    // first four is waited for on its own (28 exposed LDS latencies a frame)
    constexpr int kBatch = 8;
#pragma unroll
    for (int j0 = 0; j0 < kBlockH; j0 += 4 * kBatch) {
      float4 h[kBatch];
#pragma unroll
      for (int b = 0; b < kBatch; ++b) h[b] = *(const float4 *)(hrow + j0 + 4 * b);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int b = 0; b < kBatch; ++b) {
        const int j = j0 + 4 * b;
        a2 = fmaf(n.w2[j], h[b].x, a2);
        a2 = fmaf(n.w2[j + 1], h[b].y, a2);
        a2 = fmaf(n.w2[j + 2], h[b].z, a2);
        a2 = fmaf(n.w2[j + 3], h[b].w, a2);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    const float h2 = fmaxf(a2, 0.f);
#pragma unroll
    for (int o = 0; o < O; ++o) {
      const float t = group_sum<64>(n.w3[o] * h2);
      if ((threadIdx.x & 63) == 0) lds.part[wv][o] = t;
    }
  }
  __syncthreads();  // barrier B: the waves' sums
}

// network n's z^ from the waves' sums, and its certificate (relu_certify): the proven index or -1
template <int O>
__device__ __forceinline__ int block_certify(const BlockLds &lds, int n, float z[O]) {
#pragma unroll
  for (int o = 0; o < O; ++o) z[o] = (lds.part[2 * n][o] + lds.part[2 * n + 1][o]) + lds.c[n][o];
  return relu_certify<O>(z, lds.e[n]);
}

// The f64 forward of one pass for the networks of need (bit n: network n), as
// forward_f64_wave runs it (NeuralNetwork.run numpy_nn.py:120-137 in np.dot's
// order, blas_dot over [inputs..., 1] per unit): one unit per thread,
// activations through LDS, every thread takes the argmax of each network of
// need into idx[n].  Entered by the whole block; g, k: this thread's network's.
template <int O, typename WT>
__device__ PG_SLOW_INLINE void block_f64(const WT *__restrict__ g, int H1, int H2, const int k[6], BlockLds &lds, int wv,
                                         int hl, int need, int idx[2]) {
  asm volatile("" : "+v"(hl));  // (as in block_load: nothing of this cold path is hoisted into the frame loop)
  const int net = wv >> 1;
  const bool mine = (need >> net) & 1;  // wave-uniform
  double *d1 = lds.d[net], *d2 = d1 + kBlockH, *out = d2 + kBlockH;
  const WT *w2 = g + (long)H1 * 7;
  if (mine && hl < H1) {
    double x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = feat64(k[i]);
    const WT *row = g + (long)hl * 7;
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < 6 ? x[i] : 1.0; }, 7,
                              blas_kind(hl, H1));
    d1[hl] = relu_f64(z);
  }
  __syncthreads();
  if (mine && hl < H2) {
    const WT *row = w2 + (long)hl * (H1 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H1 ? d1[i] : 1.0; },
                              H1 + 1, blas_kind(hl, H2));
    d2[hl] = relu_f64(z);
  }
  __syncthreads();
  if (mine && hl < O) {
    const WT *row = w2 + (long)H2 * (H1 + 1) + (long)hl * (H2 + 1);
    const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return i < H2 ? d2[i] : 1.0; },
                              H2 + 1, blas_kind(hl, O));
    out[hl] = relu_f64(z);
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    if ((need >> n) & 1) {
      const double *o_n = lds.d[n] + 2 * kBlockH;
      int best = 0;  // np.argmax: the first NaN if any, else the first maximum
#pragma unroll
      for (int o = 1; o < O; ++o)
        if (!__builtin_isnan(o_n[best]) && (__builtin_isnan(o_n[o]) || o_n[o] > o_n[best])) best = o;
      idx[n] = best;
    }
  }
}

// evaluate() (main.py:28-66): a persistent grid of blocks, each playing one
// game at a time to its end; thread 0 takes the next game from p.work (one
// atomic per game) and broadcasts it through LDS.  Every frame is stepped.
template <int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_relu2_block(EvalParams params) {
  const EvalParams p = params;  // (a copy of this function's own, as cert_game's)
  __shared__ BlockLds lds;
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
    block_load<O, WT>(nw, g, H1, H2, lds, wv, hl, live);
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
        block_z32<O>(nw, k, lds, wv, hl, live);
        float z[O];
        int idx[2];
        idx[0] = block_certify<O>(lds, 0, z);
        idx[1] = live_l ? block_certify<O>(lds, 1, z) : 0;
        // the networks the certificate left undecided: the same value in every thread of the block
        const int need = __builtin_amdgcn_readfirstlane((idx[0] < 0 ? 1 : 0) | (idx[1] < 0 ? 2 : 0));
        if (__builtin_expect(need != 0, 0)) block_f64<O, WT>(g, H1, H2, k, lds, wv, hl, need, idx);
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
  __shared__ BlockLds lds;
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), net = wv >> 1, hl = tid & (kBlockH - 1);
  const WT *genomes = (const WT *)p.genomes;
  const bool live = net == 0;
  for (long t = blockIdx.x; t < p.n; t += gridDim.x) {
    const WT *g = genomes + (long)(p.gidx ? p.gidx[t] : t) * p.gstride;
    BlockNet<O> nw = {};
    block_load<O, WT>(nw, g, p.H1, p.H2, lds, wv, hl, live);
    int k[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = p.k[t * 6 + i];
    block_z32<O>(nw, k, lds, wv, hl, live);
    float z[O];
    int idx[2] = {block_certify<O>(lds, 0, z), 0};
    const int need = __builtin_amdgcn_readfirstlane(idx[0] < 0 ? 1 : 0);
    if (need) block_f64<O, WT>(g, p.H1, p.H2, k, lds, wv, hl, need, idx);
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
static bool relu2_block_shape_ok(const pg_net &n) {
  return n.n_nodes == 4 && n.nodes[0] == 6 && n.nodes[1] >= 2 && n.nodes[1] <= kBlockH && n.nodes[2] >= 2 &&
         n.nodes[2] <= kBlockH && n.nodes[3] >= 2 && n.nodes[3] <= 4;
}

int32_t relu2_block_scope(const pg_eval_args &a) {
  if (a.net.activation != PG_ACT_RELU)
    return fail(PG_ERR_UNSUPPORTED, "activation sigmoid: the relu2_block kernel evaluates PG_ACT_RELU networks only");
  if (!relu2_block_shape_ok(a.net) || !a.net.bias)
    return fail(PG_ERR_UNSUPPORTED, "relu2_block kernel needs NETWORK_SHAPE [6, 2..128, 2..128, 2..4] with bias");
  if (a.precision == PG_PREC_F64) return fail(PG_ERR_UNSUPPORTED, "relu2_block kernel is the certified-precision path");
  if (a.horizon > 0)
    return fail(PG_ERR_UNSUPPORTED, "relu2_block kernel plays whole episodes: no fixed-horizon mode (horizon must be 0)");
  if (a.hard_log) return fail(PG_ERR_UNSUPPORTED, "relu2_block kernel keeps no hard-case log (hard_log must be NULL)");
  return PG_OK;
}

#define PG_BLOCK_DISPATCH(KERNEL, O, f64, grid, s, p)                                         \
  do {                                                                                        \
    if (O == 2) {                                                                             \
      if (f64) hipLaunchKernelGGL((KERNEL<2, double>), dim3(grid), dim3(256), 0, s, p);       \
      else hipLaunchKernelGGL((KERNEL<2, float>), dim3(grid), dim3(256), 0, s, p);            \
    } else if (O == 3) {                                                                      \
      if (f64) hipLaunchKernelGGL((KERNEL<3, double>), dim3(grid), dim3(256), 0, s, p);       \
      else hipLaunchKernelGGL((KERNEL<3, float>), dim3(grid), dim3(256), 0, s, p);            \
    } else {                                                                                  \
      if (f64) hipLaunchKernelGGL((KERNEL<4, double>), dim3(grid), dim3(256), 0, s, p);       \
      else hipLaunchKernelGGL((KERNEL<4, float>), dim3(grid), dim3(256), 0, s, p);            \
    }                                                                                         \
  } while (0)

// p: a network in relu2_block_scope, row strides of at least its gene count (pg_eval_population)
int32_t launch_relu2_block(const EvalParams &p, int dtype, hipStream_t s) {
  const int cap = num_cus() * 2;  // a persistent grid: two blocks per CU
  const int grid = p.total < cap ? p.total : cap;
  if (grid <= 0) return PG_OK;
  PG_BLOCK_DISPATCH(k_relu2_block, p.nodes[3], dtype == PG_F64, grid, s, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

}  // namespace pg

extern "C" int32_t pg_relu2_block_decide(const pg_relu_decide_args *a, void *stream) {
  using namespace pg;
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  if (a->net.dtype != PG_F32 && a->net.dtype != PG_F64) return fail(PG_ERR_INVALID, "net.dtype=%d", a->net.dtype);
  if (a->net.activation != PG_ACT_RELU)
    return fail(PG_ERR_UNSUPPORTED,
                "pg_relu2_block_decide: activation=%d, the relu2_block kernel decides PG_ACT_RELU networks only",
                a->net.activation);
  if (!relu2_block_shape_ok(a->net) || !a->net.bias)
    return fail(PG_ERR_UNSUPPORTED,
                "pg_relu2_block_decide: the relu2_block kernel's shapes [6, 2..128, 2..128, 2..4] with bias only");
  if (a->n < 0) return fail(PG_ERR_INVALID, "n=%d < 0", a->n);
  if (a->n == 0) return PG_OK;
  const int H1 = a->net.nodes[1], H2 = a->net.nodes[2], O = a->net.nodes[3];
  const long G = (long)H1 * 7 + (long)H2 * (H1 + 1) + (long)O * (H2 + 1);
  if (!a->genomes || a->genome_stride < G || !a->k || !a->index)
    return fail(PG_ERR_INVALID, "genomes/k/index NULL or genome_stride < gene count %ld", G);
  const CertDecideParams p = cert_decide_params(a, H1, H2);
  const int cap = num_cus() * 2;
  const int grid = a->n < cap ? a->n : cap;
  PG_BLOCK_DISPATCH(k_relu2_block_decide, O, a->net.dtype == PG_F64, grid, (hipStream_t)stream, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}
