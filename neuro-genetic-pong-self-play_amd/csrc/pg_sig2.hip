// pg_sig2.hip -- k_sig2: evaluate() (main.py:28-66) for [6, H1 <= 64,
// H2 <= 64, 2..4] sigmoid networks with bias (two hidden layers; the reference's
// default activation, numpy_nn.py:22-26), and pg_sig2_decide, its decision code
// on given inputs (include/pong_ga.h).
//
//   k_sig2<LN, U1, U2, O, WT>  k_relu2's layout and game loop (pg_relu2.hip): an
//                         aligned group of 2 LN lanes plays one game to its
//                         end, taking games from the p.work queue; lanes
//                         [0, LN) hold the right paddle's network (the genome),
//                         lanes [LN, 2 LN) the left paddle's (a hall-of-fame
//                         row; idle against the scripted opponents and the ROM
//                         CPU), all three layers as f32 in VGPRs for the whole
//                         game.  Each frame: the f32 chain with sigmoid_f32 in
//                         both hidden layers, certify_c under the network's
//                         static bound (pg_sig2_bound.h), and for the undecided
//                         half-groups tight_gap_move, plateau_f32 and then the
//                         f64 forward in numpy's order from the genes
//                         (pg_sig2.hpp).  Every frame is stepped; no lane
//                         records, no workspace beyond the base.
// DESIGN.md 4.2f.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/pong_ga.h"
#include "pg_cascade.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_sig2.hpp"

namespace pg {

template <int LN, int U1, int U2, int O, typename WT>
__global__ __launch_bounds__(256, 2) void k_sig2(EvalParams p) {
  constexpr int L = 2 * LN, HPB = 256 / LN;
  static_assert(L >= 8 && L <= 64, "other_half / group_broadcast layouts");
  __shared__ Relu2Lds<LN, U1, U2> lds_all[HPB];
  const int lane = threadIdx.x & 63;
  const int lig = threadIdx.x & (L - 1);
  const int half = lig / LN, hl = lig & (LN - 1);
  const int leader = lane & ~(L - 1);
  Relu2Lds<LN, U1, U2> &lds = lds_all[threadIdx.x / LN];
  const WT *genomes = (const WT *)p.genomes;
  const WT *opponents = (const WT *)p.opponents;
  const int H1 = p.nodes[1], H2 = p.nodes[2];
  const int games_total = active_total(p);
  uint32_t c_steps = 0, c_fwd = 0, c_fail = 0, c_slow = 0, c_games = 0;  // per lane: far below 2^32

  bool have = false, more = true;  // a game in play; the queue may hold more
  int w = 0, kind = 0;
  bool live = false;  // this half's network plays (the left half: only against a hall-of-fame row)
  const WT *g = genomes;
  Sig2Net<LN, U1, U2, O> net = {};  // (sig2_load updates it in place)
  Pong st;
  int act_r = 0, act_l = 0, timeout = 0, total = 0, frames = 0;
  for (;;) {
    if (!have && more) {
      int ww = 0;
      if (lig == 0) ww = (int)atomicAdd(p.work, 1u);
      w = group_broadcast<L>(ww, leader);
      if (w < games_total) {
        const int i = w / p.n_games, gi = w % p.n_games;
        kind = p.kind[w];
        const WT *gr = genomes + (long)genome_row(p, i) * p.gstride;
        const WT *gl = (kind == kOppNN) ? opponents + (long)p.opp[w] * p.ostride : gr;
        g = half ? gl : gr;
        live = half == 0 || kind == kOppNN;
        sig2_load<LN, U1, U2, O, WT>(net, g, H1, H2, lds, hl);
        st.reset(game_seed(p.seed, gi), kind == kOppRomCpu);
        act_r = act_l = timeout = total = frames = 0;
        have = true;
      } else {
        more = false;
      }
    }
    if (__builtin_amdgcn_ballot_w64(have) == 0) break;
    if (have) {
      const int s1b = st.s1, s2b = st.s2;
      const int pvis = st.vis, pbx2 = 2 * st.bx + kBallW - 1, pby2 = 2 * st.by + kBallH - 1;
      st.step(act_r, act_l);
      frames += 1;
      const int vis = st.vis;
      const int bx2 = 2 * st.bx + kBallW - 1, by2 = 2 * st.by + kBallH - 1;
      const int lc2 = paddle_c2(st.lpy), rc2 = paddle_c2(st.rpy);
      int left = 0, right = 0;
      if (PG_ANY(vis) && vis) {  // get_actions main.py:143-150
        const int lbx2 = pvis ? pbx2 : bx2, lby2 = pvis ? pby2 : by2;
        // utils.inference's features (utils.py:139-153) as doubled centroids: the left
        // paddle sees the field mirrored, (160 - x) / 160 = (320 - 2x) / 320 exactly
        int k[6];
        k[0] = half ? 320 - bx2 : bx2;
        k[1] = by2;
        k[2] = half ? 320 - lbx2 : lbx2;
        k[3] = lby2;
        k[4] = half ? lc2 : rc2;
        k[5] = half ? rc2 : lc2;
        float z[O];
        int stage;
        const int mine =
            index_to_code(sig2_decide<LN, U1, U2, O, WT>(net, g, H1, H2, k, live, lds, hl, z, stage));
        const int other = other_half<L>(mine);
        right = half ? other : mine;
        left = half ? mine : other;
        c_fwd += live ? 1 : 0;
        c_fail += stage > 0 ? 1 : 0;
        c_slow += stage == 3 ? 1 : 0;
        if (kind == kOppScore)
          left = (st.s1 <= st.s2) ? hardcoded(by2, lc2) : 0;
        else if (kind != kOppNN)
          left = hardcoded(by2, lc2);
      }
      act_l = clamp_action(lc2, left);
      act_r = clamp_action(rc2, right);
      if (p.trace && w < p.trace_games && frames <= p.trace_cap && lig == 0)
        p.trace[(long)w * p.trace_cap + frames - 1] = (uint8_t)(act_r | (act_l << 2) | (vis << 4));
      if (frames > 1) {  // calculate_timeout_and_frames main.py:128-135
        if (st.s1 == s1b && st.s2 == s2b) {
          timeout += 1;
        } else {
          total += timeout;
          timeout = 0;
        }
      }
      if (st.s1 >= p.win_score || st.s2 >= p.win_score || st.done() || timeout > p.timeout_thresh) {
        c_steps += frames;
        c_games += 1;
        if (lig == 0) finish_game(p, w, st, frames, total);
        have = false;
      }
    }
  }
  if (p.counters) {
    if (lig == 0 && c_games) {
      atomicAdd((unsigned long long *)&p.counters[0], (unsigned long long)c_steps);
      atomicAdd((unsigned long long *)&p.counters[3], (unsigned long long)c_games);
    }
    if (hl == 0 && c_fwd) {  // one lane per half-group: its network's forwards
      atomicAdd((unsigned long long *)&p.counters[1], (unsigned long long)c_fwd);
      if (c_fail) atomicAdd((unsigned long long *)&p.counters[4], (unsigned long long)c_fail);
      if (c_slow) atomicAdd((unsigned long long *)&p.counters[2], (unsigned long long)c_slow);
    }
  }
}

// pg_sig2_decide: one half-group per pass, the decision code of a k_sig2 frame.
template <int LN, int U1, int U2, int O, typename WT>
__global__ __launch_bounds__(256) void k_sig2_decide(Relu2DecideParams p) {
  constexpr int HPB = 256 / LN;
  __shared__ Relu2Lds<LN, U1, U2> lds_all[HPB];
  const int hg = threadIdx.x / LN, hl = threadIdx.x & (LN - 1);
  const WT *genomes = (const WT *)p.genomes;
  for (long base = (long)blockIdx.x * HPB; base < p.n; base += (long)gridDim.x * HPB) {
    const long t = base + hg;
    if (t < p.n) {
      const WT *g = genomes + (long)(p.gidx ? p.gidx[t] : t) * p.gstride;
      Sig2Net<LN, U1, U2, O> net = {};  // (sig2_load updates it in place)
      sig2_load<LN, U1, U2, O, WT>(net, g, p.H1, p.H2, lds_all[hg], hl);
      int k[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) k[i] = p.k[t * 6 + i];
      float z[O];
      int stage;
      const int idx = sig2_decide<LN, U1, U2, O, WT>(net, g, p.H1, p.H2, k, true, lds_all[hg], hl, z, stage);
      if (hl == 0) {
        p.index[t] = idx;
        if (p.stage) p.stage[t] = stage;
        if (p.bound) p.bound[t] = net.n.e;
        if (p.z32) {
#pragma unroll
          for (int o = 0; o < O; ++o) p.z32[t * O + o] = z[o];
        }
      }
    }
  }
}

bool sig2_shape_ok(const pg_net &n) {
  return n.n_nodes == 4 && n.nodes[0] == 6 && n.nodes[1] >= 2 && n.nodes[1] <= kSig2MaxH && n.nodes[2] >= 2 &&
         n.nodes[2] <= kSig2MaxH && n.nodes[3] >= 2 && n.nodes[3] <= 4;
}

// the instances: LN = relu2_lanes(H1, H2) lanes per network, relu2_units(LN) units of each layer per lane
#define PG_SIG2_DISPATCH(KERNEL, LN, O, f64, grid, s, p)                                                        \
  do {                                                                                                          \
    constexpr int U_ = relu2_units(LN);                                                                         \
    if (O == 2) {                                                                                               \
      if (f64) hipLaunchKernelGGL((KERNEL<LN, U_, U_, 2, double>), dim3(grid), dim3(256), 0, s, p);             \
      else hipLaunchKernelGGL((KERNEL<LN, U_, U_, 2, float>), dim3(grid), dim3(256), 0, s, p);                  \
    } else if (O == 3) {                                                                                        \
      if (f64) hipLaunchKernelGGL((KERNEL<LN, U_, U_, 3, double>), dim3(grid), dim3(256), 0, s, p);             \
      else hipLaunchKernelGGL((KERNEL<LN, U_, U_, 3, float>), dim3(grid), dim3(256), 0, s, p);                  \
    } else {                                                                                                    \
      if (f64) hipLaunchKernelGGL((KERNEL<LN, U_, U_, 4, double>), dim3(grid), dim3(256), 0, s, p);             \
      else hipLaunchKernelGGL((KERNEL<LN, U_, U_, 4, float>), dim3(grid), dim3(256), 0, s, p);                  \
    }                                                                                                           \
  } while (0)

static long sig2_genes(int H1, int H2, int O) { return (long)H1 * 7 + (long)H2 * (H1 + 1) + (long)O * (H2 + 1); }

int32_t launch_sig2(const EvalParams &p, int dtype, hipStream_t s) {
  const int H1 = p.nodes[1], H2 = p.nodes[2], O = p.nodes[3];
  if (p.n_nodes != 4 || p.nodes[0] != 6 || H1 < 2 || H1 > kSig2MaxH || H2 < 2 || H2 > kSig2MaxH || O < 2 || O > 4)
    return fail(PG_ERR_UNSUPPORTED, "sig2 kernel needs NETWORK_SHAPE [6, 2..64, 2..64, 2..4]");
  if (!p.bias) return fail(PG_ERR_UNSUPPORTED, "sig2 kernel needs a network with bias");
  const int LN = relu2_lanes(H1, H2);
  if (LN * relu2_units(LN) < H1 || LN * relu2_units(LN) < H2)
    return fail(PG_ERR_UNSUPPORTED, "sig2 kernel: no layout for H1=%d H2=%d", H1, H2);
  const long G = sig2_genes(H1, H2, O);
  if (p.gstride < G || (p.n_opponents > 0 && p.ostride < G))
    return fail(PG_ERR_INVALID, "sig2 kernel: a row stride is below the gene count");
  const int GPB = 256 / (2 * LN);
  const int want = (p.total + GPB - 1) / GPB;
  const int cap = num_cus() * 2;
  const int grid = want < cap ? want : cap;
  if (grid <= 0) return PG_OK;
  const bool f64 = dtype == PG_F64;
  if (LN == 4) PG_SIG2_DISPATCH(k_sig2, 4, O, f64, grid, s, p);
  else if (LN == 16) PG_SIG2_DISPATCH(k_sig2, 16, O, f64, grid, s, p);
  else PG_SIG2_DISPATCH(k_sig2, 32, O, f64, grid, s, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

}  // namespace pg

using namespace pg;

extern "C" int32_t pg_sig2_decide(const pg_relu_decide_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  if (a->net.dtype != PG_F32 && a->net.dtype != PG_F64) return fail(PG_ERR_INVALID, "net.dtype=%d", a->net.dtype);
  if (a->net.activation != PG_ACT_SIGMOID)
    return fail(PG_ERR_UNSUPPORTED, "pg_sig2_decide: activation=%d, the sig2 kernel decides sigmoid networks only",
                a->net.activation);
  if (!sig2_shape_ok(a->net))
    return fail(PG_ERR_UNSUPPORTED, "pg_sig2_decide: the sig2 kernel's shapes [6, 2..64, 2..64, 2..4] only");
  if (!a->net.bias) return fail(PG_ERR_UNSUPPORTED, "pg_sig2_decide: the sig2 kernel needs a network with bias");
  if (a->n < 0) return fail(PG_ERR_INVALID, "n=%d < 0", a->n);
  if (a->n == 0) return PG_OK;
  const int H1 = a->net.nodes[1], H2 = a->net.nodes[2], O = a->net.nodes[3];
  const long G = sig2_genes(H1, H2, O);
  if (!a->genomes || a->genome_stride < G || !a->k || !a->index)
    return fail(PG_ERR_INVALID, "genomes/k/index NULL or genome_stride < gene count %ld", G);
  const int LN = relu2_lanes(H1, H2);
  Relu2DecideParams p;
  memset(&p, 0, sizeof(p));
  p.genomes = a->genomes;
  p.gidx = a->genome_index;
  p.k = a->k;
  p.index = a->index;
  p.stage = a->stage;
  p.z32 = a->z32;
  p.bound = a->bound;
  p.gstride = a->genome_stride;
  p.n = a->n;
  p.H1 = H1;
  p.H2 = H2;
  const int HPB = 256 / LN;
  const int want = (a->n + HPB - 1) / HPB;
  const int cap = num_cus() * 8;
  const int grid = want < cap ? want : cap;
  const bool f64 = a->net.dtype == PG_F64;
  hipStream_t s = (hipStream_t)stream;
  if (LN == 4) PG_SIG2_DISPATCH(k_sig2_decide, 4, O, f64, grid, s, p);
  else if (LN == 16) PG_SIG2_DISPATCH(k_sig2_decide, 16, O, f64, grid, s, p);
  else PG_SIG2_DISPATCH(k_sig2_decide, 32, O, f64, grid, s, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}
