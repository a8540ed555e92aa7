// pg_certgame.hpp -- what the certified f32 kernel families share: k_relu
// (pg_relu.hip), k_relu2 (pg_relu2.hip), k_sig2 (pg_sig2.hip) and k_relu3 (pg_relu3.hip) are thin
// __global__ wrappers of the one game loop cert_game<P, kAdvance, kSolo>, and
// k_relu_decide, k_relu2_decide and k_sig2_decide of the one pass
// cert_decide_pass<P>.  k_relu_adv, k_relu2_adv and k_sig2_adv wrap the same
// loop with kAdvance on (PG_KERNEL_ADVANCE), k_*_solo and k_*_adv_solo with
// kSolo on (PG_KERNEL_SOLO).  DESIGN.md 4.2g, 4.2h, 4.2i.
//
// A policy P describes one instance of a family to both bodies:
//   LN, O, WT        lanes per network (a half-group), outputs, genome type
//   kF64Stage        the stage that means "recomputed in f64": 1 where the
//                    stages are 0/1 (k_relu, k_relu2), 3 for k_sig2's 0..3
//   Net              a network's weights and bound as f32 in VGPRs; Net::e is
//                    the bound pg_*_decide reports
//   Lds              one half-group's __shared__ element
//   Dims, dims(params)   optional: the policy's own hidden sizes in place of
//                    CertDims (cert_dims below; k_relu3, pg_hidden3.hpp)
//   load(net, g, dims, lds, hl)       this lane's share of genome g, in place
//   decide(net, g, dims, k, live, lds, hl, z, stage)   one frame's np.argmax
//                    index on the doubled-centroid features k; z: the f32
//                    output pre-activations, stage: see kF64Stage
// The host side below (the dispatch over O and the genome type, grid sizes,
// pg_*_decide's parameters) serves the three .hip files.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <type_traits>

#include "../../include/pong_ga.h"
#include "pg_cascade.hpp"
#include "pg_device.hpp"
#include "pg_eval.hpp"

namespace pg {

// the hidden sizes of a network: H2 is unused by the one-hidden-layer family
struct CertDims {
  int H1, H2;
};

// pg_relu_decide's, pg_relu2_decide's and pg_sig2_decide's parameters
struct CertDecideParams {
  const void *genomes;
  const int32_t *gidx;
  const int32_t *k;
  int32_t *index;
  int32_t *stage;
  float *z32;
  float *bound;
  int64_t gstride;
  int n, H1, H2;
};

// The hidden sizes as a policy's load and decide take them, from a launch's
// parameters: CertDims, unless the policy names its own (P::Dims, made by
// P::dims(params): k_relu3's three widths, pg_hidden3.hpp) -- so the structs
// above, and with them the other families' kernels, stay what they are.
template <class P, class = void>
struct cert_dims {
  static __device__ __forceinline__ CertDims of(const EvalParams &p) { return {p.nodes[1], p.nodes[2]}; }
  static __device__ __forceinline__ CertDims of(const CertDecideParams &p) { return {p.H1, p.H2}; }
};
template <class P>
struct cert_dims<P, std::void_t<typename P::Dims>> {
  template <class Params>
  static __device__ __forceinline__ typename P::Dims of(const Params &p) {
    return P::dims(p);
  }
};

// kAdvance's per-group record (with kSolo: per half-group): Brent's saved rally
// key, the no-score count it was saved at (-1: no search open) and the span; the
// group's frames advanced in closed form.  In LDS, written by the group's lane 0
// (with kSolo: the half-group's, the counts by the game's first lane) and read only behind
// the rare tests (a bounce past the kRallyHits-th return, a serve, the end), so
// the common frame path holds none of it in registers.  The search's three
// fields go through relaxed atomics (adv_ld / adv_st): the other lanes of the
// group read what lane 0 wrote earlier in the wave's program order, which the
// compiler must not replace by a value it read before.  (Not volatile: a
// volatile access keeps its generic pointer, flat instructions and two more
// VGPRs for the address across the frame loop.)
struct CertAdvance {
  uint64_t key;
  int at, span;
  uint32_t skipped, hidden;
};
template <class T>
__device__ __forceinline__ T adv_ld(T *a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
template <class T>
__device__ __forceinline__ void adv_st(T *a, T v) { __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
template <int N>
__device__ __forceinline__ CertAdvance *cert_advance_lds() {
  __shared__ CertAdvance adv[N];
  return adv;
}

// kSolo: the next game of one of the two queues -- the kOppNN games (kNN) or the
// others -- from its counter q, which walks all games; games_total: none is left
template <bool kNN>
__device__ __forceinline__ int cert_take(const EvalParams &p, unsigned int *q, int games_total) {
  for (;;) {
    const unsigned int w = atomicAdd(q, 1u);
    if (w >= (unsigned int)games_total) return games_total;
    if ((p.kind[w] == kOppNN) == kNN) return (int)w;
  }
}

// evaluate() (main.py:28-66): an aligned group of 2 LN lanes plays one game to
// its end, taking games from the p.work queue; lanes [0, LN) hold the right
// paddle's network (the genome), lanes [LN, 2 LN) the left paddle's (a
// hall-of-fame row; idle against the scripted opponents and the ROM CPU).
// Every lane of a group steps the same Pong state.  Every frame is stepped,
// unless kAdvance (PG_KERNEL_ADVANCE, the k_*_adv wrappers; untraced launches
// only): then a serve delay's hidden-ball frames and the rest of a rally proven
// periodic are advanced in closed form, k_service's rules (pg_service.hpp,
// DESIGN.md 4.2h) -- the same results, counters [12] and [8].
//
// kSolo (PG_KERNEL_SOLO, the k_*_solo wrappers): a game against
// a scripted opponent or the ROM CPU has no left network, so a half-group plays
// it alone -- role 0, the right paddle's unmirrored features, whichever half it
// is -- and only a game against a hall-of-fame row takes the whole group (pair).
// Two queues walk the games: p.work[0] hands out the kOppNN ones, p.work[1] the
// others, each over all indices, the taking lane skipping the other queue's.  A
// free group takes NN games while that queue lasts; from then on each half takes
// solo games on its own.  Both halves of a pair game come free at the same
// frame, so no half ever waits for its sibling: no barrier, no spin.  Every game
// variable below is uniform over the lanes that play the game; the game's first
// lane (lead) writes its results.  The per-game work is the base loop's, so the
// outputs and all 16 counters are too.
template <class P, bool kAdvance, bool kSolo = false>
__device__ __forceinline__ void cert_game(const EvalParams &params) {
  // a copy of this function's own: its fields are values from here on.  Read
  // through the reference they stay loads of unknown memory until this body is
  // inlined into its kernel, and the kernels then come out differently
  // scheduled.
  const EvalParams p = params;
  using WT = typename P::WT;
  constexpr int LN = P::LN, O = P::O, L = 2 * LN, HPB = 256 / LN;
  __shared__ typename P::Lds lds_all[HPB];
  const int lane = threadIdx.x & 63;
  const int lig = threadIdx.x & (L - 1);
  const int half = lig / LN, hl = lig & (LN - 1);
  const int leader = lane & ~(L - 1);
  // (below, the first lane of what keeps a kAdvance record and reports counters
  // -- the group; kSolo: the half-group -- is spelled out as "kSolo ? hl == 0 :
  // lig == 0" and a game's first lane as "kSolo ? lead : lig == 0" at each use:
  // with either in a named bool, or took as a local of the loop body, the base
  // kernels come out differently allocated and scheduled)
  typename P::Lds &lds = lds_all[threadIdx.x / LN];
  const WT *genomes = (const WT *)p.genomes;
  const WT *opponents = (const WT *)p.opponents;
  const auto dims = cert_dims<P>::of(p);
  const int games_total = active_total(p);
  // per lane: far below 2^32.  c_fail (stage > 0) is c_f64 itself where the
  // stages are 0/1: a counter of its own there costs the frame loop registers
  uint32_t c_steps = 0, c_fwd = 0, c_fail = 0, c_f64 = 0, c_games = 0;
  [[maybe_unused]] CertAdvance *adv = nullptr;  // this group's record (kAdvance); kSolo: this half-group's
  if constexpr (kAdvance) {
    if constexpr (kSolo) adv = cert_advance_lds<HPB>() + threadIdx.x / LN;
    else adv = cert_advance_lds<256 / L>() + threadIdx.x / L;
    if (kSolo ? hl == 0 : lig == 0) {
      adv_st(&adv->at, -1);
      adv->skipped = adv->hidden = 0;
    }
  }

  bool have = false, more = true;  // a game in play; the queue may hold more (kSolo: the NN queue)
  // kSolo: the solo queue may hold more; this game takes the whole group; w is
  // a game taken this round; this lane is its game's first
  [[maybe_unused]] bool more_solo = kSolo, pair = !kSolo, took = false;
  [[maybe_unused]] bool lead = lig == 0;
  int w = 0, kind = 0;
  bool live = false;  // this half's network plays (the left half: only against a hall-of-fame row)
  const WT *g = genomes;
  typename P::Net net = {};  // (P::load updates it in place)
  Pong st;
  int act_r = 0, act_l = 0, timeout = 0, total = 0, frames = 0;
  for (;;) {
    if constexpr (kSolo) {
      took = false;
      // a free group: the next NN game.  (have and more are uniform over the
      // group while more is set: its solo games start only once it is not)
      if (!have && more) {
        int ww = 0;
        if (lig == 0) ww = cert_take<true>(p, p.work, games_total);
        w = __shfl(ww, leader, 64);
        more = took = w < games_total;
        pair = true;
        lead = lig == 0;
      }
      // a free half-group, the NN queue exhausted: the next solo game
      if (!have && !more && more_solo) {
        int ww = 0;
        if (hl == 0) ww = cert_take<false>(p, p.work + 1, games_total);
        w = __shfl(ww, lane & ~(LN - 1), 64);
        more_solo = took = w < games_total;
        pair = false;
        lead = hl == 0;
      }
    }
    if (kSolo ? took : !have && more) {
      if constexpr (!kSolo) {
        int ww = 0;
        if (lig == 0) ww = (int)atomicAdd(p.work, 1u);
        w = group_broadcast<L>(ww, leader);
      }
      if (kSolo || w < games_total) {
        const int i = w / p.n_games, gi = w % p.n_games;
        kind = p.kind[w];
        const WT *gr = genomes + (long)genome_row(p, i) * p.gstride;
        const WT *gl = (kind == kOppNN) ? opponents + (long)p.opp[w] * p.ostride : gr;
        g = half ? gl : gr;  // (kSolo: a solo game's kind is not kOppNN, so both halves get gr)
        live = kSolo || half == 0 || kind == kOppNN;
        P::load(net, g, dims, lds, hl);
        st.reset(game_seed(p.seed, gi), kind == kOppRomCpu);
        act_r = act_l = timeout = total = frames = 0;
        have = true;
        // groups reload games in place: the last game's search must not survive
        if constexpr (kAdvance) {
          if (kSolo ? hl == 0 : lig == 0) adv_st(&adv->at, -1);
        }
      } else {
        more = false;
      }
    }
    if (__builtin_amdgcn_ballot_w64(have) == 0) break;
    if (have) {
      if constexpr (kAdvance) {
        // The serve delay in closed form (pg_service.hpp): while the ball is
        // hidden no point can be scored, get_actions returns [0,0]
        // (main.py:151-153) -- the pending actions are clamp-only already: the
        // frame of a miss and a game's start decide nothing -- and a paddle only
        // drifts back inside the clamp band (Pong::drift), so the frames before
        // the serve frame are advanced at once.  The no-score counter cannot
        // pass TIMEOUT_THRESH on the way: it is at most 0 + 29 here and
        // pg_eval_population refuses a threshold below 32.
        const bool hid = !st.vis && st.timer >= 2;
        if (PG_ANY(hid) && hid) {
          const int h = st.timer - 1;
          st.rpy = Pong::drift(st.rpy, h);
          if (!st.one_player) st.lpy = Pong::drift(st.lpy, h);
          st.timer = 1;
          act_r = clamp_action(paddle_c2(st.rpy), 0);
          act_l = clamp_action(paddle_c2(st.lpy), 0);  // (a 1-player env's CPU paddle ignores it)
          // a game's frame 1 does not count towards the no-score counter
          // (main.py:128-135): after a start's 29 frames it stands at 28
          timeout += frames ? h : h - 1;
          frames += h;
          if (kSolo ? lead : lig == 0) adv->hidden += h;
        }
      }
      const int s1b = st.s1, s2b = st.s2;
      const int pvis = st.vis, pbx2 = 2 * st.bx + kBallW - 1, pby2 = 2 * st.by + kBallH - 1;
      [[maybe_unused]] const int ev = st.step(act_r, act_l);
      frames += 1;
      const int vis = st.vis;
      const int bx2 = 2 * st.bx + kBallW - 1, by2 = 2 * st.by + kBallH - 1;
      const int lc2 = paddle_c2(st.lpy), rc2 = paddle_c2(st.rpy);
      int left = 0, right = 0;
      if (PG_ANY(vis) && vis) {  // get_actions main.py:143-150
        const int lbx2 = pvis ? pbx2 : bx2, lby2 = pvis ? pby2 : by2;
        // utils.inference's features (utils.py:139-153) as doubled centroids: the left
        // paddle sees the field mirrored, (160 - x) / 160 = (320 - 2x) / 320 exactly
        // (kSolo: a half-group playing alone is the right paddle, whichever half it is)
        int role = half;
        if constexpr (kSolo) role = pair ? half : 0;
        int k[6];
        k[0] = role ? 320 - bx2 : bx2;
        k[1] = by2;
        k[2] = role ? 320 - lbx2 : lbx2;
        k[3] = lby2;
        k[4] = role ? lc2 : rc2;
        k[5] = role ? rc2 : lc2;
        float z[O];
        int stage;
        const int mine = index_to_code(P::decide(net, g, dims, k, live, lds, hl, z, stage));
        const int other = other_half<L>(mine);  // (kSolo: used in a pair game only; a solo game's left is set below)
        right = role ? other : mine;
        left = role ? mine : other;
        c_fwd += live ? 1 : 0;
        if constexpr (P::kF64Stage != 1) c_fail += stage > 0 ? 1 : 0;
        c_f64 += stage == P::kF64Stage ? 1 : 0;
        if (kind == kOppScore)
          left = (st.s1 <= st.s2) ? hardcoded(by2, lc2) : 0;
        else if (kind != kOppNN)
          left = hardcoded(by2, lc2);
      }
      act_l = clamp_action(lc2, left);
      act_r = clamp_action(rc2, right);
      if constexpr (!kAdvance) {  // (a traced launch runs the stepping kernel)
        if (p.trace && w < p.trace_games && frames <= p.trace_cap && (kSolo ? lead : lig == 0))
          p.trace[(long)w * p.trace_cap + frames - 1] = (uint8_t)(act_r | (act_l << 2) | (vis << 4));
      }
      if (frames > 1) {  // calculate_timeout_and_frames main.py:128-135
        if (st.s1 == s1b && st.s2 == s2b) {
          timeout += 1;
        } else {
          total += timeout;
          timeout = 0;
          if constexpr (kAdvance) {
            if (kSolo ? hl == 0 : lig == 0) adv_st(&adv->at, -1);  // a point: the next rally searches afresh
          }
        }
      }
      if constexpr (kAdvance) {
        // A periodic rally ends at the timeout with nothing else changed: jump
        // there.  Brent's cycle search as k_service runs it (pg_service.hpp),
        // sampled at the frames where a paddle returned the ball, from the
        // point's kRallyHits-th return on (rally_key caps hits there, so no
        // earlier state of the point can recur): a key equal to the saved one
        // proves the rally periodic; the save moves forward when the distance
        // reaches the span (kRallySpan0 frames, doubling).
        const bool check = ev == kStepBounce && st.hits >= kRallyHits && timeout <= p.timeout_thresh;
        if (PG_ANY(check) && check) {
          const uint64_t key = rally_key(st, act_r, act_l);
          const int at = adv_ld(&adv->at);
          if (at < 0 || at > timeout) {
            if (kSolo ? hl == 0 : lig == 0) {
              adv_st(&adv->key, key);
              adv_st(&adv->at, timeout);
              adv_st(&adv->span, kRallySpan0);
            }
          } else if (adv_ld(&adv->key) == key) {
            const int rest = p.timeout_thresh + 1 - timeout;
            frames += rest;  // the counter at TIMEOUT_THRESH + 1: the end test below fires
            timeout = p.timeout_thresh + 1;
            if (kSolo ? lead : lig == 0) adv->skipped += rest;
          } else if (timeout - at >= adv_ld(&adv->span)) {
            if (kSolo ? hl == 0 : lig == 0) {
              adv_st(&adv->key, key);
              adv_st(&adv->at, timeout);
              adv_st(&adv->span, 2 * adv_ld(&adv->span));
            }
          }
        }
      }
      if (st.s1 >= p.win_score || st.s2 >= p.win_score || st.done() || timeout > p.timeout_thresh) {
        if constexpr (kSolo) {  // (counted by the game's first lane alone: half-group leaders report)
          c_steps += lead ? frames : 0;
          c_games += lead ? 1 : 0;
        } else {
          c_steps += frames;
          c_games += 1;
        }
        if (kSolo ? lead : lig == 0) finish_game(p, w, st, frames, total);
        have = false;
      }
    }
  }
  if (p.counters) {
    if ((kSolo ? hl == 0 : lig == 0) && c_games) {
      if constexpr (kAdvance) {
        // [0] the frames stepped one at a time: the episodes' frames minus those
        // of periodic rallies jumped [8] and of serve delays advanced [12]
        const uint32_t skipped = adv->skipped, hidden = adv->hidden;
        atomicAdd((unsigned long long *)&p.counters[0], (unsigned long long)(c_steps - skipped - hidden));
        if (skipped) atomicAdd((unsigned long long *)&p.counters[8], (unsigned long long)skipped);
        if (hidden) atomicAdd((unsigned long long *)&p.counters[12], (unsigned long long)hidden);
      } else {
        atomicAdd((unsigned long long *)&p.counters[0], (unsigned long long)c_steps);
      }
      atomicAdd((unsigned long long *)&p.counters[3], (unsigned long long)c_games);
    }
    if (hl == 0 && c_fwd) {  // one lane per half-group: its network's forwards
      atomicAdd((unsigned long long *)&p.counters[1], (unsigned long long)c_fwd);
      // [2] the f64 forwards, [4] the frames the f32 certificate left undecided
      if constexpr (P::kF64Stage == 1) {
        if (c_f64) {
          atomicAdd((unsigned long long *)&p.counters[2], (unsigned long long)c_f64);
          atomicAdd((unsigned long long *)&p.counters[4], (unsigned long long)c_f64);
        }
      } else {
        if (c_fail) atomicAdd((unsigned long long *)&p.counters[4], (unsigned long long)c_fail);
        if (c_f64) atomicAdd((unsigned long long *)&p.counters[2], (unsigned long long)c_f64);
      }
    }
  }
}

// pg_*_decide: the decision code of a cert_game frame, one half-group per
// pass; a block's pass decides rows [base, base + 256 / LN).  The grid-stride
// loop over base is the kernels' own: with the loop in here, inlining moves a
// kernel's exit block and with it the instruction counts.
// (Params: CertDecideParams, or a family's extension of it)
template <class P, class Params>
__device__ __forceinline__ void cert_decide_pass(const Params &p, long base) {
  using WT = typename P::WT;
  constexpr int LN = P::LN, O = P::O, HPB = 256 / LN;
  __shared__ typename P::Lds lds_all[HPB];
  const int hg = threadIdx.x / LN, hl = threadIdx.x & (LN - 1);
  const WT *genomes = (const WT *)p.genomes;
  const auto dims = cert_dims<P>::of(p);
  const long t = base + hg;
  if (t < p.n) {
    const WT *g = genomes + (long)(p.gidx ? p.gidx[t] : t) * p.gstride;
    typename P::Net net = {};  // (P::load updates it in place)
    P::load(net, g, dims, lds_all[hg], hl);
    int k[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = p.k[t * 6 + i];
    float z[O];
    int stage;
    const int idx = P::decide(net, g, dims, k, true, lds_all[hg], hl, z, stage);
    if (hl == 0) {
      p.index[t] = idx;
      if (p.stage) p.stage[t] = stage;
      if (p.bound) p.bound[t] = net.e;
      if (p.z32) {
#pragma unroll
        for (int o = 0; o < O; ++o) p.z32[t * O + o] = z[o];
      }
    }
  }
}

// ------------------------------------------------------------ host side ----
// Launch KERNEL<LN, UNITS..., O, WT> for the runtime O in 2..4 and genome type;
// UNITS: the family's per-lane unit counts, in parentheses.
#define PG_CERT_UNITS(...) __VA_ARGS__
#define PG_CERT_DISPATCH(KERNEL, LN, UNITS, O, f64, grid, s, p)                                                    \
  do {                                                                                                             \
    if (O == 2) {                                                                                                  \
      if (f64) hipLaunchKernelGGL((KERNEL<LN, PG_CERT_UNITS UNITS, 2, double>), dim3(grid), dim3(256), 0, s, p);  \
      else hipLaunchKernelGGL((KERNEL<LN, PG_CERT_UNITS UNITS, 2, float>), dim3(grid), dim3(256), 0, s, p);       \
    } else if (O == 3) {                                                                                           \
      if (f64) hipLaunchKernelGGL((KERNEL<LN, PG_CERT_UNITS UNITS, 3, double>), dim3(grid), dim3(256), 0, s, p);  \
      else hipLaunchKernelGGL((KERNEL<LN, PG_CERT_UNITS UNITS, 3, float>), dim3(grid), dim3(256), 0, s, p);       \
    } else {                                                                                                       \
      if (f64) hipLaunchKernelGGL((KERNEL<LN, PG_CERT_UNITS UNITS, 4, double>), dim3(grid), dim3(256), 0, s, p);  \
      else hipLaunchKernelGGL((KERNEL<LN, PG_CERT_UNITS UNITS, 4, float>), dim3(grid), dim3(256), 0, s, p);       \
    }                                                                                                              \
  } while (0)

// blocks of a game launch: a group of 2 LN lanes per game, at most two blocks per CU
inline int cert_game_grid(const EvalParams &p, int LN) {
  const int GPB = 256 / (2 * LN);
  const int want = (p.total + GPB - 1) / GPB;
  const int cap = num_cus() * 2;
  return want < cap ? want : cap;
}

// blocks of a decide launch: a half-group of LN lanes per pass
inline int cert_decide_grid(int n, int LN) {
  const int HPB = 256 / LN;
  const int want = (n + HPB - 1) / HPB;
  const int cap = num_cus() * 8;
  return want < cap ? want : cap;
}

inline CertDecideParams cert_decide_params(const pg_relu_decide_args *a, int H1, int H2) {
  CertDecideParams p;
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
  return p;
}

}  // namespace pg
