// pg_general.hip -- the f64 path of libpong_ga.so: any NETWORK_SHAPE, in numpy's arithmetic.
//
//   k_general<WT>         evaluate() (main.py:28-66) for any NETWORK_SHAPE: one
//                         wave per game, f64 numpy_nn arithmetic in numpy's
//                         order with activations staged in LDS (sigmoid or
//                         ReLU).  launch_general is pg_eval_population's way in.
//   k_forward_general<WT> NeuralNetwork.run batched, the same arithmetic
//                         (pg_forward; its certified path for the split kernel's
//                         shapes, k_forward_resident, is in pong_ga.hip).
// Compiled with pong_ga.hip's scheduler flag (pong_amd/build.py SOURCE_FLAGS),
// under which these kernels were tuned and measured.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/pong_ga.h"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_f64math.h"
#include "pg_cascade.hpp"

namespace pg {

// ===================================================== general (f64) path ==
// One forward pass of NeuralNetwork.run (numpy_nn.py:120-137) by one wave, in
// f64 with numpy's operation order per unit (np.dot's BLAS order over
// [inputs..., 1], blas_dot); cur holds the input vector (with the trailing 1 if
// bias).  Returns the argmax index; cur/nxt are LDS buffers of max_width + 1
// doubles.  With z_all/h_all (pg_forward's diagnostics) every layer's
// pre-activations and activations are stored there as well.  act: pg_activation
// (numpy_nn.py:26) -- the sigmoid, or ReLU np.maximum(0.0, z) (numpy_nn.py:6-9:
// NaN propagates, every z <= 0 gives 0), applied to every layer.
template <typename WT>
__device__ int forward_f64_wave(const WT *__restrict__ w, const int *nodes, int n_nodes, int b,
                                double *&cur, double *&nxt, int lane, int act, double *z_all = nullptr,
                                double *h_all = nullptr) {
  long off = 0;
  int zo = 0;
  for (int l = 0; l + 1 < n_nodes; ++l) {
    const int nin = nodes[l], nout = nodes[l + 1], cols = nin + b;
    for (int j = lane; j < nout; j += 64) {
      const WT *row = w + off + (long)j * cols;
      const double *cv = cur;
      const double z = blas_dot([&](int i) { return (double)row[i]; }, [&](int i) { return cv[i]; }, cols,
                                blas_kind(j, nout));
      nxt[j] = act == PG_ACT_RELU ? (!(z <= 0.0) ? z : 0.0) : sigmoid_f64(z);
      if (z_all) z_all[zo + j] = z;
      if (h_all) h_all[zo + j] = nxt[j];
    }
    zo += nout;
    if (b && lane == 0) nxt[nout] = 1.0;
    wave_lds_sync();
    off += (long)cols * nout;
    double *t = cur;
    cur = nxt;
    nxt = t;
  }
  const int n_out = nodes[n_nodes - 1];
  int best = 0;  // np.argmax: the first NaN if any, else the first maximum
  for (int j = 1; j < n_out && !__builtin_isnan(cur[best]); ++j)
    if (__builtin_isnan(cur[j]) || cur[j] > cur[best]) best = j;
  return best;
}

template <typename WT>
__global__ __launch_bounds__(64) void k_general(EvalParams p) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int W = p.max_width + 1;
  double *bufA = lds, *bufB = lds + W;
  const WT *genomes = (const WT *)p.genomes;
  const WT *opponents = (const WT *)p.opponents;
  uint64_t c_steps = 0, c_fwd = 0, c_games = 0;
  const int games_total = active_total(p);
  for (;;) {
    int w = 0;
    if (lane == 0) w = (int)atomicAdd(p.work, 1u);
    w = __builtin_amdgcn_readfirstlane(w);
    if (w >= games_total) break;
    const int i = w / p.n_games, g = w % p.n_games;
    const int kind = p.kind[w];
    const WT *gr = genomes + (long)genome_row(p, i) * p.gstride;
    const WT *gl = (kind == kOppNN) ? opponents + (long)p.opp[w] * p.ostride : gr;
    Pong st;
    st.reset(game_seed(p.seed, g), kind == kOppRomCpu);
    int act_r = 0, act_l = 0, timeout = 0, total = 0, frames = 0;
    for (;;) {
      const int s1b = st.s1, s2b = st.s2;
      const int pvis = st.vis, pbx2 = 2 * st.bx + kBallW - 1, pby2 = 2 * st.by + kBallH - 1;
      st.step(act_r, act_l);
      frames += 1;
      const int vis = st.vis;
      const int bx2 = 2 * st.bx + kBallW - 1, by2 = 2 * st.by + kBallH - 1;
      const int lc2 = paddle_c2(st.lpy), rc2 = paddle_c2(st.rpy);
      int left = 0, right = 0;
      if (vis) {  // get_actions main.py:143-150
        const int lbx2 = pvis ? pbx2 : bx2, lby2 = pvis ? pby2 : by2;
        if (kind == kOppNN) {
          double *cur = bufA, *nxt = bufB;
          if (lane == 0) {
            cur[0] = feat64_flip(bx2); cur[1] = feat64(by2); cur[2] = feat64_flip(lbx2);
            cur[3] = feat64(lby2); cur[4] = feat64(lc2); cur[5] = feat64(rc2);
            if (p.bias) cur[6] = 1.0;
          }
          wave_lds_sync();
          left = index_to_code(forward_f64_wave(gl, p.nodes, p.n_nodes, p.bias, cur, nxt, lane, p.activation));
          wave_lds_sync();
          c_fwd += 1;
        } else if (kind == kOppScore) {
          left = (st.s1 <= st.s2) ? hardcoded(by2, lc2) : 0;
        } else {
          left = hardcoded(by2, lc2);
        }
        double *cur = bufA, *nxt = bufB;
        if (lane == 0) {
          cur[0] = feat64(bx2); cur[1] = feat64(by2); cur[2] = feat64(lbx2);
          cur[3] = feat64(lby2); cur[4] = feat64(rc2); cur[5] = feat64(lc2);
          if (p.bias) cur[6] = 1.0;
        }
        wave_lds_sync();
        right = index_to_code(forward_f64_wave(gr, p.nodes, p.n_nodes, p.bias, cur, nxt, lane, p.activation));
        wave_lds_sync();
        c_fwd += 1;
      }
      act_l = clamp_action(lc2, left);
      act_r = clamp_action(rc2, right);
      if (p.trace && w < p.trace_games && frames <= p.trace_cap && lane == 0)
        p.trace[(long)w * p.trace_cap + frames - 1] = (uint8_t)(act_r | (act_l << 2) | (vis << 4));
      if (frames > 1) {  // calculate_timeout_and_frames main.py:128-135
        if (st.s1 == s1b && st.s2 == s2b) {
          timeout += 1;
        } else {
          total += timeout;
          timeout = 0;
        }
      }
      if (st.s1 >= p.win_score || st.s2 >= p.win_score || st.done() || timeout > p.timeout_thresh) break;
    }
    c_steps += frames;
    c_games += 1;
    if (lane == 0) finish_game(p, w, st, frames, total);
  }
  if (p.counters && lane == 0 && c_games) {
    atomicAdd((unsigned long long *)&p.counters[0], (unsigned long long)c_steps);
    atomicAdd((unsigned long long *)&p.counters[1], (unsigned long long)c_fwd);
    atomicAdd((unsigned long long *)&p.counters[3], (unsigned long long)c_games);
  }
}

// both LDS buffers of max_width + 1 doubles
static int32_t general_lds_bytes(int max_width, size_t *lds) {
  *lds = 2 * (size_t)(max_width + 1) * sizeof(double);
  if (*lds > 160 * 1024) return fail(PG_ERR_UNSUPPORTED, "layer width %d too large for LDS", max_width);
  return PG_OK;
}

int32_t launch_general(const EvalParams &p, int dtype, hipStream_t s) {
  size_t lds;
  const int32_t rc = general_lds_bytes(p.max_width, &lds);
  if (rc != PG_OK) return rc;
  const int cap = num_cus() * 16;
  const int grid = p.total < cap ? p.total : cap;
  if (dtype == PG_F64)
    hipLaunchKernelGGL(k_general<double>, dim3(grid), dim3(64), lds, s, p);
  else
    hipLaunchKernelGGL(k_general<float>, dim3(grid), dim3(64), lds, s, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

// ============================================================ forward ====
template <typename WT>
__global__ __launch_bounds__(64) void k_forward_general(FwdParams p) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x;
  const int W = p.max_width + 1;
  const int n_in = p.nodes[0], n_out = p.nodes[p.n_nodes - 1];
  for (int t = blockIdx.x; t < p.n; t += gridDim.x) {
    const long row = p.gidx ? p.gidx[t] : t;
    const WT *gw = (const WT *)p.genomes + row * p.gstride;
    double *cur = lds, *nxt = lds + W;
    for (int i = lane; i < n_in; i += 64) cur[i] = p.x[(long)t * n_in + i];
    if (p.bias && lane == 0) cur[n_in] = 1.0;
    wave_lds_sync();
    const int idx = forward_f64_wave(gw, p.nodes, p.n_nodes, p.bias, cur, nxt, lane, p.activation,
                                     p.z_all ? p.z_all + (long)t * p.n_units : nullptr,
                                     p.h_all ? p.h_all + (long)t * p.n_units : nullptr);
    if (lane == 0) p.index[t] = idx;
    if (p.act)
      for (int j = lane; j < n_out; j += 64) p.act[(long)t * n_out + j] = cur[j];
    wave_lds_sync();
  }
}

}  // namespace pg

using namespace pg;

extern "C" {

int32_t pg_forward(const pg_forward_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  int32_t rc = check_net(a->net, false);
  if (rc != PG_OK) return rc;
  if (a->n < 0) return fail(PG_ERR_INVALID, "n=%d < 0", a->n);
  if (a->n == 0) return PG_OK;
  const int G = gene_count(a->net);
  if (!a->genomes || a->genome_stride < G || !a->x || !a->index)
    return fail(PG_ERR_INVALID, "genomes/x/index NULL or genome_stride < gene count %d", G);
  hipStream_t s = (hipStream_t)stream;
  FwdParams p;
  memset(&p, 0, sizeof(p));
  p.genomes = a->genomes;
  p.gidx = a->genome_index;
  p.x = a->x;
  p.index = a->index;
  p.act = a->act;
  p.z_all = a->z_all;
  p.h_all = a->h_all;
  p.counters = a->counters;
  p.gstride = a->genome_stride;
  p.n = a->n;
  set_net(p, a->net);
  for (int i = 1; i < a->net.n_nodes; ++i) p.n_units += a->net.nodes[i];
  if ((a->z_all || a->h_all) && a->precision != PG_PREC_F64)
    return fail(PG_ERR_INVALID, "z_all/h_all need precision PG_PREC_F64");
  // (ReLU networks: always the f64 forward below, whatever the precision)
  if (a->precision == PG_PREC_CERTIFIED && resident_shape_ok(a->net) && a->net.activation == PG_ACT_SIGMOID)
    return launch_forward_resident(p, a->net.dtype, s);
  if (a->precision != PG_PREC_CERTIFIED && a->precision != PG_PREC_F64)
    return fail(PG_ERR_INVALID, "precision=%d", a->precision);
  size_t lds;
  rc = general_lds_bytes(p.max_width, &lds);
  if (rc != PG_OK) return rc;
  const int cap = num_cus() * 16;
  const int grid = a->n < cap ? a->n : cap;
  if (a->net.dtype == PG_F64)
    hipLaunchKernelGGL(k_forward_general<double>, dim3(grid), dim3(64), lds, s, p);
  else
    hipLaunchKernelGGL(k_forward_general<float>, dim3(grid), dim3(64), lds, s, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

}  // extern "C"
