// pong_ga.hip -- the evaluation's C-ABI of libpong_ga.so (MI355X, gfx950):
// pg_eval_population, pg_decide and pg_wide_decide, the library's errors and
// version calls, k_fitness, and the bench instance of k_service.
//
// The hot path: evaluate() (main.py:28-66) for a whole population in one
// launch.  Every game (perform_episode, main.py:69-112) runs to termination
// inside the kernel: the Pong state and both networks' weights stay in
// registers for the whole episode, so HBM is touched once per game (weights
// in, results out) instead of once per frame.  See DESIGN.md.
//
//   k_service<L,U,O,WT>   [6, H<=256, O] networks (pg_service.hpp): an aligned
//                         group of L lanes plays one game, half a group per
//                         paddle's network in VGPRs; f32 math with a certified
//                         f64 argmax, the failures re-decided in f64 by the
//                         wave itself (8-lane groups) or a service wave.  The
//                         bench layout's instance is here, on this unit's
//                         scheduler flag; the others in pg_service_more.hip.
//   k_general<WT>         any NETWORK_SHAPE, one wave per game, f64 numpy_nn
//                         arithmetic with activations staged in LDS (sigmoid or
//                         ReLU; pg_general.hip).
//   k_wide<NG,WT,ACT>     [6, H1<=512, H2<=512, O] networks, weights streamed (pg_wide.hip).
//   the certified f32 families' kernels: one unit each, reached through the
//                         family table below (family_of; pg_eval.hpp lists the units).
//   k_fitness             sum(all_rewards) / GAMES_TO_PLAY in the reference order.
//   k_forward_resident, k_physics_*   pg_forward's certified path and the SoA
//                         Pong stepper (pg_physics_*): here because k_service's
//                         generated code depends on them (see below).
// Elsewhere: pg_forward and k_forward_general (pg_general.hip),
// pg_ga_*, pg_gather_rows, pg_row_hash (k_select, k_vary, ...: pg_ga.hip), and the
// hall-of-fame scans on the host (pg_hof_update, pg_hof_update_packed: pg_hof_scan.cpp).
// pg_eval.hpp maps every unit.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/pong_ga.h"
#include "pg_device.hpp"
#include "pg_eval.hpp"
#include "pg_f64math.h"
#include "pg_cascade.hpp"
#include "pg_service.hpp"

#ifndef PG_VERSION_STRING
#define PG_VERSION_STRING "pong_ga 0.1.0 (gfx950)"
#endif

namespace pg {

// --------------------------------------------------------------- errors ----
static thread_local std::string g_last_error;

int32_t fail(int32_t code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}


// ------------------------------------------------------------- fitness ----
// evaluate()'s return: sum(all_rewards) (left to right from int 0) / float(GAMES_TO_PLAY).
__global__ void k_fitness(const double *rewards, const int32_t *status_game, int n, const int32_t *n_active,
                          int games, double *fitness, int32_t *status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (n_active && i >= *n_active)) return;  // rows not played keep their contents
  double s = 0.0;
  int err = 0;
  for (int g = 0; g < games; ++g) {
    s = __dadd_rn(s, rewards[(long)i * games + g]);
    err |= status_game[(long)i * games + g];
  }
  fitness[i] = s / (double)games;
  if (status) status[i] = err;
}

// ------------------------------------- kernels that k_service's code needs ----
// k_forward_resident (pg_forward's certified path; the entry point is in
// pg_general.hip) and the physics stepper are here for the compiler, not for the
// reader: they share device functions with k_service (forward_f64_group<64, 1,
// 3, WT>, the serve and step helpers of pg_device.hpp), and what the compiler
// makes of those before it inlines them depends on all their callers in the
// unit.  Without either of the two, every k_service instance compiles to other
// code (4 000 of 4 750 lines, other spill counts) than the one that was
// tuned and measured; tools/isa_compare.py shows it.  All 66 k_forward_resident
// instances stay together for the same reason.
template <int L, int U, int O, typename WT>
__global__ __launch_bounds__(256) void k_forward_resident(FwdParams p) {
  constexpr int GPB = 256 / L;
  const int H = p.nodes[1], b = p.bias;
  extern __shared__ double lds_all[];
  const int lig = threadIdx.x & (L - 1);
  const int grp = threadIdx.x / L;
  double *lds = lds_all + grp * f64_lds_doubles(H, O);
  uint32_t slow = 0;
  for (int t = blockIdx.x * GPB + grp; t < p.n; t += gridDim.x * GPB) {
    const long row = p.gidx ? p.gidx[t] : t;
    const WT *gw = (const WT *)p.genomes + row * p.gstride;
    Net<U, O> net;
    load_net<L, U, O, WT>(net, gw, H, b, lig);
    float x[6], acc[O], z[O];
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = (float)p.x[(long)t * 6 + i];
    partial_f32<U, O>(net, x, acc);
#pragma unroll
    for (int o = 0; o < O; ++o) z[o] = group_sum<L>(acc[o]) + net.c[o];
    int idx = certify<O>(z, net.e);
    if (idx >= 0 && p.act) {
      // activations are reported within 2e-6: |S(z) - S(z_hat)| <= e * S'(max(|z_hat| - e, 0))
      bool tight = true;
#pragma unroll
      for (int o = 0; o < O; ++o) {
        const float tt = fmaxf(fabsf(z[o]) - net.e, 0.f);
        const float sp = __expf(-tt) / ((1.f + __expf(-tt)) * (1.f + __expf(-tt)));
        tight = tight && (net.e * sp <= 2e-6f);
      }
      if (!tight) idx = -1;
    }
    if (idx < 0) {
      // arbitrary f64 inputs here: the group's f64 pass on them directly
      double xd[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) xd[i] = p.x[(long)t * 6 + i];
      idx = forward_f64_group<L, U, O, WT>(gw, H, b, (const double *)xd, lds, lig);
      if (p.act && lig < O) p.act[(long)t * O + lig] = lds[f64_out_offset(H, O) + lig];
      wave_lds_sync();
      slow += (lig == 0);
    } else if (p.act && lig < O) {
      float zz = z[0];
#pragma unroll
      for (int o = 1; o < O; ++o) zz = (lig == o) ? z[o] : zz;
      p.act[(long)t * O + lig] = sigmoid_f64((double)zz);
    }
    if (lig == 0) p.index[t] = idx;
  }
  if (p.counters && slow) atomicAdd((unsigned long long *)&p.counters[2], (unsigned long long)slow);
}

// ============================================================ physics ====
__global__ void k_physics_reset(int32_t *s, int n, const uint64_t *seeds, const int32_t *one_player) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Pong st;
  st.reset(seeds ? seeds[i] : 0ull, one_player ? one_player[i] : 0);
  const int f[PG_STATE_FIELDS] = {st.bx, st.by, st.vx, st.vy, st.vis, st.timer, st.dir, st.hits,
                                  st.point, st.lpy, st.rpy, st.s1, st.s2, st.one_player,
                                  (int)(uint32_t)st.seed, (int)(uint32_t)(st.seed >> 32)};
#pragma unroll
  for (int k = 0; k < PG_STATE_FIELDS; ++k) s[(long)k * n + i] = f[k];
}

__global__ void k_physics_step(int32_t *s, int n, const uint8_t *actions) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Pong st;
  st.bx = s[0L * n + i]; st.by = s[1L * n + i]; st.vx = s[2L * n + i]; st.vy = s[3L * n + i];
  st.vis = s[4L * n + i]; st.timer = s[5L * n + i]; st.dir = s[6L * n + i]; st.hits = s[7L * n + i];
  st.point = s[8L * n + i]; st.lpy = s[9L * n + i]; st.rpy = s[10L * n + i];
  st.s1 = s[11L * n + i]; st.s2 = s[12L * n + i]; st.one_player = s[13L * n + i];
  st.seed = (uint64_t)(uint32_t)s[14L * n + i] | ((uint64_t)(uint32_t)s[15L * n + i] << 32);
  const int a = actions[i];
  st.step(a & 3, (a >> 2) & 3);
  s[0L * n + i] = st.bx; s[1L * n + i] = st.by; s[2L * n + i] = st.vx; s[3L * n + i] = st.vy;
  s[4L * n + i] = st.vis; s[5L * n + i] = st.timer; s[6L * n + i] = st.dir; s[7L * n + i] = st.hits;
  s[8L * n + i] = st.point; s[9L * n + i] = st.lpy; s[10L * n + i] = st.rpy;
  s[11L * n + i] = st.s1; s[12L * n + i] = st.s2;
}

// ====================================================== host dispatch ====
int gene_count(const pg_net &n) {
  const int b = n.bias ? 1 : 0;
  long t = 0;
  for (int i = 0; i + 1 < n.n_nodes; ++i) t += (long)(n.nodes[i] + b) * n.nodes[i + 1];
  return t > 0x7fffffff ? -1 : (int)t;
}

int32_t check_net(const pg_net &n, bool game) {
  if (n.n_nodes < 2 || n.n_nodes > PG_MAX_NODES)
    return fail(PG_ERR_INVALID, "net.n_nodes=%d must be in [2, %d]", n.n_nodes, PG_MAX_NODES);
  for (int i = 0; i < n.n_nodes; ++i)
    if (n.nodes[i] < 1 || n.nodes[i] > 65536)
      return fail(PG_ERR_INVALID, "net.nodes[%d]=%d out of range", i, n.nodes[i]);
  if (game && n.nodes[0] != 6)
    return fail(PG_ERR_INVALID, "the game feeds 6 inputs (utils.py:146-152); nodes[0]=%d", n.nodes[0]);
  if (n.dtype != PG_F32 && n.dtype != PG_F64) return fail(PG_ERR_INVALID, "net.dtype=%d", n.dtype);
  if (n.activation != PG_ACT_SIGMOID && n.activation != PG_ACT_RELU)
    return fail(PG_ERR_INVALID, "net.activation=%d (pg_activation: 0 sigmoid, 1 relu)", n.activation);
  if (gene_count(n) < 0) return fail(PG_ERR_INVALID, "network too large");
  return PG_OK;
}

int max_width(const pg_net &n) {
  int m = 0;
  for (int i = 0; i < n.n_nodes; ++i) m = n.nodes[i] > m ? n.nodes[i] : m;
  return m;
}

static int g_num_cus = 0;
int num_cus() {
  if (g_num_cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      g_num_cus = prop.multiProcessorCount;
    if (g_num_cus <= 0) g_num_cus = 256;
  }
  return g_num_cus;
}

// split layout for hidden width H: L lanes per game (L/2 per network).  Fewer
// lanes per game means more games per wave, so the replicated scalar work of
// a frame (physics, bookkeeping, the certificate) is shared by fewer lanes;
// L = 8 holds up to 16 units per lane (H <= 64) in 256 VGPRs (measured
// fastest for [6,64,3]: profiles/r01/sweep_lanes.log).
static int choose_split_lanes(int H) {
  if (H <= 64) return 8;
  if (H <= 128) return 32;
  return 64;
}

template <typename WT>
static int32_t launch_service_any(const EvalParams &p, int L, int O, bool solo, hipStream_t s) {
  const int H = p.nodes[1];
  // the bench layout here (H in (32, 64] with L = 8: U = 16 is the smallest
  // that holds it); every other (L, U) in pg_service_more.hip
#ifdef PG_DEV_MIN
  const bool here = L == 8 && H <= 64;
#else
  const bool here = L == 8 && H > 32 && H <= 64;
#endif
  // (only O = 3 here: the iterative scheduler's register allocator crashes
  // ROCm 7.2's compiler on the O = 2 / 4 instances, built in pg_service_more.hip)
  if (here && O == 3) return launch_service<8, 16, 3, WT, true>(p, s, solo);
#ifdef PG_DEV_MIN  // variant builds for experiments (tools/build_variant.sh): the bench layout only
  return fail(PG_ERR_UNSUPPORTED, "no service kernel for L=%d H=%d O=%d", L, H, O);
#else
  return launch_service_more(p, L, O, sizeof(WT) == 8, s, solo);
#endif
}

bool resident_shape_ok(const pg_net &n) {
  return n.n_nodes == 3 && n.nodes[0] == 6 && n.nodes[1] <= 256 && n.nodes[2] >= 2 && n.nodes[2] <= 4;
}

int32_t split_scope(const pg_eval_args &a) {
  if (a.net.activation != PG_ACT_SIGMOID)
    return fail(PG_ERR_UNSUPPORTED, "activation relu: the split kernel evaluates sigmoid networks only (use RELU, RELU2, RELU_WIDE or GENERAL)");
  if (!resident_shape_ok(a.net)) return fail(PG_ERR_UNSUPPORTED, "split kernel needs NETWORK_SHAPE [6, H<=256, 2..4]");
  if (a.precision != PG_PREC_CERTIFIED) return fail(PG_ERR_UNSUPPORTED, "split kernel is the certified-precision path");
  return PG_OK;
}

// PG_KERNEL_SOLO on a launch in split_scope (through PG_KERNEL_AUTO): the launches k_service's solo
// instances play (pg_service_solo.hip) -- the layout whose game waves decide their own certificate
// failures (L = 8, U = 16), whole untraced episodes without a hard-case log, and an (O, genome type)
// that has an instance.  Every other split launch runs the base instance, the bit changing nothing.
bool split_solo_scope(const pg_eval_args &a) {
  const int H = a.net.nodes[1];
  return H >= 33 && H <= 64 && (a.group_lanes == 0 || a.group_lanes == 8) && a.horizon == 0 && !a.trace && !a.hard_log &&
         service_solo_routed(a.net.nodes[2], a.net.dtype == PG_F64);
}

// Resident kernel table: (L, U) chosen from the hidden width H.
struct ResidentChoice {
  int L, U;
};
static ResidentChoice choose_resident(int H, int requested_L) {
  static const ResidentChoice table[] = {{4, 1}, {8, 1}, {16, 1}, {32, 1}, {16, 4}, {32, 4}, {64, 4}};
  static const ResidentChoice all[] = {{4, 1}, {8, 1}, {16, 1}, {32, 1}, {64, 1}, {16, 2}, {32, 2},
                                       {64, 2}, {16, 4}, {32, 4}, {64, 4}};
  if (requested_L > 0) {
    for (const auto &c : all)
      if (c.L == requested_L && c.L * c.U >= H) return c;
    return {0, 0};
  }
  for (const auto &c : table)
    if (c.L * c.U >= H) return c;
  return {0, 0};
}

template <int L, int U, int O, typename WT>
static int32_t launch_fwd_resident(const FwdParams &p, hipStream_t s) {
  constexpr int GPB = 256 / L;
  const size_t lds = (size_t)GPB * f64_lds_doubles(p.nodes[1], O) * sizeof(double);
  const int want = (p.n + GPB - 1) / GPB;
  const int cap = num_cus() * 8;
  const int grid = want < cap ? want : cap;
  if (grid <= 0) return PG_OK;
  hipLaunchKernelGGL((k_forward_resident<L, U, O, WT>), dim3(grid), dim3(256), lds, s, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

template <typename WT>
static int32_t launch_fwd_resident_any(const FwdParams &p, ResidentChoice c, int O, hipStream_t s) {
#define PG_FRES(LL, UU)                                                  \
  if (c.L == LL && c.U == UU) {                                          \
    if (O == 2) return launch_fwd_resident<LL, UU, 2, WT>(p, s);         \
    if (O == 3) return launch_fwd_resident<LL, UU, 3, WT>(p, s);         \
    if (O == 4) return launch_fwd_resident<LL, UU, 4, WT>(p, s);         \
  }
#ifndef PG_DEV_MIN
  PG_FRES(4, 1) PG_FRES(8, 1) PG_FRES(16, 1) PG_FRES(32, 1) PG_FRES(64, 1)
  PG_FRES(16, 2) PG_FRES(32, 2) PG_FRES(64, 2) PG_FRES(16, 4) PG_FRES(32, 4) PG_FRES(64, 4)
#endif
#undef PG_FRES
  return fail(PG_ERR_UNSUPPORTED, "no resident forward kernel for L=%d U=%d O=%d", c.L, c.U, O);
}

int32_t launch_forward_resident(const FwdParams &p, int dtype, hipStream_t s) {
  const ResidentChoice c = choose_resident(p.nodes[1], 0);
  return dtype == PG_F64 ? launch_fwd_resident_any<double>(p, c, p.nodes[2], s)
                         : launch_fwd_resident_any<float>(p, c, p.nodes[2], s);
}

}  // namespace pg

using namespace pg;

// ================================================================ C-ABI ===
extern "C" {

const char *pg_version(void) { return PG_VERSION_STRING; }
int32_t pg_abi_version(void) { return PG_ABI_VERSION; }
int32_t pg_build_flags(void) { return 0; }
const char *pg_last_error(void) { return g_last_error.c_str(); }

int32_t pg_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(PG_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

// [0, 256): dynamic game counters (PG_KERNEL_SOLO: two); then one int32 per game (zero-division
// flags); for the staged kernel, then its prepared lane records
static size_t eval_base_workspace(const pg_eval_args *a) {
  const size_t games = a ? (size_t)(a->n_genomes > 0 ? a->n_genomes : 0) * (size_t)(a->n_games > 0 ? a->n_games : 0) : 0;
  return 256 + align256(games * sizeof(int32_t));
}

// the kernel pg_eval_population runs for a (PG_KERNEL_AUTO resolved)
// (the low byte of pg_eval_args.kernel: PG_KERNEL_ADVANCE and PG_KERNEL_SOLO change no choice and no
// workspace; which instance of the kernel they select, if any: modifiers_in_effect)
static int resolve_kernel(const pg_eval_args *a) {
  const int named = a->kernel & 0xff;
  if (named != PG_KERNEL_AUTO) return named;
  if (a->net.activation == PG_ACT_RELU) {  // k_relu's or k_relu2's scope, else the general kernel (never SPLIT or WIDE)
    if (a->precision != PG_PREC_CERTIFIED) return PG_KERNEL_GENERAL;
    return relu_shape_ok(a->net) ? PG_KERNEL_RELU : (relu2_shape_ok(a->net) ? PG_KERNEL_RELU2 : PG_KERNEL_GENERAL);
  }
  if (resident_shape_ok(a->net) && a->precision == PG_PREC_CERTIFIED) return PG_KERNEL_SPLIT;
  if (wide_shape_ok(a->net, a->n_games) && (a->net.nodes[1] >= 64 || a->net.nodes[2] >= 64)) return PG_KERNEL_WIDE;
  return PG_KERNEL_GENERAL;
}

// the split kernel's lane records (k_prep_records), after the base workspace
static size_t split_records_bytes(const pg_eval_args *a) {
  if (!resident_shape_ok(a->net) || a->n_genomes <= 0) return 0;
  const int H = a->net.nodes[1];
  const int L = a->group_lanes > 0 ? a->group_lanes : choose_split_lanes(H);
  const int U = (L == 8 && H <= 64) ? 16 : service_units(L, H);  // >= what any build instantiates
  if (U <= 0) return 0;
  return align256(service_records_bytes(a->n_genomes, a->opponents ? a->n_opponents : 0, L, U, a->net.nodes[2]));
}

// The certified f32 families (pg_eval.hpp's FamilyDesc): the one list of them here.  A new family is a
// row; whether it takes the modifier bits, when its scope is asked and how it is launched are its own.
// family_of(kernel): kernel's family, or NULL for a pg_kernel that is no certified f32 family's.
static const FamilyDesc *family_of(int kernel) {
  static const FamilyDesc kFamilies[] = {relu_family(),       relu2_family(), sig2_family(), relu2_block_family(),
                                         sig2_block_family(), relu3_family(), sig3_family()};
  for (const FamilyDesc &f : kFamilies)
    if (f.kernel == kernel) return &f;
  return nullptr;
}

// the modifier bits that take effect on kernel (resolve_kernel's) for a launch in its scope:
// the closed-form advance on the untraced launches of the families that take it, solo games on theirs and
// on SPLIT's in split_solo_scope (the bit reaches SPLIT through PG_KERNEL_AUTO only: check_modifier_bits)
static int modifiers_in_effect(int kernel, const pg_eval_args &a, bool advance, bool solo) {
  const FamilyDesc *f = family_of(kernel);
  const bool cert = f && f->modifiers;
  int bits = 0;
  if (advance && cert && !a.trace) bits |= PG_KERNEL_ADVANCE;
  if (solo && (cert || (kernel == PG_KERNEL_SPLIT && split_solo_scope(a)))) bits |= PG_KERNEL_SOLO;
  return bits;
}

// ABI 10: the caller's struct must be this header's (pg_eval_args.struct_size)
static int32_t check_struct_size(const pg_eval_args *a) {
  if (a->struct_size != sizeof(pg_eval_args))
    return fail(PG_ERR_INVALID, "pg_eval_args.struct_size=%u, this library's struct is %zu bytes (ABI %d)",
                a->struct_size, sizeof(pg_eval_args), PG_ABI_VERSION);
  return PG_OK;
}

size_t pg_eval_workspace_bytes(const pg_eval_args *a) {
  if (a && check_struct_size(a) != PG_OK) return 0;
  size_t n = eval_base_workspace(a);
  if (!a) return n;
  const int kernel = resolve_kernel(a);
  if (kernel == PG_KERNEL_SPLIT) n += split_records_bytes(a);
  if ((kernel == PG_KERNEL_WIDE || kernel == PG_KERNEL_RELU_WIDE) && wide_shape_ok(a->net, a->n_games))
    n += align256(wide_workspace_bytes(a));
  return n;
}

int32_t pg_gene_count(const pg_net *net) {
  if (!net) return fail(PG_ERR_INVALID, "net is NULL");
  int32_t rc = check_net(*net, false);
  if (rc != PG_OK) return rc;
  return gene_count(*net);
}

// ------------------------------ pg_eval_population's steps, in its order ----
// the arguments' ranges, whatever the kernel
static int32_t check_eval_ranges(const pg_eval_args *a) {
  int32_t rc = check_struct_size(a);
  if (rc != PG_OK) return rc;
  rc = check_net(a->net, true);
  if (rc != PG_OK) return rc;
  if (a->n_genomes < 0) return fail(PG_ERR_INVALID, "n_genomes=%d < 0", a->n_genomes);
  if (a->n_games < 1 || a->n_games > 64) return fail(PG_ERR_INVALID, "n_games=%d not in [1, 64]", a->n_games);
  if (a->horizon < 0) return fail(PG_ERR_INVALID, "horizon=%d < 0", a->horizon);
  if (a->timeout_thresh != 0 && (a->timeout_thresh < 32 || a->timeout_thresh > (1 << 20)))
    return fail(PG_ERR_INVALID, "timeout_thresh=%d not 0 or in [32, 1048576]", a->timeout_thresh);
  if (a->win_score < 0) return fail(PG_ERR_INVALID, "win_score=%d < 0", a->win_score);
  if (a->kernel & ~(0xff | PG_KERNEL_ADVANCE | PG_KERNEL_SOLO))
    return fail(PG_ERR_INVALID,
                "kernel=0x%x: unknown bits above the pg_kernel (PG_KERNEL_ADVANCE = 0x100 and PG_KERNEL_SOLO = 0x800 only)",
                (unsigned)a->kernel);
  return PG_OK;
}

// PG_KERNEL_ADVANCE and PG_KERNEL_SOLO go with the kernels of the families that have such instances
// (FamilyDesc::modifiers), named or through AUTO.  The refusals below name the families of the day they
// were worded; their text is pinned (tests/golden/), the table is what decides.
// (SPLIT takes the solo bit through AUTO only: the refusal of an explicit SPLIT | SOLO is kept for now)
static bool takes_modifier_bits(int kernel) {
  const FamilyDesc *f = family_of(kernel);
  return kernel == PG_KERNEL_AUTO || (f && f->modifiers);
}

static int32_t check_modifier_bits(int kernel, bool advance, bool solo) {
  if (advance && !takes_modifier_bits(kernel))
    return fail(PG_ERR_UNSUPPORTED,
                "PG_KERNEL_ADVANCE: kernel=%d has no closed-form frame advance to switch on (the advance bit goes "
                "with AUTO, RELU, RELU2 and SIG2; SPLIT and WIDE always advance)", kernel);
  if (solo && !takes_modifier_bits(kernel))
    return fail(PG_ERR_UNSUPPORTED,
                "PG_KERNEL_SOLO: kernel=%d has no solo games on half a lane group to switch on (the solo bit goes "
                "with AUTO, RELU, RELU2 and SIG2)", kernel);
  return PG_OK;
}

// Scope (pg_eval.hpp: each family states its own, activation first).  When a
// kernel is asked is today's order of refusals, an asymmetry that is kept:
// RELU_WIDE and every certified f32 family but RELU are refused out of scope
// on entry, even for an empty launch (scope_on_entry, FamilyDesc's flag of
// that name); RELU, SPLIT and WIDE only after the
// n_genomes == 0 return -- for a network of the other activation before the
// workspace check (scope_of_activation), for the rest at the launch (launch_games).
static int32_t scope_on_entry(const pg_eval_args &a) {
  if (a.kernel == PG_KERNEL_RELU_WIDE) return wide_scope(a, true);
  const FamilyDesc *f = family_of(a.kernel);
  return f && f->scope_on_entry ? f->scope(a) : PG_OK;
}

// the buffers and modes of a launch that plays games (n_genomes > 0)
static int32_t check_eval_buffers(const pg_eval_args *a) {
  const long total = (long)a->n_genomes * a->n_games;
  if (total > 0x7fffffffL) return fail(PG_ERR_INVALID, "too many games (%ld)", total);
  const int G = gene_count(a->net);
  if (!a->genomes || a->genome_stride < G)
    return fail(PG_ERR_INVALID, "genomes NULL or genome_stride=%lld < gene count %d", (long long)a->genome_stride, G);
  if (!a->game_kind || !a->game_opp || !a->game_mult || !a->fitness || !a->rewards || !a->scores ||
      !a->frames || !a->total_frames || !a->status)
    return fail(PG_ERR_INVALID, "a required per-game array is NULL");
  if (a->n_opponents > 0 && (!a->opponents || a->opponent_stride < G))
    return fail(PG_ERR_INVALID, "opponents NULL or opponent_stride < gene count");
  if (a->precision != PG_PREC_CERTIFIED && a->precision != PG_PREC_F64)
    return fail(PG_ERR_INVALID, "precision=%d", a->precision);
  if (a->trace && (a->trace_games < 0 || a->trace_cap < 1))
    return fail(PG_ERR_INVALID, "trace needs trace_games >= 0 and trace_cap >= 1");
  if (a->prep < PG_PREP_ALL || a->prep > PG_PREP_REST) return fail(PG_ERR_INVALID, "prep=%d", a->prep);
  return PG_OK;
}

// ReLU networks run on the ReLU families' kernels, k_wide's ReLU instances or
// k_general: whole episodes, no hard-case log.  The fixed horizon is the SPLIT kernel's.
static int32_t scope_of_activation(const pg_eval_args &a) {
  const FamilyDesc *f = family_of(a.kernel);
  if (a.net.activation == PG_ACT_RELU) {
    // (a sigmoid-only kernel's scope of a ReLU network is its refusal of the activation)
    if (a.kernel == PG_KERNEL_SPLIT) return split_scope(a);
    if (a.kernel == PG_KERNEL_WIDE) return wide_scope(a, false);
    if (a.horizon > 0) return fail(PG_ERR_UNSUPPORTED, "activation relu: no fixed-horizon mode (horizon must be 0)");
    if (a.hard_log) return fail(PG_ERR_UNSUPPORTED, "activation relu: no hard-case log (hard_log must be NULL)");
  } else if (f && !f->scope_on_entry) {  // (the same of a sigmoid network on a family scoped at the launch: RELU)
    const int32_t rc = f->scope(a);
    if (rc != PG_OK) return rc;
  }
  if (a.horizon > 0 && a.trace) return fail(PG_ERR_INVALID, "horizon mode runs untraced (trace must be NULL)");
  if (a.horizon > 0 && resolve_kernel(&a) != PG_KERNEL_SPLIT)
    return fail(PG_ERR_UNSUPPORTED, "horizon mode runs on the SPLIT kernel ([6, H<=64, 3], certified)");
  return PG_OK;
}

static EvalParams eval_params(const pg_eval_args *a) {
  EvalParams p;
  memset(&p, 0, sizeof(p));
  p.genomes = a->genomes;
  p.opponents = a->opponents ? a->opponents : a->genomes;
  p.kind = a->game_kind;
  p.opp = a->game_opp;
  p.mult = a->game_mult;
  p.rewards = a->rewards;
  p.scores = a->scores;
  p.frames = a->frames;
  p.total_frames = a->total_frames;
  p.counters = a->counters;
  p.trace = a->trace;
  p.trace_games = a->trace ? a->trace_games : 0;
  p.trace_cap = a->trace_cap;
  p.hard_log = a->hard_cap > 0 ? a->hard_log : nullptr;
  p.hard_cap = a->hard_cap;
  p.work = (unsigned int *)a->workspace;
  p.status_game = (int32_t *)((char *)a->workspace + 256);
  p.gstride = a->genome_stride;
  p.ostride = a->opponent_stride;
  p.n_opponents = a->opponents ? a->n_opponents : 0;
  p.rows = a->genome_rows;
  p.n_active = a->n_active;
  p.seed = a->seed;
  p.n_genomes = a->n_genomes;
  p.n_games = a->n_games;
  p.total = a->n_genomes * a->n_games;
  set_net(p, a->net);
  p.prep = a->prep;
  p.horizon = a->horizon;
  p.timeout_thresh = a->timeout_thresh > 0 ? a->timeout_thresh : kTimeoutThresh;
  // above the env's own end (a score of 21, Pong::done) WIN_SCORE changes nothing
  p.win_score = a->win_score > 0 ? (a->win_score < kDoneScore ? a->win_score : kDoneScore) : kWinScore;
  return p;
}

// the games on kernel (resolve_kernel's); RELU_WIDE and the families with scope_on_entry were found in scope
// on entry, the others are asked here
// (advance, solo: modifiers_in_effect's)
static int32_t launch_games(int kernel, const pg_eval_args *a, EvalParams &p, bool advance, bool solo, hipStream_t s) {
  void *const after_base = (char *)a->workspace + eval_base_workspace(a);
  const int dtype = a->net.dtype;
  int32_t rc = PG_OK;
  if (const FamilyDesc *f = family_of(kernel)) {
    if (!f->scope_on_entry) rc = f->scope(*a);
    return rc != PG_OK ? rc : f->launch(p, dtype, advance, solo, s);
  }
  switch (kernel) {
    case PG_KERNEL_RELU_WIDE:
      return launch_wide(p, dtype, after_base, s);
    case PG_KERNEL_WIDE:
      rc = wide_scope(*a, false);
      return rc != PG_OK ? rc : launch_wide(p, dtype, after_base, s);
    case PG_KERNEL_SPLIT: {
      rc = split_scope(*a);
      if (rc != PG_OK) return rc;
      const int L = a->group_lanes > 0 ? a->group_lanes : choose_split_lanes(a->net.nodes[1]);
      p.recs = (float *)after_base;
      return dtype == PG_F64 ? launch_service_any<double>(p, L, a->net.nodes[2], solo, s)
                             : launch_service_any<float>(p, L, a->net.nodes[2], solo, s);
    }
    case PG_KERNEL_RESIDENT:
    case PG_KERNEL_STAGED:
      // retired layouts (correct, measured slower than SPLIT; removed in round 4)
      return fail(PG_ERR_UNSUPPORTED, "the %s kernel was retired (DESIGN 4.1b-c); use SPLIT",
                  kernel == PG_KERNEL_RESIDENT ? "resident" : "staged");
    case PG_KERNEL_GENERAL:
      return launch_general(p, dtype, s);
    default:
      return fail(PG_ERR_INVALID, "kernel=%d", a->kernel);
  }
}

// pg_eval_population's checks ahead of its n_genomes == 0 return, and pg_eval_resolve's: the ranges,
// the modifier bits, the scopes asked on entry.  pg_eval_args.kernel is a pg_kernel in the low byte
// with modifier bits above it: named is the caller's struct with the pg_kernel alone, so every scope
// check and message after this is the base kernel's
static int32_t check_eval_entry(const pg_eval_args *a, pg_eval_args &named, bool &advance, bool &solo) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  int32_t rc = check_eval_ranges(a);
  if (rc != PG_OK) return rc;
  advance = (a->kernel & PG_KERNEL_ADVANCE) != 0;
  solo = (a->kernel & PG_KERNEL_SOLO) != 0;
  named = *a;
  named.kernel = a->kernel & 0xff;
  rc = check_modifier_bits(named.kernel, advance, solo);
  if (rc != PG_OK) return rc;
  return scope_on_entry(named);
}

int32_t pg_eval_resolve(const pg_eval_args *a) {
  pg_eval_args named;
  bool advance, solo;
  const int32_t rc = check_eval_entry(a, named, advance, solo);
  if (rc != PG_OK) return rc;
  const int kernel = resolve_kernel(&named);
  return kernel | modifiers_in_effect(kernel, named, advance, solo);
}

int32_t pg_eval_population(const pg_eval_args *a, void *stream) {
  pg_eval_args named;
  bool advance, solo;
  int32_t rc = check_eval_entry(a, named, advance, solo);
  if (rc != PG_OK) return rc;
  a = &named;
  hipStream_t s = (hipStream_t)stream;
  if (a->n_genomes == 0) {  // nothing to play (e.g. an empty shard); the counters still read zero
    if (a->counters) PG_HIP(hipMemsetAsync(a->counters, 0, 16 * sizeof(uint64_t), s));
    return PG_OK;
  }
  rc = check_eval_buffers(a);
  if (rc != PG_OK) return rc;
  rc = scope_of_activation(*a);
  if (rc != PG_OK) return rc;
  const size_t need = pg_eval_workspace_bytes(a);
  if (!a->workspace || a->workspace_bytes < need)
    return fail(PG_ERR_INVALID, "workspace of %zu bytes required (got %zu)", need, a->workspace_bytes);

  EvalParams p = eval_params(a);
  const int kernel = resolve_kernel(a);
  if (kernel != PG_KERNEL_SPLIT) {
    if (a->prep == PG_PREP_GENOMES) return PG_OK;  // no records outside the split kernel
    p.prep = PG_PREP_ALL;
    PG_HIP(hipMemsetAsync(a->workspace, 0, 256, s));
    if (a->counters) PG_HIP(hipMemsetAsync(a->counters, 0, 16 * sizeof(uint64_t), s));
  }  // the split kernel's k_prep_records zeroes the work header and the counters itself
  const int bits = modifiers_in_effect(kernel, *a, advance, solo);
  rc = launch_games(kernel, a, p, (bits & PG_KERNEL_ADVANCE) != 0, (bits & PG_KERNEL_SOLO) != 0, s);
  if (rc != PG_OK) return rc;
  if (kernel == PG_KERNEL_SPLIT && a->prep == PG_PREP_GENOMES) return PG_OK;  // records only: no games, no fitness
  hipLaunchKernelGGL(k_fitness, dim3((a->n_genomes + 255) / 256), dim3(256), 0, s, a->rewards,
                     p.status_game, a->n_genomes, a->n_active, a->n_games, a->fitness, a->status);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_decide(const pg_decide_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  int32_t rc = check_net(a->net, false);
  if (rc != PG_OK) return rc;
  if (a->net.activation != PG_ACT_SIGMOID)
    return fail(PG_ERR_UNSUPPORTED, "pg_decide: activation relu -- the split kernel's cascade is the sigmoid's (pg_relu_decide)");
  if (!resident_shape_ok(a->net)) return fail(PG_ERR_UNSUPPORTED, "pg_decide: the split kernel's shapes only");
  if (a->n < 0) return fail(PG_ERR_INVALID, "n=%d < 0", a->n);
  if (a->n == 0) return PG_OK;
  const int G = gene_count(a->net);
  if (!a->genomes || a->genome_stride < G || !a->k || !a->index)
    return fail(PG_ERR_INVALID, "genomes/k/index NULL or genome_stride < gene count %d", G);
  DecideParams p;
  memset(&p, 0, sizeof(p));
  p.genomes = a->genomes;
  p.gidx = a->genome_index;
  p.k = a->k;
  p.index = a->index;
  p.stage = a->stage;
  p.gstride = a->genome_stride;
  p.n = a->n;
  p.H = a->net.nodes[1];
  p.b = a->net.bias ? 1 : 0;
  const int H = p.H, O = a->net.nodes[2];
  const int L = choose_split_lanes(H);
  const size_t lds = (size_t)f64_lds_doubles(H, O) * sizeof(double);
  return launch_decide(p, L, O, a->net.dtype == PG_F64, lds, (hipStream_t)stream);
}

// pg_wide_decide runs k_wide as a one-game evaluation of n genomes: the
// evaluation's sizes for its workspace (a game counter, then the blocks' W2 copies)
static pg_eval_args wide_decide_eval(const pg_wide_decide_args *a) {
  pg_eval_args e;
  memset(&e, 0, sizeof(e));
  e.struct_size = sizeof(e);
  e.net = a->net;
  e.n_genomes = a->n;
  e.n_games = 1;
  return e;
}

size_t pg_wide_decide_workspace_bytes(const pg_wide_decide_args *a) {
  if (!a || a->n <= 0 || !wide_shape_ok(a->net, 1)) return 256;
  const pg_eval_args e = wide_decide_eval(a);
  return 256 + align256(wide_workspace_bytes(&e));
}

// one frame of k_wide (the instance of a->net.activation) per pass; name: the entry point, for its messages
static int32_t wide_decide_run(const char *name, const pg_wide_decide_args *a, void *stream) {
  if (!wide_shape_ok(a->net, 1))
    return fail(PG_ERR_UNSUPPORTED, "%s: the wide kernel's shapes [6, H1<=512, H2<=512, 1..4] only", name);
  if (a->n < 0) return fail(PG_ERR_INVALID, "n=%d < 0", a->n);
  if (a->n == 0) return PG_OK;
  const int G = gene_count(a->net);
  if (!a->genomes || a->genome_stride < G || !a->k || !a->index)
    return fail(PG_ERR_INVALID, "genomes/k/index NULL or genome_stride < gene count %d", G);
  const size_t need = pg_wide_decide_workspace_bytes(a);
  if (!a->workspace || a->workspace_bytes < need)
    return fail(PG_ERR_INVALID, "workspace of %zu bytes required (got %zu)", need, a->workspace_bytes);
  hipStream_t s = (hipStream_t)stream;
  EvalParams p;
  memset(&p, 0, sizeof(p));
  p.genomes = a->genomes;
  p.opponents = a->genomes;
  p.rows = a->genome_index;
  p.work = (unsigned int *)a->workspace;
  p.gstride = a->genome_stride;
  p.ostride = a->genome_stride;
  p.n_genomes = a->n;
  p.n_games = 1;
  p.total = a->n;
  set_net(p, a->net);
  p.wide_probe_k = a->k;
  p.wide_probe_index = a->index;
  p.wide_probe_act = a->act;
  PG_HIP(hipMemsetAsync(a->workspace, 0, 256, s));
  return launch_wide(p, a->net.dtype, (char *)a->workspace + 256, s);
}

int32_t pg_wide_decide(const pg_wide_decide_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  int32_t rc = check_net(a->net, false);
  if (rc != PG_OK) return rc;
  if (a->net.activation != PG_ACT_SIGMOID)
    return fail(PG_ERR_UNSUPPORTED, "pg_wide_decide: activation relu -- the wide kernel evaluates sigmoid networks only");
  return wide_decide_run("pg_wide_decide", a, stream);
}

// The same frame on k_wide's ReLU instances (PG_KERNEL_RELU_WIDE); the workspace is pg_wide_decide's.
size_t pg_relu_wide_decide_workspace_bytes(const pg_wide_decide_args *a) { return pg_wide_decide_workspace_bytes(a); }

int32_t pg_relu_wide_decide(const pg_wide_decide_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  int32_t rc = check_net(a->net, false);
  if (rc != PG_OK) return rc;
  if (a->net.activation != PG_ACT_RELU)
    return fail(PG_ERR_UNSUPPORTED, "pg_relu_wide_decide: activation sigmoid -- PG_ACT_RELU networks only (pg_wide_decide)");
  return wide_decide_run("pg_relu_wide_decide", a, stream);
}

int32_t pg_physics_reset(int32_t *state, int32_t n, const uint64_t *seeds, const int32_t *one_player,
                         void *stream) {
  if (n < 0 || (n > 0 && !state)) return fail(PG_ERR_INVALID, "state NULL or n < 0");
  if (n == 0) return PG_OK;
  hipLaunchKernelGGL(k_physics_reset, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, n,
                     seeds, one_player);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

int32_t pg_physics_step(int32_t *state, int32_t n, const uint8_t *actions, void *stream) {
  if (n < 0 || (n > 0 && (!state || !actions))) return fail(PG_ERR_INVALID, "state/actions NULL or n < 0");
  if (n == 0) return PG_OK;
  hipLaunchKernelGGL(k_physics_step, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, n,
                     actions);
  PG_HIP(hipGetLastError());
  return PG_OK;
}
}  // extern "C"
