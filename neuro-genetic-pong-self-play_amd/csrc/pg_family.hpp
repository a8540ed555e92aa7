// pg_family.hpp -- the host side of a certified f32 family, stated once: its
// scope (pg_eval.hpp), its game launch and its pg_*_decide entry point, and the
// descriptor that pong_ga.hip's family table holds.  Host code only.
//
// A family F (ReluFamily in pg_relu.hip, Relu2Family, Sig2Family,
// Relu2BlockFamily, Sig2BlockFamily, Relu3Family, Sig3Family in theirs) supplies
//   kKernel, kActivation      its pg_kernel and the pg_activation it evaluates
//   kModifiers                it has k_*_adv and k_*_solo instances (PG_KERNEL_ADVANCE, PG_KERNEL_SOLO)
//   kScopeOnEntry             FamilyDesc::scope_on_entry
//   kName                     as its messages spell it
//   shape_ok(n_nodes, nodes)  its shapes, the bias apart
//   genes(nodes)              the gene count of a shape in scope, with bias
//   game_grid(p), game(p, f64, advance, solo, grid, s)
//                             the blocks of a game launch, and that launch on its instance for p.nodes
//   DecideParams, decide_params(a), decide_grid(a), decide(nodes, f64, grid, s, params)
//                             the same for its decide kernel
//   kBadActivation, kBadShape, kNoBias   its scope refusals, as literals (a family that folds the bias into
//                             the shape's message names that one twice)
//   kNoHorizon, kNoHardLog    both or neither: the ReLU lane families have no rule of their own, because
//                             pg_eval_population refuses both for every ReLU network (scope_of_activation)
//   kDecideBadActivation (with one %d, the activation), kDecideBadShape, kDecideNoBias
//                             pg_*_decide's refusals
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pg_certgame.hpp"
#include "pg_eval.hpp"

namespace pg {

template <class F, class = void>
struct has_episode_rules : std::false_type {};
template <class F>
struct has_episode_rules<F, std::void_t<decltype(F::kNoHorizon), decltype(F::kNoHardLog)>> : std::true_type {};

// The family's scope, in its words and in the order every family keeps:
// activation, shape, bias, precision, horizon, hard-case log.
template <class F>
int32_t family_scope(const pg_eval_args &a) {
  if (a.net.activation != F::kActivation) return fail(PG_ERR_UNSUPPORTED, "%s", F::kBadActivation);
  if (!F::shape_ok(a.net.n_nodes, a.net.nodes)) return fail(PG_ERR_UNSUPPORTED, "%s", F::kBadShape);
  if (!a.net.bias) return fail(PG_ERR_UNSUPPORTED, "%s", F::kNoBias);
  if (a.precision == PG_PREC_F64) return fail(PG_ERR_UNSUPPORTED, "%s kernel is the certified-precision path", F::kName);
  if constexpr (has_episode_rules<F>::value) {
    if (a.horizon > 0) return fail(PG_ERR_UNSUPPORTED, "%s", F::kNoHorizon);
    if (a.hard_log) return fail(PG_ERR_UNSUPPORTED, "%s", F::kNoHardLog);
  }
  return PG_OK;
}

// p: a network in family_scope<F>, row strides of at least its gene count (pg_eval_population)
template <class F>
int32_t family_launch(const EvalParams &p, int dtype, bool advance, bool solo, hipStream_t s) {
  const int grid = F::game_grid(p);
  if (grid <= 0) return PG_OK;
  // a traced launch records every frame: it runs with the advance off
  F::game(p, dtype == PG_F64, advance && !p.trace, solo, grid, s);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

template <class F>
int32_t family_decide(const pg_relu_decide_args *a, void *stream) {
  if (!a) return fail(PG_ERR_INVALID, "args is NULL");
  if (a->net.dtype != PG_F32 && a->net.dtype != PG_F64) return fail(PG_ERR_INVALID, "net.dtype=%d", a->net.dtype);
  if (a->net.activation != F::kActivation) return fail(PG_ERR_UNSUPPORTED, F::kDecideBadActivation, a->net.activation);
  if (!F::shape_ok(a->net.n_nodes, a->net.nodes)) return fail(PG_ERR_UNSUPPORTED, "%s", F::kDecideBadShape);
  if (!a->net.bias) return fail(PG_ERR_UNSUPPORTED, "%s", F::kDecideNoBias);
  if (a->n < 0) return fail(PG_ERR_INVALID, "n=%d < 0", a->n);
  if (a->n == 0) return PG_OK;
  const long G = F::genes(a->net.nodes);
  if (!a->genomes || a->genome_stride < G || !a->k || !a->index)
    return fail(PG_ERR_INVALID, "genomes/k/index NULL or genome_stride < gene count %ld", G);
  const typename F::DecideParams p = F::decide_params(a);
  F::decide(a->net.nodes, a->net.dtype == PG_F64, F::decide_grid(a), (hipStream_t)stream, p);
  PG_HIP(hipGetLastError());
  return PG_OK;
}

// the family's row of pong_ga.hip's table
template <class F>
constexpr FamilyDesc family_desc() {
  return {F::kKernel, F::kModifiers, F::kScopeOnEntry, family_scope<F>, family_launch<F>};
}

}  // namespace pg
