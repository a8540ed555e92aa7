// pg_service_solo.hip -- k_service's kSolo instances (pg_service.hpp, DESIGN.md
// 4.2j; PG_KERNEL_SOLO where PG_KERNEL_AUTO resolves to SPLIT): the bench
// layout L = 8, U = 16 ([6, 33..64, O]) on the untraced, non-horizon frame, a
// game against a scripted opponent played by half a lane group.  A unit of its
// own, so the objects of pong_ga.hip and pg_service_more.hip keep what they hold.
//
// pong_amd/build.py compiles this file twice, as the base instances are: with
// -DPG_SOLO_O3 under pong_ga.hip's iterative-ILP scheduler the O = 3 instances,
// without it under the default scheduler the O = 2 and 4 ones and the dispatch.
#include "pg_service.hpp"

namespace pg {

template <int O, typename WT>
static void solo_launch(int grid, size_t lds, hipStream_t s, const EvalParams &p) {
  hipLaunchKernelGGL((k_service<8, 16, O, WT, true, false, true>), dim3(grid), dim3(svc_threads<16>()), lds, s, p);
}

#ifdef PG_SOLO_O3
void service_solo_game_o3(bool f64, int grid, size_t lds, hipStream_t s, const EvalParams &p) {
  if (f64) solo_launch<3, double>(grid, lds, s, p);
  else solo_launch<3, float>(grid, lds, s, p);
}
#else
void service_solo_game_o3(bool f64, int grid, size_t lds, hipStream_t s, const EvalParams &p);

void service_solo_game(int O, bool f64, int grid, size_t lds, hipStream_t s, const EvalParams &p) {
  if (O == 3) return service_solo_game_o3(f64, grid, lds, s, p);
  if (O == 2) {
    if (f64) solo_launch<2, double>(grid, lds, s, p);
    else solo_launch<2, float>(grid, lds, s, p);
  } else {
    if (f64) solo_launch<4, double>(grid, lds, s, p);
    else solo_launch<4, float>(grid, lds, s, p);
  }
}
#endif

}  // namespace pg
