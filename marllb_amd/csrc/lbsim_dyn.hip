// lbsim_dyn.hip — dynamics launchers, one object per mode: built with
// -DLBSIM_DYN_MODE=0 (kModeStep, launch_dynamics_step), =1 (kModeReset, launch_dynamics_reset)
// and =2 (kModeStepNR, launch_dynamics_step_nr: the step of a next-step auto-reset handle) so the
// thirds of the template instantiations compile in parallel.
#include "lbsim_internal.h"
#include "lbsim_dyn_group.h"
#include "lbsim_dyn_wave.h"

#ifndef LBSIM_DYN_MODE
#error "build with -DLBSIM_DYN_MODE=0 (step), 1 (reset) or 2 (step with next-step resets)"
#endif

namespace lbk {
namespace {

constexpr int MODE = LBSIM_DYN_MODE == 0 ? kModeStep : (LBSIM_DYN_MODE == 1 ? kModeReset : kModeStepNR);

// The dynamics the plan names (DynPlan, lbsim_plan.h), one launch site per kernel.
void launch_dynamics_t(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                       const uint8_t* mask, hipStream_t stream) {
  const DynPlan& d = MODE == kModeReset ? L.plan.reset_dyn : L.plan.dyn;
  const dim3 grid(d.grid), block(d.block);
  const bool trace = L.prm.trace != 0;
  if (d.kernel == LBSIM_DYN_KERNEL_WAVE) {  // one wave per env: NG ring registers; no ALIAS
    pick<1, 2, 4>(d.width, [&](auto NG) { pick<0, 1, 2, 3>(L.prm.policy, [&](auto P) {
      pick_bool(trace, [&](auto T) {
        LBSIM_LAUNCH((dynamics_wave_kernel<decltype(NG)::value, MODE, decltype(P)::value,
                                           decltype(T)::value>),
                     grid, block, 0, stream, L.st, L.prm, action, dtype, assign, mask);
      });
    }); });
    return;
  }
  if (d.kernel == LBSIM_DYN_KERNEL_ENV_LANE) {  // one lane per env, kDynWaves waves per workgroup
    pick<4, 8, 16>(d.width, [&](auto M) { pick<0, 1, 2, 3, 4>(L.prm.policy, [&](auto P) {
      pick_bool(trace, [&](auto T) {
        constexpr int MAXS = decltype(M)::value;
        static_assert(64u * kDynWaves<MAXS> == env_lane_block(MAXS), "the plan's block size");
        LBSIM_LAUNCH((dynamics_kernel<MAXS, MODE, decltype(P)::value, decltype(T)::value>), grid,
                     block, 0, stream, L.st, L.prm, action, dtype, assign, mask);
      });
    }); });
    return;
  }
#if LBSIM_DYN_MODE != 1
  // a step of an action-delay handle (a full one): its own kernels, in their own objects
  if (d.full && L.delay.wring != nullptr) {
    if (MODE == kModeStep) launch_dynamics_delay_step(L, action, dtype, assign, mask, stream);
    else launch_dynamics_delay_step_nr(L, action, dtype, assign, mask, stream);
    return;
  }
#endif
  // server per lane: G lanes per env (32 / 64 for S > 16), epw <= 64 / G envs per wave, which
  // only this kernel's own copy of the parameters carries
  SimParams prm = L.prm;
  prm.dyn_epw = d.epw;
  pick<2, 4, 8, 16, 32, 64>(d.width, [&](auto GG) { pick<0, 1, 2, 3, 4>(L.prm.policy, [&](auto P) {
    pick_bool(trace, [&](auto T) {
      constexpr int G = decltype(GG)::value, POLICY = decltype(P)::value;
      constexpr bool TRACE = decltype(T)::value;
      if (d.full) {  // every feature's code (group_event_loop FULL), its own register budget
        LBSIM_LAUNCH((dynamics_group_full_kernel<G, MODE, POLICY, TRACE>), grid, block, 0, stream,
                     L.st, prm, action, dtype, assign, mask, L.flow, L.cross, L.workers);
        return;
      }
      // the register budgets that exist: 4 waves for every next-step auto-reset step, 1 for the
      // rest, and 5 beside it where the plan may ask for it (the SED step, 4 / 8 lanes).  The
      // next-step unit has always held the 1-wave kernels too, which no plan asks it for: they
      // stay listed, since without them the compiler schedules its 4-wave kernels differently.
      constexpr int W = MODE == kModeStepNR ? 4 : 1;
      constexpr int W5 = MODE == kModeStep && POLICY == 0 && (G == 4 || G == 8) ? 5 : W;
      pick<W5, W, 1>(d.waves, [&](auto WAVES) {
        LBSIM_LAUNCH((dynamics_group_kernel<G, MODE, POLICY, TRACE, decltype(WAVES)::value>), grid,
                     block, 0, stream, L.st, prm, action, dtype, assign, mask);
      });
    });
  }); });
}

}  // namespace

#if LBSIM_DYN_MODE == 0
void launch_dynamics_step(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                          const uint8_t* mask, hipStream_t s) {
  launch_dynamics_t(L, action, dtype, assign, mask, s);
}
#elif LBSIM_DYN_MODE == 2
void launch_dynamics_step_nr(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                             const uint8_t* mask, hipStream_t s) {
  launch_dynamics_t(L, action, dtype, assign, mask, s);
}
#else
void launch_dynamics_reset(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                           const uint8_t* mask, hipStream_t s) {
  launch_dynamics_t(L, action, dtype, assign, mask, s);
}
#endif

}  // namespace lbk
