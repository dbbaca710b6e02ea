// lbsim_dyn_delay.hip -- the dynamics launchers of a handle with action latency:
// dynamics_group_delay_kernel, the full server-per-lane form with the delay code, one object per
// step mode: built with -DLBSIM_DYN_MODE=0 (kModeStep, launch_dynamics_delay_step) and =2
// (kModeStepNR, launch_dynamics_delay_step_nr).  A reset has no delay and runs lbsim_dyn.hip's
// full kernel.  Objects of their own, so the full kernels of every other handle are the code they
// were, and these compile beside them.
#include "lbsim_internal.h"
#include "lbsim_dyn_group.h"

#if !defined(LBSIM_DYN_MODE) || (LBSIM_DYN_MODE != 0 && LBSIM_DYN_MODE != 2)
#error "build with -DLBSIM_DYN_MODE=0 (step) or 2 (step with next-step resets)"
#endif

namespace lbk {
namespace {

constexpr int MODE = LBSIM_DYN_MODE == 0 ? kModeStep : kModeStepNR;

void launch_delay_t(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                    const uint8_t* mask, hipStream_t stream) {
  const DynPlan& d = L.plan.dyn;  // a full group plan (make_plan: action_delay is full_only)
  const dim3 grid(d.grid), block(d.block);
  const bool trace = L.prm.trace != 0;
  SimParams prm = L.prm;
  prm.dyn_epw = d.epw;
  pick<2, 4, 8, 16, 32, 64>(d.width, [&](auto GG) { pick<0, 1, 2, 3, 4>(L.prm.policy, [&](auto P) {
    pick_bool(trace, [&](auto T) {
      LBSIM_LAUNCH((dynamics_group_delay_kernel<decltype(GG)::value, MODE, decltype(P)::value,
                                                decltype(T)::value>),
                   grid, block, 0, stream, L.st, prm, action, dtype, assign, mask, L.flow, L.cross,
                   L.workers, L.delay);
    });
  }); });
}

}  // namespace

#if LBSIM_DYN_MODE == 0
void launch_dynamics_delay_step(const LaunchCtx& L, const void* action, int dtype,
                                int32_t* assign, const uint8_t* mask, hipStream_t s) {
  launch_delay_t(L, action, dtype, assign, mask, s);
}
#else
void launch_dynamics_delay_step_nr(const LaunchCtx& L, const void* action, int dtype,
                                   int32_t* assign, const uint8_t* mask, hipStream_t s) {
  launch_delay_t(L, action, dtype, assign, mask, s);
}
#endif

}  // namespace lbk
