// lbsim_dyn_ack.hip -- the dynamics launchers of a handle with duration samples at every data ACK
// (DESIGN.md §3.25): dynamics_group_ack_kernel, the full server-per-lane form with the ACK code,
// one object per mode: built with -DLBSIM_DYN_MODE=0 (kModeStep, launch_dynamics_ack_step) and =1
// (kModeReset, launch_dynamics_ack_reset: a reset's warm-up records its ACKs too).  Objects of
// their own, so the full kernels of every other handle are the code they were, and these compile
// beside them.
#include "lbsim_internal.h"
#include "lbsim_dyn_group.h"

#if !defined(LBSIM_DYN_MODE) || (LBSIM_DYN_MODE != 0 && LBSIM_DYN_MODE != 1)
#error "build with -DLBSIM_DYN_MODE=0 (step) or 1 (reset)"
#endif

namespace lbk {
namespace {

constexpr int MODE = LBSIM_DYN_MODE == 0 ? kModeStep : kModeReset;

void launch_ack_t(const LaunchCtx& L, const AckSamples& as, const void* action, int dtype,
                  int32_t* assign, const uint8_t* mask, hipStream_t stream) {
  // a full group plan of kernel LBSIM_DYN_KERNEL_ACK (make_plan: ack_samples)
  const DynPlan& d = MODE == kModeReset ? L.plan.reset_dyn : L.plan.dyn;
  const dim3 grid(d.grid), block(d.block);
  const bool trace = L.prm.trace != 0;
  SimParams prm = L.prm;
  prm.dyn_epw = d.epw;
  pick<2, 4, 8, 16, 32, 64>(d.width, [&](auto GG) { pick<0, 1, 2, 3, 4>(L.prm.policy, [&](auto P) {
    pick_bool(trace, [&](auto T) {
      LBSIM_LAUNCH((dynamics_group_ack_kernel<decltype(GG)::value, MODE, decltype(P)::value,
                                              decltype(T)::value>),
                   grid, block, 0, stream, L.st, prm, action, dtype, assign, mask, as);
    });
  }); });
}

}  // namespace

#if LBSIM_DYN_MODE == 0
void launch_dynamics_ack_step(const LaunchCtx& L, const AckSamples& as, const void* action,
                              int dtype, int32_t* assign, hipStream_t s) {
  launch_ack_t(L, as, action, dtype, assign, nullptr, s);
}
#else
void launch_dynamics_ack_reset(const LaunchCtx& L, const AckSamples& as, const uint8_t* mask,
                               hipStream_t s) {
  launch_ack_t(L, as, nullptr, 0, nullptr, mask, s);
}
#endif

}  // namespace lbk
