// lbsim_internal.h — host-side glue between the extern "C" API (lbsim_api.hip) and the translation
// units that instantiate the templated kernels (compiled in parallel, linked into liblbsim.so):
//
//   lbsim_cross.h      hidden cross traffic: the host / device rule and its conversion kernel
//   lbsim_workers.h    multi-worker servers: the host / device rule and its conversion kernel
//   lbsim_delay.h      action latency: the host / device rule, its conversion and gather kernels
//   lbsim_plan.h       make_plan: which kernels a handle's step and reset launch, decided once
//                      (host-only; the launchers below turn the plan into template arguments)
//   lbsim_dyn_delay.hip  dynamics_group_delay_kernel launchers (action latency); built twice
//                      (-DLBSIM_DYN_MODE=0 step, 2 step_nr)
//   lbsim_acks.h       duration samples at every data ACK: the host / device rule of a flow's ACKs
//   lbsim_dyn_ack.hip  dynamics_group_ack_kernel launchers (ACK samples); built twice
//                      (-DLBSIM_DYN_MODE=0 step, 1 reset)
//   lbsim_pool.h       shared server pools: the host / device rule of a pool and its physical FIFOs
//   lbsim_dyn_pool.hip  dynamics_pool_kernel launchers (shared server pools); built twice
//                      (-DLBSIM_DYN_MODE=0 step, 1 reset, with the pool handle's two small kernels)
//   lbsim_ps.h         processor-sharing servers: the host / device rule of a server's virtual clock
//   lbsim_dyn_ps.hip   dynamics_ps_kernel launchers (processor sharing); built twice
//                      (-DLBSIM_DYN_MODE=0 step, 1 reset)
//   lbsim_dyn_pool_ps.hip  dynamics_pool_ps_kernel launchers (pools of processor-sharing servers);
//                      built twice (-DLBSIM_DYN_MODE=0 step, 1 reset, with lbsim_pool_ps_state's kernel)
//   lbsim_dyn.hip      dynamics_kernel / dynamics_group_kernel launchers; built three times
//                      (-DLBSIM_DYN_MODE=0: step, 1: reset, 2: the next-step auto-reset step)
//   lbsim_obs.hip      observe_kernel launchers
//   lbsim_step.hip     the one-launch steps (fused_step_kernel, step_wave_kernel)
//   lbsim_pol.hip      one-kernel policy networks (lbsim_fused.h)
//
// Non-template kernels live only in lbsim_api.hip (a __global__ defined in two objects would be
// defined twice); templates are instantiated where they are launched.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "../../include/lbsim.h"
#include "lbsim_acks.h"
#include "lbsim_cross.h"
#include "lbsim_delay.h"
#include "lbsim_kernels.h"
#include "lbsim_plan.h"
#include "lbsim_pool.h"
#include "lbsim_workers.h"

namespace lbk {

// Launch log: every kernel launch of the library goes through LBSIM_LAUNCH, which records the
// launched kernel's host stub for the API call in progress (lbsim_launch_names resolves the stubs
// to their names afterwards, off the step path).  bench.py keys its committed PMC counter files by
// these names, so counters of a kernel that did not run are never attached to a measurement.
void note_launch(const void* host_fn);
#define LBSIM_LAUNCH(KERNEL, GRID, BLOCK, LDS, STREAM, ...)                 \
  do {                                                                    \
    ::lbk::note_launch(reinterpret_cast<const void*>(&KERNEL));           \
    hipLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, STREAM, __VA_ARGS__);    \
  } while (0)

// An integer override from the environment, else dflt, for the handle-free policy entry points
// (the simulator's own overrides: Overrides::from_env, lbsim_plan.h).  Callers keep the value in a
// function-local static: read once per process.
inline int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}

// What a launcher needs of a handle: its plan (made once, at lbsim_create) and its state.
struct LaunchCtx {
  const StepPlan& plan;
  const DevState& st;
  const SimParams& prm;
  const FlowStats& flow;  // the full group dynamics' flow statistics (null pointers: off)
  const CrossTraffic& cross;  // and its cross traffic (lbsim_cross.h; null pointers: none)
  const ServerWorkers& workers;  // and its servers' worker counts (lbsim_workers.h; null: none)
  const ActionDelay& delay;  // and its action latency's arrays (lbsim_delay.h; null: none)
};

// Runtime value -> template argument: pick<2, 4, 8>(v, f) calls f(std::integral_constant<int, v>)
// for the listed value that v equals, else for the last one; f reads it as decltype(V)::value.
template <int... Vs, typename F>
void pick(int v, F&& f) {
  constexpr int vs[] = {Vs...}, last = vs[sizeof...(Vs) - 1];
  [[maybe_unused]] bool done = false;
  ((!done && (v == Vs || Vs == last) ? (f(std::integral_constant<int, Vs>{}), done = true) : false),
   ...);
}
template <typename F>
void pick_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

// Dynamics of one step (mode kModeStep) or of a reset with warm-up (kModeReset).
void launch_dynamics_step(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                          const uint8_t* mask, hipStream_t s);
void launch_dynamics_reset(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                           const uint8_t* mask, hipStream_t s);
// The step of a next-step auto-reset handle (kModeStepNR): envs done last step reset instead.
void launch_dynamics_step_nr(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                             const uint8_t* mask, hipStream_t s);
// The same two for a handle with action latency (lbsim_dyn_delay.hip: dynamics_group_delay_kernel;
// the plan is a full group one and L.delay holds the arrays).
void launch_dynamics_delay_step(const LaunchCtx& L, const void* action, int dtype,
                                int32_t* assign, const uint8_t* mask, hipStream_t s);
void launch_dynamics_delay_step_nr(const LaunchCtx& L, const void* action, int dtype,
                                   int32_t* assign, const uint8_t* mask, hipStream_t s);

// The dynamics of a handle with duration samples at every data ACK (lbsim_dyn_ack.hip:
// dynamics_group_ack_kernel; the plan is a full group one of kernel
// LBSIM_DYN_KERNEL_ACK; as: the envs' ACK intervals and max_acks).
void launch_dynamics_ack_step(const LaunchCtx& L, const AckSamples& as, const void* action,
                              int dtype, int32_t* assign, hipStream_t s);
void launch_dynamics_ack_reset(const LaunchCtx& L, const AckSamples& as, const uint8_t* mask,
                               hipStream_t s);

// The dynamics of a handle with shared server pools (lbsim_dyn_pool.hip: dynamics_pool_kernel; the
// plan is a pool one and pa holds the physical FIFOs).  A reset's mask is the widened one.
void launch_dynamics_pool_step(const LaunchCtx& L, const PoolArrays& pa, const void* action,
                               int dtype, int32_t* assign, hipStream_t s);
void launch_dynamics_pool_reset(const LaunchCtx& L, const PoolArrays& pa, const uint8_t* mask,
                                hipStream_t s);
// pa.mask[b] = whether any member of env b's pool is in `mask` (B bytes, non-NULL).
void launch_pool_mask(const PoolArrays& pa, const uint8_t* mask, int B, hipStream_t s);
// lbsim_ground_truth of a pool handle: the physical servers' rows; mu: the config's rates.
void launch_pool_truth(const LaunchCtx& L, const PoolArrays& pa, const float* mu, float* out,
                       hipStream_t s);

// The dynamics of a handle with processor-sharing servers (lbsim_dyn_ps.hip: dynamics_ps_kernel;
// the plan is a PS one, L.flow holds the flow statistics' arrays or null pointers; cores: the
// servers' core counts [B * S], §3.23, or nullptr: one each).
void launch_dynamics_ps_step(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                             const int32_t* cores, hipStream_t s);
void launch_dynamics_ps_reset(const LaunchCtx& L, const uint8_t* mask, const int32_t* cores,
                              hipStream_t s);

// The dynamics of a handle whose shared server pools have processor-sharing servers
// (lbsim_dyn_pool_ps.hip: dynamics_pool_ps_kernel, §3.24; the plan is a PS pool one, pa holds the
// physical servers' words and owners; cores: the physical servers' core counts [C * S], or
// nullptr: one each).  A reset's mask is the widened one.
void launch_dynamics_pool_ps_step(const LaunchCtx& L, const PoolArrays& pa, const void* action,
                                  int dtype, int32_t* assign, const int32_t* cores, hipStream_t s);
void launch_dynamics_pool_ps_reset(const LaunchCtx& L, const PoolArrays& pa, const uint8_t* mask,
                                   const int32_t* cores, hipStream_t s);
// lbsim_pool_ps_state: out[B, S, 5], each member's row the physical server's.
void launch_pool_ps_state(const LaunchCtx& L, const PoolArrays& pa, const int32_t* cores,
                          float* out, hipStream_t s);

void launch_observe_step(const LaunchCtx& L, const ObsOutputs& o, const uint8_t* mask,
                         hipStream_t s);
void launch_observe_reset(const LaunchCtx& L, const ObsOutputs& o, const uint8_t* mask,
                          hipStream_t s);

struct SacActorArgs;
struct QmixArgs;
// The one-launch steps (lbsim_step.hip), for a plan of form kStepGroupFused (dynamics of a wave's
// groups, then their observe) / kStepWave (dynamics_wave then observe per env).
void launch_fused_step(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                       const ObsOutputs& o, hipStream_t s);
void launch_step_wave(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                      const ObsOutputs& o, hipStream_t s);

// The fused policy kernels (lbsim_pol.hip), which own their LDS layout: the launchers set the
// args' row strides (ld, lda, sld), halve the wanted tile size mt (1 | 2 | 4: 16 mt envs per
// workgroup) until its LDS fits, and launch.  LBSIM_OK / LBSIM_EDEVICE / LBSIM_ENOTSUP.
int launch_sac_actor(SacActorArgs& a, int64_t B, int mt, hipStream_t s);
// form: 0 = layer-split tile kernel, 1 = one wave per agent, 2 = two waves per agent where the
// kernel has that form (A = 4), else one; forms 1 and 2 need mt = 1 after the back-off, else the
// tile kernel runs.
int launch_qmix_policy(QmixArgs& a, int64_t B, int form, int mt, hipStream_t s);

}  // namespace lbk
