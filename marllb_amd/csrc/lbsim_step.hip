// lbsim_step.hip — the fused steps: one launch per step runs a wave's dynamics and then observes
// the same envs ("fused step").  step_wave_kernel (one wave per env, the default
// for small S <= 4 batches) is below; fused_step_kernel (server-per-lane groups, opt-in):
//
// fused_step_kernel<G, MAXS, POLICY, TRACE>: one 64-lane workgroup = the 64 / G envs of one
// dynamics wave (dyn_group_wave, lbsim_dyn_group.h).  Phase 1 steps them; a workgroup barrier makes
// the wave's state writes visible to its own loads (L1 shared by the workgroup); phase 2 observes
// them one env after the other with observe_env_wave (every chunk of an env by this wave).  The
// dynamics LDS and the observe scratch share one union.  Compared with the two launches:
//   - no dynamics -> observe kernel boundary: a wave whose envs finish their event loops early
//     starts observing while slower waves still simulate (the latency-bound event loop leaves VALU
//     issue slots that the VALU-bound observe fills) instead of the whole chip draining first;
//   - the reservoir records observe reads were written microseconds earlier by the same CU: L2
//     hits instead of a second HBM pass over the state.
// Same routines in the same order per env, so the same bits as the two-launch step (tested).
#include "lbsim_internal.h"
#include "lbsim_dyn_group.h"
#include "lbsim_dyn_wave.h"


namespace lbk {
namespace {

template <int G, int MAXS, int POLICY, bool TRACE>
__global__ void __launch_bounds__(64)
    fused_step_kernel(DevState st, SimParams p, const void* action, int action_dtype,
                      int32_t* assign_out, ObsOutputs out) {
  __shared__ union {
    DynGroupLds<POLICY> dyn;
    ObsScratch obs;
  } L;
  __shared__ float s_obs[MAXS * NF];
  __shared__ float s_act[MAXS];
  const int lane = (int)threadIdx.x;
  dyn_group_wave<G, kModeStep, POLICY, TRACE>(st, p, action, action_dtype, assign_out, nullptr,
                                              blockIdx.x, lane, L.dyn);
  __syncthreads();  // state stores complete and visible to this workgroup; LDS reused below
  constexpr int EPW = 64 / G;
  for (int i = 0; i < EPW; ++i) {
    const size_t b = (size_t)blockIdx.x * EPW + (size_t)i;
    if (b >= (size_t)p.B) break;
    observe_env_wave<MAXS>(st, p, out, b, L.obs, s_obs, s_act, lane);
  }
}

// The small-batch step (kStepWave: S <= 8, at most 4 envs per SIMD): one wave per env steps it
// (dyn_wave_env) and then observes it (observe_env_wave: one chunk for S <= 4, two for 5-8), so the
// step is ONE launch and each env's observation runs as soon as its own event loop ends, while
// slower envs still simulate.  Same routines, same order: the same bits as the two launches.
// OCC waves per SIMD.  2: batches of at most 2 envs per SIMD, with the VALU queue counts (the
// shorter chain).  4: 2-4 envs per SIMD, with the scalar counts (profiles/r03w/ab_step_wave_fused.txt).
// Both take 118-120 VGPRs with no spill since the one-chunk observe is straight-line code (the
// chunk loop took 194 and spilled 64 under the 128 cap: profiles/r03o/).  Out of line, the observe
// phase's call frames went through 1 KB of scratch per lane (0.141 ms).
// MAXS = 8 (S = 5-8): the wave dynamics' S <= 8 form, then both chunks, one after the other, in a
// rolled loop whose inputs are opaque to the compiler (observe_env_wave), so that no chunk-invariant
// value is held across the two: 124 VGPRs, no scratch, hence OCC 4 too (hoisted, 170 and 184 B of
// spills per lane at the 128 cap).
template <int NG, int POLICY, bool TRACE, int OCC, int MAXS = kObsChunk>
__global__ void __launch_bounds__(64, OCC)
    step_wave_kernel(DevState st, SimParams p, const void* action, int action_dtype,
                     int32_t* assign_out, ObsOutputs out) {
  __shared__ union {
    WaveLds dyn;
    ObsScratch obs;
  } L;
  __shared__ float s_obs[MAXS * NF];
  __shared__ float s_act[MAXS];
  const int lane = (int)threadIdx.x;
  if (!dyn_wave_env<NG, kModeStep, POLICY, TRACE, OCC == 2>(st, p, action, action_dtype,
                                                            assign_out, nullptr, blockIdx.x, lane,
                                                            L.dyn))
    return;
  __syncthreads();  // state stores complete and visible to this workgroup; LDS reused below
  observe_env_wave<MAXS>(st, p, out, blockIdx.x, L.obs, s_obs, s_act, lane);
}

}  // namespace

// StepPlan (lbsim_plan.h) form kStepWave: width = NG, occ, obs_maxs (4, or 8 with NG = 4: S = 5-8,
// both chunks -- the pairs that are instantiated); no ALIAS.
void launch_step_wave(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                      const ObsOutputs& o, hipStream_t s) {
  const StepPlan& p = L.plan;
  pick<1, 2, 4>(p.width, [&](auto N) { pick<0, 1, 2, 3>(L.prm.policy, [&](auto P) {
    pick_bool(L.prm.trace != 0, [&](auto T) { pick<2, 4>(p.occ, [&](auto OCC) {
      constexpr int NG = decltype(N)::value;
      LBSIM_LAUNCH((step_wave_kernel<NG, decltype(P)::value, decltype(T)::value,
                                     decltype(OCC)::value, (NG == 4 ? 8 : kObsChunk)>),
                   dim3(p.grid), dim3(64), 0, s, L.st, L.prm, action, dtype, assign, o);
    }); });
  }); });
}

// Form kStepGroupFused: width = G <= 16, obs_maxs = max(G, 4); 64 / G envs per wave (dyn_epw 0).
void launch_fused_step(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                       const ObsOutputs& o, hipStream_t s) {
  const StepPlan& p = L.plan;
  pick<2, 4, 8, 16>(p.width, [&](auto GG) { pick<0, 1, 2, 3, 4>(L.prm.policy, [&](auto P) {
    pick_bool(L.prm.trace != 0, [&](auto T) {
      constexpr int G = decltype(GG)::value;
      LBSIM_LAUNCH((fused_step_kernel<G, (G < 4 ? 4 : G), decltype(P)::value, decltype(T)::value>),
                   dim3(p.grid), dim3(64), 0, s, L.st, L.prm, action, dtype, assign, o);
    });
  }); });
}

}  // namespace lbk
