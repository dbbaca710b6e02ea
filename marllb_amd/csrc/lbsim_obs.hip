// lbsim_obs.hip — observe launchers: one wave per 4-server chunk, each with its own
// ObsScratch in dynamic LDS; which form serves a handle, and its grid: ObsPlan (lbsim_plan.h).
#include "lbsim_internal.h"

namespace lbk {
namespace {

static_assert(kObsChunkServers == kObsChunk && kObsReset8Envs == kObsResetEnvs &&
              kObsScratchBytes == sizeof(ObsScratch), "lbsim_plan.h sizes the observe launches");

template <int MODE>
void launch_observe_m(const LaunchCtx& L, const ObsOutputs& o, const uint8_t* mask,
                      hipStream_t stream) {
  const ObsPlan& ob = MODE == kModeStep ? L.plan.obs : L.plan.reset_obs;
  const dim3 grid(ob.grid), block(ob.block), chunk_grid(ob.chunk_grid);
  // the problem-05 facade rows (agent_obs / state) come from their own instantiation
  pick_bool(o.agent_obs != nullptr || o.state != nullptr, [&](auto F) {
    constexpr bool FAC = decltype(F)::value;
    switch (ob.form) {
      case kObsPair:  // 8 rows per wave: 8 / S envs
        LBSIM_LAUNCH((observe_pair_kernel<MODE, FAC>), grid, block, 0, stream, L.st, L.prm, o);
        return;
      case kObsPair16:  // 8 rows per wave, two waves per env
        if constexpr (MODE == kModeStep)
          LBSIM_LAUNCH((observe_pair16_kernel<MODE, FAC>), grid, block, 0, stream, L.st, L.prm, o);
        return;
      case kObsPairChunks:  // S / 8 waves per env, then the rows (every env: no mask)
      case kObsSplit:       // S / 4 waves per env, then the rows
        if (ob.form == kObsSplit) {
          LBSIM_LAUNCH(observe_chunks_kernel<MODE>, chunk_grid, dim3(64), 0, stream, L.st, L.prm,
                       o, mask, ob.nchunks);
        } else if constexpr (MODE == kModeStep) {
          LBSIM_LAUNCH(observe_pair_chunks_kernel<MODE>, chunk_grid, dim3(64), 0, stream, L.st,
                       L.prm, o, ob.nchunks);
        }
        pick<8, 16, 64>(ob.maxs, [&](auto M) {
          LBSIM_LAUNCH((observe_rows_kernel<decltype(M)::value, MODE, FAC>), grid, block, 0, stream,
                       L.st, L.prm, o, ob.form == kObsSplit ? mask : nullptr);
        });
        return;
      case kObsReset8:  // kObsResetEnvs single-wave envs per workgroup
        LBSIM_LAUNCH(observe_reset_kernel<FAC>, grid, block, ob.lds, stream, L.st, L.prm, o, mask);
        return;
      default:  // kObsChunked: the chunks of an env in one workgroup
        if (ob.lds > 65536) {  // S > 32: 9-16 chunk waves
          static const bool ok = hipFuncSetAttribute(
              reinterpret_cast<const void*>(&observe_kernel<64, MODE, FAC>),
              hipFuncAttributeMaxDynamicSharedMemorySize, 16 * (int)sizeof(ObsScratch)) == hipSuccess;
          (void)ok;
        }
        pick<4, 8, 16, 64>(ob.maxs, [&](auto M) {
          LBSIM_LAUNCH((observe_kernel<decltype(M)::value, MODE, FAC>), grid, block, ob.lds, stream,
                       L.st, L.prm, o, mask);
        });
    }
  });
}

}  // namespace

void launch_observe_step(const LaunchCtx& L, const ObsOutputs& o, const uint8_t* mask,
                         hipStream_t s) {
  launch_observe_m<kModeStep>(L, o, mask, s);
}

void launch_observe_reset(const LaunchCtx& L, const ObsOutputs& o, const uint8_t* mask,
                          hipStream_t s) {
  launch_observe_m<kModeReset>(L, o, mask, s);
}

}  // namespace lbk
