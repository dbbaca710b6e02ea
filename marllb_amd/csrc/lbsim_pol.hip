// lbsim_pol.hip — launchers of the one-kernel policy networks (lbsim_fused.h).
#include <algorithm>

#include "lbsim_internal.h"
#include "lbsim_fused.h"

namespace lbk {
namespace {

template <typename Args>
int launch_fused(void (*kern)(Args), int64_t B, int mt, size_t lds, hipStream_t s, Args a,
                 unsigned threads = 256) {
  const void* f = reinterpret_cast<const void*>(kern);
  if (lds > 65536 &&
      hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return LBSIM_EDEVICE;
  void* args[] = {&a};
  const dim3 grid((unsigned)((B + 16 * mt - 1) / (16 * mt))), block(threads);
  return hipLaunchKernel(f, grid, block, args, lds, s) == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

}  // namespace

int launch_sac_actor(SacActorArgs& a, int64_t B, int mt, hipStream_t s) {
  constexpr int H = 128, F = 256;
  a.ld = fused_ld(std::max(a.kxp + H, F));
  while (mt > 1 && sac_actor_lds_bytes(mt, a.ld, a.A) > kFusedLdsMax) mt >>= 1;
  const size_t lds = sac_actor_lds_bytes(mt, a.ld, a.A);
  if (mt == 4) return launch_fused(&sac_actor_kernel<4, H, F>, B, 4, lds, s, a);
  if (mt == 2) return launch_fused(&sac_actor_kernel<2, H, F>, B, 2, lds, s, a);
  return launch_fused(&sac_actor_kernel<1, H, F>, B, 1, lds, s, a);
}

int launch_qmix_policy(QmixArgs& a, int64_t B, int form, int mt, hipStream_t s) {
  constexpr int H = 64, F = 128;
  a.ld = fused_ld(std::max({a.kxp + H, F, a.ksp, 3 * a.he + a.E}));
  while (mt > 1 && qmix_policy_lds_bytes(mt, a.ld, a.A) > kFusedLdsMax) mt >>= 1;
  if (mt == 1 && form != 0) {  // one or two waves per agent, 16 envs per workgroup
    a.lda = fused_ld(std::max(a.kxp + H, F));
    // the mixer's [16][ld] tile lies over the four [16][lda] agent regions
    if (a.ld > 4 * a.lda) return LBSIM_ENOTSUP;
    if (form == 2 && a.A == 4) {  // two waves per agent: 8-wave workgroups
      // the mixer's state rows are staged at the start when they fit (sld = 0: staged by the
      // mixer, as in the other forms)
      a.sld = fused_ld(a.ksp);
      if (qmix_pair_lds_bytes(a.lda, a.A, a.sld) > kFusedLdsMax) a.sld = 0;
      const size_t lds = qmix_pair_lds_bytes(a.lda, a.A, a.sld);
      if (lds > kFusedLdsMax) return LBSIM_ENOTSUP;
      return launch_fused(&qmix_agent_pair_kernel<H, F>, B, 1, lds, s, a, 512);
    }
    const size_t lds = qmix_wave_lds_bytes(a.lda, a.A);
    if (lds > kFusedLdsMax) return LBSIM_ENOTSUP;
    return launch_fused(&qmix_agent_wave_kernel<H, F>, B, 1, lds, s, a);
  }
  const size_t lds = qmix_policy_lds_bytes(mt, a.ld, a.A);
  if (mt == 4) return launch_fused(&qmix_policy_kernel<4, H, F>, B, 4, lds, s, a);
  if (mt == 2) return launch_fused(&qmix_policy_kernel<2, H, F>, B, 2, lds, s, a);
  return launch_fused(&qmix_policy_kernel<1, H, F>, B, 1, lds, s, a);
}

}  // namespace lbk

#if LBSIM_EXP_PHASES
// timing diagnostic (lbsim_fused.h LB_PHASE): the last policy launch's phase clocks, 64 x 16 u64
extern "C" int lbsim_exp_phase_read(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(lbk::lbsim_exp_ts), sizeof(lbk::lbsim_exp_ts)) ==
                 hipSuccess
             ? 0
             : -1;
}
#endif
