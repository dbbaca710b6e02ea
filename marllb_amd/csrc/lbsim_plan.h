// lbsim_plan.h — which kernels a handle's step and reset launch, and with what grid.  make_plan()
// is the only place a dispatch condition is written: lbsim_create calls it once (every input is
// fixed by then) and keeps the StepPlan in the handle; lbsim_dynamics_kernel, lbsim_step_ex and
// lbsim_reset_ex read it, the launchers (lbsim_dyn.hip, lbsim_obs.hip, lbsim_step.hip) turn it
// into template arguments.  What a call decides stays with the call: facade outputs, the reset
// mask, step vs reset.  Plain host C++17 with no HIP header (lbsim_pool.h is one too): tests/plan_probe.cpp compiles it alone
// and tests/test_step_plan.py checks it against tests/golden/step_plan.jsonl without a GPU.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/lbsim.h"
#include "lbsim_pool.h"

namespace lbk {

// The simulator's dispatch overrides (tests, bench.py and the A/B tools set them).  The API reads
// them once per process.
struct Overrides {
  bool group_lanes_set = false;  // LBSIM_DYN_GROUP_LANES set at all: no wave kernel, valid or not
  int group_lanes = 0;           // its value; 4 | 8 | 16 | 32 | 64 and >= S forces the group width
  int dyn_wave = -1;             // LBSIM_DYN_WAVE: 0 never the wave kernel, 1 at every batch size
  int dyn_epw = 0;               // LBSIM_DYN_EPW: envs per wave of the two-launch group dynamics
  int step_kernel = LBSIM_STEP_AUTO;  // LBSIM_STEP_KERNEL=split|fused, for configs that say AUTO
  int step_wave_occ = 0;         // LBSIM_STEP_WAVE_OCC = 2 | 4: one step_wave_kernel form

  static Overrides from_env() {
    const auto num = [](const char* name, int dflt) {
      const char* e = std::getenv(name);
      return e ? std::atoi(e) : dflt;
    };
    Overrides o;
    o.group_lanes_set = std::getenv("LBSIM_DYN_GROUP_LANES") != nullptr;
    o.group_lanes = num("LBSIM_DYN_GROUP_LANES", 0);
    o.dyn_wave = num("LBSIM_DYN_WAVE", -1);
    o.dyn_epw = num("LBSIM_DYN_EPW", 0);
    const char* k = std::getenv("LBSIM_STEP_KERNEL");
    if (k != nullptr && std::strcmp(k, "split") == 0) o.step_kernel = LBSIM_STEP_SPLIT;
    if (k != nullptr && std::strcmp(k, "fused") == 0) o.step_kernel = LBSIM_STEP_FUSED;
    o.step_wave_occ = num("LBSIM_STEP_WAVE_OCC", 0);
    return o;
  }
};

// What the plan depends on: fixed when the handle is created, but for flow_stats,
// cross_traffic, server_workers and action_delay (set before the first reset) and work_tables (the plan is made again when tables
// come into force or are cleared).
struct PlanInput {
  int B, S, Q;
  int policy;       // lbsim_assign_policy
  bool trace;       // arrival_source TRACE
  bool fail;        // fail_thr != 0: server failures
  bool leak;        // n_flow_on_mode VPP's lost-flow counts
  bool split;       // lost-FIN deferral (split reservoirs, pending guesses)
  bool res_vpp;     // reservoir_mode VPP
  bool dur_plane;   // the state has a duration plane (duration_mode SERVICE or lost FINs)
  bool next_reset;  // next-step auto-reset
  int dyn_mapping;  // lbsim_dyn_mapping
  int step_kernel;  // lbsim_step_kernel
  int simds;        // SIMDs of the device (CUs x 4)
  bool flow_stats;  // exact flow statistics are on (lbsim_flow_stats_enable)
  bool work_tables;  // workload tables are in force (lbsim_set_workload_tables)
  bool cross_traffic = false;  // hidden cross traffic is on (lbsim_cross_traffic_enable)
  bool server_workers = false;  // multi-worker servers are on (lbsim_server_workers_enable)
  bool action_delay = false;  // action latency is on (lbsim_action_delay_enable)
  int pool = 0;  // balancers per shared server pool (lbsim_server_pool_enable); 0: no pools
  bool ps = false;  // processor-sharing servers (lbsim_processor_sharing_enable)
  bool pool_ps = false;  // the pools' servers are processor-sharing ones (lbsim_server_pool_enable_ps)
  bool ack_samples = false;  // duration samples at every data ACK (lbsim_ack_samples_enable)
};

enum StepForm { kStepWave, kStepGroupFused, kStepTwoLaunch };
enum ObsForm { kObsPair, kObsPair16, kObsPairChunks, kObsSplit, kObsReset8, kObsChunked };

constexpr int kObsChunkServers = 4;     // kObsChunk
constexpr int kObsScratchBytes = 7840;  // sizeof(ObsScratch): one chunk wave's dynamic LDS
constexpr int kObsReset8Envs = 8;       // kObsResetEnvs
// Envs of more than kObserveSplitS servers observe in two launches (observe_chunks_kernel +
// observe_rows_kernel) instead of one workgroup of S / 4 waves per env.
constexpr int kObserveSplitS = 16;
// dynamics_kernel's workgroup: 64 envs per wave, kDynWaves<MAXS> waves
constexpr unsigned env_lane_block(int maxs) { return maxs <= 8 ? 256u : 128u; }

struct DynPlan {
  int kernel;   // lbsim_dyn_kernel: LBSIM_DYN_KERNEL_ENV_LANE | _GROUP | _WAVE | _POOL | _PS | _POOL_PS
                // | _ACK
  int width;    // env-lane: MAXS 4 | 8 | 16; group: G lanes per env; wave: NG ring registers;
                // pool: G lanes per pool; ps: G lanes per env
  bool full;    // group: dynamics_group_full_kernel (every feature's code, its own budget)
  int waves;    // group, not full: the WAVES register budget 1 | 4 | 5
  int epw;      // group: envs per wave
  unsigned grid, block;
};

struct ObsPlan {
  int form;      // ObsForm
  int maxs;      // chunked: observe_kernel's MAXS; split / pair-chunks: observe_rows_kernel's
  int nchunks;   // waves per env of the chunk launch (split, pair-chunks) or workgroup (chunked)
  unsigned chunk_grid;        // split / pair-chunks: grid of the first launch (64 lanes each)
  unsigned grid, block, lds;  // the launch that writes the rows; lds: dynamic LDS bytes
};

struct StepPlan {
  int form;        // StepForm
  int width;       // one-launch step: NG (wave) or G (group-fused)
  int occ;         // wave step: 2 | 4 waves per SIMD
  int obs_maxs;    // one-launch step: observe_env_wave's MAXS
  unsigned grid;   // one-launch step: workgroups of 64 lanes
  bool nr;         // a two-launch step runs the dynamics' next-step auto-reset instantiation
  DynPlan dyn, reset_dyn;  // dyn also says what lbsim_dynamics_kernel reports
  ObsPlan obs, reset_obs;  // a reset is always two launches
};

inline StepPlan make_plan(const PlanInput& in, const Overrides& ov) {
  const int S = in.S;
  const int64_t B = in.B, simds = in.simds;
  const auto blocks = [](int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); };
  StepPlan p{};

  // One wave per env (lbsim_dyn_wave.h): S <= 8, Q <= 32, SED / SED2 / LSQ / LSQ2 and the default
  // mapping.  Server failures and n_flow_on_mode VPP's lost-flow counts run the group / env-lane
  // kernels; lost-FIN deferral and reservoir_mode VPP the group kernel.  LBSIM_DYN_WAVE = 0
  // disables the wave kernel, and so does LBSIM_DYN_GROUP_LANES, whatever its value.
  // Flow statistics are accumulated by the lane that owns a server for the whole launch (no
  // atomics, bitwise reproducible): only the server-per-lane kernel's full form has that code, so
  // a statistics handle plans exactly as a reservoir_mode VPP one does.
  // Workload tables: their lookups are compiled into the full form alone (the runtime test in the
  // shared instantiations moved the headline kernel's registers).
  // Cross traffic: the hidden flows' decision, flag and count are compiled into the full form alone.
  // Multi-worker servers: so are the start rule and the sorted insert.
  // Action latency: so are the weight ring and the mid-step switch.
  // ACK samples: so are the ACK inserts, in instantiations of their own.
  const bool full_only = in.res_vpp || in.flow_stats || in.work_tables || in.cross_traffic ||
                         in.server_workers || in.action_delay || in.ack_samples;
  // Shared server pools: dynamics_pool_kernel for step and reset, one group of
  // pow2 >= max(S, A) lanes per pool (LBSIM_DYN_GROUP_LANES = 4 | 8 | 16 where it holds both), and
  // the ordinary two-launch observe: no wave kernel, no one-launch step.
  const bool pool = in.pool > 0;
  // Processor-sharing servers: dynamics_ps_kernel for step and reset, one group
  // of pow2 >= S lanes per env (LBSIM_DYN_GROUP_LANES forces the width as for the FIFO groups), and
  // the ordinary two-launch paired observe: no wave kernel, no env-per-lane kernel, no one-launch
  // step.
  const bool ps = in.ps;
  const bool wave_fits = !pool && !ps && ov.dyn_wave != 0 && !ov.group_lanes_set &&
                         in.dyn_mapping != LBSIM_DYN_ENV_PER_LANE && S <= 8 && in.Q <= 32 &&
                         in.policy != LBSIM_POLICY_ALIAS && !in.fail && !in.leak && !in.split &&
                         !full_only;
  // ... and a batch small enough that one env's event-loop chain, not issue throughput, sets the
  // step time: at most 4 waves (envs) per SIMD for S <= 4 (B <= 4096 on 256 CUs), 2 for S <= 8.
  // Measured dynamics, wave vs server-per-lane groups (profiles/r03w/wave_sweep*.txt): S = 4 1024
  // envs 0.041 vs 0.084 ms, 4096 0.066 vs 0.090, 8192 0.108 vs 0.095 (8 waves per SIMD:
  // issue-bound, the groups win); S = 8 2048 envs 0.058 vs 0.078, 4096 0.087 vs 0.083.
  // LBSIM_DYN_WAVE = 1 uses it at every batch size.
  const bool wave_ok = wave_fits && (ov.dyn_wave == 1 || B <= (S <= 4 ? 4 : 2) * simds);
  const int ng = S <= 2 ? 1 : S <= 4 ? 2 : 4;  // ring registers: two servers of 32 positions each

  // Lanes per env of the server-per-lane dynamics; 0: one lane per env, which has to be asked for
  // (LBSIM_DYN_AUTO is one lane per server: with arrivals drawn G at a time it is faster at every
  // measured shape, profiles/r02_round2/mapping_sweep.jsonl: 65536 x 4 0.182 vs 0.214 ms,
  // 131072 x 4 0.316 vs 0.402, 65536 x 8 0.267 vs 0.320, configs[2] trace replay 0.317 vs 0.381,
  // 16384 x 4 0.117 vs 0.198) and keeps its per-server state in registers / LDS rows sized for
  // S <= 16; split lost-FIN handles and reservoir_mode VPP run the server-per-lane kernel only.
  // LBSIM_DYN_GROUP_LANES forces the width (lanes past S hold no server and only draw arrivals
  // ahead): tests use 4 to run the headline 4-lane kernel on small batches, experiments the wider
  // forms.  Otherwise pow2 >= S, except small batches with S <= 4: 8 lanes when 4-lane groups
  // would give at most one wave per two SIMDs (B <= 8192 on 256 CUs) -- twice the waves for SIMDs
  // that would sit idle, the draw-ahead spread over 8 lanes: 4096 x 4 0.0908 -> 0.0894 ms,
  // 8192 x 4 0.0962 -> 0.0947 (profiles/r02_round2b/ab_group_lanes_small.txt); slower from 16384
  // envs on.
  const int fl = ov.group_lanes;
  int g = 8;
  if (in.dyn_mapping == LBSIM_DYN_ENV_PER_LANE && S <= 16 && !in.split && !full_only) g = 0;
  else if (fl >= S && (fl == 4 || fl == 8 || fl == 16 || fl == 32 || fl == 64)) g = fl;
  else if (S <= 2) g = 2;
  else if (S <= 4) g = B * 4 / 64 <= in.simds / 2 ? 8 : 4;
  else while (g < S) g <<= 1;
  // a full handle (n_flow_on_mode VPP, a duration plane, lost-FIN deferral, reservoir_mode VPP,
  // flow statistics)
  const bool full = in.leak || in.dur_plane || full_only;

  const auto dynamics = [&](bool step) {
    DynPlan d{};
    if (pool) {
      const int pg = pool_group_lanes(S, in.pool, fl);
      // (pools of processor-sharing servers, DESIGN.md §3.24: dynamics_pool_ps_kernel, the same
      // groups and grid)
      const int kernel = in.pool_ps ? LBSIM_DYN_KERNEL_POOL_PS : LBSIM_DYN_KERNEL_POOL;
      d = {kernel, pg, false, 0, 64 / pg, blocks(B / in.pool, 64 / pg), 64u};
    } else if (ps) {
      int pg = 2;
      if (fl >= S && (fl == 4 || fl == 8 || fl == 16 || fl == 32 || fl == 64)) pg = fl;
      else while (pg < S) pg <<= 1;
      d = {LBSIM_DYN_KERNEL_PS, pg, false, 0, 64 / pg, blocks(B, 64 / pg), 64u};
    } else if (wave_ok) {
      d = {LBSIM_DYN_KERNEL_WAVE, ng, false, 0, 0, (unsigned)B, 64u};
    } else if (g == 0) {
      const int maxs = S <= 4 ? 4 : S <= 8 ? 8 : 16;
      d = {LBSIM_DYN_KERNEL_ENV_LANE, maxs, false, 0, 0, blocks(B, env_lane_block(maxs)),
           env_lane_block(maxs)};
    } else {
      // LBSIM_DYN_EPW (1 .. 64 / G) runs fewer envs per wave, more waves
      const int epw = ov.dyn_epw >= 1 && ov.dyn_epw <= 64 / g ? ov.dyn_epw : 64 / g;
      d = {LBSIM_DYN_KERNEL_GROUP, g, full, 1, epw, blocks(B, epw), 64u};
      // The step of a next-step auto-reset handle inlines the event loop twice (the reset's
      // warm-up and the step): unconstrained it took 133-137 VGPRs, 3 waves per SIMD, and ran
      // 190 us against the plain step's 149 at 65536 x 4 (profiles/r06b/modes): the 4-wave budget.
      // A plain step grid of more than 4 waves per SIMD: the 5-wave budget (SED, 4 / 8 lanes; it
      // costs 9 % at exactly 4 per SIMD, profiles/r03/ab_dyn_round_keys.txt).
      if (full) d.waves = 0;
      else if (step && in.next_reset) d.waves = 4;
      else if (step && in.policy == LBSIM_POLICY_SED && (g == 4 || g == 8) && d.grid > 4 * simds)
        d.waves = 5;
      // ACK samples: dynamics_group_ack_kernel, the full form's groups and grid
      if (in.ack_samples) d.kernel = LBSIM_DYN_KERNEL_ACK;
    }
    return d;
  };
  p.dyn = dynamics(true);
  p.reset_dyn = dynamics(false);
  p.nr = in.next_reset;

  // The step kernel a handle asks for: its config, else LBSIM_STEP_KERNEL, else AUTO.  Next-step
  // auto-reset handles step in two launches (the dynamics' kModeStepNR instantiation).
  const int k = in.step_kernel != LBSIM_STEP_AUTO ? in.step_kernel : ov.step_kernel;
  p.form = kStepTwoLaunch;
  // The one-launch wave step (step_wave_kernel): FUSED asked for, or AUTO on batches of at most 4
  // envs per SIMD, where one launch instead of two pays: 2048 x 4 0.0711 -> 0.0620 ms per step,
  // 4096 x 4 +2.5 % (profiles/r03w/ab_step_wave_fused.txt).  S = 5-8 between 2 and 4 envs per
  // SIMD: the wave dynamics alone lose to the server-per-lane groups there (wave_ok), the one
  // launch with both chunks observed in it wins (profiles/r04s/).
  if (wave_fits && !in.next_reset &&
      (k == LBSIM_STEP_FUSED ? wave_ok : k == LBSIM_STEP_AUTO && B <= 4 * simds)) {
    p.form = kStepWave;
    p.width = ng;
    // OCC 2 (the VALU queue counts, the shorter chain) up to 2 envs per SIMD, else 4 (the scalar
    // counts; profiles/r03w/ab_step_wave_fused.txt); LBSIM_STEP_WAVE_OCC forces one form at every
    // batch size (the parity tests run the OCC-4 kernel that serves BASELINE configs[1]'s
    // 4096 x 4 on every small-batch case).
    const bool occ2 = ov.step_wave_occ == 2 || (ov.step_wave_occ != 4 && B <= 2 * simds);
    p.occ = occ2 ? 2 : 4;
    p.obs_maxs = ng == 4 ? 8 : kObsChunkServers;  // S = 5-8: both chunks
    p.grid = (unsigned)B;
  } else if (k == LBSIM_STEP_FUSED && !pool && !ps && !in.next_reset && !full && g >= 2 && g <= 16) {
    // The group-fused step is opt-in (AUTO = SPLIT: it measured slower at every shape tried,
    // DESIGN.md §5), not for full handles, and has no form for S > 16 or one lane per env.  It
    // runs 64 / G envs per wave whatever LBSIM_DYN_EPW says.
    p.form = kStepGroupFused;
    p.width = g;
    p.obs_maxs = g < 4 ? 4 : g;
    p.grid = blocks(B, 64 / g);
  }

  const int nw = (S + kObsChunkServers - 1) / kObsChunkServers;  // one wave per 4-server chunk
  const auto observe = [&](bool step) {
    ObsPlan o{};
    // The paired step observe: no duration plane (duration == fct by construction: duration_mode
    // AGE, lost-FIN off) and 8 rows per wave: S <= 8 (8 / S whole envs per wave:
    // observe_pair_kernel), or S a multiple of 8 (S / 8 waves per env: observe_pair16_kernel,
    // observe_pair_chunks_kernel + observe_rows_kernel).
    // (ACK samples: the duration reservoir has records and a count of its own: the general observe)
    if (step && !in.dur_plane && !in.ack_samples && (S <= 8 || S % 8 == 0)) {
      if (S <= 8) o = {kObsPair, 0, 0, 0u, blocks(B, 8 / S), 64u, 0u};
      else if (S == 16) o = {kObsPair16, 0, 0, 0u, (unsigned)B, 128u, 0u};
      else o = {kObsPairChunks, 64, S / 8, (unsigned)(B * (S / 8)), (unsigned)B, 64u, 0u};
    } else if (S > kObsChunkServers && S > kObserveSplitS) {
      o = {kObsSplit, S <= 8 ? 8 : S <= 16 ? 16 : 64, nw, (unsigned)(B * nw), (unsigned)B, 64u, 0u};
    } else if (!step && S <= kObsChunkServers) {  // 8 single-wave envs per workgroup
      o = {kObsReset8, 0, 0, 0u, blocks(B, kObsReset8Envs), 64u * kObsReset8Envs,
           (unsigned)(kObsReset8Envs * kObsScratchBytes)};
    } else {  // the chunks of an env in one workgroup, each with its own ObsScratch
      o = {kObsChunked, S <= 4 ? 4 : S <= 8 ? 8 : S <= 16 ? 16 : 64, nw, 0u, (unsigned)B,
           64u * nw, (unsigned)(nw * kObsScratchBytes)};
    }
    return o;
  };
  p.obs = observe(true);
  p.reset_obs = observe(false);
  return p;
}

}  // namespace lbk
