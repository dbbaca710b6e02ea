// lbsim_api.hip — extern "C" boundary of liblbsim (include/lbsim.h) over the gfx950 kernels.
//
// The handle owns the device state (one hipMalloc per section, SoA); the caller
// owns every I/O buffer.  No allocation, no host synchronisation and no host<->device copy
// happens inside lbsim_reset / lbsim_step, so a caller may capture them into a hipGraph.
#include <hip/hip_runtime.h>

#include <cxxabi.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define LBSIM_CROSS_KERNELS  // cross_convert_kernel is defined in this object (lbsim_cross.h)
#define LBSIM_WORKERS_KERNELS  // and workers_convert_kernel (lbsim_workers.h)
#define LBSIM_DELAY_KERNELS  // and delay_convert_kernel / delay_gather_kernel (lbsim_delay.h)
#include "../../include/lbsim.h"
#include "lbsim_avail.h"
#include "lbsim_internal.h"
#include "lbsim_fused.h"
#include "lbsim_nets.h"
#include "lbsim_ps.h"
#include "lbsim_snapshot.h"
#include "lbsim_stateless.h"
#include "lbsim_truth.h"
#include "lbsim_vpp.h"

using namespace lbk;

// The launch log of LBSIM_LAUNCH (lbsim_internal.h): (profile class, host stub) of each kernel
// the API call in progress launched.  The calls that launch simulator kernels set the class
// before each launch; a scoped LaunchLog copies the log into the handle when the call returns.
namespace {
constexpr int kLogMax = 8;
thread_local const void* g_log_fn[kLogMax];
thread_local int g_log_cls[kLogMax];
thread_local int g_log_n = 0;
thread_local int g_log_lost = 0;  // launches past kLogMax (reported, not dropped silently)
thread_local int g_log_class = -1;
}  // namespace

void lbk::note_launch(const void* host_fn) {
  if (g_log_n < kLogMax) {
    g_log_fn[g_log_n] = host_fn;
    g_log_cls[g_log_n] = g_log_class;
    ++g_log_n;
  } else {
    ++g_log_lost;
  }
}

struct Profiler {
  bool on = false;
  std::vector<hipEvent_t> ev;  // at most 2 per timed launch
  std::vector<int> cls;        // kernel class per timed launch
  std::vector<int> beg, end;   // event indices bracketing each timed launch
  size_t used = 0;             // events recorded
  size_t cap = 0;              // events this profile may record (2 per requested launch)
  // lbsim_step: the event that ends the dynamics launch also starts the observe launch (one
  // event between the two kernels instead of two)
  bool chain = false;
  int chain_ev = -1;
};

struct lbsim {
  lbsim_config_t cfg;
  Profiler prof;
  int device;
  int simds;  // SIMDs of the device (CUs x 4): the env-per-lane mapping fills them at B >= 64·simds
  int B, S, Q;
  DevState st;
  SimParams prm;
  StepPlan plan;  // which kernels a step / reset launches (lbsim_plan.h): made once, at create
  std::vector<void*> allocs;
  void* trace_buf = nullptr;  // gap_us[rows] then work[rows]
  // the bank in trace_buf (lbsim_set_trace: one trace): its row offsets (T + 1; empty: no trace
  // set), and their device copy as u32, made when a selection first needs it
  std::vector<int64_t> bank_begin;
  uint32_t* bank_begin_dev = nullptr;
  // lbsim_set_trace_schedule: the selection's block for tsel_alloc_P phases (TraceSelBuf below),
  // moved only by a call with another P, and the selection in force: tsel_P phases (0: none),
  // each held for tsel_H steps, cyclic or clamped.
  void* tsel_buf = nullptr;
  int tsel_alloc_P = 0;
  int tsel_P = 0, tsel_H = 0, tsel_wrap = 0;
  unsigned long long* stats_buf = nullptr;  // lbsim_step_stats sums (2 x u64)
  // lbsim_set_env_rates: one block, allocated by the first call and never moved (EnvRates below)
  float* rates_buf = nullptr;
  bool rates_on = false;  // per-env rates are set (what dropping a schedule goes back to)
  // lbsim_set_rate_schedule: the tables' block for sched_alloc_P phases (sched_floats below),
  // moved only by a call with another P, and the schedule in force: sched_P phases (0: none), each
  // held for sched_H steps, cyclic or clamped.
  float* sched_buf = nullptr;
  int sched_alloc_P = 0;
  int sched_P = 0, sched_H = 0, sched_wrap = 0;
  // lbsim_set_workload_tables: the block for wtab_alloc_T tables (WorkTabBuf below), moved only by
  // a call with another T; wtab_T tables in force (0: the closed form) and wtab_wmax, the largest
  // entry of the tables some env uses for work
  void* wtab_buf = nullptr;
  int wtab_alloc_T = 0;
  int wtab_T = 0;
  float wtab_wmax = 0.0f;
  // lbsim_flow_stats_enable: one block (sum_us, hist, count, max_us), allocated once, never moved
  void* flow_buf = nullptr;
  FlowStats flow{};  // its arrays (null pointers: statistics off)
  // lbsim_server_avail_enable: the handle has a down section whatever fail_prob says, and every
  // step starts with avail_apply_kernel.  lbsim_set_server_avail: the table's block for
  // avail_alloc_P phases ([B, P, S] bytes), moved only by a call with another P, and the table in
  // force: avail_P phases (0: none, every server wanted up), each held for avail_H steps, cyclic
  // or clamped.
  bool avail_on = false;
  uint8_t* avail_buf = nullptr;
  int avail_alloc_P = 0;
  int avail_P = 0, avail_H = 0, avail_wrap = 0;
  // lbsim_cross_traffic_enable: one block of u32, allocated once and never moved -- the live
  // thr[B] and cum[B*S] the full dynamics kernel reads (CrossTraffic), their staging copies (a call
  // converts into these and only a valid one is copied over the live arrays), the offender count
  void* cross_buf = nullptr;
  CrossTraffic cross{};  // the live arrays (null pointers: the handle has no cross traffic)
  // lbsim_server_workers_enable: one block of 32-bit words, allocated once and never moved -- the
  // live c[B*S] the full dynamics kernel reads (ServerWorkers), its staging copy and the
  // offender count
  void* workers_buf = nullptr;
  ServerWorkers workers{};  // the live array (a null pointer: every server one FIFO pipe)
  // lbsim_action_delay_enable: one block of 32-bit words, allocated once and never moved -- the
  // weight ring wring[B, R, S] and the live delay_us[B] the full dynamics kernel reads
  // (ActionDelay), the delays' staging copy and the offender count
  void* delay_buf = nullptr;
  ActionDelay delay{};  // the live arrays (null pointers: actions act at once)
  int32_t delay_M = 0;  // max_delay_steps
  // lbsim_server_pool_enable: the physical FIFOs' words and owners (two state sections after all
  // the others, sections() below) and the widened reset mask, allocated once and never moved
  PoolArrays pool{};  // (A = 0: the handle has no pools)
  // lbsim_server_pool_enable_ps (§3.24): the pools' servers are processor-sharing ones, and
  // lbsim_set_pool_ps_cores' block, as ps_cores_buf below with one row per pool: the live c[C*S]
  // dynamics_pool_ps_kernel reads, its staging copy and the offender count (nullptr: never set)
  bool pool_ps = false;
  int32_t* pool_ps_cores_buf = nullptr;
  bool ps = false;  // lbsim_processor_sharing_enable: processor-sharing servers
  // lbsim_set_ps_cores (§3.23): one block of 32-bit words, allocated by the first call and never
  // moved -- the live c[B*S] the PS dynamics kernel reads, its staging copy and the offender count
  // (nullptr: never set, every server one core)
  int32_t* ps_cores_buf = nullptr;
  // lbsim_ack_samples_enable: max_acks (0: off) and the envs' ACK intervals
  // [B] in us on the device, allocated once and never moved; the enable also allocates the
  // res_dur / res_count_dur state sections (sections() below)
  int32_t ack_max = 0;
  int32_t* ack_us = nullptr;
  bool initialised;  // a full reset has been issued
  bool reset_seen = false;  // any lbsim_reset (or lbsim_set_state) has been issued
  std::string err;
  // (class, host stub) of the kernels the last lbsim_step_ex / lbsim_reset_ex launched
  std::vector<std::pair<int, const void*>> launched[2];
  int launched_lost[2] = {0, 0};  // launches of that call past the log's capacity
};

namespace {

thread_local std::string g_create_err;

int fail(lbsim_t* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (h) h->err = buf;
  else g_create_err = buf;
  return code;
}

// An opt-in refused on a handle with shared server pools (not composed).
const char kPoolNoCompose[] = "%s on a handle with shared server pools "
                              "(lbsim_server_pool_enable): not supported together";

// An opt-in refused on a handle with processor-sharing servers (not composed).
const char kPsNoCompose[] = "%s on a handle with processor-sharing servers "
                            "(lbsim_processor_sharing_enable): not supported together";

// An opt-in refused on a handle with duration samples at every data ACK.
const char kAckNoCompose[] = "%s on a handle with ack samples (lbsim_ack_samples_enable): not "
                             "supported together";

// Scoped hipSetDevice that restores the caller's current device (torch keeps its own).
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int bad_msg(char* msg, size_t n, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int bad_msg(char* msg, size_t n, const char* fmt, ...) {
  if (msg && n) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, n, fmt, ap);
    va_end(ap);
  }
  return LBSIM_EINVAL;
}

int validate(const lbsim_config_t* c, char* msg, size_t n) {
#define bad(...) bad_msg(msg, n, __VA_ARGS__)
  if (c == nullptr) return bad("config is NULL");
  if (c->num_envs < 1) return bad("num_envs must be >= 1 (got %d)", c->num_envs);
  if (c->num_servers < 1 || c->num_servers > LBSIM_MAX_SERVERS)
    return bad("num_servers must be in [1, %d] (got %d)", LBSIM_MAX_SERVERS, c->num_servers);
  if ((int64_t)c->env_id_offset < 0 ||
      (uint64_t)c->env_id_offset + (uint64_t)c->num_envs > 0xFFFFFFFFull)
    return bad("global env ids must fit in 32 bits");
  if (c->action_type != LBSIM_ACTION_DISCRETE && c->action_type != LBSIM_ACTION_CONTINUOUS)
    return bad("Unknown action_type: %d", c->action_type);
  if (c->action_type == LBSIM_ACTION_DISCRETE &&
      (c->num_discrete < 1 || c->num_discrete > LBSIM_MAX_DISCRETE))
    return bad("num_discrete must be in [1, %d]", LBSIM_MAX_DISCRETE);
  if (c->reward_metric < LBSIM_METRIC_JAIN || c->reward_metric > LBSIM_METRIC_GINI)
    return bad("Unsupported metric: %d", c->reward_metric);
  if (c->reward_field < -1 || c->reward_field >= LBSIM_NUM_FEATURES)
    return bad("reward_field must be -1 or a column in [0, 10]");
  if (!(c->step_interval > 0.0f) || c->step_interval > 100.0f)
    return bad("step_interval must be in (0, 100] seconds");
  if ((int64_t)std::llround((double)c->step_interval * 1e6) < 1)
    return bad("step_interval must be >= 1 us");
  if (c->max_steps < 1) return bad("max_steps must be >= 1");
  if (c->assign_policy < LBSIM_POLICY_SED || c->assign_policy > LBSIM_POLICY_ALIAS)
    return bad("unknown assign_policy %d", c->assign_policy);
  if (c->arrival_source != LBSIM_ARRIVAL_POISSON && c->arrival_source != LBSIM_ARRIVAL_TRACE)
    return bad("unknown arrival_source");
  if (!(c->arrival_rate >= 0.1f) || !(c->arrival_rate <= 1.0e6f))
    return bad("arrival_rate must be in [0.1, 1e6] flows/s");
  for (int s = 0; s < c->num_servers; ++s)
    if (!(c->server_rate[s] >= 1.0f) || !(c->server_rate[s] <= 1.0e7f))
      return bad("server_rate[%d] must be in [1, 1e7] flows/s", s);
  if (!(c->decay_factor > 0.0f) || !(c->decay_factor < 1.0f))
    return bad("decay_factor must be in (0, 1)");
  if (c->queue_capacity < 1 || c->queue_capacity > 64)
    return bad("queue_capacity must be in [1, 64]");
  if (c->warmup_steps < 0 || c->warmup_steps > 100000) return bad("warmup_steps out of range");
  if (c->dyn_mapping < LBSIM_DYN_AUTO || c->dyn_mapping > LBSIM_DYN_SERVER_PER_LANE)
    return bad("unknown dyn_mapping %d", c->dyn_mapping);
  if (c->step_kernel < LBSIM_STEP_AUTO || c->step_kernel > LBSIM_STEP_FUSED)
    return bad("unknown step_kernel %d", c->step_kernel);
  if (!(c->lost_fin_prob >= 0.0f) || !(c->lost_fin_prob <= 1.0f))
    return bad("lost_fin_prob must be in [0, 1]");
  if (c->lost_fin_prob > 0.0f) {
    if (!(c->flow_timeout_s >= 0.0f)) return bad("flow_timeout_s must be >= 0");
    if (c->flow_buckets < 1) return bad("flow_buckets must be >= 1");
    // the guess fct + (flow_timeout - 40 s) + wait and its wrap-up delay flow_timeout + wait are
    // signed int32 us: with the wait <= 16.7 x its mean flow_buckets / arrival_rate (24-bit
    // uniforms) and an fct of at most ~1,070 s (64 queued flows of <= 16.7 s service each at
    // >= 1 flow/s), flow_timeout + 16.7 x the mean wait <= 1040 s keeps both below 2^31 us
    // (lost_fct also saturates, for trace work beyond that bound)
    const double wmean = (double)c->flow_buckets / (double)c->arrival_rate;
    if ((double)c->flow_timeout_s + 16.7 * wmean > 1040.0) {
      if ((double)c->flow_timeout_s >= 1040.0)
        return bad("lost-FIN: flow_timeout_s must be < 1040 s (got %.1f)", c->flow_timeout_s);
      return bad("lost-FIN: flow_timeout_s + 16.7 * flow_buckets / arrival_rate must be <= 1040 s "
                 "(signed 32-bit us guesses): with flow_timeout_s = %.1f, flow_buckets / "
                 "arrival_rate must be <= %.3f s (got %.3f)",
                 c->flow_timeout_s, (1040.0 - (double)c->flow_timeout_s) / 16.7, wmean);
    }
    if (c->lost_fin_pending < 1 || c->lost_fin_pending > 4096)
      return bad("lost_fin_pending must be in [1, 4096]");
  }
  if (c->lost_fin_prob > 0.0f && std::llround((double)c->lost_fin_prob * 16777216.0) == 0)
    return bad("lost_fin_prob must be 0 or >= 2^-25 (a 24-bit threshold)");
  if (!(c->fail_prob >= 0.0f) || !(c->fail_prob <= 1.0f)) return bad("fail_prob must be in [0, 1]");
  if (c->fail_prob > 0.0f && std::llround((double)c->fail_prob * 16777216.0) == 0)
    return bad("fail_prob must be 0 or >= 2^-25 (a 24-bit threshold)");
  if (c->next_step_reset != 0 && c->next_step_reset != 1) return bad("next_step_reset must be 0 or 1");
  if (c->duration_mode != LBSIM_DURATION_AGE && c->duration_mode != LBSIM_DURATION_SERVICE)
    return bad("unknown duration_mode %d", c->duration_mode);
  if (c->n_flow_on_mode != LBSIM_NFLOW_QUEUE && c->n_flow_on_mode != LBSIM_NFLOW_VPP)
    return bad("unknown n_flow_on_mode %d", c->n_flow_on_mode);
  if (c->reservoir_mode != LBSIM_RESERVOIR_ALGR && c->reservoir_mode != LBSIM_RESERVOIR_VPP)
    return bad("unknown reservoir_mode %d", c->reservoir_mode);
  if (!(c->recover_prob >= 0.0f) || !(c->recover_prob <= 1.0f))
    return bad("recover_prob must be in [0, 1]");
  if (c->dyn_mapping == LBSIM_DYN_ENV_PER_LANE && c->num_servers > 16)
    return bad("the env-per-lane dynamics mapping takes at most 16 servers (got %d)",
               c->num_servers);
  return LBSIM_OK;
#undef bad
}

void derive_params(const lbsim_config_t& c, SimParams& p) {
  memset(&p, 0, sizeof(p));
  p.B = c.num_envs;
  p.S = c.num_servers;
  p.Q = c.queue_capacity;
  p.dt_us = (int32_t)std::llround((double)c.step_interval * 1e6);
  p.mean_gap_us = (float)(1e6 / (double)c.arrival_rate);
  for (int s = 0; s < MAX_S; ++s)
    p.svc_scale[s] = s < c.num_servers ? (float)(1e6 / (double)c.server_rate[s]) : 0.0f;
  p.key0 = (uint32_t)(c.seed & 0xFFFFFFFFull);
  p.key1 = (uint32_t)(c.seed >> 32);
  p.env_id_offset = (uint32_t)c.env_id_offset;
  p.policy = c.assign_policy;
  p.action_type = c.action_type;
  p.num_discrete = c.num_discrete;
  for (int i = 0; i < 8; ++i) p.dw[i] = c.discrete_weights[i];
  p.min_w = c.min_weight;
  p.max_w = c.max_weight;
  p.warmup_steps = c.warmup_steps;
  p.max_steps = c.max_steps;
  p.reward_metric = c.reward_metric;
  p.reward_field = c.reward_field;
  p.decay_c = (float)(std::log2((double)c.decay_factor) / 1000.0);
  p.normalize = c.normalize_obs ? 1 : 0;
  p.trace = c.arrival_source == LBSIM_ARRIVAL_TRACE ? 1 : 0;
  p.trace_rows = 0;
  p.lf_thr = (uint32_t)std::llround((double)c.lost_fin_prob * 16777216.0);
  p.lf_off_us = (int32_t)(std::llround((double)c.flow_timeout_s * 1e6) - 40000000LL);
  p.lf_wait_us = c.lost_fin_prob > 0.0f
                     ? (float)((double)c.flow_buckets * 1e6 / (double)c.arrival_rate) : 0.0f;
  p.fail_thr = (uint32_t)std::llround((double)c.fail_prob * 16777216.0);
  p.rec_thr = (uint32_t)std::llround((double)c.recover_prob * 16777216.0);
  p.big_in_step = (p.dt_us >= (int32_t)kPackLimit || p.lf_thr != 0u) ? 1 : 0;
  p.next_reset = c.next_step_reset ? 1 : 0;
  p.dur_service = c.duration_mode == LBSIM_DURATION_SERVICE ? 1 : 0;
  p.leak = (c.n_flow_on_mode == LBSIM_NFLOW_VPP && p.lf_thr != 0u) ? 1 : 0;
  p.split = p.lf_thr != 0u ? 1 : 0;
  p.pend_P = p.split ? c.lost_fin_pending : 0;
  p.res_vpp = c.reservoir_mode == LBSIM_RESERVOIR_VPP ? 1 : 0;
}

// Whether a handle keeps a duration plane (DevState::res_dur): duration_mode SERVICE (the service
// time differs from the age) or lost-FIN guesses (their fct differs from the duration).  Otherwise
// every duration sample equals its fct sample, and the duration reservoir is the fct reservoir.
bool dur_plane(const SimParams& p) { return p.dur_service != 0 || p.lf_thr != 0u; }

// State sections in snapshot order.
struct Section {
  void** ptr;
  size_t bytes;
};

std::vector<Section> sections(lbsim_t* h) {
  const size_t B = h->B, BS = (size_t)h->B * h->S, BSQ = BS * h->Q, BSK = BS * K;
  DevState& s = h->st;
  std::vector<Section> v = {
      {(void**)&s.next_arr, B * 4},   {(void**)&s.next_work, B * 4}, {(void**)&s.next_u2, B * 4},
      {(void**)&s.next_u3, B * 4},    {(void**)&s.arr_idx, B * 4},   {(void**)&s.episode, B * 4},
      {(void**)&s.clock, B * 4},      {(void**)&s.ep_step, B * 4},   {(void**)&s.dropped, B * 4},
      {(void**)&s.norm_count, B * 4}, {(void**)&s.ep_return, B * 8}, {(void**)&s.hc, BS * 4},
      {(void**)&s.last_tc, BS * 4},   {(void**)&s.res_count, BS * 4}, {(void**)&s.ring, BSQ * 8},
      {(void**)&s.res, BSK * 8},      {(void**)&s.chg, BS * 16},      {(void**)&s.fcache, BS * 40},
  };
  if (h->cfg.normalize_obs) {
    v.push_back({(void**)&s.norm_mean, BS * NF * 8});
    v.push_back({(void**)&s.norm_std, BS * NF * 8});
  }
  if (h->cfg.fail_prob > 0.0f || s.down != nullptr) v.push_back({(void**)&s.down, BS * 4});
  // (a cross-traffic handle keeps minus its hidden flows there: lbsim_cross_traffic_enable)
  if (h->prm.leak || h->cross_buf != nullptr) v.push_back({(void**)&s.lost_on, BS * 4});
  // the duration plane: only when a flow's duration sample can differ from its fct; split
  // handles (lost-FIN): {us, ts} records, the duration count, the pending guesses, lf_over
  // (an ACK-samples handle, §3.25: {us, ts} records and the duration count, nothing pending)
  const bool ack = h->ack_max > 0;
  if (dur_plane(h->prm) || ack)
    v.push_back({(void**)&s.res_dur, BSK * (h->prm.split || ack ? 8 : 4)});
  if (ack) v.push_back({(void**)&s.res_count_dur, BS * 4});
  if (h->prm.split) {
    v.push_back({(void**)&s.res_count_dur, BS * 4});
    v.push_back({(void**)&s.pend_hc, BS * 4});
    v.push_back({(void**)&s.pend, BS * (size_t)h->prm.pend_P * 8});
    v.push_back({(void**)&s.lf_over, B * 4});
  }
  // shared server pools: the physical FIFO of every (pool, server), after every other section
  if (h->pool.A > 0) {
    const size_t CS = BS / (size_t)h->pool.A;
    v.push_back({(void**)&h->pool.hc, CS * 4});
    v.push_back({(void**)&h->pool.owner, CS * h->Q});
  }
  return v;
}

__global__ void init_norm_std(double* p, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1.0;  // env.py:153 obs_std = ones
}

// lbsim_step_stats: popcount of the written-slot masks and the sum of the queue counts, one
// device-wide sum each (wave shuffles, then one vector atomic per wave).
__global__ void __launch_bounds__(256)
    step_stats_kernel(const uint32_t* chg, const uint32_t* hc, int64_t n_srv,
                      unsigned long long* out) {
  unsigned long long slots = 0, flows = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_srv;
       i += (int64_t)gridDim.x * 256) {
    const uint4 m = reinterpret_cast<const uint4*>(chg)[i];
    slots += __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
    flows += hc[i] >> 16;
  }
  for (int d = 32; d > 0; d >>= 1) {
    slots += __shfl_xor(slots, d, 64);
    flows += __shfl_xor(flows, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out, slots);
    atomicAdd(out + 1, flows);
  }
}

__global__ void copy_episode_stats(const int32_t* steps, const double* ret, int32_t* lo,
                                   double* ro, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  if (lo) lo[i] = steps[i];
  if (ro) ro[i] = ret[i];
}

// Per-env rates (lbsim_set_env_rates).  The handle's block holds, in floats: the live arrays the
// kernels and lbsim_get_env_rates read -- arrival[B], server[B*S] (flows/s as given), gap[B],
// scale[B*S] (us, what the event loops consume) -- then staging copies of the four (a call
// converts into these and only a valid one is copied over the live arrays), the config's own
// rates {arrival, server[MAX_S]}, and the offender count (one u32).
struct EnvRates {
  float *arrival, *server, *gap, *scale;
};
EnvRates env_rates_at(float* base, size_t B, size_t BS) {
  return EnvRates{base, base + B, base + B + BS, base + 2 * B + BS};
}
EnvRates env_rates_live(const lbsim_t* h) {
  return env_rates_at(h->rates_buf, (size_t)h->B, (size_t)h->B * h->S);
}
EnvRates env_rates_staging(const lbsim_t* h) {
  const size_t B = (size_t)h->B, BS = B * h->S;
  return env_rates_at(h->rates_buf + 2 * (B + BS), B, BS);
}
float* env_rates_defaults(const lbsim_t* h) {
  return h->rates_buf + 4 * ((size_t)h->B + (size_t)h->B * h->S);
}
uint32_t* env_rates_bad(const lbsim_t* h) {
  return reinterpret_cast<uint32_t*>(env_rates_defaults(h) + 1 + MAX_S);
}

// Rates (flows/s) to the event loops' constants: mean_gap_us = 1e6 / rate and svc_scale = 1e6 / mu,
// divided in f64 and rounded once to f32 as derive_params does (so an env given the config's own
// rates computes the config's bits).  Element (b, s) of either input is in[b * stride + s]: the
// caller's [B] / [B, S] arrays (strides 1, S) or the config's rates for every env (stride 0).
// Values outside the config's ranges (NaN included) are counted into *bad.  mu_lo: the lower bound
// of a server rate, 1 (the config's) or what the workload tables in force ask for (mu_floor).
__global__ void __launch_bounds__(256)
    env_rates_kernel(const float* arr_in, int64_t arr_stride, const float* srv_in,
                     int64_t srv_stride, int B, int S, EnvRates out, uint32_t* bad, float mu_lo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t off = 0u;
  if (srv_in != nullptr && i < (int64_t)B * S) {
    const int64_t b = i / S;
    const float mu = srv_in[b * srv_stride + (i - b * S)];
    off += (!(mu >= mu_lo) || !(mu <= 1.0e7f)) ? 1u : 0u;
    out.server[i] = mu;
    out.scale[i] = (float)(1e6 / (double)mu);
  }
  if (arr_in != nullptr && i < (int64_t)B) {
    const float r = arr_in[i * arr_stride];
    off += (!(r >= 0.1f) || !(r <= 1.0e6f)) ? 1u : 0u;
    out.arrival[i] = r;
    out.gap[i] = (float)(1e6 / (double)r);
  }
  for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
  if ((threadIdx.x & 63) == 0 && off != 0u) atomicAdd(bad, off);
}

// The same conversion for a rate schedule (lbsim_set_rate_schedule): B * P rows.  Element
// (b, phase, s) of either input is in[b * row_stride + phase * phase_stride (+ s)]: the caller's
// [B, P] / [B, P, S] arrays, one shared schedule (row stride 0), or per-env rates held constant
// over the phases (phase stride 0).  out: tables of N = B * P rows, row b * P + phase.
__global__ void __launch_bounds__(256)
    rate_table_kernel(const float* arr_in, int64_t arr_row, int64_t arr_phase, const float* srv_in,
                      int64_t srv_row, int64_t srv_phase, int B, int P, int S, EnvRates out,
                      uint32_t* bad, float mu_lo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t off = 0u;
  if (i < (int64_t)B * P * S) {
    const int64_t r = i / S, b = r / P;
    const float mu = srv_in[b * srv_row + (r - b * P) * srv_phase + (i - r * S)];
    off += (!(mu >= mu_lo) || !(mu <= 1.0e7f)) ? 1u : 0u;
    out.server[i] = mu;
    out.scale[i] = (float)(1e6 / (double)mu);
  }
  if (i < (int64_t)B * P) {
    const int64_t b = i / P;
    const float r = arr_in[b * arr_row + (i - b * P) * arr_phase];
    off += (!(r >= 0.1f) || !(r <= 1.0e6f)) ? 1u : 0u;
    out.arrival[i] = r;
    out.gap[i] = (float)(1e6 / (double)r);
  }
  for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
  if ((threadIdx.x & 63) == 0 && off != 0u) atomicAdd(bad, off);
}

// The phase of a rate schedule at episode step k (k / H, cyclic or clamped): the rule that
// marllb_amd.randomize.schedule_phase states on the host.  P >= 1, H >= 1.
__device__ __forceinline__ uint32_t sched_phase(int32_t k, uint32_t P, uint32_t H, bool wrap) {
  const uint32_t j = (uint32_t)(k > 0 ? k : 0) / H;
  return wrap ? j % P : (j < P ? j : P - 1u);
}

// The schedule's gather, one thread per (env, server): row b * P + phase of the [B, P] table
// `per_env` and of the [B, P, S] table `per_srv` into env_out[B] / srv_out[B, S], and the phase
// into phase_out[B] (each output optional).  The phase of env b is that of its next step launch,
// from k = ep_step[b], the steps it has completed in its episode: sched_phase(k), or 0 when that
// launch resets the env instead (next-step auto-reset, k >= max_steps).  reset != 0: the launch is
// a reset of the envs of `mask` (nullptr: all), which runs at phase 0; the other envs are skipped.
// It runs in front of every dynamics launch of a scheduled handle (sched_select: the tables' gap
// and scale rows into the per-env arrays the dynamics kernels read) and behind
// lbsim_get_env_rates / lbsim_rate_phase.  P <= 1 (no schedule, or one phase): phase 0, row b.
__global__ void __launch_bounds__(256)
    rate_gather_kernel(const int32_t* ep_step, const uint8_t* mask, int reset, int B, int S, int P,
                       int H, int wrap, int max_steps, int next_reset, const float* per_env,
                       const float* per_srv, float* env_out, float* srv_out, int32_t* phase_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * S) return;
  const int64_t b = i / S;
  if (reset && mask != nullptr && mask[b] == 0) return;
  uint32_t phase = 0u;
  if (P > 1 && !reset) {
    const int32_t k = ep_step[b];
    if (!(next_reset && k >= max_steps))
      phase = sched_phase(k, (uint32_t)P, (uint32_t)H, wrap != 0);
  }
  const int64_t row = P > 1 ? b * P + (int64_t)phase : b;
  if (srv_out != nullptr) srv_out[i] = per_srv[row * S + (i - b * S)];
  if (i - b * S == 0) {
    if (env_out != nullptr) env_out[b] = per_env[row];
    if (phase_out != nullptr) phase_out[b] = (int32_t)phase;
  }
}

// ---- ground-truth server state (lbsim_ground_truth; the rule: lbsim_truth.h)
static_assert(kTruthCols == LBSIM_TRUTH_COLS && kTruthCols == 8, "a row is two 16-byte stores");
static_assert(kHcHead == 0x7FFFu, "truth_head restates the mask for its host build");

// What the kernel reads, all by value: the state's arrays (hc, ring and ep_step of DevState) and
// the optional ones, nullptr where the handle has none -- down, hidden (the lost_on section of a
// cross-traffic handle only: elsewhere its words count lost-FIN flows), workers, and server, the
// rates in flows/s: a schedule's live table [B * P, S] (P >= 1), the per-env live array [B, S]
// (P = 0), or nullptr: the config's mu[].  Arguments of this kernel alone, not a part of DevState
// or SimParams (§3.11).
struct TruthArgs {
  const uint32_t* hc;
  const int2* ring;
  const int32_t* ep_step;
  const uint32_t* down;
  const uint32_t* hidden;
  const int32_t* workers;
  const float* server;
  int32_t B, S, Q;
  int32_t P, H, wrap, max_steps, next_reset;
  float mu[MAX_S];
};

// The ring of one server, by queue position.  The index is clamped into the ring: a state whose hc
// word breaks n <= Q, head < Q (only lbsim_set_state could load one) reads no other memory.
struct TruthRing {
  const int2* ring;
  int head, Q;
  __device__ __forceinline__ int2 get(int pos) const {
    const uint32_t r = (uint32_t)workers_ring_index(head, pos, Q);
    return ring[r < (uint32_t)Q ? r : (uint32_t)Q - 1u];
  }
};

// One lane per (env, server): coalesced loads of the server's words, at most two scattered 8-byte
// ring loads (none from an empty queue, one where n - c == n - 1), the row as two 16-byte stores.
// The rate is that of the env's next step launch: rate_gather_kernel's phase.
__global__ void __launch_bounds__(256) ground_truth_kernel(TruthArgs a, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.S) return;
  const int64_t b = i / a.S;
  const int s = (int)(i - b * a.S);
  const uint32_t hc = a.hc[i];
  const int32_t c = a.workers != nullptr ? a.workers[i] : 1;
  const int32_t lost = a.hidden != nullptr ? (int32_t)a.hidden[i] : 0;
  const bool down = a.down != nullptr && a.down[i] != 0u;
  float mu;
  if (a.server != nullptr) {
    int64_t row = b;
    if (a.P > 1) {
      const int32_t k = a.ep_step[b];
      const uint32_t phase = (a.next_reset && k >= a.max_steps)
                                 ? 0u : sched_phase(k, (uint32_t)a.P, (uint32_t)a.H, a.wrap != 0);
      row = b * a.P + (int64_t)phase;
    }
    mu = a.server[row * a.S + s];
  } else {
    mu = a.mu[s];
  }
  const TruthRing q{a.ring + (size_t)i * (size_t)a.Q, truth_head(hc), a.Q};
  float r[kTruthCols];
  truth_row(q, hc, c, lost, down, mu, r);
  float4* const o = reinterpret_cast<float4*>(out) + 2 * i;
  o[0] = make_float4(r[0], r[1], r[2], r[3]);
  o[1] = make_float4(r[4], r[5], r[6], r[7]);
}

// ---- the privileged view of processor-sharing servers (lbsim_ps_server_state, DESIGN.md §3.23;
//      the rule: lbsim_ps.h's ps_server_state)
struct PsStateArgs {
  const uint32_t* hc;
  const int2* ring;
  const int32_t* acc;    // the last_tc words
  const int32_t* cores;  // nullptr: one core each
  int32_t B, S, Q;
};

// One lane per (env, server), as ground_truth_kernel: coalesced loads of the server's words, its n
// ring entries through the clamped accessor, the row as one 16-byte store.  n, head and acc are
// read as the dynamics prologue reads them.
__global__ void __launch_bounds__(256) ps_state_kernel(PsStateArgs a, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.S) return;
  const uint32_t hc = a.hc[i];
  const int head = (int)(hc & kHcHead), cnt = (int)(hc >> 16);
  const int n = cnt <= a.Q ? cnt : a.Q;
  const int32_t c = a.cores != nullptr ? a.cores[i] : 1;
  const int32_t w = a.acc[i];
  const int32_t acc = (n > 0 && w > 0 && w < n) ? w : 0;
  const TruthRing q{a.ring + (size_t)i * (size_t)a.Q, head < a.Q ? head : 0, a.Q};
  int32_t work = 0, drain = 0;
  ps_server_state(q, n, c, acc, work, drain);
  reinterpret_cast<float4*>(out)[i] = make_float4((float)n, (float)(n < c ? n : c),
                                                  truth_seconds(work), truth_seconds(drain));
}

// A trace schedule's ids (lbsim_set_trace_schedule) expanded to B rows: out[b * P + phase] =
// in[b * row_stride + phase] (row stride 0: one shared schedule).  Ids outside [0, T) are counted
// into *bad, as rate_table_kernel counts rates out of range.
__global__ void __launch_bounds__(256)
    trace_table_kernel(const int32_t* in, int64_t row_stride, int B, int P, int T, int32_t* out,
                       uint32_t* bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t off = 0u;
  if (i < (int64_t)B * P) {
    const int64_t b = i / P;
    const int32_t t = in[b * row_stride + (i - b * P)];
    off = (t < 0 || t >= T) ? 1u : 0u;
    out[i] = t;
  }
  for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
  if ((threadIdx.x & 63) == 0 && off != 0u) atomicAdd(bad, off);
}

// The trace selection's gather, one thread per env: the id at row b * P + phase of the [B, P]
// table `ids` (nullptr, or P == 0: id 0), and its trace's descriptor {begin[t], begin[t + 1] -
// begin[t]} into desc_out[b] (what env_trace(DevState) points to: one 8-byte vector store), the
// id into id_out[b] and the phase into phase_out[b] (each output optional).  The phase is
// rate_gather_kernel's: sched_phase of k = ep_step[b], or 0 when the env's next step launch resets
// it instead (next-step auto-reset, k >= max_steps); reset != 0: a reset of the envs of `mask`
// (nullptr: all) at phase 0, the other envs skipped.  It runs in front of every dynamics launch
// of a handle with a selection (trace_select) and behind lbsim_env_trace.
__global__ void __launch_bounds__(256)
    trace_gather_kernel(const int32_t* ep_step, const uint8_t* mask, int reset, int B, int P, int H,
                        int wrap, int max_steps, int next_reset, const int32_t* ids,
                        const uint32_t* begin, uint2* desc_out, int32_t* id_out,
                        int32_t* phase_out) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= (int64_t)B) return;
  if (reset && mask != nullptr && mask[b] == 0) return;
  uint32_t phase = 0u;
  if (P > 1 && !reset) {
    const int32_t k = ep_step[b];
    if (!(next_reset && k >= max_steps))
      phase = sched_phase(k, (uint32_t)P, (uint32_t)H, wrap != 0);
  }
  const int32_t t = (ids != nullptr && P > 0) ? ids[b * P + (int64_t)phase] : 0;
  if (desc_out != nullptr) {
    const uint32_t lo = begin[t];
    desc_out[b] = make_uint2(lo, begin[t + 1] - lo);
  }
  if (id_out != nullptr) id_out[b] = t;
  if (phase_out != nullptr) phase_out[b] = (int32_t)phase;
}

// ---- workload tables (lbsim_set_workload_tables): validation and conversion
static_assert(kTableBins == LBSIM_TABLE_BINS && kTableBins % 64 == 0,
              "work_table_kernel: whole passes of one wave");
constexpr int kMaxWorkTables = 1024;  // ids are 16-bit halves of one word per env

// The ids of a call to one word per env, out[b] = gap_id | work_id << 16.  Element b of either
// input is in[b * stride] (stride 0: one id for every env); a NULL input keeps the env's id of
// `cur`, the descriptors in force.  Ids outside [0, T) are counted into *bad; used[t] gets bit 0
// when some env draws gaps from table t and bit 1 when some env draws work from it.
__global__ void __launch_bounds__(256)
    work_ids_kernel(const int32_t* gap_in, int64_t gap_stride, const int32_t* work_in,
                    int64_t work_stride, const uint32_t* cur, int B, int T, uint32_t* out,
                    uint32_t* used, uint32_t* bad) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t off = 0u;
  if (b < (int64_t)B) {
    const int32_t g = gap_in != nullptr ? gap_in[b * gap_stride] : (int32_t)(cur[b] & 0xFFFFu);
    const int32_t w = work_in != nullptr ? work_in[b * work_stride] : (int32_t)(cur[b] >> 16);
    const bool g_ok = g >= 0 && g < T, w_ok = w >= 0 && w < T;
    off = (g_ok ? 0u : 1u) + (w_ok ? 0u : 1u);
    if (g_ok) atomicOr(used + g, 1u);
    if (w_ok) atomicOr(used + w, 2u);
    out[b] = g_ok && w_ok ? (uint32_t)g | (uint32_t)w << 16 : 0u;
  }
  for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
  if ((threadIdx.x & 63) == 0 && off != 0u) atomicAdd(bad, off);
}

// One wave per table: the entries into `out`, the offenders into res[0] (an entry that is not
// finite or < 0; in a table used for gaps an entry > 64, or a mass-weighted mean < 2^-4), and the
// largest entry of the tables used for work into res[1] (f32 bits: entries are >= 0, so the bits
// order as the values).  The mean weighs bin k with its count of Philox words, summed in f64.
__global__ void __launch_bounds__(64)
    work_table_kernel(const float* in, const uint32_t* used, float* out, uint32_t* res) {
  const int lane = (int)threadIdx.x;
  const size_t base = (size_t)blockIdx.x * (size_t)kTableBins;
  const uint32_t use = used[blockIdx.x];
  uint32_t off = 0u;
  double m = 0.0;
  float mx = 0.0f;
  for (int k = lane; k < kTableBins; k += 64) {
    const float x = in[base + (size_t)k];
    const bool ok = x >= 0.0f && x <= 3.402823466e38f;  // false for NaN
    off += (!ok || ((use & 1u) && x > 64.0f)) ? 1u : 0u;
    out[base + (size_t)k] = x;
    m += (double)x * (k < 32 ? 1.0 : (double)(1ull << (k / 32 - 1)));
    mx = ok && x > mx ? x : mx;
  }
  for (int d = 32; d > 0; d >>= 1) {
    off += __shfl_xor(off, d, 64);
    m += __shfl_xor(m, d, 64);
    const float o = __shfl_xor(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if (lane == 0) {
    if (off == 0u && (use & 1u) && !(m >= 268435456.0)) off = 1u;  // mean < 2^-4 (m is mean * 2^32)
    if (off != 0u) atomicAdd(res, off);
    if (use & 2u) atomicMax(res + 1, __float_as_uint(mx));
  }
}

// The largest of n positive floats into *out, as f32 bits (the servers' 1e6 / mu in force).
__global__ void __launch_bounds__(256) scale_max_kernel(const float* x, int64_t n, uint32_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t v = i < n ? __float_as_uint(x[i]) : 0u;
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(out, v);
}

// The descriptors back to ids (lbsim_get_env_workload); either output may be NULL.
__global__ void __launch_bounds__(256)
    work_ids_get_kernel(const uint32_t* desc, int B, int32_t* gap_out, int32_t* work_out) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= (int64_t)B) return;
  const uint32_t d = desc[b];
  if (gap_out != nullptr) gap_out[b] = (int32_t)(d & 0xFFFFu);
  if (work_out != nullptr) work_out[b] = (int32_t)(d >> 16);
}

int launch_check(lbsim_t* h, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(h, LBSIM_EDEVICE, "%s: %s", what, hipGetErrorString(e));
  return LBSIM_OK;
}

// ---- flow statistics (lbsim_flow_stats_*)
static_assert(kFlowBins == LBSIM_FLOW_STATS_BINS && kFlowBins == 3 * 64,
              "flow_quantiles_kernel: three bins per lane");

// The block's arrays: sum_us[BS] (u64, first for its alignment), hist[BS * 192], count[BS],
// max_us[BS]: 784 bytes per server.
size_t flow_stats_bytes(size_t BS) { return BS * (8 + 4 * (size_t)kFlowBins + 4 + 4); }

// One wave per output row (an env: its servers' rows summed, or one server).  Lane l holds bins
// 3 l .. 3 l + 2, so the 64 lanes read a server's 768-byte row as one contiguous span; a wave-wide
// inclusive scan of the lanes' totals gives the cumulative counts; per quantile a ballot finds the
// first lane at or past the rank and that lane resolves the bin among its three.
__global__ void __launch_bounds__(64)
    flow_quantiles_kernel(const uint32_t* hist, const uint32_t* max_us, const uint32_t* q_ppm,
                          int nq, int S, int per_server, uint32_t* out) {
  const int lane = (int)threadIdx.x;
  const size_t row = blockIdx.x;
  const size_t srv0 = per_server ? row : row * (size_t)S;
  const int ns = per_server ? 1 : S;
  unsigned long long c0 = 0, c1 = 0, c2 = 0;  // an env's bin can pass 2^32 over 64 servers
  uint32_t mx = 0u;
  for (int s = 0; s < ns; ++s) {
    const uint32_t* r = hist + (srv0 + (size_t)s) * kFlowBins + 3 * lane;
    c0 += r[0];
    c1 += r[1];
    c2 += r[2];
    const uint32_t m = max_us[srv0 + (size_t)s];  // wave-uniform
    mx = m > mx ? m : mx;
  }
  const unsigned long long own = c0 + c1 + c2;
  unsigned long long incl = own;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  const unsigned long long n = __shfl(incl, 63, 64);
  for (int i = 0; i < nq; ++i) {
    uint32_t q = q_ppm[i];
    q = q < 1u ? 1u : (q > 1000000u ? 1000000u : q);
    unsigned long long rank = ((unsigned long long)q * n + 999999ull) / 1000000ull;
    rank = rank < 1ull ? 1ull : rank;
    const unsigned long long past = __ballot(incl >= rank);  // n > 0: lane 63 at least
    if (n == 0ull) {
      if (lane == 0) out[row * (size_t)nq + (size_t)i] = 0u;
    } else if (lane == __builtin_ctzll(past)) {
      const unsigned long long before = incl - own;
      const int k = 3 * lane + (before + c0 >= rank ? 0 : (before + c0 + c1 >= rank ? 1 : 2));
      const uint32_t hi = k == kFlowBins - 1 ? mx : flow_bin_lower(k + 1) - 1u;
      out[row * (size_t)nq + (size_t)i] = hi < mx ? hi : mx;
    }
  }
}

// Zeroes the rows of the masked envs (mask nullptr: all): one thread per histogram word, the
// thread of a row's first word its count, sum and maximum too.
__global__ void __launch_bounds__(256)
    flow_clear_kernel(uint32_t* count, unsigned long long* sum, uint32_t* max_us, uint32_t* hist,
                      int64_t n_words, int S, const uint8_t* mask) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_words) return;
  const int64_t sb = i / kFlowBins;
  if (mask != nullptr && mask[sb / S] == 0) return;
  hist[i] = 0u;
  if (i - sb * kFlowBins == 0) {
    count[sb] = 0u;
    sum[sb] = 0ull;
    max_us[sb] = 0u;
  }
}

// The config's rates into the live per-env arrays (every env the same), on stream s.
void env_rates_fill_defaults(lbsim_t* h, hipStream_t s) {
  const float* def = env_rates_defaults(h);
  const int64_t n = (int64_t)h->B * h->S;
  hipLaunchKernelGGL(env_rates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, def,
                     (int64_t)0, def + 1, (int64_t)0, h->B, h->S, env_rates_live(h),
                     env_rates_bad(h), 1.0f);
}

// The per-env rate block: allocated once, its live arrays holding the config's rates.
int env_rates_ensure(lbsim_t* h, hipStream_t s) {
  if (h->rates_buf != nullptr) return LBSIM_OK;
  const size_t B = (size_t)h->B, BS = B * h->S;
  const size_t bytes = (4 * (B + BS) + 1 + MAX_S) * sizeof(float) + sizeof(uint32_t);
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", bytes);
  h->rates_buf = (float*)p;
  float def[1 + MAX_S];
  def[0] = h->cfg.arrival_rate;
  for (int k = 0; k < MAX_S; ++k) def[1 + k] = k < h->S ? h->cfg.server_rate[k] : 1.0f;
  if (hipMemcpy(env_rates_defaults(h), def, sizeof(def), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(env_rates_bad(h), 0, sizeof(uint32_t)) != hipSuccess) {
    (void)hipFree(p);
    h->rates_buf = nullptr;
    return fail(h, LBSIM_EDEVICE, "per-env rates: upload of the config's rates failed");
  }
  env_rates_fill_defaults(h, s);
  return launch_check(h, "env_rates_kernel");
}

// ---- rate schedules (lbsim_set_rate_schedule).  A block for P phases holds, in
// floats, with N = B * P rows: the live tables arrival[N], server[N*S], gap[N], scale[N*S] (row
// b * P + phase), their staging copies, base[B + B*S] (the per-env rates in force before a call,
// the source of a NULL argument), cur_gap[B] and cur_scale[B*S] (each env's row of gap / scale at
// the phase of the launch in progress: what DevState::env_gap / env_scale point to, written by
// sched_select), and the offender count (one u32).
size_t sched_floats(const lbsim_t* h, int P) {
  const size_t B = (size_t)h->B, N = B * (size_t)P, S = (size_t)h->S;
  return 4 * (N + N * S) + 2 * (B + B * S);
}
EnvRates sched_live(const lbsim_t* h, float* buf, int P) {
  const size_t N = (size_t)h->B * (size_t)P;
  return env_rates_at(buf, N, N * h->S);
}
EnvRates sched_staging(const lbsim_t* h, float* buf, int P) {
  const size_t N = (size_t)h->B * (size_t)P;
  return env_rates_at(buf + 2 * (N + N * h->S), N, N * h->S);
}
float* sched_base(const lbsim_t* h, float* buf, int P) {
  const size_t N = (size_t)h->B * (size_t)P;
  return buf + 4 * (N + N * h->S);
}
float* sched_cur(const lbsim_t* h, float* buf, int P) {  // cur_gap, then cur_scale
  return sched_base(h, buf, P) + (size_t)h->B + (size_t)h->B * h->S;
}
uint32_t* sched_bad(const lbsim_t* h, float* buf, int P) {
  return reinterpret_cast<uint32_t*>(buf + sched_floats(h, P));
}
unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

// The per-env arrays the dynamics kernels read.  A TRACE handle draws no gap: its env_gap word
// carries the trace selection (env_trace(DevState)), which only lbsim_set_trace_schedule sets.
void set_env_arrays(lbsim_t* h, const float* gap, const float* scale) {
  if (!h->prm.trace) h->st.env_gap = gap;
  h->st.env_scale = scale;
}

// ---- trace selection (lbsim_set_trace_schedule).  A block for P phases holds
// cur[B] (uint2: each env's descriptor at the phase of the launch in progress, what
// env_trace(DevState) points to, written by trace_select), the live ids [B * P] (row b * P +
// phase), their staging copy, and the offender count (one u32).
struct TraceSelBuf {
  uint2* cur;
  int32_t *live, *staging;
  uint32_t* bad;
};
size_t trace_sel_bytes(const lbsim_t* h, int P) {
  const size_t B = (size_t)h->B;
  return B * sizeof(uint2) + 2 * B * (size_t)P * sizeof(int32_t) + sizeof(uint32_t);
}
TraceSelBuf trace_sel_at(const lbsim_t* h, void* buf, int P) {
  const size_t B = (size_t)h->B, N = B * (size_t)P;
  TraceSelBuf t;
  t.cur = (uint2*)buf;
  t.live = (int32_t*)(t.cur + B);
  t.staging = t.live + N;
  t.bad = (uint32_t*)(t.staging + N);
  return t;
}

// The rates each env's next step launch will use (and / or its phase), on stream s: the phase's
// row of a schedule's tables, else the per-env arrays (the config's rates when none are set).
int rates_in_force(lbsim_t* h, float* arr_out, float* srv_out, int32_t* phase_out, hipStream_t s) {
  const SimParams& p = h->prm;
  EnvRates src{};
  if (arr_out != nullptr || srv_out != nullptr) {
    if (h->sched_P > 0) {
      src = sched_live(h, h->sched_buf, h->sched_P);
    } else {
      const int rc = env_rates_ensure(h, s);
      if (rc != LBSIM_OK) return rc;
      src = env_rates_live(h);
    }
  }
  hipLaunchKernelGGL(rate_gather_kernel, dim3(blocks256((size_t)h->B * h->S)), dim3(256), 0, s,
                     h->st.ep_step, (const uint8_t*)nullptr, 0, h->B, h->S, h->sched_P, h->sched_H,
                     h->sched_wrap, p.max_steps, p.next_reset, src.arrival, src.server, arr_out,
                     srv_out, phase_out);
  return launch_check(h, "rate_gather_kernel");
}

// In front of a dynamics launch of a scheduled handle (a step, or a reset of the envs of `mask`):
// each env's gap and scale rows at the launch's phase into the per-env arrays the dynamics
// kernels read.  One small launch on the step's stream, no allocation, no synchronisation; a
// handle without a schedule launches nothing.  Not in the launch log or the profiler's classes:
// those describe the step's own kernels.
int sched_select(lbsim_t* h, const uint8_t* mask, int mode, hipStream_t s) {
  if (h->sched_P == 0) return LBSIM_OK;
  const SimParams& p = h->prm;
  const EnvRates live = sched_live(h, h->sched_buf, h->sched_P);
  float* const cur = sched_cur(h, h->sched_buf, h->sched_P);
  hipLaunchKernelGGL(rate_gather_kernel, dim3(blocks256((size_t)h->B * h->S)), dim3(256), 0, s,
                     h->st.ep_step, mask, mode == kModeReset ? 1 : 0, h->B, h->S, h->sched_P,
                     h->sched_H, h->sched_wrap, p.max_steps, p.next_reset, live.gap, live.scale,
                     cur, cur + h->B, (int32_t*)nullptr);
  return launch_check(h, "rate_gather_kernel");
}

// Drops the schedule in force (if any): the kernels go back to the per-env arrays that were in
// force before it, or to the config's shared rates.  The tables stay allocated.
void sched_drop(lbsim_t* h) {
  if (h->sched_P == 0) return;
  h->sched_P = h->sched_H = h->sched_wrap = 0;
  const EnvRates live = h->rates_on ? env_rates_live(h) : EnvRates{};
  set_env_arrays(h, live.gap, live.scale);
}

// In front of a dynamics launch of a handle with a trace selection (a step, or a reset of the
// envs of `mask`): each env's trace descriptor at the launch's phase into the array the TRACE
// kernels read.  As sched_select: one small launch on the step's stream, no allocation, no
// synchronisation, not in the launch log; a handle without a selection pays the one test.
int trace_select(lbsim_t* h, const uint8_t* mask, int mode, hipStream_t s) {
  if (h->tsel_P == 0) return LBSIM_OK;
  const SimParams& p = h->prm;
  const TraceSelBuf t = trace_sel_at(h, h->tsel_buf, h->tsel_P);
  hipLaunchKernelGGL(trace_gather_kernel, dim3(blocks256((size_t)h->B)), dim3(256), 0, s,
                     h->st.ep_step, mask, mode == kModeReset ? 1 : 0, h->B, h->tsel_P, h->tsel_H,
                     h->tsel_wrap, p.max_steps, p.next_reset, t.live, h->bank_begin_dev, t.cur,
                     (int32_t*)nullptr, (int32_t*)nullptr);
  return launch_check(h, "trace_gather_kernel");
}

// ---- scripted server availability (lbsim_set_server_avail; lbsim_avail.h)
static_assert(kAvailK == K && kAvailHcHead == kHcHead && kAvailLastNone == kLastNone &&
                  kAvailFeat + 1 == NF,
              "lbsim_avail.h restates these for its host build");

AvailState avail_state(const lbsim_t* h) {
  const DevState& st = h->st;
  const SimParams& p = h->prm;
  AvailState a{};
  a.ep_step = st.ep_step;
  a.hc = st.hc;
  a.last_tc = st.last_tc;
  a.res_count = st.res_count;
  a.res = reinterpret_cast<uint32_t*>(st.res);
  a.fcache = st.fcache;
  a.down = st.down;
  a.lost_on = st.lost_on;
  a.res_dur = st.res_dur;
  a.res_count_dur = st.res_count_dur;
  a.pend_hc = st.pend_hc;
  a.B = h->B, a.S = h->S;
  a.split = p.split, a.res_vpp = p.res_vpp;
  a.max_steps = p.max_steps, a.next_reset = p.next_reset;
  return a;
}

AvailTable avail_table(const lbsim_t* h) {
  return AvailTable{h->avail_P > 0 ? h->avail_buf : nullptr, h->avail_P, h->avail_H,
                    h->avail_wrap};
}

// In front of the first launch of a step of a handle with lbsim_server_avail_enable: each (env,
// server) brought to what the table wants at the env's phase.  As sched_select: one small launch
// on the step's stream, no allocation, no synchronisation, not in the launch log; any other
// handle pays the one test.
int avail_apply(lbsim_t* h, hipStream_t s) {
  if (!h->avail_on) return LBSIM_OK;
  hipLaunchKernelGGL(avail_apply_kernel, dim3(blocks256((size_t)h->B * h->S)), dim3(256), 0, s,
                     avail_state(h), avail_table(h), AvailOut{}, 1, h->st.dropped);
  return launch_check(h, "avail_apply_kernel");
}

// The bank's row offsets to the device (u32: fewer than 2^31 rows), for trace_gather_kernel.
// Off the step path: it waits for the copy.
int bank_begin_upload(lbsim_t* h) {
  const size_t n = h->bank_begin.size();
  if (h->bank_begin_dev == nullptr && hipMalloc((void**)&h->bank_begin_dev, n * 4) != hipSuccess) {
    h->bank_begin_dev = nullptr;
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", n * 4);
  }
  std::vector<uint32_t> b32(h->bank_begin.begin(), h->bank_begin.end());
  if (hipMemcpy(h->bank_begin_dev, b32.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "trace bank: upload of the row offsets failed");
  return LBSIM_OK;
}

// Drops the trace selection in force (if any): every env replays trace 0 again.  The tables stay
// allocated.
void trace_sel_drop(lbsim_t* h) {
  h->tsel_P = h->tsel_H = h->tsel_wrap = 0;
  if (h->prm.trace) set_env_trace(h->st, nullptr);
}

// ---- workload tables (lbsim_set_workload_tables).  A block for T tables holds
// the live tables [T * 896] and descriptors [B] (what work_tables / work_ids of DevState point
// to), their staging copies (a call converts into these and only a valid one is copied over the
// live ones), used[T] (bit 0: some env's gap table, bit 1: some env's work table) and res[4]:
// the offender count, the largest work entry and the largest 1e6 / mu in force, as f32 bits.
struct WorkTabBuf {
  float* live_tab;
  uint32_t* live_ids;
  float* stg_tab;
  uint32_t *stg_ids, *used, *res;
};
size_t work_tab_bytes(const lbsim_t* h, int T) {
  return 2 * ((size_t)T * kTableBins + (size_t)h->B) * 4 + ((size_t)T + 4) * 4;
}
WorkTabBuf work_tab_at(const lbsim_t* h, void* buf, int T) {
  const size_t n = (size_t)T * kTableBins, B = (size_t)h->B;
  WorkTabBuf w;
  w.live_tab = (float*)buf;
  w.live_ids = (uint32_t*)(w.live_tab + n);
  w.stg_tab = (float*)(w.live_ids + B);
  w.stg_ids = (uint32_t*)(w.stg_tab + n);
  w.used = w.stg_ids + B;
  w.res = w.used + T;
  return w;
}
// The bound that keeps the 32-bit relative times safe with work tables: wmax * (1e6 / mu) * Q <=
// 2^30 for every server (without tables the worst case is 16.64 * 1e6 * 64 < 2^30).
constexpr double kWorkTimeBound = 1073741824.0;
// The lower bound of a server rate that lbsim_set_env_rates / lbsim_set_rate_schedule accept: 1,
// or what the work tables in force ask for (rounded up, with a margin for the f32 division that
// makes 1e6 / mu, so a rate accepted here passes the tables' own check later).
float mu_floor(const lbsim_t* h) {
  if (h->wtab_T == 0) return 1.0f;
  const double lo = (double)h->wtab_wmax * (double)h->Q * 1e6 / kWorkTimeBound * (1.0 + 1e-6);
  return lo > 1.0 ? (float)lo : 1.0f;
}

// The common body of lbsim_set_workload_tables and lbsim_set_env_workload: T tables at `tables`
// (the caller's, or the live ones) and ids (element b at in[b * stride]; NULL: the id in force)
// validated into the staging arrays of the block for T tables, then copied over the live ones.
int work_tables_apply(lbsim_t* h, const float* tables, int T, const int32_t* gap_id,
                      int64_t gap_stride, const int32_t* work_id, int64_t work_stride,
                      hipStream_t s) {
  const size_t B = (size_t)h->B, n = (size_t)T * kTableBins;
  void* buf = h->wtab_buf;
  const bool fresh = buf == nullptr || h->wtab_alloc_T != T;
  if (fresh) {
    const size_t bytes = work_tab_bytes(h, T);
    if (hipMalloc(&buf, bytes) != hipSuccess)
      return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", bytes);
  }
  auto give_up = [&](int code, const char* fmt, double a = 0.0, double b = 0.0, double c = 0.0) {
    if (fresh) (void)hipFree(buf);  // (waits for the device)
    return fail(h, code, fmt, a, b, c);
  };
  const WorkTabBuf w = work_tab_at(h, buf, T);
  const uint32_t* const cur =
      h->wtab_T > 0 ? work_tab_at(h, h->wtab_buf, h->wtab_alloc_T).live_ids : nullptr;
  if (hipMemsetAsync(w.used, 0, ((size_t)T + 4) * 4, s) != hipSuccess)
    return give_up(LBSIM_EDEVICE, "workload tables: hipMemsetAsync failed");
  hipLaunchKernelGGL(work_ids_kernel, dim3(blocks256(B)), dim3(256), 0, s, gap_id, gap_stride,
                     work_id, work_stride, cur, h->B, T, w.stg_ids, w.used, w.res);
  hipLaunchKernelGGL(work_table_kernel, dim3((unsigned)T), dim3(64), 0, s, tables,
                     (const uint32_t*)w.used, w.stg_tab, w.res);
  // the largest 1e6 / mu in force: a schedule's tables, the per-env arrays, or the config's
  double scale_max = 0.0;
  if (h->sched_P > 0) {
    const size_t NS = B * (size_t)h->sched_P * (size_t)h->S;
    hipLaunchKernelGGL(scale_max_kernel, dim3(blocks256(NS)), dim3(256), 0, s,
                       (const float*)sched_live(h, h->sched_buf, h->sched_P).scale, (int64_t)NS,
                       w.res + 2);
  } else if (h->rates_on) {
    const size_t BS = B * (size_t)h->S;
    hipLaunchKernelGGL(scale_max_kernel, dim3(blocks256(BS)), dim3(256), 0, s,
                       (const float*)env_rates_live(h).scale, (int64_t)BS, w.res + 2);
  } else {
    for (int k = 0; k < h->S; ++k)
      scale_max = h->prm.svc_scale[k] > scale_max ? h->prm.svc_scale[k] : scale_max;
  }
  if (launch_check(h, "work_table_kernel") != LBSIM_OK) {
    if (fresh) (void)hipFree(buf);
    return LBSIM_EDEVICE;
  }
  uint32_t res[4] = {0u, 0u, 0u, 0u};
  if (hipMemcpyAsync(res, w.res, sizeof(res), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return give_up(LBSIM_EDEVICE, "workload tables: validation failed");
  if (res[0] != 0u)  // nothing live was touched: what was in force stays in force
    return give_up(LBSIM_EINVAL,
                   "workload tables: %.0f offender(s): ids must be in [0, %.0f), entries finite and "
                   ">= 0, a table used for gaps <= 64 with a mass-weighted mean >= 1/16",
                   (double)res[0], (double)T);
  float wmax, smax;
  memcpy(&wmax, &res[1], 4);
  memcpy(&smax, &res[2], 4);
  if (scale_max == 0.0) scale_max = (double)smax;
  if ((double)wmax * scale_max * (double)h->Q > kWorkTimeBound)
    return give_up(LBSIM_EINVAL,
                   "workload tables: the largest work entry %g breaks wmax * (1e6 / mu_min) * "
                   "queue_capacity <= 2^30 (mu_min = %g flows/s, queue_capacity = %.0f)",
                   (double)wmax, 1e6 / scale_max, (double)h->Q);
  bool ok = true;
  if (tables != w.live_tab)
    ok &= hipMemcpyAsync(w.live_tab, w.stg_tab, n * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  ok &= hipMemcpyAsync(w.live_ids, w.stg_ids, B * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (!ok) return give_up(LBSIM_EDEVICE, "workload tables: device copy failed");
  if (fresh) {
    if (h->wtab_buf != nullptr) (void)hipFree(h->wtab_buf);  // (waits for the device)
    h->wtab_buf = buf;
    h->wtab_alloc_T = T;
  }
  set_work_tables(h->st, w.live_tab, w.live_ids);
  h->wtab_T = T;
  h->wtab_wmax = wmax;
  return LBSIM_OK;
}

// Brackets one launch with profiler events when profiling is on (class: see lbsim.h).
struct ProfScope {
  lbsim_t* h;
  hipStream_t s;
  bool rec = false;
  ProfScope(lbsim_t* h_, hipStream_t s_, int cls) : h(h_), s(s_) {
    g_log_class = cls;  // the launch log's class of the kernel launched in this scope
    Profiler& p = h->prof;
    if (!p.on) return;
    if (p.chain_ev >= 0 && p.used + 1 <= p.cap) {
      p.beg.push_back(p.chain_ev);  // the previous launch's end event, on the same stream
      rec = true;
    } else if (p.used + 2 <= p.cap && hipEventRecord(p.ev[p.used], s) == hipSuccess) {
      p.beg.push_back((int)p.used++);
      rec = true;
    }
    p.chain_ev = -1;
    if (rec) p.cls.push_back(cls);
  }
  ~ProfScope() {
    g_log_class = -1;  // a launch outside any scope is logged with class -1, not a stale one
    if (!rec) return;
    Profiler& p = h->prof;
    (void)hipEventRecord(p.ev[p.used], s);
    p.end.push_back((int)p.used);
    p.chain_ev = p.chain ? (int)p.used : -1;
    ++p.used;
  }
};

// Scope of one lbsim_step_ex (which = 0) / lbsim_reset_ex (1): the launch log starts empty and
// is kept in the handle when the call returns (lbsim_launch_names).
struct LaunchLog {
  lbsim_t* h;
  int which;
  LaunchLog(lbsim_t* h_, int w) : h(h_), which(w) {
    g_log_n = 0;
    g_log_lost = 0;
  }
  ~LaunchLog() {
    auto& v = h->launched[which];
    v.clear();
    for (int i = 0; i < g_log_n; ++i) v.emplace_back(g_log_cls[i], g_log_fn[i]);
    h->launched_lost[which] = g_log_lost;
    g_log_n = 0;
    g_log_lost = 0;
    g_log_class = -1;
  }
};

// "void lbk::observe_kernel<4, 0, false>(lbk::DevState, ...)" -> "observe_kernel<4, 0, false>":
// the form tools/pmc_traffic.py and tools/pmc_valu.py key their counter files by.
std::string short_kernel_name(const char* raw) {
  std::string s = raw ? raw : "?";
  int st = 0;
  if (char* d = abi::__cxa_demangle(s.c_str(), nullptr, nullptr, &st)) {
    if (st == 0) s = d;
    free(d);
  }
  int depth = 0;  // cut the parameter list: the first '(' outside template brackets
  for (size_t i = 0; i < s.size(); ++i) {
    if (s[i] == '<') ++depth;
    else if (s[i] == '>') --depth;
    else if (s[i] == '(' && depth == 0 && s.compare(i, 21, "(anonymous namespace)") != 0) {
      s.resize(i);
      break;
    }
  }
  for (const char* pre : {"void ", "lbk::", "(anonymous namespace)::"}) {
    for (size_t at; (at = s.find(pre)) != std::string::npos;) s.erase(at, strlen(pre));
  }
  return s;
}

LaunchCtx ctx(const lbsim_t* h) {
  return LaunchCtx{h->plan, h->st, h->prm, h->flow, h->cross, h->workers, h->delay};
}

// The handle's plan: the process's overrides are read on the first call and kept.
StepPlan plan_of(const lbsim_t* h) {
  static const Overrides ov = Overrides::from_env();
  const SimParams& p = h->prm;
  PlanInput in{};
  in.B = h->B, in.S = h->S, in.Q = p.Q, in.policy = p.policy;
  in.trace = p.trace != 0, in.fail = p.fail_thr != 0u || h->avail_on, in.leak = p.leak != 0;
  in.split = p.split != 0, in.res_vpp = p.res_vpp != 0, in.dur_plane = dur_plane(p);
  in.next_reset = p.next_reset != 0;
  in.flow_stats = h->flow.hist != nullptr;
  in.work_tables = h->wtab_T > 0;
  in.cross_traffic = h->cross_buf != nullptr;
  in.server_workers = h->workers_buf != nullptr;
  in.action_delay = h->delay_buf != nullptr;
  in.pool = h->pool.A;
  in.ps = h->ps;
  in.pool_ps = h->pool_ps;
  in.ack_samples = h->ack_max > 0;
  in.dyn_mapping = h->cfg.dyn_mapping, in.step_kernel = h->cfg.step_kernel, in.simds = h->simds;
  return make_plan(in, ov);
}

int launch_dynamics(lbsim_t* h, const void* action, int dtype, int32_t* assign,
                    const uint8_t* mask, int mode, hipStream_t stream) {
  ProfScope ps(h, stream, mode == kModeStep ? 0 : 2);
  if (h->pool_ps) {  // pools of processor-sharing servers: their own kernel (§3.24)
    if (mode == kModeStep)
      launch_dynamics_pool_ps_step(ctx(h), h->pool, action, dtype, assign, h->pool_ps_cores_buf,
                                   stream);
    else
      launch_dynamics_pool_ps_reset(ctx(h), h->pool, mask, h->pool_ps_cores_buf, stream);
    return launch_check(h, "dynamics_pool_ps_kernel");
  }
  if (h->pool.A > 0) {  // shared server pools: their own kernel (mask: the widened one)
    if (mode == kModeStep) launch_dynamics_pool_step(ctx(h), h->pool, action, dtype, assign, stream);
    else launch_dynamics_pool_reset(ctx(h), h->pool, mask, stream);
    return launch_check(h, "dynamics_pool_kernel");
  }
  if (h->ack_max > 0) {  // ACK samples: the full form with the ACK code, step and reset (§3.25)
    const AckSamples as{h->ack_us, h->ack_max};
    if (mode == kModeStep) launch_dynamics_ack_step(ctx(h), as, action, dtype, assign, stream);
    else launch_dynamics_ack_reset(ctx(h), as, mask, stream);
    return launch_check(h, "dynamics_group_ack_kernel");
  }
  if (h->ps) {  // processor-sharing servers: their own kernel
    if (mode == kModeStep)
      launch_dynamics_ps_step(ctx(h), action, dtype, assign, h->ps_cores_buf, stream);
    else
      launch_dynamics_ps_reset(ctx(h), mask, h->ps_cores_buf, stream);
    return launch_check(h, "dynamics_ps_kernel");
  }
  if (mode == kModeStep && h->plan.nr)  // next-step auto-reset: done envs reset instead
    launch_dynamics_step_nr(ctx(h), action, dtype, assign, mask, stream);
  else if (mode == kModeStep)
    launch_dynamics_step(ctx(h), action, dtype, assign, mask, stream);
  else
    launch_dynamics_reset(ctx(h), action, dtype, assign, mask, stream);
  return launch_check(h, "dynamics_kernel");
}

bool facade_bad(const lbsim_t* h, const lbsim_step_outputs_t* out) {
  if (out->agent_obs == nullptr && out->state == nullptr) return false;
  return out->num_agents < 1 || out->servers_per_agent < 1 ||
         (int64_t)out->num_agents * out->servers_per_agent != h->S;
}

ObsOutputs obs_outputs(const lbsim_step_outputs_t* out, bool reset) {
  ObsOutputs o{};
  o.obs = out->obs;
  o.raw_obs = out->raw_obs;
  if (!reset) {
    o.reward = out->reward;
    o.done = out->done;
    o.ep_len = out->episode_length;
    o.ep_ret = out->episode_return;
    o.done_word = out->done_word;
    o.done_value = out->done_value;
  }
  o.agent_obs = out->agent_obs;
  o.state = out->state;
  o.num_agents = out->num_agents;
  o.servers_per_agent = out->servers_per_agent;
  return o;
}

int launch_observe(lbsim_t* h, const ObsOutputs& o, const uint8_t* mask, int mode,
                   hipStream_t stream) {
  ProfScope ps(h, stream, mode == kModeStep ? 1 : 3);
  if (mode == kModeStep) launch_observe_step(ctx(h), o, mask, stream);
  else launch_observe_reset(ctx(h), o, mask, stream);
  return launch_check(h, "observe_kernel");
}

// ---- one-kernel policy inference (lbsim_fused.h; the LDS layout and its sizing: lbsim_pol.hip)

int round16(int x) { return (x + 15) / 16 * 16; }

// Envs per workgroup = 16 MT.  QMIX's tile kernel: MT = 1 (8192 x 16 0.121 / 0.157 / 0.251 ms at
// MT = 1 / 2 / 4, profiles/r01s3a).  The SAC actor: MT = 2 since round 6 -- with its staging one
// HBM round trip (r06n), a 32-env tile halves the weight stream per env, and the weight stream is
// what the staging waited behind: 187-188 -> 179.3-179.7 us at 65536 x 8, 0.53 -> 0.556 of the
// f32 MFMA peak (profiles/r06q/; round 1, with the staging serialised, MT = 2 was the slower:
// 0.231 vs 0.267 ms).  LBSIM_FUSED_MT = 1 | 2 | 4 forces it for both.  The launchers halve it
// until the tile's LDS fits.
int fused_mt(int dflt) {
  static const int forced = env_int("LBSIM_FUSED_MT", 0);
  return (forced == 1 || forced == 2 || forced == 4) ? forced : dflt;
}

}  // namespace

extern "C" {

const char* lbsim_version(void) { return "lbsim 0.1.0 (gfx950, HIP)"; }
int lbsim_abi_version(void) { return LBSIM_ABI_VERSION; }

int lbsim_config_default(lbsim_config_t* c) {
  if (c == nullptr) return LBSIM_EINVAL;
  memset(c, 0, sizeof(*c));
  c->num_envs = 1;
  c->num_servers = 4;
  c->env_id_offset = 0;
  c->seed = 0;
  c->action_type = LBSIM_ACTION_DISCRETE;
  c->num_discrete = 3;
  c->discrete_weights[0] = 1.0f;
  c->discrete_weights[1] = 1.5f;
  c->discrete_weights[2] = 2.0f;
  c->min_weight = 0.1f;
  c->max_weight = 10.0f;
  c->reward_metric = LBSIM_METRIC_JAIN;
  c->reward_field = 10;
  c->step_interval = 0.25f;
  c->max_steps = 10000;
  c->normalize_obs = 0;
  c->assign_policy = LBSIM_POLICY_SED;
  c->arrival_source = LBSIM_ARRIVAL_POISSON;
  c->arrival_rate = 400.0f;
  for (int s = 0; s < LBSIM_MAX_SERVERS; ++s) c->server_rate[s] = 125.0f;
  c->decay_factor = 0.9f;
  c->queue_capacity = 32;
  c->warmup_steps = 8;
  c->lost_fin_prob = 0.0f;
  c->flow_timeout_s = 40.0f;  // LB_DEFAULT_FLOW_TIMEOUT (lb.c:1437)
  c->flow_buckets = 1024;     // LB_DEFAULT_PER_CPU_STICKY_BUCKETS (lb.h:46)
  c->fail_prob = 0.0f;
  c->recover_prob = 0.1f;
  c->duration_mode = LBSIM_DURATION_AGE;  // lbhash.h:129-136: the flow's age
  c->lost_fin_pending = 256;
  c->reservoir_mode = LBSIM_RESERVOIR_ALGR;
  return LBSIM_OK;
}

int lbsim_config_validate(const lbsim_config_t* cfg, char* msg, size_t msg_len) {
  return validate(cfg, msg, msg_len);
}

int lbsim_create(const lbsim_config_t* cfg, int device, lbsim_t** out) {
  if (out == nullptr) return fail(nullptr, LBSIM_EINVAL, "out is NULL");
  *out = nullptr;
  char msg[256] = {0};
  if (validate(cfg, msg, sizeof(msg)) != LBSIM_OK) return fail(nullptr, LBSIM_EINVAL, "%s", msg);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, LBSIM_EDEVICE, "no HIP device available");
  if (device < 0 || device >= ndev)
    return fail(nullptr, LBSIM_EINVAL, "device %d out of range [0, %d)", device, ndev);
  DeviceGuard g(device);
  if (!g.ok) return fail(nullptr, LBSIM_EDEVICE, "hipSetDevice(%d) failed", device);

  lbsim_t* h = new lbsim_t();
  h->cfg = *cfg;
  h->device = device;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      cus < 1)
    cus = 256;
  h->simds = 4 * cus;
  h->B = cfg->num_envs;
  h->S = cfg->num_servers;
  h->Q = cfg->queue_capacity;
  h->initialised = false;
  memset(&h->st, 0, sizeof(h->st));
  derive_params(*cfg, h->prm);
  h->plan = plan_of(h);
  for (Section& sec : sections(h)) {
    void* p = nullptr;
    if (hipMalloc(&p, sec.bytes) != hipSuccess) {
      lbsim_destroy(h);
      return fail(nullptr, LBSIM_ENOMEM, "hipMalloc(%zu) failed", sec.bytes);
    }
    h->allocs.push_back(p);
    *sec.ptr = p;
    if (hipMemset(p, 0, sec.bytes) != hipSuccess) {
      lbsim_destroy(h);
      return fail(nullptr, LBSIM_EDEVICE, "hipMemset failed");
    }
  }
  if (cfg->normalize_obs) {
    const size_t n = (size_t)h->B * h->S * NF;
    hipLaunchKernelGGL(init_norm_std, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                       h->st.norm_std, n);
  }
  if (hipDeviceSynchronize() != hipSuccess) {
    lbsim_destroy(h);
    return fail(nullptr, LBSIM_EDEVICE, "device init failed");
  }
  *out = h;
  return LBSIM_OK;
}

int lbsim_destroy(lbsim_t* h) {
  if (h == nullptr) return LBSIM_OK;
  {
    DeviceGuard g(h->device);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->trace_buf) (void)hipFree(h->trace_buf);
    if (h->bank_begin_dev) (void)hipFree(h->bank_begin_dev);
    if (h->tsel_buf) (void)hipFree(h->tsel_buf);
    if (h->stats_buf) (void)hipFree(h->stats_buf);
    if (h->rates_buf) (void)hipFree(h->rates_buf);
    if (h->sched_buf) (void)hipFree(h->sched_buf);
    if (h->flow_buf) (void)hipFree(h->flow_buf);
    if (h->cross_buf) (void)hipFree(h->cross_buf);
    if (h->workers_buf) (void)hipFree(h->workers_buf);
    if (h->ps_cores_buf) (void)hipFree(h->ps_cores_buf);
    if (h->pool_ps_cores_buf) (void)hipFree(h->pool_ps_cores_buf);
    if (h->delay_buf) (void)hipFree(h->delay_buf);
    if (h->avail_buf) (void)hipFree(h->avail_buf);
    if (h->wtab_buf) (void)hipFree(h->wtab_buf);
    for (hipEvent_t e : h->prof.ev) (void)hipEventDestroy(e);
  }
  delete h;
  return LBSIM_OK;
}

const char* lbsim_last_error(const lbsim_t* h) {
  return h ? h->err.c_str() : g_create_err.c_str();
}

int lbsim_dynamics_kernel(const lbsim_t* h) {
  if (h == nullptr) return -1;
  return h->plan.dyn.kernel;
}

int lbsim_seed(lbsim_t* h, uint64_t seed) {
  if (h == nullptr) return LBSIM_EINVAL;
  DeviceGuard g(h->device);
  h->cfg.seed = seed;
  h->prm.key0 = (uint32_t)(seed & 0xFFFFFFFFull);
  h->prm.key1 = (uint32_t)(seed >> 32);
  if (hipMemset(h->st.episode, 0, (size_t)h->B * 4) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "hipMemset failed");
  return LBSIM_OK;
}

int lbsim_reset(lbsim_t* h, const uint8_t* env_mask, float* obs_out, void* stream) {
  lbsim_step_outputs_t o;
  memset(&o, 0, sizeof(o));
  o.obs = obs_out;
  return lbsim_reset_ex(h, env_mask, &o, stream);
}

int lbsim_reset_ex(lbsim_t* h, const uint8_t* env_mask, const lbsim_step_outputs_t* out,
                   void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (out == nullptr || out->obs == nullptr) return fail(h, LBSIM_EINVAL, "obs_out is NULL");
  if (facade_bad(h, out)) return fail(h, LBSIM_EINVAL, "agent_obs / state need num_agents * "
                                                       "servers_per_agent == num_servers");
  if (h->prm.trace && h->prm.trace_rows == 0)
    return fail(h, LBSIM_EINVAL, "arrival_source TRACE: call lbsim_set_trace before lbsim_reset");
  DeviceGuard g(h->device);
  LaunchLog log(h, 1);
  const hipStream_t s = (hipStream_t)stream;
  h->reset_seen = true;
  int rc = sched_select(h, env_mask, kModeReset, s);  // a rate schedule: a reset runs at phase 0
  if (rc != LBSIM_OK) return rc;
  rc = trace_select(h, env_mask, kModeReset, s);  // a trace schedule: the same
  if (rc != LBSIM_OK) return rc;
  // shared server pools: a pool resets iff any member's byte is set, and then all of it.  The
  // mask is widened here, once, for both launches: the observe kernels read one byte per env
  const uint8_t* mask = env_mask;
  if (h->pool.A > 1 && env_mask != nullptr) {
    launch_pool_mask(h->pool, env_mask, h->B, s);
    mask = h->pool.mask;
  }
  rc = launch_dynamics(h, nullptr, 0, nullptr, mask, kModeReset, s);
  if (rc != LBSIM_OK) return rc;
  const ObsOutputs o = obs_outputs(out, true);
  rc = launch_observe(h, o, mask, kModeReset, s);
  if (rc != LBSIM_OK) return rc;
  if (env_mask == nullptr) h->initialised = true;
  return LBSIM_OK;
}

int lbsim_step(lbsim_t* h, const void* action, int action_dtype, float* obs_out,
               float* reward_out, uint8_t* done_out, int32_t* assign_count_out, void* stream) {
  lbsim_step_outputs_t o;
  memset(&o, 0, sizeof(o));
  o.obs = obs_out;
  o.reward = reward_out;
  o.done = done_out;
  o.assign_count = assign_count_out;
  return lbsim_step_ex(h, action, action_dtype, &o, stream);
}

size_t lbsim_config_size(void) { return sizeof(lbsim_config_t); }
size_t lbsim_step_outputs_size(void) { return sizeof(lbsim_step_outputs_t); }

int lbsim_step_ex(lbsim_t* h, const void* action, int action_dtype,
                  const lbsim_step_outputs_t* out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->initialised) return fail(h, LBSIM_EINVAL, "call lbsim_reset before lbsim_step");
  if (out == nullptr || action == nullptr || out->obs == nullptr || out->reward == nullptr ||
      out->done == nullptr)
    return fail(h, LBSIM_EINVAL, "action/obs/reward/done buffers must be non-NULL");
  if (h->cfg.action_type == LBSIM_ACTION_DISCRETE) {
    if (action_dtype != LBSIM_DTYPE_I32 && action_dtype != LBSIM_DTYPE_I64)
      return fail(h, LBSIM_EINVAL, "discrete actions must be int32 or int64");
  } else if (action_dtype != LBSIM_DTYPE_F32) {
    return fail(h, LBSIM_EINVAL, "continuous actions must be float32");
  }
  if (facade_bad(h, out)) return fail(h, LBSIM_EINVAL, "agent_obs / state need num_agents * "
                                                       "servers_per_agent == num_servers");
  if (out->done_word != nullptr && h->B != 1)
    return fail(h, LBSIM_EINVAL, "done_word needs a one-env handle (num_envs = 1)");
  DeviceGuard g(h->device);
  LaunchLog log(h, 0);
  const hipStream_t s = (hipStream_t)stream;
  const ObsOutputs o = obs_outputs(out, false);
  if (sched_select(h, nullptr, kModeStep, s) != LBSIM_OK)  // a rate schedule: each env's phase
    return LBSIM_EDEVICE;
  if (trace_select(h, nullptr, kModeStep, s) != LBSIM_OK)  // a trace schedule: each env's trace
    return LBSIM_EDEVICE;
  if (avail_apply(h, s) != LBSIM_OK)  // scripted availability: each env's servers at its phase
    return LBSIM_EDEVICE;
  if (h->plan.form == kStepWave) {
    ProfScope ps(h, s, 4);
    launch_step_wave(ctx(h), action, action_dtype, out->assign_count, o, s);
    return launch_check(h, "step_wave_kernel");
  }
  if (h->plan.form == kStepGroupFused) {
    ProfScope ps(h, s, 4);
    launch_fused_step(ctx(h), action, action_dtype, out->assign_count, o, s);
    return launch_check(h, "fused_step_kernel");
  }
  h->prof.chain = true;  // dynamics then observe back to back on s: one event between them
  int rc = launch_dynamics(h, action, action_dtype, out->assign_count, nullptr, kModeStep, s);
  h->prof.chain = false;
  if (rc != LBSIM_OK) {
    h->prof.chain_ev = -1;
    return rc;
  }
  return launch_observe(h, o, nullptr, kModeStep, s);
}

int lbsim_step_stats(lbsim_t* h, int64_t* stats_out) {
  if (h == nullptr || stats_out == nullptr) return LBSIM_EINVAL;
  DeviceGuard g(h->device);
  if (h->stats_buf == nullptr && hipMalloc(&h->stats_buf, 16) != hipSuccess) {
    h->stats_buf = nullptr;
    return fail(h, LBSIM_ENOMEM, "hipMalloc(16) failed");
  }
  const int64_t n = (int64_t)h->B * h->S;
  unsigned long long host[2] = {0, 0};
  if (hipDeviceSynchronize() != hipSuccess || hipMemset(h->stats_buf, 0, 16) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "sync / memset failed");
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(step_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, nullptr, h->st.chg,
                     h->st.hc, n, h->stats_buf);
  if (hipMemcpy(host, h->stats_buf, 16, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "step_stats_kernel failed");
  stats_out[0] = (int64_t)host[0];
  stats_out[1] = (int64_t)host[1];
  return LBSIM_OK;
}

int lbsim_episode_stats(lbsim_t* h, int32_t* length_out, double* return_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  DeviceGuard g(h->device);
  hipLaunchKernelGGL(copy_episode_stats, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, h->st.ep_step, h->st.ep_return, length_out, return_out,
                     h->B);
  return launch_check(h, "copy_episode_stats");
}

int lbsim_reward(const lbsim_config_t* cfg, const float* obs, int64_t n, float* reward_out,
                 void* stream) {
  if (cfg == nullptr || obs == nullptr || reward_out == nullptr || n < 0) return LBSIM_EINVAL;
  if (cfg->num_servers < 1 || cfg->num_servers > LBSIM_MAX_SERVERS) return LBSIM_EINVAL;
  if (cfg->reward_metric < 0 || cfg->reward_metric > 8) return LBSIM_EINVAL;
  if (n == 0) return LBSIM_OK;
  hipLaunchKernelGGL(reward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, obs, n, cfg->num_servers, cfg->reward_metric,
                     cfg->reward_field, reward_out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_set_trace(lbsim_t* h, const uint32_t* gap_us, const float* work, int64_t rows,
                    void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->prm.trace) return fail(h, LBSIM_EINVAL, "lbsim_set_trace needs arrival_source TRACE");
  if (gap_us == nullptr || work == nullptr || rows < 1 || rows > (int64_t)0x7FFFFFFF)
    return fail(h, LBSIM_EINVAL, "trace: need device gap_us/work and 1 <= rows < 2^31");
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  if (hipStreamSynchronize(s) != hipSuccess) return fail(h, LBSIM_EDEVICE, "stream sync failed");
  trace_sel_drop(h);  // a new trace: every env replays it (the bank of one trace)
  h->bank_begin.clear();
  if (h->bank_begin_dev) {
    (void)hipFree(h->bank_begin_dev);
    h->bank_begin_dev = nullptr;
  }
  if (h->trace_buf) {
    (void)hipFree(h->trace_buf);
    h->trace_buf = nullptr;
    h->prm.trace_rows = 0;
  }
  const size_t n = (size_t)rows;
  if (hipMalloc(&h->trace_buf, n * 8) != hipSuccess) {
    h->trace_buf = nullptr;
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", n * 8);
  }
  uint32_t* g_dev = (uint32_t*)h->trace_buf;
  float* w_dev = (float*)(g_dev + n);
  if (hipMemcpyAsync(g_dev, gap_us, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(w_dev, work, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "trace copy failed");
  h->st.trace_gap = g_dev;
  h->st.trace_work = w_dev;
  h->prm.trace_rows = (uint32_t)rows;
  h->bank_begin = {0, rows};
  return LBSIM_OK;
}

int lbsim_set_trace_bank(lbsim_t* h, const uint32_t* gap_us, const float* work,
                         const int64_t* row_begin, int n_traces, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->prm.trace)
    return fail(h, LBSIM_EINVAL, "lbsim_set_trace_bank needs arrival_source TRACE");
  if (gap_us == nullptr || work == nullptr || row_begin == nullptr)
    return fail(h, LBSIM_EINVAL, "trace bank: need device gap_us / work and host row_begin");
  if (h->ack_max > 0 && n_traces > 1)
    return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "a trace bank");
  if (n_traces < 1 || n_traces > 4096)
    return fail(h, LBSIM_EINVAL, "trace bank: n_traces must be in [1, 4096] (got %d)", n_traces);
  if (row_begin[0] != 0) return fail(h, LBSIM_EINVAL, "trace bank: row_begin[0] must be 0");
  for (int t = 0; t < n_traces; ++t)
    if (row_begin[t + 1] <= row_begin[t])
      return fail(h, LBSIM_EINVAL, "trace bank: trace %d has no rows (row_begin must ascend)", t);
  const int64_t rows = row_begin[n_traces];
  if (rows > (int64_t)0x7FFFFFFF)
    return fail(h, LBSIM_EINVAL, "trace bank: %lld rows in all, need fewer than 2^31",
                (long long)rows);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  if (hipStreamSynchronize(s) != hipSuccess) return fail(h, LBSIM_EDEVICE, "stream sync failed");
  trace_sel_drop(h);  // a new bank: every env back on its trace 0
  const size_t n = (size_t)rows;
  // a bank of the size of the one it replaces is rewritten in place (a captured graph keeps
  // valid pointers and offsets of the same count); any other moves the buffer
  const bool same = h->trace_buf != nullptr && (int)h->bank_begin.size() == n_traces + 1 &&
                    h->bank_begin.back() == rows;
  if (!same) {
    if (h->trace_buf) (void)hipFree(h->trace_buf);
    if (h->bank_begin_dev) (void)hipFree(h->bank_begin_dev);
    h->trace_buf = nullptr;
    h->bank_begin_dev = nullptr;
    h->bank_begin.clear();
    h->prm.trace_rows = 0;
    if (hipMalloc(&h->trace_buf, n * 8) != hipSuccess) {
      h->trace_buf = nullptr;
      return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", n * 8);
    }
  }
  uint32_t* g_dev = (uint32_t*)h->trace_buf;
  float* w_dev = (float*)(g_dev + n);
  if (hipMemcpyAsync(g_dev, gap_us, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(w_dev, work, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "trace bank copy failed");
  h->st.trace_gap = g_dev;
  h->st.trace_work = w_dev;
  h->prm.trace_rows = (uint32_t)row_begin[1];  // no selection: every env on trace 0
  h->bank_begin.assign(row_begin, row_begin + n_traces + 1);
  if (h->bank_begin_dev != nullptr) {  // rewritten in place: the offsets too
    const int rc = bank_begin_upload(h);
    if (rc != LBSIM_OK) return rc;
  }
  return LBSIM_OK;
}

int lbsim_set_trace_schedule(lbsim_t* h, const int32_t* trace_id, int rows, int P,
                             int steps_per_phase, int wrap, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "a trace schedule");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "a trace schedule");
  if (!h->prm.trace)
    return fail(h, LBSIM_EINVAL, "a trace schedule needs arrival_source TRACE");
  if (h->bank_begin.empty())
    return fail(h, LBSIM_EINVAL, "trace schedule: call lbsim_set_trace_bank (or lbsim_set_trace) "
                                 "first");
  if (trace_id == nullptr) return fail(h, LBSIM_EINVAL, "trace schedule: trace_id is NULL");
  if (h->prm.lf_thr != 0u)
    return fail(h, LBSIM_ENOTSUP, "a trace selection on a lost-FIN handle (lost_fin_prob > 0): "
                                  "the bucket-wait mean is derived from the handle's one arrival "
                                  "rate (a bank with every env on trace 0 is allowed)");
  if (P < 1 || P > 4096)
    return fail(h, LBSIM_EINVAL, "trace schedule: phases must be in [1, 4096] (got %d)", P);
  if (steps_per_phase < 1)
    return fail(h, LBSIM_EINVAL, "trace schedule: steps_per_phase must be >= 1 (got %d)",
                steps_per_phase);
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "trace schedule: rows must be 1 or num_envs = %d (got %d)", h->B,
                rows);
  const size_t N = (size_t)h->B * (size_t)P;
  if (N > (size_t)INT32_MAX)
    return fail(h, LBSIM_ENOMEM, "trace schedule: num_envs * phases = %zu exceeds 2^31 - 1 table "
                                 "elements", N);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  if (h->bank_begin_dev == nullptr) {
    const int rc = bank_begin_upload(h);
    if (rc != LBSIM_OK) return rc;
  }
  // the tables: allocated by the first call for this P, rewritten in place by later ones
  void* buf = h->tsel_buf;
  const bool fresh = buf == nullptr || h->tsel_alloc_P != P;
  if (fresh && hipMalloc(&buf, trace_sel_bytes(h, P)) != hipSuccess)
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", trace_sel_bytes(h, P));
  auto give_up = [&](int code, const char* what) {
    if (fresh) (void)hipFree(buf);  // (waits for the device)
    return fail(h, code, "trace schedule: %s", what);
  };
  const TraceSelBuf t = trace_sel_at(h, buf, P);
  const int T = (int)h->bank_begin.size() - 1;
  if (hipMemsetAsync(t.bad, 0, sizeof(uint32_t), s) != hipSuccess)
    return give_up(LBSIM_EDEVICE, "hipMemsetAsync failed");
  hipLaunchKernelGGL(trace_table_kernel, dim3(blocks256(N)), dim3(256), 0, s, trace_id,
                     (int64_t)(rows == 1 ? 0 : P), h->B, P, T, t.staging, t.bad);
  if (launch_check(h, "trace_table_kernel") != LBSIM_OK) {
    if (fresh) (void)hipFree(buf);
    return LBSIM_EDEVICE;
  }
  uint32_t nbad = 0;
  if (hipMemcpyAsync(&nbad, t.bad, sizeof(nbad), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return give_up(LBSIM_EDEVICE, "conversion failed");
  if (nbad != 0u) {  // nothing live was touched: the previous selection stays in force
    if (fresh) (void)hipFree(buf);
    return fail(h, LBSIM_EINVAL, "trace schedule: %u id(s) outside [0, %d)", nbad, T);
  }
  if (hipMemcpyAsync(t.live, t.staging, N * sizeof(int32_t), hipMemcpyDeviceToDevice, s) !=
      hipSuccess)
    return give_up(LBSIM_EDEVICE, "device copy failed");
  if (fresh) {
    if (h->tsel_buf != nullptr) (void)hipFree(h->tsel_buf);  // (waits for the device)
    h->tsel_buf = buf;
    h->tsel_alloc_P = P;
  }
  h->tsel_P = P;
  h->tsel_H = steps_per_phase;
  h->tsel_wrap = wrap != 0 ? 1 : 0;
  // every env's descriptor is valid from here on: a masked reset rewrites only its own envs'
  const int rc = trace_select(h, nullptr, kModeStep, s);
  if (rc != LBSIM_OK) {
    trace_sel_drop(h);
    return rc;
  }
  set_env_trace(h->st, t.cur);
  return LBSIM_OK;
}

int lbsim_clear_trace_schedule(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->prm.trace)
    return fail(h, LBSIM_EINVAL, "a trace schedule needs arrival_source TRACE");
  const int P = h->tsel_alloc_P;
  trace_sel_drop(h);
  if (h->tsel_buf == nullptr) return LBSIM_OK;
  // a step captured into a graph while the selection was set keeps gathering from the tables:
  // they take id 0 in every phase (no stream argument: the whole device is waited for)
  DeviceGuard g(h->device);
  const TraceSelBuf t = trace_sel_at(h, h->tsel_buf, P);
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemset(t.live, 0, (size_t)h->B * (size_t)P * sizeof(int32_t)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "trace schedule: clearing the tables failed");
  return LBSIM_OK;
}

int lbsim_env_trace(lbsim_t* h, int32_t* trace_id_out, int32_t* phase_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (trace_id_out == nullptr && phase_out == nullptr) return LBSIM_OK;
  DeviceGuard g(h->device);
  const SimParams& p = h->prm;
  const int32_t* ids =
      h->tsel_P > 0 ? trace_sel_at(h, h->tsel_buf, h->tsel_P).live : (const int32_t*)nullptr;
  hipLaunchKernelGGL(trace_gather_kernel, dim3(blocks256((size_t)h->B)), dim3(256), 0,
                     (hipStream_t)stream, h->st.ep_step, (const uint8_t*)nullptr, 0, h->B,
                     h->tsel_P, h->tsel_H, h->tsel_wrap, p.max_steps, p.next_reset, ids,
                     (const uint32_t*)nullptr, (uint2*)nullptr, trace_id_out, phase_out);
  return launch_check(h, "trace_gather_kernel");
}

int lbsim_set_workload_tables(lbsim_t* h, const float* tables, int n_tables, const int32_t* gap_id,
                              const int32_t* work_id, int rows, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "workload tables");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "workload tables");
  if (h->prm.trace)
    return fail(h, LBSIM_EINVAL, "workload tables on a TRACE handle: the trace supplies gap and "
                                 "work");
  if (tables == nullptr || gap_id == nullptr || work_id == nullptr)
    return fail(h, LBSIM_EINVAL, "workload tables: tables, gap_id and work_id must not be NULL");
  if (n_tables < 1 || n_tables > kMaxWorkTables)
    return fail(h, LBSIM_EINVAL, "workload tables: n_tables must be in [1, %d] (got %d)",
                kMaxWorkTables, n_tables);
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "workload tables: rows must be 1 or num_envs = %d (got %d)", h->B,
                rows);
  DeviceGuard g(h->device);
  const int64_t stride = rows == 1 ? 0 : 1;
  const int rc = work_tables_apply(h, tables, n_tables, gap_id, stride, work_id, stride,
                                   (hipStream_t)stream);
  // a handle with tables is a full handle (make_plan): its steps and resets run
  // dynamics_group_full_kernel, the one kernel that carries the lookups
  if (rc == LBSIM_OK) h->plan = plan_of(h);
  return rc;
}

int lbsim_set_env_workload(lbsim_t* h, const int32_t* gap_id, const int32_t* work_id,
                           void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->wtab_T == 0)
    return fail(h, LBSIM_EINVAL, "env workload: no workload tables in force "
                                 "(lbsim_set_workload_tables first)");
  if (gap_id == nullptr && work_id == nullptr) return LBSIM_OK;
  DeviceGuard g(h->device);
  return work_tables_apply(h, work_tab_at(h, h->wtab_buf, h->wtab_T).live_tab, h->wtab_T, gap_id,
                           1, work_id, 1, (hipStream_t)stream);
}

int lbsim_get_env_workload(lbsim_t* h, int32_t* gap_id_out, int32_t* work_id_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->wtab_T == 0) return fail(h, LBSIM_EINVAL, "env workload: no workload tables in force");
  if (gap_id_out == nullptr && work_id_out == nullptr) return LBSIM_OK;
  DeviceGuard g(h->device);
  hipLaunchKernelGGL(work_ids_get_kernel, dim3(blocks256((size_t)h->B)), dim3(256), 0,
                     (hipStream_t)stream, work_ids(h->st), h->B, gap_id_out, work_id_out);
  return launch_check(h, "work_ids_get_kernel");
}

int lbsim_clear_workload_tables(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->prm.trace) return LBSIM_OK;  // (never had any: its two words are the trace)
  set_work_tables(h->st, nullptr, nullptr);
  h->wtab_T = 0;
  h->wtab_wmax = 0.0f;
  h->plan = plan_of(h);  // back to the kernels of a handle without tables
  return LBSIM_OK;
}

int lbsim_set_env_rates(lbsim_t* h, const float* arrival_rate, const float* server_rate,
                        void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->pool.A > 0 && server_rate != nullptr)
    return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "per-env server rates");
  if (arrival_rate != nullptr && h->prm.lf_thr != 0u)
    return fail(h, LBSIM_ENOTSUP, "per-env arrival rates on a lost-FIN handle (lost_fin_prob > 0): "
                                  "the bucket-wait mean and the 32-bit guess bound depend on the "
                                  "arrival rate (per-env server rates are allowed)");
  if (arrival_rate != nullptr && h->prm.trace)
    return fail(h, LBSIM_ENOTSUP, "per-env arrival rates on a TRACE handle: the trace sets the "
                                  "arrival rate (per-env server rates are allowed)");
  if (arrival_rate == nullptr && server_rate == nullptr) return LBSIM_OK;
  if (server_rate == nullptr && h->sched_P > 0 && h->wtab_T > 0)
    return fail(h, LBSIM_EINVAL, "per-env rates: on a handle with workload tables and a rate "
                                 "schedule, give server_rate too (dropping the schedule would "
                                 "bring back server rates the tables were not checked against)");
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  int rc = env_rates_ensure(h, s);
  if (rc != LBSIM_OK) return rc;
  const size_t B = (size_t)h->B, BS = B * h->S;
  const EnvRates live = env_rates_live(h), stg = env_rates_staging(h);
  uint32_t* const bad = env_rates_bad(h);
  const float mu_lo = mu_floor(h);
  if (hipMemsetAsync(bad, 0, sizeof(uint32_t), s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "per-env rates: hipMemsetAsync failed");
  hipLaunchKernelGGL(env_rates_kernel, dim3((unsigned)((BS + 255) / 256)), dim3(256), 0, s,
                     arrival_rate, (int64_t)1, server_rate, (int64_t)h->S, h->B, h->S, stg, bad,
                     mu_lo);
  rc = launch_check(h, "env_rates_kernel");
  if (rc != LBSIM_OK) return rc;
  uint32_t nbad = 0;
  if (hipMemcpyAsync(&nbad, bad, sizeof(nbad), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "per-env rates: conversion failed");
  if (nbad != 0u)  // the live arrays are untouched: the previous rates stay in force
    return fail(h, LBSIM_EINVAL, "per-env rates: %u value(s) out of range (arrival_rate must be in "
                                 "[0.1, 1e6] flows/s, server_rate in [%g, 1e7]; NaN rejected)", nbad,
                (double)mu_lo);
  sched_drop(h);  // (a scheduled handle: back to its per-env arrays first)
  bool ok = true;
  if (arrival_rate != nullptr) {
    ok &= hipMemcpyAsync(live.arrival, stg.arrival, B * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
    ok &= hipMemcpyAsync(live.gap, stg.gap, B * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  }
  if (server_rate != nullptr) {
    ok &= hipMemcpyAsync(live.server, stg.server, BS * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
    ok &= hipMemcpyAsync(live.scale, stg.scale, BS * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  }
  if (!ok) return fail(h, LBSIM_EDEVICE, "per-env rates: device copy failed");
  set_env_arrays(h, live.gap, live.scale);
  h->rates_on = true;
  return LBSIM_OK;
}

int lbsim_clear_env_rates(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  {  // work tables in force were validated against the rates being dropped: the config's own
     // server rates must satisfy their floor too
    const float mu_lo = mu_floor(h);
    for (int k = 0; k < h->S; ++k)
      if (h->cfg.server_rate[k] < mu_lo)
        return fail(h, LBSIM_EINVAL, "clearing the rates: the config's server_rate[%d] = %g is "
                                     "below %g, the floor of the workload tables in force (clear "
                                     "or replace the tables first)", k,
                    (double)h->cfg.server_rate[k], (double)mu_lo);
  }
  sched_drop(h);
  h->rates_on = false;
  set_env_arrays(h, nullptr, nullptr);
  if (h->rates_buf == nullptr) return LBSIM_OK;
  // a step captured into a graph while the rates were set keeps reading the live arrays: they
  // take the config's rates (no stream argument here, so the whole device is waited for)
  DeviceGuard g(h->device);
  if (hipDeviceSynchronize() != hipSuccess) return fail(h, LBSIM_EDEVICE, "sync failed");
  env_rates_fill_defaults(h, nullptr);
  const int rc = launch_check(h, "env_rates_kernel");
  if (rc != LBSIM_OK) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return fail(h, LBSIM_EDEVICE, "sync failed");
  return LBSIM_OK;
}

int lbsim_get_env_rates(lbsim_t* h, float* arrival_rate_out, float* server_rate_out,
                        void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (arrival_rate_out == nullptr && server_rate_out == nullptr) return LBSIM_OK;
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  if (h->sched_P > 0)  // a schedule: each env's rates at the phase of its next step
    return rates_in_force(h, arrival_rate_out, server_rate_out, nullptr, s);
  const int rc = env_rates_ensure(h, s);
  if (rc != LBSIM_OK) return rc;
  const size_t B = (size_t)h->B, BS = B * h->S;
  const EnvRates live = env_rates_live(h);
  bool ok = true;
  if (arrival_rate_out != nullptr)
    ok &= hipMemcpyAsync(arrival_rate_out, live.arrival, B * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (server_rate_out != nullptr)
    ok &= hipMemcpyAsync(server_rate_out, live.server, BS * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return ok ? LBSIM_OK : fail(h, LBSIM_EDEVICE, "per-env rates: device copy failed");
}

int lbsim_set_rate_schedule(lbsim_t* h, const float* arrival_rate, const float* server_rate,
                            int32_t rows, int32_t phases, int32_t steps_per_phase, int32_t wrap,
                            void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "a rate schedule");
  if (phases < 1 || phases > 4096)
    return fail(h, LBSIM_EINVAL, "rate schedule: phases must be in [1, 4096] (got %d)", phases);
  if (steps_per_phase < 1)
    return fail(h, LBSIM_EINVAL, "rate schedule: steps_per_phase must be >= 1 (got %d)",
                steps_per_phase);
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "rate schedule: rows must be 1 or num_envs = %d (got %d)", h->B,
                rows);
  if (arrival_rate != nullptr && h->prm.lf_thr != 0u)
    return fail(h, LBSIM_ENOTSUP, "an arrival schedule on a lost-FIN handle (lost_fin_prob > 0): "
                                  "the bucket-wait mean and the 32-bit guess bound depend on the "
                                  "arrival rate (server schedules are allowed)");
  if (arrival_rate != nullptr && h->prm.trace)
    return fail(h, LBSIM_ENOTSUP, "an arrival schedule on a TRACE handle: the trace sets the "
                                  "arrival rate (server schedules are allowed)");
  const int P = phases, S = h->S;
  const size_t B = (size_t)h->B, N = B * (size_t)P, NS = N * (size_t)S;
  if (NS > (size_t)INT32_MAX)
    return fail(h, LBSIM_ENOMEM, "rate schedule: num_envs * phases * num_servers = %zu exceeds "
                                 "2^31 - 1 table elements", NS);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  // the tables: allocated by the first call for this P, rewritten in place by later ones
  float* buf = h->sched_buf;
  const bool fresh = buf == nullptr || h->sched_alloc_P != P;
  if (fresh) {
    const size_t bytes = sched_floats(h, P) * sizeof(float) + sizeof(uint32_t);
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess)
      return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", bytes);
    buf = (float*)p;
  }
  auto give_up = [&](int code, const char* what) {
    if (fresh) (void)hipFree(buf);  // (waits for the device)
    return fail(h, code, "rate schedule: %s", what);
  };
  // the per-env rates in force before this call (of the old schedule's tables, when there is
  // one): what a NULL argument holds constant over the phases
  float* const base = sched_base(h, buf, P);
  int rc = rates_in_force(h, base, base + B, nullptr, s);
  if (rc != LBSIM_OK) {
    if (fresh) (void)hipFree(buf);
    return rc;
  }
  const EnvRates live = sched_live(h, buf, P), stg = sched_staging(h, buf, P);
  uint32_t* const bad = sched_bad(h, buf, P);
  if (hipMemsetAsync(bad, 0, sizeof(uint32_t), s) != hipSuccess)
    return give_up(LBSIM_EDEVICE, "hipMemsetAsync failed");
  const int64_t per_row = rows == 1 ? 0 : 1;  // one shared schedule: every env reads row 0
  const float mu_lo = mu_floor(h);
  const float* const arr_in = arrival_rate != nullptr ? arrival_rate : base;
  const float* const srv_in = server_rate != nullptr ? server_rate : base + B;
  hipLaunchKernelGGL(rate_table_kernel, dim3(blocks256(NS)), dim3(256), 0, s, arr_in,
                     arrival_rate != nullptr ? per_row * P : (int64_t)1,
                     (int64_t)(arrival_rate != nullptr ? 1 : 0), srv_in,
                     server_rate != nullptr ? per_row * P * S : (int64_t)S,
                     (int64_t)(server_rate != nullptr ? S : 0), h->B, P, S, stg, bad, mu_lo);
  if (launch_check(h, "rate_table_kernel") != LBSIM_OK) {
    if (fresh) (void)hipFree(buf);
    return LBSIM_EDEVICE;
  }
  uint32_t nbad = 0;
  if (hipMemcpyAsync(&nbad, bad, sizeof(nbad), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return give_up(LBSIM_EDEVICE, "conversion failed");
  if (nbad != 0u) {  // nothing live was touched: the previous schedule or rates stay in force
    if (fresh) (void)hipFree(buf);
    return fail(h, LBSIM_EINVAL, "rate schedule: %u value(s) out of range (arrival_rate must be in "
                                 "[0.1, 1e6] flows/s, server_rate in [%g, 1e7]; NaN rejected)", nbad,
                (double)mu_lo);
  }
  // staging over the live tables (the two halves are contiguous: one copy)
  if (hipMemcpyAsync(live.arrival, stg.arrival, 2 * (N + NS) * sizeof(float),
                     hipMemcpyDeviceToDevice, s) != hipSuccess)
    return give_up(LBSIM_EDEVICE, "device copy failed");
  if (fresh) {
    if (h->sched_buf != nullptr) (void)hipFree(h->sched_buf);  // (waits for the device)
    h->sched_buf = buf;
    h->sched_alloc_P = P;
  }
  // the dynamics kernels read the per-env arrays that sched_select fills before every launch
  float* const cur = sched_cur(h, buf, P);
  set_env_arrays(h, cur, cur + B);
  h->sched_P = P;
  h->sched_H = steps_per_phase;
  h->sched_wrap = wrap != 0 ? 1 : 0;
  return LBSIM_OK;
}

int lbsim_clear_rate_schedule(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  for (int k = 0; k < h->S; ++k)  // (as lbsim_clear_env_rates, before anything is dropped)
    if (h->cfg.server_rate[k] < mu_floor(h)) return lbsim_clear_env_rates(h);
  sched_drop(h);
  if (h->sched_buf != nullptr) {
    // a step captured into a graph while the schedule was set keeps reading the tables: they take
    // the config's rates in every phase (no stream argument: the whole device is waited for)
    DeviceGuard g(h->device);
    int rc = env_rates_ensure(h, nullptr);
    if (rc != LBSIM_OK) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return fail(h, LBSIM_EDEVICE, "sync failed");
    const float* def = env_rates_defaults(h);
    const int P = h->sched_alloc_P;
    hipLaunchKernelGGL(rate_table_kernel, dim3(blocks256((size_t)h->B * P * h->S)), dim3(256), 0,
                       nullptr, def, (int64_t)0, (int64_t)0, def + 1, (int64_t)0, (int64_t)0, h->B,
                       P, h->S, sched_live(h, h->sched_buf, P), sched_bad(h, h->sched_buf, P),
                       1.0f);
    rc = launch_check(h, "rate_table_kernel");
    if (rc != LBSIM_OK) return rc;
  }
  return lbsim_clear_env_rates(h);
}

int lbsim_rate_phase(lbsim_t* h, int32_t* phase_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (phase_out == nullptr) return LBSIM_OK;
  DeviceGuard g(h->device);
  return rates_in_force(h, nullptr, nullptr, phase_out, (hipStream_t)stream);
}

int lbsim_flow_stats_enable(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "flow statistics");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "flow statistics");
  if (h->flow_buf != nullptr) return LBSIM_OK;
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_flow_stats_enable must precede the handle's first "
                                 "lbsim_reset (the statistics change which kernels it launches)");
  DeviceGuard g(h->device);
  const size_t BS = (size_t)h->B * h->S, bytes = flow_stats_bytes(BS);
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", bytes);
  if (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(p);
    return fail(h, LBSIM_EDEVICE, "flow statistics: hipMemset failed");
  }
  h->flow_buf = p;
  h->flow.sum = (unsigned long long*)p;
  h->flow.hist = (uint32_t*)(h->flow.sum + BS);
  h->flow.count = h->flow.hist + BS * kFlowBins;
  h->flow.max_us = h->flow.count + BS;
  h->plan = plan_of(h);  // a statistics handle is a full handle (make_plan)
  return LBSIM_OK;
}

// ---- hidden cross traffic (the rule and the conversion kernel: lbsim_cross.h)

int lbsim_cross_traffic_enable(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->ps) return fail(h, LBSIM_ENOTSUP, kPsNoCompose, "cross traffic");
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "cross traffic");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "cross traffic");
  if (h->cross_buf != nullptr) return LBSIM_OK;
  if (h->prm.lf_thr != 0u)
    return fail(h, LBSIM_ENOTSUP, "cross traffic on a lost-FIN handle (lost_fin_prob > 0): the "
                                  "split reservoirs and n_flow_on_mode VPP use the lost_on "
                                  "counter with the opposite sign");
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_cross_traffic_enable must precede the handle's first "
                                 "lbsim_reset (it adds a state section and changes which kernels "
                                 "the handle launches)");
  DeviceGuard g(h->device);
  const size_t B = (size_t)h->B, BS = B * h->S;
  const size_t words = 2 * (B + BS) + 1, lost_bytes = BS * 4;
  void *p = nullptr, *lost = nullptr;
  if (hipMalloc(&p, words * 4) != hipSuccess)
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", words * 4);
  if (hipMalloc(&lost, lost_bytes) != hipSuccess) {
    (void)hipFree(p);
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", lost_bytes);
  }
  // share 0 and uniform edges in the live arrays
  uint32_t* const w = (uint32_t*)p;
  bool ok = hipMemset(p, 0, words * 4) == hipSuccess && hipMemset(lost, 0, lost_bytes) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(cross_convert_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0,
                       nullptr, (const float*)nullptr, (int64_t)0, (const float*)nullptr,
                       (int64_t)0, h->B, h->S, w, w + B, w + 2 * (B + BS));
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  if (!ok) {
    (void)hipFree(p);
    (void)hipFree(lost);
    return fail(h, LBSIM_EDEVICE, "cross traffic: device init failed");
  }
  h->cross_buf = p;
  h->cross.thr = w;
  h->cross.cum = w + B;
  h->allocs.push_back(lost);
  h->st.lost_on = (uint32_t*)lost;
  h->plan = plan_of(h);  // a cross-traffic handle is a full handle (make_plan)
  return LBSIM_OK;
}

int lbsim_set_cross_traffic(lbsim_t* h, const float* share, const float* weight, int32_t rows,
                            void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->cross_buf == nullptr)
    return fail(h, LBSIM_ENOTSUP, "cross traffic is off: call lbsim_cross_traffic_enable first");
  if (share == nullptr) return fail(h, LBSIM_EINVAL, "cross traffic: share is NULL");
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "cross traffic: rows must be 1 or num_envs = %d (got %d)", h->B,
                rows);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  const size_t B = (size_t)h->B, BS = B * h->S;
  uint32_t* const live = (uint32_t*)h->cross_buf;
  uint32_t* const stg = live + (B + BS);
  uint32_t* const bad = live + 2 * (B + BS);
  if (hipMemsetAsync(bad, 0, sizeof(uint32_t), s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "cross traffic: hipMemsetAsync failed");
  const int64_t rs = rows == 1 ? 0 : 1;
  hipLaunchKernelGGL(cross_convert_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s,
                     share, rs, weight, rs * (int64_t)h->S, h->B, h->S, stg, stg + B, bad);
  const int rc = launch_check(h, "cross_convert_kernel");
  if (rc != LBSIM_OK) return rc;
  uint32_t nbad = 0;
  if (hipMemcpyAsync(&nbad, bad, sizeof(nbad), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "cross traffic: conversion failed");
  if (nbad != 0u)  // the live arrays are untouched: the previous values stay in force
    return fail(h, LBSIM_EINVAL, "cross traffic: %u row(s) out of range (share must be in [0, 1]; "
                                 "weights finite and >= 0 with a positive sum; NaN rejected)", nbad);
  if (hipMemcpyAsync(live, stg, (B + BS) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "cross traffic: device copy failed");
  return LBSIM_OK;
}

int lbsim_get_cross_traffic(lbsim_t* h, uint32_t* thr_out, uint32_t* cum_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->cross_buf == nullptr)
    return fail(h, LBSIM_ENOTSUP, "cross traffic is off: call lbsim_cross_traffic_enable first");
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  const size_t B = (size_t)h->B, BS = B * h->S;
  bool ok = true;
  if (thr_out != nullptr)
    ok &= hipMemcpyAsync(thr_out, h->cross.thr, B * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (cum_out != nullptr)
    ok &= hipMemcpyAsync(cum_out, h->cross.cum, BS * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  return ok ? LBSIM_OK : fail(h, LBSIM_EDEVICE, "cross traffic: device copy failed");
}

int lbsim_clear_cross_traffic(lbsim_t* h, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->cross_buf == nullptr)
    return fail(h, LBSIM_ENOTSUP, "cross traffic is off: call lbsim_cross_traffic_enable first");
  DeviceGuard g(h->device);
  if (hipMemsetAsync(h->cross.thr, 0, (size_t)h->B * 4, (hipStream_t)stream) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "cross traffic: hipMemsetAsync failed");
  return LBSIM_OK;
}

// ---- multi-worker servers (the rule and the conversion kernel: lbsim_workers.h)

int lbsim_server_workers_enable(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->ps) return fail(h, LBSIM_ENOTSUP, kPsNoCompose, "server workers");
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "server workers");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "server workers");
  if (h->workers_buf != nullptr) return LBSIM_OK;
  if (h->prm.lf_thr != 0u)
    return fail(h, LBSIM_ENOTSUP, "server workers on a lost-FIN handle (lost_fin_prob > 0): the "
                                  "pending guesses rely on completion times that do not decrease "
                                  "in arrival order");
  if (h->prm.dur_service != 0)
    return fail(h, LBSIM_ENOTSUP, "server workers with duration_mode SERVICE: a carried-in "
                                  "flow's service time is not tc - max(ta, its predecessor's tc) "
                                  "on a multi-worker server, and the ring does not hold it");
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_server_workers_enable must precede the handle's first "
                                 "lbsim_reset (it changes which kernels the handle launches)");
  DeviceGuard g(h->device);
  const size_t BS = (size_t)h->B * h->S, words = 2 * BS + 1;
  void* p = nullptr;
  if (hipMalloc(&p, words * 4) != hipSuccess)
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", words * 4);
  int32_t* const w = (int32_t*)p;
  bool ok = hipMemset(p, 0, words * 4) == hipSuccess;
  if (ok) {  // every count 1 in the live array
    hipLaunchKernelGGL(workers_convert_kernel, dim3((unsigned)((BS + 255) / 256)), dim3(256), 0,
                       nullptr, (const int32_t*)nullptr, 1, (int64_t)BS, h->S, w,
                       (uint32_t*)(w + 2 * BS));
    ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  if (!ok) {
    (void)hipFree(p);
    return fail(h, LBSIM_EDEVICE, "server workers: device init failed");
  }
  h->workers_buf = p;
  h->workers.c = w;
  h->plan = plan_of(h);  // a server-workers handle is a full handle (make_plan)
  return LBSIM_OK;
}

int lbsim_set_server_workers(lbsim_t* h, const int32_t* workers, int32_t rows, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->workers_buf == nullptr)
    return fail(h, LBSIM_EINVAL, "server workers are off: call lbsim_server_workers_enable first");
  if (workers == nullptr) return fail(h, LBSIM_EINVAL, "server workers: workers is NULL");
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "server workers: rows must be 1 or num_envs = %d (got %d)", h->B,
                rows);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  const size_t BS = (size_t)h->B * h->S;
  int32_t* const live = (int32_t*)h->workers_buf;
  int32_t* const stg = live + BS;
  uint32_t* const bad = (uint32_t*)(live + 2 * BS);
  if (hipMemsetAsync(bad, 0, sizeof(uint32_t), s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "server workers: hipMemsetAsync failed");
  hipLaunchKernelGGL(workers_convert_kernel, dim3((unsigned)((BS + 255) / 256)), dim3(256), 0, s,
                     workers, (int)rows, (int64_t)BS, h->S, stg, bad);
  const int rc = launch_check(h, "workers_convert_kernel");
  if (rc != LBSIM_OK) return rc;
  uint32_t nbad = 0;
  if (hipMemcpyAsync(&nbad, bad, sizeof(nbad), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "server workers: conversion failed");
  if (nbad != 0u)  // the live array is untouched: the previous counts stay in force
    return fail(h, LBSIM_EINVAL, "server workers: %u count(s) outside [1, %d]", nbad,
                (int)kMaxWorkers);
  if (hipMemcpyAsync(live, stg, BS * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "server workers: device copy failed");
  return LBSIM_OK;
}

int lbsim_get_server_workers(lbsim_t* h, int32_t* workers_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->workers_buf == nullptr)
    return fail(h, LBSIM_EINVAL, "server workers are off: call lbsim_server_workers_enable first");
  if (workers_out == nullptr) return fail(h, LBSIM_EINVAL, "server workers: workers_out is NULL");
  DeviceGuard g(h->device);
  if (hipMemcpyAsync(workers_out, h->workers.c, (size_t)h->B * h->S * 4, hipMemcpyDeviceToDevice,
                     (hipStream_t)stream) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "server workers: device copy failed");
  return LBSIM_OK;
}

size_t lbsim_ground_truth_cols(void) { return (size_t)LBSIM_TRUTH_COLS; }

int lbsim_ground_truth(lbsim_t* h, float* truth_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (truth_out == nullptr) return fail(h, LBSIM_EINVAL, "ground truth: truth_out is NULL");
  if (((uintptr_t)truth_out & 15u) != 0u)
    return fail(h, LBSIM_EINVAL, "ground truth: truth_out must be aligned to 16 bytes");
  if (!h->initialised)
    return fail(h, LBSIM_EINVAL, "call lbsim_reset before lbsim_ground_truth");
  if (h->ps)
    return fail(h, LBSIM_ENOTSUP, "lbsim_ground_truth on a handle with processor-sharing servers "
                                  "(lbsim_processor_sharing_enable): its wait and backlog columns "
                                  "are FIFO quantities");
  if (h->pool_ps)
    return fail(h, LBSIM_ENOTSUP, "lbsim_ground_truth on a handle with pools of processor-sharing "
                                  "servers (lbsim_server_pool_enable_ps): its wait and backlog "
                                  "columns are FIFO quantities; lbsim_pool_ps_state is these "
                                  "servers' view");
  DeviceGuard g(h->device);
  if (h->pool.A > 0) {  // shared server pools: the physical servers' rows
    launch_pool_truth(ctx(h), h->pool, h->cfg.server_rate, truth_out, (hipStream_t)stream);
    return launch_check(h, "pool_truth_kernel");
  }
  TruthArgs a{};
  a.hc = h->st.hc;
  a.ring = h->st.ring;
  a.ep_step = h->st.ep_step;
  a.down = h->st.down;
  a.hidden = h->cross_buf != nullptr ? h->st.lost_on : nullptr;
  a.workers = h->workers.c;
  a.B = h->B, a.S = h->S, a.Q = h->Q;
  a.max_steps = h->prm.max_steps, a.next_reset = h->prm.next_reset;
  if (h->sched_P > 0) {  // the phase's row of the schedule's table
    a.server = sched_live(h, h->sched_buf, h->sched_P).server;
    a.P = h->sched_P, a.H = h->sched_H, a.wrap = h->sched_wrap;
  } else if (h->rates_buf != nullptr) {  // the per-env array (the config's rates while none are set)
    a.server = env_rates_live(h).server;
  }
  for (int k = 0; k < MAX_S; ++k) a.mu[k] = k < h->S ? h->cfg.server_rate[k] : 1.0f;
  hipLaunchKernelGGL(ground_truth_kernel, dim3(blocks256((size_t)h->B * h->S)), dim3(256), 0,
                     (hipStream_t)stream, a, truth_out);
  return launch_check(h, "ground_truth_kernel");
}

int lbsim_clear_server_workers(lbsim_t* h, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->workers_buf == nullptr)
    return fail(h, LBSIM_EINVAL, "server workers are off: call lbsim_server_workers_enable first");
  DeviceGuard g(h->device);
  const size_t BS = (size_t)h->B * h->S;
  int32_t* const live = (int32_t*)h->workers_buf;
  hipLaunchKernelGGL(workers_convert_kernel, dim3((unsigned)((BS + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const int32_t*)nullptr, 1, (int64_t)BS, h->S, live,
                     (uint32_t*)(live + 2 * BS));
  return launch_check(h, "workers_convert_kernel");
}

// ---- shared server pools (the rule: lbsim_pool.h, the kernels: lbsim_dyn_pool.hip)

namespace {
// lbsim_server_pool_enable (ps false) and lbsim_server_pool_enable_ps (§3.24): one rule, the
// discipline of the pool's servers a property of the pool.
int server_pool_enable(lbsim_t* h, int32_t balancers, bool ps);
}  // namespace

int lbsim_server_pool_enable(lbsim_t* h, int32_t balancers) {
  return server_pool_enable(h, balancers, false);
}
int lbsim_server_pool_enable_ps(lbsim_t* h, int32_t balancers) {
  return server_pool_enable(h, balancers, true);
}
int lbsim_server_pool_discipline(const lbsim_t* h) {
  return h != nullptr && h->pool_ps ? 1 : 0;
}

namespace {
int server_pool_enable(lbsim_t* h, int32_t balancers, bool ps) {
  if (h == nullptr) return LBSIM_EINVAL;
  switch (pool_enable_check(h->B, h->cfg.env_id_offset, balancers)) {
    case 1:
      return fail(h, LBSIM_EINVAL, "server pools: balancers must be in [1, %d] (got %d)",
                  kPoolMaxBalancers, (int)balancers);
    case 2:
      return fail(h, LBSIM_EINVAL, "server pools: num_envs = %d is no multiple of balancers = %d",
                  h->B, (int)balancers);
    case 3:
      return fail(h, LBSIM_EINVAL, "server pools: env_id_offset = %lld is no multiple of balancers "
                                   "= %d (a pool never straddles a shard)",
                  (long long)h->cfg.env_id_offset, (int)balancers);
    default: break;
  }
  if (h->pool.A > 0) {
    if (ps != h->pool_ps)
      return fail(h, LBSIM_EINVAL, "server pools are already on with %s servers",
                  h->pool_ps ? "processor-sharing" : "FIFO");
    if (balancers == h->pool.A) return LBSIM_OK;
    return fail(h, LBSIM_EINVAL, "server pools are already on with balancers = %d", (int)h->pool.A);
  }
  if (h->ps) return fail(h, LBSIM_ENOTSUP, kPsNoCompose, "server pools");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "server pools");
  // what the pool kernel has no code for (marllb_amd/pools.py check_pool_config states the
  // config's and the constructor's part of this list, with the same words, before a handle
  // exists: keep the two together; tests/test_server_pools.py walks both)
  const char* no = nullptr;
  const lbsim_config_t& c = h->cfg;
  if (h->S > kPoolMaxServers) no = "num_servers > 16";
  else if (c.assign_policy == LBSIM_POLICY_ALIAS) no = "assign_policy ALIAS";
  else if (c.arrival_source == LBSIM_ARRIVAL_TRACE) no = "arrival_source TRACE";
  else if (c.lost_fin_prob > 0.0f) no = "lost_fin_prob > 0";
  else if (c.fail_prob > 0.0f) no = "fail_prob > 0";
  else if (c.reservoir_mode == LBSIM_RESERVOIR_VPP) no = "reservoir_mode VPP";
  else if (c.n_flow_on_mode == LBSIM_NFLOW_VPP) no = "n_flow_on_mode VPP";
  else if (c.duration_mode == LBSIM_DURATION_SERVICE) no = "duration_mode SERVICE";
  else if (c.next_step_reset != 0) no = "next_step_reset";
  else if (h->flow_buf != nullptr) no = "flow statistics";
  else if (h->wtab_T > 0) no = "workload tables";
  else if (h->avail_on) no = "server availability";
  else if (h->cross_buf != nullptr) no = "cross traffic";
  else if (h->workers_buf != nullptr) no = "server workers";
  else if (h->delay_buf != nullptr) no = "action delay";
  else if (h->sched_P > 0) no = "a rate schedule";
  else if (h->rates_on)  // (they may hold per-env server rates, which a pool cannot have)
    no = "per-env rates in force (lbsim_clear_env_rates, enable, then set the arrival rates)";
  if (no != nullptr) return fail(h, LBSIM_ENOTSUP, "server pools with %s: not supported", no);
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_server_pool_enable must precede the handle's first "
                                 "lbsim_reset (it changes which kernels the handle launches)");
  DeviceGuard g(h->device);
  const size_t CS = (size_t)h->B / (size_t)balancers * (size_t)h->S;
  const size_t bytes[3] = {CS * 4, CS * (size_t)h->Q, (size_t)h->B};
  void* ptr[3] = {nullptr, nullptr, nullptr};
  bool ok = true;
  for (int i = 0; i < 3 && ok; ++i)
    ok = hipMalloc(&ptr[i], bytes[i]) == hipSuccess && hipMemset(ptr[i], 0, bytes[i]) == hipSuccess;
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    for (void* q : ptr)
      if (q != nullptr) (void)hipFree(q);
    return fail(h, LBSIM_ENOMEM, "server pools: device allocation failed");
  }
  for (void* q : ptr) h->allocs.push_back(q);
  h->pool.hc = (uint32_t*)ptr[0];
  h->pool.owner = (uint8_t*)ptr[1];
  h->pool.mask = (uint8_t*)ptr[2];
  h->pool.A = balancers;
  h->pool_ps = ps;
  h->plan = plan_of(h);  // the pool dynamics and the two-launch observe (make_plan)
  return LBSIM_OK;
}
}  // namespace

int lbsim_server_pool_size(const lbsim_t* h) { return h == nullptr ? 0 : (int)h->pool.A; }

// ---- processor-sharing servers (the rule: lbsim_ps.h, the kernel:
//      lbsim_dyn_ps.hip)

int lbsim_processor_sharing_enable(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->ps) return LBSIM_OK;
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "processor sharing");
  // what the PS kernel has no code for (marllb_amd/ps.py check_ps_config states the config's and
  // the constructor's part of this list, with the same words, before a handle exists: keep the
  // two together; tests/test_processor_sharing.py walks both)
  const char* no = nullptr;
  const lbsim_config_t& c = h->cfg;
  if (c.assign_policy == LBSIM_POLICY_ALIAS) no = "assign_policy ALIAS";
  else if (c.arrival_source == LBSIM_ARRIVAL_TRACE) no = "arrival_source TRACE";
  else if (c.lost_fin_prob > 0.0f) no = "lost_fin_prob > 0";
  else if (c.fail_prob > 0.0f) no = "fail_prob > 0";
  else if (c.reservoir_mode == LBSIM_RESERVOIR_VPP) no = "reservoir_mode VPP";
  else if (c.n_flow_on_mode == LBSIM_NFLOW_VPP) no = "n_flow_on_mode VPP";
  else if (c.duration_mode == LBSIM_DURATION_SERVICE) no = "duration_mode SERVICE";
  else if (c.next_step_reset != 0) no = "next_step_reset";
  else if (h->avail_on) no = "server availability";
  else if (h->cross_buf != nullptr) no = "cross traffic";
  else if (h->workers_buf != nullptr) no = "server workers";
  else if (h->delay_buf != nullptr) no = "action delay";
  else if (h->pool.A > 0) no = "server pools";
  if (no != nullptr) return fail(h, LBSIM_ENOTSUP, "processor sharing with %s: not supported", no);
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_processor_sharing_enable must precede the handle's first "
                                 "lbsim_reset (it changes which kernels the handle launches)");
  h->ps = true;
  h->plan = plan_of(h);  // the PS dynamics and the two-launch paired observe (make_plan)
  return LBSIM_OK;
}

int lbsim_processor_sharing(const lbsim_t* h) { return h != nullptr && h->ps ? 1 : 0; }

// ---- duration samples at every data ACK (the rule: lbsim_acks.h, the kernel:
//      lbsim_dyn_ack.hip)
namespace {
const char kAckOff[] = "%s: ack samples are off: call lbsim_ack_samples_enable first";
}  // namespace

int lbsim_ack_samples_enable(lbsim_t* h, int32_t max_acks) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!ack_max_ok(max_acks))
    return fail(h, LBSIM_EINVAL, "ack samples: max_acks must be in [1, %d] (got %d)",
                (int)kAckMaxAcks, (int)max_acks);
  if (h->ack_max > 0) {
    if (max_acks == h->ack_max) return LBSIM_OK;
    return fail(h, LBSIM_EINVAL, "ack samples are already on with max_acks = %d", (int)h->ack_max);
  }
  // what the ACK kernel has no code for, or what its model does not cover (marllb_amd/acks.py
  // check_ack_config states the config's and the constructor's part of this list, with the same
  // words, before a handle exists: keep the two together; tests/test_ack_samples.py walks both)
  const char* no = nullptr;
  const lbsim_config_t& c = h->cfg;
  if (c.lost_fin_prob > 0.0f) no = "lost_fin_prob > 0";
  else if (c.fail_prob > 0.0f) no = "fail_prob > 0";
  else if (c.duration_mode == LBSIM_DURATION_SERVICE) no = "duration_mode SERVICE";
  else if (c.reservoir_mode == LBSIM_RESERVOIR_VPP) no = "reservoir_mode VPP";
  else if (c.n_flow_on_mode == LBSIM_NFLOW_VPP) no = "n_flow_on_mode VPP";
  else if (c.next_step_reset != 0) no = "next_step_reset";
  else if (h->avail_on) no = "server availability";
  else if (h->cross_buf != nullptr) no = "cross traffic";
  else if (h->workers_buf != nullptr) no = "server workers";
  else if (h->delay_buf != nullptr) no = "action delay";
  else if (h->pool.A > 0) no = "server pools";
  else if (h->ps) no = "processor sharing";
  else if (h->flow_buf != nullptr) no = "flow statistics";
  else if (h->wtab_T > 0) no = "workload tables";
  else if (h->bank_begin.size() > 2) no = "a trace bank";
  else if (h->tsel_P > 0) no = "a trace schedule";
  if (no != nullptr) return fail(h, LBSIM_ENOTSUP, "ack samples with %s: not supported", no);
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_ack_samples_enable must precede the handle's first "
                                 "lbsim_reset (it adds state sections and changes which kernels "
                                 "the handle launches)");
  DeviceGuard g(h->device);
  // the duration reservoir's {us, ts} records and its count (zeroed), and the intervals
  const size_t BS = (size_t)h->B * h->S;
  const size_t bytes[3] = {BS * K * 8, BS * 4, (size_t)h->B * 4};
  void* p[3] = {nullptr, nullptr, nullptr};
  bool ok = true;
  for (int i = 0; i < 3 && ok; ++i)
    ok = hipMalloc(&p[i], bytes[i]) == hipSuccess && hipMemset(p[i], 0, bytes[i]) == hipSuccess;
  std::vector<int32_t> us((size_t)h->B, kAckDefaultInterval);
  ok = ok && hipMemcpy(p[2], us.data(), bytes[2], hipMemcpyHostToDevice) == hipSuccess &&
       hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    for (void* q : p)
      if (q != nullptr) (void)hipFree(q);
    return fail(h, LBSIM_ENOMEM, "ack samples: device allocation failed");
  }
  for (void* q : p) h->allocs.push_back(q);
  h->st.res_dur = (uint32_t*)p[0];
  h->st.res_count_dur = (uint32_t*)p[1];
  h->ack_us = (int32_t*)p[2];
  h->ack_max = max_acks;
  h->plan = plan_of(h);  // the ACK dynamics and the general observe (make_plan)
  return LBSIM_OK;
}

int lbsim_ack_samples(const lbsim_t* h) { return h != nullptr ? (int)h->ack_max : 0; }

int lbsim_set_ack_interval(lbsim_t* h, const int32_t* us, int rows) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->ack_max == 0) return fail(h, LBSIM_ENOTSUP, kAckOff, "lbsim_set_ack_interval");
  if (us == nullptr) return fail(h, LBSIM_EINVAL, "ack interval: us is NULL");
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "ack interval: rows must be 1 or num_envs = %d (got %d)", h->B,
                rows);
  for (int i = 0; i < rows; ++i)
    if (!ack_interval_ok(us[i]))  // the device array is untouched: the previous intervals stay
      return fail(h, LBSIM_EINVAL, "ack interval: us[%d] = %d is not in [1, 2^30]", i, (int)us[i]);
  std::vector<int32_t> v((size_t)h->B);
  for (int b = 0; b < h->B; ++b) v[(size_t)b] = us[rows == 1 ? 0 : b];
  DeviceGuard g(h->device);
  if (hipMemcpy(h->ack_us, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "ack interval: hipMemcpy H2D failed");
  return LBSIM_OK;
}

int lbsim_get_ack_interval(lbsim_t* h, int32_t* us_out) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->ack_max == 0) return fail(h, LBSIM_ENOTSUP, kAckOff, "lbsim_get_ack_interval");
  if (us_out == nullptr) return fail(h, LBSIM_EINVAL, "ack interval: us_out is NULL");
  DeviceGuard g(h->device);
  if (hipMemcpy(us_out, h->ack_us, (size_t)h->B * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "ack interval: hipMemcpy D2H failed");
  return LBSIM_OK;
}

int lbsim_clear_ack_interval(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->ack_max == 0) return fail(h, LBSIM_ENOTSUP, kAckOff, "lbsim_clear_ack_interval");
  const int32_t us = kAckDefaultInterval;
  return lbsim_set_ack_interval(h, &us, 1);
}

// ---- cores of processor-sharing servers (the rule: lbsim_ps.h; the conversion
//      is lbsim_workers.h's kernel: the same range, the same offender count)
namespace {
const char kPsCoresOff[] = "%s on a handle without processor-sharing servers: call "
                           "lbsim_processor_sharing_enable first";
static_assert(kMaxWorkers == 64, "a PS server has 1 to 64 cores, a FIFO one 1 to 64 workers");

// The three cores calls over one block of N = units * S counts: `buf` is the handle's
// ps_cores_buf (units = num_envs, what = "ps cores") or pool_ps_cores_buf (units = the pools,
// what = "pool ps cores", §3.24); unit_name names the row count a caller may pass.
int cores_set(lbsim_t* h, int32_t*& buf, int units, const char* what, const char* unit_name,
              const int32_t* cores, int32_t rows, void* stream) {
  if (cores == nullptr) return fail(h, LBSIM_EINVAL, "%s: cores is NULL", what);
  if (rows != 1 && rows != units)
    return fail(h, LBSIM_ESHAPE, "%s: rows must be 1 or %s = %d (got %d)", what, unit_name, units,
                rows);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)units * h->S, words = 2 * N + 1;
  const bool first = buf == nullptr;
  int32_t* live = buf;
  if (first) {  // (the first call: before a graph capture, as §3.10's rate arrays)
    void* p = nullptr;
    if (hipMalloc(&p, words * 4) != hipSuccess)
      return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", words * 4);
    live = (int32_t*)p;
  }
  int32_t* const stg = live + N;
  uint32_t* const bad = (uint32_t*)(live + 2 * N);
  int rc = LBSIM_OK;
  uint32_t nbad = 0;
  if (hipMemsetAsync(bad, 0, sizeof(uint32_t), s) != hipSuccess) {
    rc = fail(h, LBSIM_EDEVICE, "%s: hipMemsetAsync failed", what);
  } else {
    hipLaunchKernelGGL(workers_convert_kernel, dim3(blocks256(N)), dim3(256), 0, s, cores,
                       (int)rows, (int64_t)N, h->S, stg, bad);
    rc = launch_check(h, "workers_convert_kernel");
    if (rc == LBSIM_OK &&
        (hipMemcpyAsync(&nbad, bad, sizeof(nbad), hipMemcpyDeviceToHost, s) != hipSuccess ||
         hipStreamSynchronize(s) != hipSuccess))
      rc = fail(h, LBSIM_EDEVICE, "%s: conversion failed", what);
  }
  if (rc == LBSIM_OK && nbad != 0u)  // what was in force stays (before the first call: one each)
    rc = fail(h, LBSIM_EINVAL, "%s: %u count(s) outside [1, %d]", what, nbad, (int)kMaxWorkers);
  if (rc == LBSIM_OK &&
      hipMemcpyAsync(live, stg, N * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    rc = fail(h, LBSIM_EDEVICE, "%s: device copy failed", what);
  if (first) {
    // the block is the handle's only once it holds valid counts (the copy is ordered on s before
    // every later launch of the caller's on it, as a set call's always is)
    if (rc == LBSIM_OK) {
      buf = live;
    } else {
      (void)hipStreamSynchronize(s);
      (void)hipFree(live);
    }
  }
  return rc;
}

int cores_get(lbsim_t* h, const int32_t* buf, int units, const char* what, int32_t* cores_out,
              void* stream) {
  if (cores_out == nullptr) return fail(h, LBSIM_EINVAL, "%s: cores_out is NULL", what);
  DeviceGuard g(h->device);
  const size_t N = (size_t)units * h->S;
  if (buf == nullptr) {  // never set: every count 1 (no offender: bad is not touched)
    hipLaunchKernelGGL(workers_convert_kernel, dim3(blocks256(N)), dim3(256), 0,
                       (hipStream_t)stream, (const int32_t*)nullptr, 1, (int64_t)N, h->S,
                       cores_out, (uint32_t*)nullptr);
    return launch_check(h, "workers_convert_kernel");
  }
  if (hipMemcpyAsync(cores_out, buf, N * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
      hipSuccess)
    return fail(h, LBSIM_EDEVICE, "%s: device copy failed", what);
  return LBSIM_OK;
}

int cores_clear(lbsim_t* h, int32_t* buf, int units, void* stream) {
  if (buf == nullptr) return LBSIM_OK;  // never set: one core each already
  DeviceGuard g(h->device);
  const size_t N = (size_t)units * h->S;
  hipLaunchKernelGGL(workers_convert_kernel, dim3(blocks256(N)), dim3(256), 0,
                     (hipStream_t)stream, (const int32_t*)nullptr, 1, (int64_t)N, h->S, buf,
                     (uint32_t*)(buf + 2 * N));
  return launch_check(h, "workers_convert_kernel");
}
}  // namespace

int lbsim_set_ps_cores(lbsim_t* h, const int32_t* cores, int32_t rows, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->ps) return fail(h, LBSIM_ENOTSUP, kPsCoresOff, "lbsim_set_ps_cores");
  return cores_set(h, h->ps_cores_buf, h->B, "ps cores", "num_envs", cores, rows, stream);
}

int lbsim_get_ps_cores(lbsim_t* h, int32_t* cores_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->ps) return fail(h, LBSIM_ENOTSUP, kPsCoresOff, "lbsim_get_ps_cores");
  return cores_get(h, h->ps_cores_buf, h->B, "ps cores", cores_out, stream);
}

int lbsim_clear_ps_cores(lbsim_t* h, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->ps) return fail(h, LBSIM_ENOTSUP, kPsCoresOff, "lbsim_clear_ps_cores");
  return cores_clear(h, h->ps_cores_buf, h->B, stream);
}

// ---- pools of processor-sharing servers (the kernels: lbsim_dyn_pool_ps.hip):
//      the physical servers' cores, one row per pool, and their privileged view
namespace {
const char kPoolPsOff[] = "%s on a handle without pools of processor-sharing servers: call "
                          "lbsim_server_pool_enable_ps first";
int pool_count(const lbsim_t* h) { return h->B / (int)h->pool.A; }
}  // namespace

int lbsim_set_pool_ps_cores(lbsim_t* h, const int32_t* cores, int32_t rows, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->pool_ps) return fail(h, LBSIM_ENOTSUP, kPoolPsOff, "lbsim_set_pool_ps_cores");
  return cores_set(h, h->pool_ps_cores_buf, pool_count(h), "pool ps cores", "the pools", cores,
                   rows, stream);
}

int lbsim_get_pool_ps_cores(lbsim_t* h, int32_t* cores_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->pool_ps) return fail(h, LBSIM_ENOTSUP, kPoolPsOff, "lbsim_get_pool_ps_cores");
  return cores_get(h, h->pool_ps_cores_buf, pool_count(h), "pool ps cores", cores_out, stream);
}

int lbsim_clear_pool_ps_cores(lbsim_t* h, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->pool_ps) return fail(h, LBSIM_ENOTSUP, kPoolPsOff, "lbsim_clear_pool_ps_cores");
  return cores_clear(h, h->pool_ps_cores_buf, pool_count(h), stream);
}

size_t lbsim_pool_ps_state_cols(void) { return (size_t)LBSIM_POOL_PS_STATE_COLS; }

int lbsim_pool_ps_state(lbsim_t* h, float* state_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->pool_ps) return fail(h, LBSIM_ENOTSUP, kPoolPsOff, "lbsim_pool_ps_state");
  if (state_out == nullptr) return fail(h, LBSIM_EINVAL, "pool ps state: state_out is NULL");
  if (((uintptr_t)state_out & 3u) != 0u)
    return fail(h, LBSIM_EINVAL, "pool ps state: state_out must be aligned to 4 bytes");
  if (!h->initialised)
    return fail(h, LBSIM_EINVAL, "call lbsim_reset before lbsim_pool_ps_state");
  DeviceGuard g(h->device);
  launch_pool_ps_state(ctx(h), h->pool, h->pool_ps_cores_buf, state_out, (hipStream_t)stream);
  return launch_check(h, "pool_ps_state_kernel");
}

size_t lbsim_ps_server_state_cols(void) { return (size_t)LBSIM_PS_STATE_COLS; }

int lbsim_ps_server_state(lbsim_t* h, float* state_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->ps) return fail(h, LBSIM_ENOTSUP, kPsCoresOff, "lbsim_ps_server_state");
  if (state_out == nullptr) return fail(h, LBSIM_EINVAL, "ps server state: state_out is NULL");
  if (((uintptr_t)state_out & 15u) != 0u)
    return fail(h, LBSIM_EINVAL, "ps server state: state_out must be aligned to 16 bytes");
  if (!h->initialised)
    return fail(h, LBSIM_EINVAL, "call lbsim_reset before lbsim_ps_server_state");
  DeviceGuard g(h->device);
  PsStateArgs a{};
  a.hc = h->st.hc;
  a.ring = h->st.ring;
  a.acc = h->st.last_tc;
  a.cores = h->ps_cores_buf;
  a.B = h->B, a.S = h->S, a.Q = h->Q;
  hipLaunchKernelGGL(ps_state_kernel, dim3(blocks256((size_t)h->B * h->S)), dim3(256), 0,
                     (hipStream_t)stream,
                     a, state_out);
  return launch_check(h, "ps_state_kernel");
}

// ---- action latency (the rule and the kernels: lbsim_delay.h)
namespace {
const char kDelayOff[] = "action delay is off: call lbsim_action_delay_enable first";
size_t delay_ring_words(const lbsim_t* h) {
  return (size_t)h->B * (size_t)h->delay.R * (size_t)h->S;
}
uint32_t* delay_live(lbsim_t* h) { return (uint32_t*)h->delay_buf + delay_ring_words(h); }
int delay_convert_launch(lbsim_t* h, const float* src, int rows, uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(delay_convert_kernel, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, s,
                     src, rows, (int32_t)h->B, h->delay_M, (int32_t)h->prm.dt_us, out,
                     delay_live(h) + 2 * (size_t)h->B);
  return launch_check(h, "delay_convert_kernel");
}
int delay_gather(lbsim_t* h, const char* who, void* dev_buf, size_t bytes, const uint8_t* mask,
                 const int32_t* src_env, int dir, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->delay_buf == nullptr) return fail(h, LBSIM_EINVAL, "%s", kDelayOff);
  if (dev_buf == nullptr) return fail(h, LBSIM_EINVAL, "%s: dev_buf is NULL", who);
  const size_t words = delay_ring_words(h);
  if (bytes != words * 4)
    return fail(h, LBSIM_ESHAPE, "%s: the buffer is %zu bytes, need %zu", who, bytes, words * 4);
  DeviceGuard g(h->device);
  hipLaunchKernelGGL(delay_gather_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, h->delay.wring, (float*)dev_buf, mask, src_env, dir,
                     (int32_t)h->B, (int32_t)(h->delay.R * h->S));
  return launch_check(h, "delay_gather_kernel");
}
}  // namespace

int lbsim_action_delay_enable(lbsim_t* h, int32_t max_delay_steps) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "action delay");
  if (h->ps) return fail(h, LBSIM_ENOTSUP, kPsNoCompose, "action delay");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "action delay");
  if (!delay_steps_ok(max_delay_steps))
    return fail(h, LBSIM_EINVAL, "action delay: max_delay_steps must be in [1, %d] (got %d)",
                (int)kMaxDelaySteps, (int)max_delay_steps);
  if (h->delay_buf != nullptr) {
    if (max_delay_steps == h->delay_M) return LBSIM_OK;
    return fail(h, LBSIM_EINVAL, "action delay is already on with max_delay_steps = %d",
                (int)h->delay_M);
  }
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_action_delay_enable must precede the handle's first "
                                 "lbsim_reset (it changes which kernels the handle launches)");
  DeviceGuard g(h->device);
  const int32_t R = delay_rows(max_delay_steps);
  const size_t ring = (size_t)h->B * (size_t)R * (size_t)h->S, words = ring + 2 * (size_t)h->B + 1;
  if (ring > 0x7FFFFFFFu)  // (the gather kernel's row arithmetic and the launch's grid)
    return fail(h, LBSIM_ENOTSUP, "action delay: a weight ring of %zu words", ring);
  void* p = nullptr;
  if (hipMalloc(&p, words * 4) != hipSuccess)
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", words * 4);
  // a zeroed ring (no row is read before the episode wrote it; a snapshot of it is then defined)
  // and every delay 0
  if (hipMemset(p, 0, words * 4) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(p);
    return fail(h, LBSIM_EDEVICE, "action delay: device init failed");
  }
  h->delay_buf = p;
  h->delay_M = max_delay_steps;
  h->delay.wring = (float*)p;
  h->delay.delay_us = (const uint32_t*)p + ring;
  h->delay.R = R;
  h->plan = plan_of(h);  // an action-delay handle is a full handle (make_plan)
  return LBSIM_OK;
}

int lbsim_set_action_delay(lbsim_t* h, const float* delay_s, int32_t rows, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->delay_buf == nullptr) return fail(h, LBSIM_EINVAL, "%s", kDelayOff);
  if (delay_s == nullptr) return fail(h, LBSIM_EINVAL, "action delay: delay_s is NULL");
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "action delay: rows must be 1 or num_envs = %d (got %d)", h->B,
                rows);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  uint32_t* const live = delay_live(h);
  uint32_t* const stg = live + h->B;
  uint32_t* const bad = live + 2 * (size_t)h->B;
  if (hipMemsetAsync(bad, 0, sizeof(uint32_t), s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "action delay: hipMemsetAsync failed");
  const int rc = delay_convert_launch(h, delay_s, (int)rows, stg, s);
  if (rc != LBSIM_OK) return rc;
  uint32_t nbad = 0;
  if (hipMemcpyAsync(&nbad, bad, sizeof(nbad), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "action delay: conversion failed");
  if (nbad != 0u)  // the live array is untouched: the previous delays stay in force
    return fail(h, LBSIM_EINVAL, "action delay: %u delay(s) NaN, negative or above "
                                 "max_delay_steps * step_interval = %u us", nbad,
                delay_max_us(h->delay_M, h->prm.dt_us));
  if (hipMemcpyAsync(live, stg, (size_t)h->B * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "action delay: device copy failed");
  return LBSIM_OK;
}

int lbsim_get_action_delay(lbsim_t* h, uint32_t* delay_us_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->delay_buf == nullptr) return fail(h, LBSIM_EINVAL, "%s", kDelayOff);
  if (delay_us_out == nullptr) return fail(h, LBSIM_EINVAL, "action delay: delay_us_out is NULL");
  DeviceGuard g(h->device);
  if (hipMemcpyAsync(delay_us_out, h->delay.delay_us, (size_t)h->B * 4, hipMemcpyDeviceToDevice,
                     (hipStream_t)stream) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "action delay: device copy failed");
  return LBSIM_OK;
}

int lbsim_clear_action_delay(lbsim_t* h, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->delay_buf == nullptr) return fail(h, LBSIM_EINVAL, "%s", kDelayOff);
  DeviceGuard g(h->device);
  return delay_convert_launch(h, nullptr, 1, delay_live(h), (hipStream_t)stream);
}

int lbsim_action_delay_size(const lbsim_t* h, size_t* bytes_out) {
  if (h == nullptr || bytes_out == nullptr) return LBSIM_EINVAL;
  if (h->delay_buf == nullptr) return fail(const_cast<lbsim_t*>(h), LBSIM_EINVAL, "%s", kDelayOff);
  *bytes_out = delay_ring_words(h) * 4;
  return LBSIM_OK;
}

int lbsim_action_delay_save(lbsim_t* h, void* dev_buf, size_t bytes, const uint8_t* env_mask,
                            void* stream) {
  return delay_gather(h, "lbsim_action_delay_save", dev_buf, bytes, env_mask, nullptr, 0, stream);
}

int lbsim_action_delay_load(lbsim_t* h, const void* dev_buf, size_t bytes, const int32_t* src_env,
                            void* stream) {
  return delay_gather(h, "lbsim_action_delay_load", const_cast<void*>(dev_buf), bytes, nullptr,
                      src_env, 1, stream);
}

int lbsim_server_avail_enable(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->pool.A > 0) return fail(h, LBSIM_ENOTSUP, kPoolNoCompose, "server availability");
  if (h->ps) return fail(h, LBSIM_ENOTSUP, kPsNoCompose, "server availability");
  if (h->ack_max > 0) return fail(h, LBSIM_ENOTSUP, kAckNoCompose, "server availability");
  if (h->avail_on) return LBSIM_OK;
  if (h->prm.fail_thr != 0u)
    return fail(h, LBSIM_ENOTSUP, "scripted availability on a handle with random failures "
                                  "(fail_prob > 0): a random recovery would bring a scripted-down "
                                  "server back");
  if (h->reset_seen)
    return fail(h, LBSIM_EINVAL, "lbsim_server_avail_enable must precede the handle's first "
                                 "lbsim_reset (it adds a state section and changes which kernels "
                                 "the handle launches)");
  DeviceGuard g(h->device);
  // the down section (fail_thr == 0 means fail_prob == 0: the config allocated none)
  const size_t bytes = (size_t)h->B * h->S * 4;
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess)
    return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", bytes);
  if (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    (void)hipFree(p);
    return fail(h, LBSIM_EDEVICE, "server availability: hipMemset failed");
  }
  h->allocs.push_back(p);
  h->st.down = (uint32_t*)p;
  h->avail_on = true;
  h->plan = plan_of(h);  // planned as a handle with failures: no one-wave kernel (make_plan)
  return LBSIM_OK;
}

int lbsim_set_server_avail(lbsim_t* h, const uint8_t* up, int32_t rows, int32_t phases,
                           int32_t steps_per_phase, int32_t wrap, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->avail_on)
    return fail(h, LBSIM_ENOTSUP, "server availability is off: call lbsim_server_avail_enable "
                                  "first");
  if (up == nullptr) return fail(h, LBSIM_EINVAL, "server availability: up is NULL");
  if (phases < 1 || phases > kAvailMaxPhases)
    return fail(h, LBSIM_EINVAL, "server availability: phases must be in [1, %d] (got %d)",
                kAvailMaxPhases, phases);
  if (steps_per_phase < 1)
    return fail(h, LBSIM_EINVAL, "server availability: steps_per_phase must be >= 1 (got %d)",
                steps_per_phase);
  if (rows != 1 && rows != h->B)
    return fail(h, LBSIM_ESHAPE, "server availability: rows must be 1 or num_envs = %d (got %d)",
                h->B, rows);
  const int P = phases;
  const size_t per_env = (size_t)P * (size_t)h->S, n = (size_t)h->B * per_env;
  if (n > (size_t)INT32_MAX)
    return fail(h, LBSIM_ENOMEM, "server availability: num_envs * phases * num_servers = %zu "
                                 "exceeds 2^31 - 1 table entries", n);
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  // the table: allocated by the first call for this P, rewritten in place by later ones
  if (h->avail_buf == nullptr || h->avail_alloc_P != P) {
    void* p = nullptr;
    if (hipMalloc(&p, n) != hipSuccess) return fail(h, LBSIM_ENOMEM, "hipMalloc(%zu) failed", n);
    if (h->avail_buf != nullptr) (void)hipFree(h->avail_buf);  // (waits for the device)
    h->avail_buf = (uint8_t*)p;
    h->avail_alloc_P = P;
    h->avail_P = 0;  // (until the table below is in place)
  }
  hipLaunchKernelGGL(avail_table_kernel, dim3(blocks256(n)), dim3(256), 0, s, up,
                     rows == 1 ? (int64_t)0 : (int64_t)per_env, (int64_t)per_env, (int64_t)n,
                     h->avail_buf);
  const int rc = launch_check(h, "avail_table_kernel");
  if (rc != LBSIM_OK) return rc;
  h->avail_P = P;
  h->avail_H = steps_per_phase;
  h->avail_wrap = wrap != 0 ? 1 : 0;
  return LBSIM_OK;
}

int lbsim_clear_server_avail(lbsim_t* h) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->avail_on)
    return fail(h, LBSIM_ENOTSUP, "server availability is off: call lbsim_server_avail_enable "
                                  "first");
  h->avail_P = h->avail_H = h->avail_wrap = 0;
  if (h->avail_buf != nullptr) {
    // a step captured into a graph while the table was set keeps reading it: every server up in
    // every phase (no stream argument: the whole device is waited for)
    DeviceGuard g(h->device);
    const size_t n = (size_t)h->B * (size_t)h->avail_alloc_P * (size_t)h->S;
    if (hipDeviceSynchronize() != hipSuccess || hipMemset(h->avail_buf, 1, n) != hipSuccess)
      return fail(h, LBSIM_EDEVICE, "server availability: clearing the table failed");
  }
  return LBSIM_OK;
}

int lbsim_get_server_avail(lbsim_t* h, uint8_t* want_out, uint8_t* up_now_out, int32_t* phase_out,
                           void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (!h->avail_on)
    return fail(h, LBSIM_ENOTSUP, "server availability is off: call lbsim_server_avail_enable "
                                  "first");
  if (want_out == nullptr && up_now_out == nullptr && phase_out == nullptr) return LBSIM_OK;
  DeviceGuard g(h->device);
  hipLaunchKernelGGL(avail_apply_kernel, dim3(blocks256((size_t)h->B * h->S)), dim3(256), 0,
                     (hipStream_t)stream, avail_state(h), avail_table(h),
                     AvailOut{want_out, up_now_out, phase_out}, 0, (uint32_t*)nullptr);
  return launch_check(h, "avail_apply_kernel");
}

int lbsim_flow_stats_get(lbsim_t* h, uint32_t* count, uint64_t* sum_us, uint32_t* max_us,
                         uint32_t* hist, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->flow_buf == nullptr)
    return fail(h, LBSIM_ENOTSUP, "flow statistics are off: call lbsim_flow_stats_enable first");
  DeviceGuard g(h->device);
  const hipStream_t s = (hipStream_t)stream;
  const size_t BS = (size_t)h->B * h->S;
  const FlowStats& f = h->flow;
  bool ok = true;
  if (count != nullptr)
    ok &= hipMemcpyAsync(count, f.count, BS * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (sum_us != nullptr)
    ok &= hipMemcpyAsync(sum_us, f.sum, BS * 8, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (max_us != nullptr)
    ok &= hipMemcpyAsync(max_us, f.max_us, BS * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (hist != nullptr)
    ok &= hipMemcpyAsync(hist, f.hist, BS * kFlowBins * 4, hipMemcpyDeviceToDevice, s) ==
          hipSuccess;
  return ok ? LBSIM_OK : fail(h, LBSIM_EDEVICE, "flow statistics: device copy failed");
}

int lbsim_flow_stats_quantiles(lbsim_t* h, const uint32_t* q_ppm, int nq, int per_server,
                               uint32_t* out_us, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->flow_buf == nullptr)
    return fail(h, LBSIM_ENOTSUP, "flow statistics are off: call lbsim_flow_stats_enable first");
  if (q_ppm == nullptr || out_us == nullptr || nq < 1 || nq > 16)
    return fail(h, LBSIM_EINVAL, "flow quantiles: need device q_ppm / out_us and 1 <= nq <= 16 "
                                 "(got %d)", nq);
  DeviceGuard g(h->device);
  const size_t rows = per_server ? (size_t)h->B * h->S : (size_t)h->B;
  hipLaunchKernelGGL(flow_quantiles_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream,
                     h->flow.hist, h->flow.max_us, q_ppm, nq, h->S, per_server ? 1 : 0, out_us);
  return launch_check(h, "flow_quantiles_kernel");
}

int lbsim_flow_stats_clear(lbsim_t* h, const uint8_t* env_mask, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (h->flow_buf == nullptr)
    return fail(h, LBSIM_ENOTSUP, "flow statistics are off: call lbsim_flow_stats_enable first");
  DeviceGuard g(h->device);
  const int64_t n = (int64_t)h->B * h->S * kFlowBins;
  hipLaunchKernelGGL(flow_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, h->flow.count, h->flow.sum, h->flow.max_us,
                     h->flow.hist, n, h->S, env_mask);
  return launch_check(h, "flow_clear_kernel");
}

int lbsim_agent_obs(const float* obs, int64_t n, int S, int num_agents, int servers_per_agent,
                    float* out, void* stream) {
  if (n < 0 || S < 1 || S > LBSIM_MAX_SERVERS || num_agents < 1 || servers_per_agent < 1 ||
      num_agents * servers_per_agent != S)
    return LBSIM_EINVAL;
  if (n == 0) return LBSIM_OK;
  if (!obs || !out) return LBSIM_EINVAL;
  const int64_t total = n * num_agents * (4 * servers_per_agent + 7 * S);
  hipLaunchKernelGGL(agent_obs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, obs, n, S, num_agents, servers_per_agent, out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_gru_gates(const float* gi, const float* gh, const float* h, float* h_out, int64_t B,
                    int H, void* stream) {
  if (B < 0 || H < 1 || (B > 0 && (!gi || !gh || !h || !h_out))) return LBSIM_EINVAL;
  if (B == 0) return LBSIM_OK;
  const int64_t n = B * H;
  hipLaunchKernelGGL(gru_gates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, gi, gh, h, h_out, B, H);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_sac_head(const float* y, int64_t B, int A, float log_std_min, float log_std_max,
                   float action_scale, float action_bias, int deterministic, uint64_t seed,
                   uint32_t step, float* action_out, float* log_std_out, void* stream) {
  if (B < 0 || A < 1 || (B > 0 && (!y || !action_out))) return LBSIM_EINVAL;
  if (B == 0) return LBSIM_OK;
  const int64_t n = B * A;
  hipLaunchKernelGGL(sac_head_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, y, B, A, log_std_min, log_std_max, action_scale,
                     action_bias, deterministic, (uint32_t)(seed & 0xFFFFFFFFull),
                     (uint32_t)(seed >> 32), step, action_out, log_std_out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_qmix_tail(const float* q, const float* w1, int64_t w1_ld, const float* b1,
                    int64_t b1_ld, const float* w2, int64_t w2_ld, const float* b2, int64_t b2_ld,
                    int64_t B, int A, int E, float* q_tot, void* stream) {
  if (B < 0 || A < 1 || E < 1) return LBSIM_EINVAL;
  if (B == 0) return LBSIM_OK;
  if (!q || !w1 || !b1 || !w2 || !b2 || !q_tot) return LBSIM_EINVAL;
  hipLaunchKernelGGL(qmix_tail_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, q, w1, w1_ld, b1, b1_ld, w2, w2_ld, b2, b2_ld, B, A, E,
                     q_tot);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

size_t lbsim_sac_actor_size(void) { return sizeof(lbsim_sac_actor_t); }
size_t lbsim_qmix_policy_size(void) { return sizeof(lbsim_qmix_policy_t); }

int lbsim_sac_actor_step(const lbsim_sac_actor_t* n, const float* state, float* hidden,
                         const uint8_t* reset_mask, int64_t B, int deterministic, uint64_t seed,
                         uint32_t step, float* action_out, float* log_std_out, void* stream) {
  if (n == nullptr || B < 0 || n->state_dim < 1 || n->state_dim > 512 || n->action_dim < 1 ||
      n->action_dim > 16)
    return LBSIM_EINVAL;
  if (n->gru_dim != 128 || n->hidden_dim != 256) return LBSIM_ENOTSUP;
  if (B == 0) return LBSIM_OK;
  if (!state || !hidden || !action_out || !n->w_ih || !n->w_hh || !n->b_ih || !n->b_hh ||
      !n->w1 || !n->b1 || !n->wh || !n->bh)
    return LBSIM_EINVAL;
  SacActorArgs a{};
  a.state = state;
  a.hidden = hidden;
  a.reset = reset_mask;
  a.w_ih = n->w_ih;
  a.w_hh = n->w_hh;
  a.b_ih = n->b_ih;
  a.b_hh = n->b_hh;
  a.w1 = n->w1;
  a.b1 = n->b1;
  a.wh = n->wh;
  a.bh = n->bh;
  a.action = action_out;
  a.log_std = log_std_out;
  a.B = B;
  a.I = n->state_dim;
  a.kxp = round16(n->state_dim);
  a.A = n->action_dim;
  a.lo = n->log_std_min;
  a.hi = n->log_std_max;
  a.scale = n->action_scale;
  a.bias = n->action_bias;
  a.deterministic = deterministic;
  a.key0 = (uint32_t)(seed & 0xFFFFFFFFull);
  a.key1 = (uint32_t)(seed >> 32);
  a.step = step;
  a.step_dev = n->step_dev;
  return launch_sac_actor(a, B, fused_mt(2), (hipStream_t)stream);
}

int lbsim_qmix_policy_step(const lbsim_qmix_policy_t* n, const float* obs, float* hidden,
                           const uint8_t* reset_mask, const float* state, int64_t B,
                           uint64_t seed, uint32_t step, int64_t* actions_out,
                           int32_t* server_actions_out, float* q_out, float* q_chosen_out,
                           float* q_tot_out, void* stream) {
  if (n == nullptr || B < 0) return LBSIM_EINVAL;
  const int A = n->num_agents, E = n->mixing_embed_dim, he = n->hypernet_embed_dim;
  if (A < 1 || A > 16 || n->obs_dim < 1 || n->obs_dim > 512 || n->state_dim < 1 ||
      n->state_dim > 512 || n->n_actions < 1 || n->n_actions > 16 || n->servers_per_agent < 1 ||
      !(n->epsilon >= 0.0f && n->epsilon <= 1.0f))
    return LBSIM_EINVAL;
  // layer widths the kernel is built for; the mixer's second-layer outputs [0, A E + E + 16)
  // must not reach hyper_b1's columns [3 he, 3 he + E) of the same LDS rows
  if (n->gru_dim != 64 || n->hidden_dim != 128 || E < 16 || E % 16 != 0 || he < 16 ||
      he % 16 != 0 || 3 * he + E > 256 || A * E / 16 + E / 16 + 1 > 16 || A * E + E + 16 > 3 * he)
    return LBSIM_ENOTSUP;
  if (B == 0) return LBSIM_OK;
  if (!obs || !hidden || !state || !actions_out || !q_tot_out || !n->w_ih || !n->w_hh ||
      !n->b_ih || !n->b_hh || !n->w1 || !n->b1 || !n->w2 || !n->b2 || !n->w3 || !n->b3 ||
      !n->m0 || !n->mb0 || !n->mw1 || !n->mbw1 || !n->mw2 || !n->mbw2 || !n->mb2 || !n->mbb2)
    return LBSIM_EINVAL;
  QmixArgs a{};
  a.obs = obs;
  a.hidden = hidden;
  a.reset = reset_mask;
  a.state = state;
  a.w_ih = n->w_ih;
  a.w_hh = n->w_hh;
  a.b_ih = n->b_ih;
  a.b_hh = n->b_hh;
  a.w1 = n->w1;
  a.b1 = n->b1;
  a.w2 = n->w2;
  a.b2 = n->b2;
  a.w3 = n->w3;
  a.b3 = n->b3;
  a.m0 = n->m0;
  a.mb0 = n->mb0;
  a.mw1 = n->mw1;
  a.mbw1 = n->mbw1;
  a.mw2 = n->mw2;
  a.mbw2 = n->mbw2;
  a.mb2 = n->mb2;
  a.mbb2 = n->mbb2;
  a.actions = actions_out;
  a.server_actions = server_actions_out;
  a.q_out = q_out;
  a.q_chosen = q_chosen_out;
  a.q_tot = q_tot_out;
  a.B = B;
  a.A = A;
  a.I = n->obs_dim;
  a.kxp = round16(n->obs_dim);
  a.Ds = n->state_dim;
  a.ksp = round16(n->state_dim);
  a.n_act = n->n_actions;
  a.k = n->servers_per_agent;
  a.he = he;
  a.E = E;
  a.epsilon = n->epsilon;
  a.key0 = (uint32_t)(seed & 0xFFFFFFFFull);
  a.key1 = (uint32_t)(seed >> 32);
  a.step = step;
  a.step_dev = n->step_dev;
  // LBSIM_QMIX_KERNEL = tile | wave | pair (default: pair when A = 4, else wave)
  static const int form = [] {
    const char* e = std::getenv("LBSIM_QMIX_KERNEL");
    if (e != nullptr && std::strcmp(e, "tile") == 0) return 0;
    if (e != nullptr && std::strcmp(e, "wave") == 0) return 1;
    return 2;
  }();
  return launch_qmix_policy(a, B, form, fused_mt(1), (hipStream_t)stream);
}

int lbsim_alias_tables(const float* weights, int64_t n, int S, float* odd_out, int32_t* alias_out,
                       int32_t* active_out, void* stream) {
  if (n < 0 || S < 1 || S > LBSIM_MAX_SERVERS) return LBSIM_EINVAL;
  if (n == 0) return LBSIM_OK;
  if (!weights || !odd_out || !alias_out || !active_out) return LBSIM_EINVAL;
  hipLaunchKernelGGL(alias_tables_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, weights, n, S, odd_out, alias_out, active_out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_vose_tables(const float* weights, int64_t n, int S, float* prob_out,
                      uint32_t* alias_out, void* stream) {
  if (n < 0 || S < 1 || S > LBSIM_MAX_SERVERS) return LBSIM_EINVAL;
  if (n == 0) return LBSIM_OK;
  if (!weights || !prob_out || !alias_out) return LBSIM_EINVAL;
  hipLaunchKernelGGL(vose_tables_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, weights, n, S, prob_out, alias_out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_vose_sample(const float* prob, const uint32_t* alias, int64_t n, int S,
                      uint32_t* state_io, int64_t k, int32_t* idx_out, uint64_t* hist_out,
                      void* stream) {
  if (n < 0 || S < 1 || S > LBSIM_MAX_SERVERS || k < 0 || k > INT32_MAX) return LBSIM_EINVAL;
  if (n == 0) return LBSIM_OK;
  if (!prob || !alias || !state_io) return LBSIM_EINVAL;
  hipLaunchKernelGGL(vose_sample_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, prob, alias, n, S, state_io, k, idx_out, hist_out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_reservoir_features(const float* values, const uint32_t* ts_ms, const uint32_t* counts,
                             int64_t n, float decay_factor, float* feats_out, void* stream) {
  if (values == nullptr || ts_ms == nullptr || counts == nullptr || feats_out == nullptr || n < 0)
    return LBSIM_EINVAL;
  if (!(decay_factor > 0.0f) || !(decay_factor < 1.0f)) return LBSIM_EINVAL;
  if (n == 0) return LBSIM_OK;
  const float c = (float)(std::log2((double)decay_factor) / 1000.0);
  hipLaunchKernelGGL(features_kernel, dim3((unsigned)((n + 3) / 4)), dim3(64), 0,
                     (hipStream_t)stream, values, ts_ms, counts, n, c, feats_out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_vpp_export(lbsim_t* h, int64_t env_begin, int64_t n_envs, float* tv_out,
                     int32_t* n_flow_on_out, float* ts_out, void* stream) {
  if (h == nullptr) return LBSIM_EINVAL;
  if (env_begin < 0 || n_envs < 0 || env_begin + n_envs > h->B)
    return fail(h, LBSIM_EINVAL, "envs [%lld, %lld) outside [0, %d)", (long long)env_begin,
                (long long)(env_begin + n_envs), h->B);
  if (!h->initialised) return fail(h, LBSIM_EINVAL, "call lbsim_reset before lbsim_vpp_export");
  if (n_envs == 0) return LBSIM_OK;
  if (tv_out == nullptr) return fail(h, LBSIM_EINVAL, "tv_out is NULL");
  DeviceGuard g(h->device);
  hipLaunchKernelGGL(vpp_export_kernel, dim3((unsigned)(n_envs * h->S)), dim3(64), 0,
                     (hipStream_t)stream, h->st, h->prm, env_begin, n_envs,
                     reinterpret_cast<float2*>(tv_out), n_flow_on_out, ts_out);
  return launch_check(h, "vpp_export_kernel");
}

int lbsim_vpp_features(const float* tv, const float* ts, int64_t res_per_ts, int64_t n,
                       double decay, double* feats_out, void* stream) {
  if (n < 0 || res_per_ts < 1 || !(decay > 0.0) || !(decay < 1.0)) return LBSIM_EINVAL;
  if (n == 0) return LBSIM_OK;
  if (!tv || !ts || !feats_out || n > 0x7FFFFFFF) return LBSIM_EINVAL;
  hipLaunchKernelGGL(vpp_features_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2*>(tv), ts, res_per_ts, n, decay, feats_out);
  return hipGetLastError() == hipSuccess ? LBSIM_OK : LBSIM_EDEVICE;
}

int lbsim_profile_begin(lbsim_t* h, int max_launches) {
  if (h == nullptr || max_launches < 1) return LBSIM_EINVAL;
  DeviceGuard g(h->device);
  Profiler& p = h->prof;
  const size_t need = 2 * (size_t)max_launches;
  // Timing-only events: no system-scope fence when they are recorded.  A default event's record
  // writes back and invalidates the caches between the launches it brackets, which costs the
  // timed step itself (the caller synchronises the device before reading the times, so nothing
  // needs the fence).
  while (p.ev.size() < need) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess)
      return fail(h, LBSIM_EDEVICE, "hipEventCreateWithFlags failed");
    p.ev.push_back(e);
  }
  p.used = 0;
  p.cap = need;
  p.cls.clear();
  p.beg.clear();
  p.end.clear();
  p.chain = false;
  p.chain_ev = -1;
  p.on = true;
  return LBSIM_OK;
}

int lbsim_profile_end(lbsim_t* h, double* ms_out, int64_t* count_out) {
  return lbsim_profile_end_ex(h, ms_out, count_out, 4);
}

int lbsim_profile_end_ex(lbsim_t* h, double* ms_out, int64_t* count_out, int n_classes) {
  if (h == nullptr || n_classes < 0 || n_classes > LBSIM_PROFILE_CLASSES) return LBSIM_EINVAL;
  DeviceGuard g(h->device);
  Profiler& p = h->prof;
  double ms[LBSIM_PROFILE_CLASSES] = {0, 0, 0, 0, 0};
  int64_t cnt[LBSIM_PROFILE_CLASSES] = {0, 0, 0, 0, 0};
  if (p.used > 0 && hipEventSynchronize(p.ev[p.used - 1]) != hipSuccess)
    return fail(h, LBSIM_EDEVICE, "hipEventSynchronize failed");
  for (size_t i = 0; i < p.cls.size(); ++i) {
    float t = 0.0f;
    if (hipEventElapsedTime(&t, p.ev[p.beg[i]], p.ev[p.end[i]]) != hipSuccess)
      return fail(h, LBSIM_EDEVICE, "hipEventElapsedTime failed");
    ms[p.cls[i]] += t;
    cnt[p.cls[i]] += 1;
  }
  p.on = false;
  p.used = 0;
  p.cls.clear();
  p.beg.clear();
  p.end.clear();
  p.chain_ev = -1;
  for (int i = 0; i < n_classes; ++i) {
    if (ms_out) ms_out[i] = ms[i];
    if (count_out) count_out[i] = cnt[i];
  }
  return LBSIM_OK;
}

int lbsim_launch_names(lbsim_t* h, int which, char* buf, size_t buf_len) {
  if (h == nullptr || which < 0 || which > 1 || buf == nullptr || buf_len == 0)
    return LBSIM_EINVAL;
  DeviceGuard g(h->device);
  std::string txt;
  for (const auto& [cls, fn] : h->launched[which]) {
    const char* raw = hipKernelNameRefByPtr(fn, nullptr);
    if (!txt.empty()) txt += ';';
    txt += std::to_string(cls) + "=" + short_kernel_name(raw);
  }
  // more launches than the log holds: a marker no counter file is keyed by
  if (h->launched_lost[which] > 0)
    txt += (txt.empty() ? "" : ";") + std::string("-1=truncated(") +
           std::to_string(h->launched_lost[which]) + " more)";
  if (txt.size() + 1 > buf_len)
    return fail(h, LBSIM_ESHAPE, "launch names need %zu bytes", txt.size() + 1);
  memcpy(buf, txt.c_str(), txt.size() + 1);
  return LBSIM_OK;
}

int lbsim_state_size(const lbsim_t* h, size_t* bytes_out) {
  if (h == nullptr || bytes_out == nullptr) return LBSIM_EINVAL;
  size_t t = 0;
  for (const Section& s : sections(const_cast<lbsim_t*>(h))) t += s.bytes;
  *bytes_out = t;
  return LBSIM_OK;
}

int lbsim_get_state(lbsim_t* h, void* host_buf, size_t bytes) {
  if (h == nullptr || host_buf == nullptr) return LBSIM_EINVAL;
  size_t need = 0;
  lbsim_state_size(h, &need);
  if (bytes != need) return fail(h, LBSIM_ESHAPE, "state buffer is %zu bytes, need %zu", bytes, need);
  DeviceGuard g(h->device);
  if (hipDeviceSynchronize() != hipSuccess) return fail(h, LBSIM_EDEVICE, "sync failed");
  char* dst = (char*)host_buf;
  for (const Section& s : sections(h)) {
    if (hipMemcpy(dst, *s.ptr, s.bytes, hipMemcpyDeviceToHost) != hipSuccess)
      return fail(h, LBSIM_EDEVICE, "hipMemcpy D2H failed");
    dst += s.bytes;
  }
  return LBSIM_OK;
}

int lbsim_set_state(lbsim_t* h, const void* host_buf, size_t bytes) {
  if (h == nullptr || host_buf == nullptr) return LBSIM_EINVAL;
  size_t need = 0;
  lbsim_state_size(h, &need);
  if (bytes != need) return fail(h, LBSIM_ESHAPE, "state buffer is %zu bytes, need %zu", bytes, need);
  DeviceGuard g(h->device);
  if (hipDeviceSynchronize() != hipSuccess) return fail(h, LBSIM_EDEVICE, "sync failed");
  const char* src = (const char*)host_buf;
  for (const Section& s : sections(h)) {
    if (hipMemcpy(*s.ptr, src, s.bytes, hipMemcpyHostToDevice) != hipSuccess)
      return fail(h, LBSIM_EDEVICE, "hipMemcpy H2D failed");
    src += s.bytes;
  }
  h->initialised = true;
  h->reset_seen = true;
  return LBSIM_OK;
}

}  // extern "C"

// ---- on-device snapshots (lbsim_state_save / lbsim_state_load)
namespace {

// One state_gather_kernel launch on `stream` over every section of the handle: no allocation, no
// synchronisation, no copy (the section table travels by value in the kernel's arguments).
int state_gather(lbsim_t* h, const char* who, void* dev_buf, size_t bytes, const uint8_t* mask,
                 const int32_t* src_env, int dir, void* stream) {
  if (h == nullptr) return fail(nullptr, LBSIM_EINVAL, "%s: handle is NULL", who);
  if (h->pool.A > 0)
    return fail(h, LBSIM_ENOTSUP, "%s on a handle with shared server pools: a per-env copy would "
                                  "tear a pool apart (lbsim_get_state / lbsim_set_state carry "
                                  "whole handles)", who);
  if (dev_buf == nullptr) return fail(h, LBSIM_EINVAL, "%s: dev_buf is NULL", who);
  if ((uintptr_t)dev_buf % 16u != 0)
    return fail(h, LBSIM_EINVAL, "%s: dev_buf must be 16-byte aligned", who);
  const std::vector<Section> secs = sections(h);
  static_assert(kSnapMaxSections >= 27, "sections() lists up to 27 sections");
  if (secs.size() > (size_t)kSnapMaxSections)
    return fail(h, LBSIM_ENOTSUP, "%s: %zu state sections, the kernel's table holds %d", who,
                secs.size(), kSnapMaxSections);
  SnapInput in[kSnapMaxSections];
  size_t need = 0;
  for (size_t i = 0; i < secs.size(); ++i) {
    in[i] = SnapInput{*secs[i].ptr, secs[i].bytes};
    need += secs[i].bytes;
  }
  if (bytes != need)
    return fail(h, LBSIM_ESHAPE, "%s: state buffer is %zu bytes, need %zu", who, bytes, need);
  if (dir == kSnapLoad && src_env != nullptr && !h->initialised)
    return fail(h, LBSIM_EINVAL, "%s with src_env needs a handle that was reset or loaded: the "
                                 "envs it keeps have no state yet", who);
  SnapTable t;
  const uint64_t blocks = snap_table_build(t, in, (int)secs.size(), h->B, dev_buf);
  DeviceGuard g(h->device);
  const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 1u << 20);
  hipLaunchKernelGGL(state_gather_kernel, dim3(grid), dim3(kSnapBlock), 0, (hipStream_t)stream, t,
                     static_cast<char*>(dev_buf), mask, src_env, dir, (int64_t)h->B);
  const int rc = launch_check(h, "state_gather_kernel");
  if (rc == LBSIM_OK && dir == kSnapLoad && src_env == nullptr) {
    h->initialised = true;
    h->reset_seen = true;
  }
  return rc;
}

}  // namespace

extern "C" {

int lbsim_state_save(lbsim_t* h, void* dev_buf, size_t bytes, const uint8_t* env_mask,
                     void* stream) {
  return state_gather(h, "lbsim_state_save", dev_buf, bytes, env_mask, nullptr, kSnapSave, stream);
}

int lbsim_state_load(lbsim_t* h, const void* dev_buf, size_t bytes, const int32_t* src_env,
                     void* stream) {
  return state_gather(h, "lbsim_state_load", const_cast<void*>(dev_buf), bytes, nullptr, src_env,
                      kSnapLoad, stream);
}

}  // extern "C"
