/*
 * lbsim.h — C ABI of the MI355X-native vectorised load-balancing environment.
 *
 * One handle = B independent LB environments (a shard of the global env range) resident in the
 * HBM of one GPU.  Every entry point is extern "C", takes plain pointers and sizes, never throws,
 * and returns an int status (LBSIM_OK or a negative LBSIM_E* code; message via lbsim_last_error).
 *
 * Buffers passed to reset/step/reward/features are DEVICE pointers owned by the caller (e.g. a
 * torch tensor's data_ptr()); nothing is allocated inside lbsim_reset/lbsim_step, so both can be
 * captured into a hipGraph.  `stream` is a hipStream_t (NULL = default stream).  Calls on one
 * handle are stream-ordered and NOT thread-safe across host threads.
 *
 * Reference interfaces replaced (paths relative to the MARLLB reference tree):
 *   LoadBalanceEnv.__init__ / _setup_spaces   simulation-mode/problem-03-rl-environment/src/env.py:71-184
 *   LoadBalanceEnv.reset                      env.py:186-213
 *   LoadBalanceEnv.step                       env.py:215-286
 *   LoadBalanceEnv.seed / close               env.py:321-330
 *   RewardFunction.compute + active rule      src/rewards.py:290-381, env.py:391-423
 *   ReservoirSampler.add / get_features       problem-01-reservoir-sampling/src/reservoir.py:50-196
 *   C twin reservoir_add / compute_stats      problem-01-reservoir-sampling/src/reservoir.h:118-268
 *   server assignment SED/SED2/LSQ/LSQ2       src/vpp/lb/node.c:388-441
 *   flow-completion samples (fct, duration)   src/vpp/lb/lbhash.h:87-172 (duration: :129-136)
 * Full semantics: DESIGN.md §3 (the simulator spec the GPU kernels and oracle/ both implement).
 */
#ifndef LBSIM_H
#define LBSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBSIM_ABI_VERSION 10 /* 10: lbsim_step_outputs_t ends with done_word / done_value (the */
                             /* one-env completion word); 9: lost-FIN guesses deferred to their */
                             /* wrap-up time, reservoir_mode VPP                                 */
#define LBSIM_MAX_SERVERS 64   /* S <= 64: BASELINE configs[4] read literally is 4 agents x 16 */
                               /* servers = 64 (S > 16: server-per-lane dynamics only)       */
#define LBSIM_RESERVOIR_K 128  /* reservoir.py:31 capacity=128, reservoir.h:24               */
#define LBSIM_NUM_FEATURES 11  /* env.py:46-48 (S, 11) observation                           */
#define LBSIM_MAX_DISCRETE 8

/* ---- status codes (never thrown across the ABI) ---- */
#define LBSIM_OK 0
#define LBSIM_EINVAL (-1)  /* bad argument / config (Python facade re-raises ValueError)      */
#define LBSIM_ENOMEM (-2)  /* device allocation failed                                        */
#define LBSIM_EDEVICE (-3) /* HIP runtime error (no GPU, launch failure, ...)                 */
#define LBSIM_ESHAPE (-4)  /* buffer size does not match the handle's B/S                     */
#define LBSIM_ENOTSUP (-5) /* option not built in this version                                */

/* ---- enums ---- */
enum lbsim_action_type { LBSIM_ACTION_DISCRETE = 0, LBSIM_ACTION_CONTINUOUS = 1 };
enum lbsim_dtype { LBSIM_DTYPE_I32 = 0, LBSIM_DTYPE_I64 = 1, LBSIM_DTYPE_F32 = 2 };

/* rewards.py:297-307 SUPPORTED_METRICS, same order */
enum lbsim_reward_metric {
  LBSIM_METRIC_JAIN = 0,
  LBSIM_METRIC_VARIANCE = 1,
  LBSIM_METRIC_STD = 2,
  LBSIM_METRIC_CV = 3,
  LBSIM_METRIC_MAX = 4,
  LBSIM_METRIC_MIN = 5,
  LBSIM_METRIC_PRODUCT = 6,
  LBSIM_METRIC_RANGE = 7,
  LBSIM_METRIC_GINI = 8
};

/* node.c:393-441: LB_SED, LB_SED2 (power of two), LB_LSQ, LB_LSQ2; node.c:442-460 LB_ALIAS with
 * the table of gen_alias (src/lb/shm_proxy.py:127-146) over the action weights */
enum lbsim_assign_policy {
  LBSIM_POLICY_SED = 0,
  LBSIM_POLICY_SED2 = 1,
  LBSIM_POLICY_LSQ = 2,
  LBSIM_POLICY_LSQ2 = 3,
  LBSIM_POLICY_ALIAS = 4
};

/* POISSON: exponential gaps of mean 1/arrival_rate, Exp(1) work.  TRACE: replay of an arrival
 * trace set with lbsim_set_trace (data/trace/poisson_for_loop/rate_N.csv). */
enum lbsim_arrival_source { LBSIM_ARRIVAL_POISSON = 0, LBSIM_ARRIVAL_TRACE = 1 };

/* The flow-duration sample of a completed flow (the reservoir behind obs columns 6-10 and the
 * default reward field).  AGE (default): the flow's age at its last data packet, tc - t_arrival --
 * VPP records time_now - t_init on every plain ACK after the first (src/vpp/lb/lbhash.h:129-136),
 * the last one at the flow's completion, so the backlog wait is included (problem-01 README:
 * "from first packet to last packet").  SERVICE: tc - max(t_arrival, predecessor's tc), the
 * service time alone (the ABI-6 sample; independent of the queue, so a duration-based reward
 * does not see the policy). */
enum lbsim_duration_mode { LBSIM_DURATION_AGE = 0, LBSIM_DURATION_SERVICE = 1 };

/* Observation column 0 (n_flow_on).  QUEUE (default): the flows in flight at the server.  VPP:
 * the data plane's as_stat_t n_flow_on, +1 at a flow's first ACK and -1 at its RSTACK
 * (src/vpp/lb/lbhash.h:116-120,138-142,167): a lost-FIN flow is never decremented (the decrement
 * is commented out, lbhash.h:193,214), so the column is the flows in flight plus the server's
 * lost-FIN flows completed since the episode start (or its last failure).  Only differs from
 * QUEUE with lost_fin_prob > 0. */
enum lbsim_n_flow_on_mode { LBSIM_NFLOW_QUEUE = 0, LBSIM_NFLOW_VPP = 1 };

/* Reservoir replacement rule.  ALGR (default): problem-01's Algorithm R (reservoir.py:64-85) --
 * slot `count` while count < 128, else slot j = randint(0, count + 1) if j < 128; observe takes
 * the features over the first min(count, 128) slots.  VPP: the live data plane's rule
 * (src/vpp/lb/lbhash.h:108,179 `res_id = rand() % RESERVOIR_N_BIN`, register_reservoir_as): every
 * sample overwrites slot rand() % 128 unconditionally, and the bins start zeroed at reset (VPP's
 * zeroed shm), so the upstream agent's process_reservoir over ALL 128 bins (shm_proxy.py:518-543,
 * lbsim_vpp_export / feature_mode "upstream") sees a sparse, recency-biased reservoir until every
 * bin was hit.  The counts still count samples. */
enum lbsim_reservoir_mode { LBSIM_RESERVOIR_ALGR = 0, LBSIM_RESERVOIR_VPP = 1 };

/* Dynamics-kernel mapping; every choice produces the same bits.  AUTO = SERVER_PER_LANE (faster
 * than one lane per env at every measured shape). */
enum lbsim_dyn_mapping {
  LBSIM_DYN_AUTO = 0,
  LBSIM_DYN_ENV_PER_LANE = 1,    /* one lane = one env                                        */
  LBSIM_DYN_SERVER_PER_LANE = 2  /* a group of G lanes = one env, one lane per server: G =     */
                                 /* pow2 >= S, except S <= 4 on small batches (B*4/64 <= half */
                                 /* the device's SIMDs), which get G = 8 (twice the waves);    */
                                 /* S <= 8 batches of at most 4 (S <= 4) or 2 envs per SIMD   */
                                 /* (Q <= 32, no ALIAS) run one WAVE per env    */
};

/* The dynamics kernel a handle's launches use (lbsim_dynamics_kernel). */
enum lbsim_dyn_kernel {
  LBSIM_DYN_KERNEL_ENV_LANE = 0,  /* dynamics_kernel: one lane per env                        */
  LBSIM_DYN_KERNEL_GROUP = 1,     /* dynamics_group_kernel: one lane per server, G-lane groups */
  LBSIM_DYN_KERNEL_WAVE = 2,      /* dynamics_wave_kernel: one wave per env                    */
  LBSIM_DYN_KERNEL_POOL = 3,      /* dynamics_pool_kernel: one G-lane group per server pool    */
  LBSIM_DYN_KERNEL_PS = 4,        /* dynamics_ps_kernel: processor-sharing servers, G-lane groups */
  LBSIM_DYN_KERNEL_POOL_PS = 5,   /* dynamics_pool_ps_kernel: a pool's servers processor-sharing   */
  LBSIM_DYN_KERNEL_ACK = 6        /* dynamics_group_ack_kernel: duration samples at every data ACK */
};

/* How lbsim_step runs; every choice produces the same bits.  FUSED: one launch per step whose
 * workgroups simulate their envs and then observe them: step_wave_kernel for
 * one-wave-per-env handles, fused_step_kernel for server-per-lane groups of <= 16 lanes (else
 * SPLIT); SPLIT: a dynamics launch and an observe launch.  AUTO: the one-launch step_wave_kernel
 * for one-wave-per-env handles with S <= 8 and at most 4 envs per SIMD (the single-env facade
 * and BASELINE configs[1]'s 4096 x 4 on 256 CUs),
 * else SPLIT (the server-per-lane fused form measured slower).  The environment
 * variable LBSIM_STEP_KERNEL=split|fused overrides AUTO. */
enum lbsim_step_kernel { LBSIM_STEP_AUTO = 0, LBSIM_STEP_SPLIT = 1, LBSIM_STEP_FUSED = 2 };

/*
 * POD configuration.  Mirrors the LoadBalanceEnv kwargs (env.py:71-87) plus the simulator knobs
 * the reference leaves implicit.  Fill with lbsim_config_default() and override.
 */
typedef struct lbsim_config {
  int32_t num_envs;          /* B: envs in this handle (this GPU's shard)                    */
  int32_t num_servers;       /* S: 1..LBSIM_MAX_SERVERS                         env.py:73   */
  int64_t env_id_offset;     /* global id of local env 0 (RNG key; sharding-invariant)       */
  uint64_t seed;             /* Philox4x32-10 key                               env.py:86   */
  int32_t action_type;       /* lbsim_action_type                               env.py:74   */
  int32_t num_discrete;      /* len(discrete_weights)                           env.py:75   */
  float discrete_weights[LBSIM_MAX_DISCRETE]; /* default [1.0, 1.5, 2.0]         env.py:69   */
  float min_weight;          /* continuous clip lower bound, default 0.1        env.py:77   */
  float max_weight;          /* continuous clip upper bound, default 10.0       env.py:76   */
  int32_t reward_metric;     /* lbsim_reward_metric, default JAIN               env.py:78   */
  int32_t reward_field;      /* obs column 0..10 (default 10 =                               */
                             /* 'flow_duration_avg_decay', env.py:79,377-381);               */
                             /* -1 = field name unknown -> reward 0.0 (rewards.py:375-376)  */
  float step_interval;       /* simulated seconds per step, default 0.25        env.py:80   */
  int32_t max_steps;         /* done when episode step >= max_steps (10000)     env.py:81   */
  int32_t normalize_obs;     /* running mean/std normalisation    env.py:85,450-470   */
  int32_t assign_policy;     /* lbsim_assign_policy, default SED                             */
  int32_t arrival_source;    /* lbsim_arrival_source, default POISSON                        */
  float arrival_rate;        /* lambda, flows/s per env, default 400 (poisson_for_loop);     */
                             /* TRACE: informational (the trace sets the rate)               */
  float server_rate[LBSIM_MAX_SERVERS]; /* mu_s, flows/s each server can serve (Exp work)   */
  float decay_factor;        /* reservoir decay, default 0.9          reservoir.py:106       */
  int32_t queue_capacity;    /* Q: max flows in flight per server (1..64), default 32       */
  int32_t warmup_steps;      /* simulated steps run inside reset() with weights 1.0         */
  int32_t dyn_mapping;       /* lbsim_dyn_mapping: how envs map onto lanes (results identical) */
  int32_t step_kernel;       /* lbsim_step_kernel: one fused launch or two (results identical) */
  /* Lost-FIN flows (VPP's timed-out flow sample, src/vpp/lb/lbhash.h:175-217, stats.h:27): a
   * flow's FIN/RST is missed with probability lost_fin_prob; its flow-table entry expires
   * flow_timeout_s after its last packet and the next flow hashed into its bucket (an exponential
   * wait of mean flow_buckets / arrival_rate) wraps it up with fct = now - t_init - 40 s.  That
   * signed-us sample enters the server's fct reservoir at the wrap-up time (completion +
   * flow_timeout + wait), stamped with it, in time order with the server's other samples: each
   * server holds its pending guesses in a ring of lost_fin_pending entries sorted by due time (a
   * guess arriving at a full ring is dropped and counted).  The flow's duration sample is
   * recorded at its completion, so under lost-FIN the fct and duration reservoirs are separate
   * (own counts, own timestamps).  0 = off. */
  float lost_fin_prob;       /* [0, 1], default 0                                            */
  float flow_timeout_s;      /* the lb plugin's flow timeout, default 40 (lb.c:1437)        */
  int32_t flow_buckets;      /* sticky buckets per core, default 1024 (lb.h:46)             */
  /* Server failure / recovery (THEORY.md §6.4 "server_failure ~ Bernoulli(p_fail)"): at the
   * start of each step an up server fails with probability fail_prob (its queued flows are lost
   * and counted as dropped, its reservoirs emptied: an all-zero observation row, inactive in the
   * reward, env.py:410-413) and a down server recovers with probability recover_prob.  A down
   * server takes no flows (as a full one).  fail_prob 0 = off (no state is allocated). */
  float fail_prob;           /* [0, 1], default 0                                            */
  float recover_prob;        /* [0, 1], default 0.1                                          */
  /* Next-step auto-reset (gymnasium's NEXT_STEP autoreset mode): lbsim_step resets, in place of
   * stepping, every env whose previous step returned done (episode step >= max_steps), ignoring
   * its action; that env's outputs are its reset observation, reward 0, done 0, episode length
   * and return 0, assignment counts 0.  Inside the step launches: no extra kernel, so a captured
   * step needs no masked-reset launch; such a handle steps in two launches
   * (dynamics, observe), not the one-launch forms.  0 = off (the caller resets).             */
  int32_t next_step_reset;
  int32_t duration_mode;     /* lbsim_duration_mode, default AGE            */
  int32_t n_flow_on_mode;    /* lbsim_n_flow_on_mode, default QUEUE         */
  int32_t lost_fin_pending;  /* pending lost-FIN guesses held per server, 1..4096, default 256 */
  int32_t reservoir_mode;    /* lbsim_reservoir_mode, default ALGR           */
} lbsim_config_t;

typedef struct lbsim lbsim_t; /* opaque handle */

/* Library identity; never fails, no GPU needed. */
const char* lbsim_version(void);
int lbsim_abi_version(void);

/* Fill *cfg with the reference defaults (env.py:71-87) and the simulator defaults. */
int lbsim_config_default(lbsim_config_t* cfg);

/* Validate a config without touching the GPU (ValueError paths of env.py:184, rewards.py:321). */
int lbsim_config_validate(const lbsim_config_t* cfg, char* msg, size_t msg_len);

/* Allocate device state for cfg->num_envs envs on `device`.  Replaces LoadBalanceEnv.__init__. */
int lbsim_create(const lbsim_config_t* cfg, int device, lbsim_t** out);

/* Free device state.  Replaces LoadBalanceEnv.close (env.py:321-325). */
int lbsim_destroy(lbsim_t* h);

/* Thread-local message of the last failure on this handle (or of the last create if h==NULL). */
const char* lbsim_last_error(const lbsim_t* h);

/* Re-key the RNG and rewind every env's episode counter (env.py:327-330 seed()). */
int lbsim_seed(lbsim_t* h, uint64_t seed);

/* Which dynamics kernel (lbsim_dyn_kernel) this handle's step and reset launches use, for the
 * handle's shape, config and the LBSIM_DYN_* environment overrides; -1 on a NULL handle.  No
 * GPU work (measurement labels; the reference has no counterpart). */
int lbsim_dynamics_kernel(const lbsim_t* h);

/*
 * Reset the envs whose env_mask[b] != 0 (env_mask == NULL: all envs) and write their first
 * observation into obs_out[b, S, 11] (f32); rows of unmasked envs are left untouched.
 * Replaces LoadBalanceEnv.reset (env.py:186-213).
 */
int lbsim_reset(lbsim_t* h, const uint8_t* env_mask, float* obs_out, void* stream);

/*
 * Advance every env by one step of step_interval simulated seconds.
 *   action        [B, S]: discrete indices (I32 or I64) or continuous weights (F32)
 *   obs_out       [B, S, 11] f32   reward_out [B] f32   done_out [B] u8
 *   assign_count_out [B, S] i32 (optional, NULL = skip): flows assigned per server this step
 * Replaces LoadBalanceEnv.step (env.py:215-286).
 */
int lbsim_step(lbsim_t* h, const void* action, int action_dtype, float* obs_out,
               float* reward_out, uint8_t* done_out, int32_t* assign_count_out, void* stream);

/*
 * Optional outputs of one step, all device pointers, NULL = not wanted.  Written by the same
 * launch as obs/reward/done (no extra kernel, no host sync).
 */
typedef struct lbsim_step_outputs {
  float* obs;              /* [B, S, 11] f32 observation (normalised if normalize_obs)        */
  float* reward;           /* [B] f32                                                         */
  uint8_t* done;           /* [B] u8                                                          */
  int32_t* assign_count;   /* [B, S] i32 flows assigned per server this step                  */
  float* raw_obs;          /* [B, S, 11] f32 un-normalised obs (reward/active_servers basis)  */
  int32_t* episode_length; /* [B] i32 step count of the episode after this step (info['step'])*/
  double* episode_return;  /* [B] f64 return of the episode after this step                   */
  /* problem-05 MultiAgentLoadBalanceEnv facade (multi_agent_env.py:152-188, 240-258), written by
   * the same launch; num_agents * servers_per_agent must equal S when either is requested */
  float* agent_obs;        /* [B, A, 4k + 7S] f32: agent a = flat[4ak, 4(a+1)k) ++ flat[4S:] of */
                           /* the returned (S, 11) rows                                        */
  float* state;            /* [B, 4S + 10] f32 get_state(): zeros, episode step / max_steps, A */
  int32_t num_agents;      /* A                                                               */
  int32_t servers_per_agent; /* k                                                             */
  /* Completion word (one-env handles, B = 1, lbsim_step_ex only; NULL = none): the step launch
   * stores done_value to *done_word (device-accessible host memory) after every other output of
   * the step, with a system-scope release, so a host polling the word sees the outputs complete
   * without a stream synchronisation (the single-env facade's step, problem-04 Trainer path). */
  uint32_t* done_word;
  uint32_t done_value;
} lbsim_step_outputs_t;

/* lbsim_step with every output optional except obs, reward and done. */
int lbsim_step_ex(lbsim_t* h, const void* action, int action_dtype,
                  const lbsim_step_outputs_t* out, void* stream);

/* lbsim_reset with the step outputs that make sense after a reset: out->obs (required),
 * out->raw_obs, out->agent_obs and out->state (rows of reset envs only). */
int lbsim_reset_ex(lbsim_t* h, const uint8_t* env_mask, const lbsim_step_outputs_t* out,
                   void* stream);

/* sizeof(lbsim_config_t) / sizeof(lbsim_step_outputs_t) for binding-side layout checks. */
size_t lbsim_config_size(void);
size_t lbsim_step_outputs_size(void);

/* Per-env episode length (i32 [B]) and return (f64 [B]) into device buffers (info['episode']). */
int lbsim_episode_stats(lbsim_t* h, int32_t* length_out, double* return_out, void* stream);

/* Accounting of the last step (bench.py's algorithmic bytes; synchronises the device): HOST
 * stats_out[0] = reservoir slots the last dynamics launch wrote (popcount of the written-slot
 * masks: each an 8-B record store, + 4 B with a duration plane), stats_out[1] = flows in flight after it (sum of the queue
 * counts: ring entries carried into the next step). */
int lbsim_step_stats(lbsim_t* h, int64_t* stats_out);

/* Stateless reward of given raw observations obs[n, S, 11] -> reward_out[n] (f32), using
 * cfg->reward_metric / reward_field and the active rule any(obs[s] > 0) (env.py:410-417,
 * rewards.py:329-381). */
int lbsim_reward(const lbsim_config_t* cfg, const float* obs, int64_t n, float* reward_out,
                 void* stream);

/* Stateless reservoir features: for r in [0, n): values[r, K] f32, ts_ms[r, K] u32 sample
 * timestamps (integer ms), counts[r] u32 (samples seen; min(count, K) valid slots) ->
 * feats_out[r, 5] = {mean, p90, std, mean_decay, p90_decay} (reservoir.py:105-196). */
int lbsim_reservoir_features(const float* values, const uint32_t* ts_ms, const uint32_t* counts,
                             int64_t n, float decay_factor, float* feats_out, void* stream);

/* Stateless: n alias tables of S weights each (weights[n, S] f32, device pointers): gen_alias
 * (src/lb/shm_proxy.py:127-146) over the weights > 0 of each row, as the ALIAS policy builds it
 * every step -> odd_out[n, S] (float32, as packed into shm.h alias_t), alias_out[n, S] (position
 * in the row's active list), active_out[n, S] (server of each active position; -1 past the end).
 * Entries past a row's active count are (1, 0, -1). */
/* Stateless: problem-05 per-agent observations (multi_agent_env.py:152-188) of n flattened
 * (S, 11) observations (device pointers), num_agents * servers_per_agent == S.  Agent a gets the
 * 4-value slices of the flattened obs for its servers -- flat[4 a k : 4 (a+1) k], the wrapper's
 * `server_features_per_server = 4` -- then flat[4 S :]: out[n, A, 4 k + 7 S] (128 at 4 x 4). */
int lbsim_agent_obs(const float* obs, int64_t n, int S, int num_agents, int servers_per_agent,
                    float* out, void* stream);

/* Policy-network epilogues (device pointers, row-major), used between hipBLASLt GEMMs by
 * marllb_amd/policies.py for problem-04 PolicyNetwork (networks.py:82-146) and problem-05
 * AgentQNetwork (agent_network.py:63-87):
 *  lbsim_gru_gates: torch.nn.GRU cell from gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh ([B, 3H],
 *    gates r, z, n): h_out = (1 - z) n + z h, r = sig(gi_r + gh_r), z = sig(gi_z + gh_z),
 *    n = tanh(gi_n + r gh_n).
 *  lbsim_sac_head: y = [B, 2A] = [mean | log_std]: log_std clamped to [min, max]; action =
 *    tanh(mean) (deterministic) or tanh(mean + exp(log_std) eps), eps ~ N(0,1) from Philox
 *    (key = seed, counter = (row, step, a, 3 << 24)); times scale plus bias.  log_std_out optional. */
int lbsim_gru_gates(const float* gi, const float* gh, const float* h, float* h_out, int64_t B,
                    int H, void* stream);
int lbsim_sac_head(const float* y, int64_t B, int A, float log_std_min, float log_std_max,
                   float action_scale, float action_bias, int deterministic, uint64_t seed,
                   uint32_t step, float* action_out, float* log_std_out, void* stream);
/* QMIX mixing tail (mixing_network.py:96-116) after the hypernetwork GEMMs, per env b:
 *  hidden_e = elu(b1[b,e] + sum_a q[b,a] |w1[b, a E + e]|), q_tot[b] = sum_e hidden_e |w2[b,e]| + b2[b]
 * (row strides *_ld in floats, so the outputs of one concatenated GEMM can be passed directly). */
int lbsim_qmix_tail(const float* q, const float* w1, int64_t w1_ld, const float* b1,
                    int64_t b1_ld, const float* w2, int64_t w2_ld, const float* b2, int64_t b2_ld,
                    int64_t B, int A, int E, float* q_tot, void* stream);

/* ---- one-kernel policy inference (marllb_amd/csrc/lbsim_fused.h) ----
 * The whole network of a tile of envs per workgroup on v_mfma_f32_16x16x4_f32, activations in LDS,
 * one launch per step.  Weights are device pointers packed once by marllb_amd/policies.py
 * `pack_linear`: a Linear weight W [N, K] zero-padded to [16 ceil(N/16), 16 ceil(K/16)] and stored
 * in MFMA-fragment order P[nt][kb][lane 0..63][4] = W[16 nt + (lane & 15)][16 kb + 4 (lane >> 4)
 * + s]; biases zero-padded to the padded N.  Layer widths other than the reference defaults return
 * LBSIM_ENOTSUP (callers then use the GEMM + epilogue entry points above). */
typedef struct lbsim_sac_actor { /* problem-04 PolicyNetwork (networks.py:19-146)             */
  int32_t state_dim;             /* S * 11, <= 512                                            */
  int32_t gru_dim;               /* 128 (networks.py default)                                 */
  int32_t hidden_dim;            /* 256                                                       */
  int32_t action_dim;            /* A <= 16                                                   */
  const float* w_ih;             /* gru.weight_ih_l0 [3 gru, state_dim] packed (gates r, z, n) */
  const float* w_hh;             /* gru.weight_hh_l0 [3 gru, gru] packed                      */
  const float* b_ih;             /* [3 gru]                                                   */
  const float* b_hh;             /* [3 gru]                                                   */
  const float* w1;               /* fc1 [hidden, gru] packed                                  */
  const float* b1;               /* [hidden]                                                  */
  const float* wh;               /* [fc_mean; fc_logstd] [2 A, hidden] packed                 */
  const float* bh;               /* [2 A], zero-padded to a multiple of 16                    */
  float log_std_min, log_std_max; /* clamp (networks.py:93)                                   */
  float action_scale, action_bias;
  const uint32_t* step_dev;      /* NULL, or a device u32 read as the Philox `step` counter      */
                                 /* instead of the argument (hipGraph replays: the caller        */
                                 /* advances it in the graph)                                     */
} lbsim_sac_actor_t;
size_t lbsim_sac_actor_size(void);

/* PolicyNetwork.sample (networks.py:113-146) of B envs in one launch: state [B, state_dim];
 * hidden [B, gru] updated IN PLACE, rows whose reset_mask byte is set starting from zeros
 * (init_hidden at an episode start; reset_mask may be NULL); action_out [B, A] = tanh(x) * scale +
 * bias, x = mean (deterministic) or mean + exp(clamped log_std) eps with eps ~ N(0,1) drawn from
 * Philox exactly as lbsim_sac_head; log_std_out [B, A] optional. */
int lbsim_sac_actor_step(const lbsim_sac_actor_t* net, const float* state, float* hidden,
                         const uint8_t* reset_mask, int64_t B, int deterministic, uint64_t seed,
                         uint32_t step, float* action_out, float* log_std_out, void* stream);

typedef struct lbsim_qmix_policy { /* problem-05 QMIXAgent agents + QMixingNetwork            */
  int32_t num_agents;            /* A <= 16                                                   */
  int32_t obs_dim;               /* per-agent observation (128 at 4 x 4), <= 512              */
  int32_t gru_dim;               /* 64 (agent_network.py default)                             */
  int32_t hidden_dim;            /* 128                                                       */
  int32_t n_actions;             /* <= 16                                                     */
  int32_t state_dim;             /* global state (74 at 4 x 4), <= 512                        */
  int32_t mixing_embed_dim;      /* E = 32 (mixing_network.py default)                        */
  int32_t hypernet_embed_dim;    /* 64                                                        */
  int32_t servers_per_agent;     /* k: server_actions_out repeats each agent's action k times */
  float epsilon;                 /* exploration rate (qmix_agent.py:153)                      */
  /* agent networks, A copies stacked agent-major (packed / padded as above) */
  const float *w_ih, *w_hh, *b_ih, *b_hh; /* GRU [3 gru, obs_dim], [3 gru, gru]; [3 gru]      */
  const float *w1, *b1, *w2, *b2;         /* fc1 [hidden, gru], fc2 [hidden, hidden]           */
  const float *w3, *b3;                   /* fc3 [n_actions padded to 16, hidden]; [16]        */
  /* mixer: m0 = the first layers stacked [hyper_w1[0]; hyper_w2[0]; hyper_b2[0]; hyper_b1[0]]
   * [3 he + E, state_dim]; then hyper_w1[2] [A E, he], hyper_w2[2] [E, he], hyper_b2[2] [1, he]
   * (rows padded to 16) with their biases */
  const float *m0, *mb0, *mw1, *mbw1, *mw2, *mbw2, *mb2, *mbb2;
  const uint32_t* step_dev;      /* as lbsim_sac_actor_t.step_dev                              */
} lbsim_qmix_policy_t;
size_t lbsim_qmix_policy_size(void);

/* QMIXAgent.select_actions (qmix_agent.py:138-178) for every agent + QMixingNetwork.forward
 * (mixing_network.py:78-117) of B envs in one launch: obs [B, A, obs_dim]; hidden [B, A, gru]
 * updated in place (reset_mask as above); state [B, state_dim]; per agent the greedy action
 * (first maximum, as torch.argmax) or, with probability epsilon, a uniform one, drawn from Philox
 * (key = seed, counter = (env, step, agent, 4 << 24)); actions_out [B, A] int64,
 * server_actions_out [B, A k] int32 or NULL, q_out [B, A, n_actions] or NULL, q_chosen_out
 * [B, A] or NULL, q_tot_out [B] = the mixer on the chosen Q-values. */
int lbsim_qmix_policy_step(const lbsim_qmix_policy_t* net, const float* obs, float* hidden,
                           const uint8_t* reset_mask, const float* state, int64_t B,
                           uint64_t seed, uint32_t step, int64_t* actions_out,
                           int32_t* server_actions_out, float* q_out, float* q_chosen_out,
                           float* q_tot_out, void* stream);

/* Arrival trace for arrival_source == TRACE (the TRACE counterpart of the Poisson draw in
 * env.py's simulation; rows of replay_fork_io.py:95-121's `time<TAB>query` CSV): gap_us[rows]
 * (us since the previous row; row 0: the wrap-around gap) and work[rows] (service demand in mean-1
 * units, row N / mean N), device pointers, copied into the handle.  Env gid in episode e replays
 * rows (gid * 7919 + (e - 1) * 1000003 + k) mod rows for its k-th arrival.  Must precede the
 * first lbsim_reset of a TRACE handle; setting it again takes effect at the next reset. */
int lbsim_set_trace(lbsim_t* h, const uint32_t* gap_us, const float* work, int64_t rows,
                    void* stream);

int lbsim_alias_tables(const float* weights, int64_t n, int S, float* odd_out, int32_t* alias_out,
                       int32_t* active_out, void* stream);

/* ---- per-env workload (domain randomisation) ----
 * lbsim_set_env_rates: arrival_rate[B] flows/s and/or server_rate[B, S] flows/s (f32 DEVICE
 * pointers, either may be NULL = leave that one as it is).  Converted (1e6 / rate, divided in f64
 * and rounded once to f32, as the config's own rates are) into handle-owned device arrays that
 * every later dynamics launch of this handle (step, reset, warm-up) reads in place of the config's
 * shared arrival_rate / server_rate[]: from the next launch on every arrival gap drawn and every
 * service time computed uses the env's own rate; the next arrival already drawn keeps its time
 * and work.  Ranges are the config's (arrival in [0.1, 1e6], server in [1, 1e7], NaN rejected):
 * the call waits on `stream`, and with any value out of range returns LBSIM_EINVAL (the count in
 * lbsim_last_error) and leaves the previous rates in force.  LBSIM_ENOTSUP: a non-NULL
 * arrival_rate on a lost-FIN handle (lost_fin_prob > 0: the bucket-wait mean and the signed 32-bit
 * bound of lbsim_config_validate depend on the arrival rate) or on a TRACE handle (the trace sets
 * the rate); server_rate is allowed on both.
 * The arrays are allocated by the first call and never moved; later calls rewrite them in place,
 * so a step captured into a hipGraph AFTER the first call sees later updates on replay (the first
 * call allocates and synchronises: it must precede the capture).  lbsim_step / lbsim_reset gain
 * no synchronisation and no allocation.  The rates are NOT part of the snapshot
 * (lbsim_get_state / lbsim_set_state): a handle that loads a state keeps its own rates.
 * lbsim_clear_env_rates: back to the config's shared rates (waits for the device; the handle's
 * arrays take the config's values, so a graph captured while rates were set replays with those).
 * lbsim_get_env_rates: the current effective rates into device buffers [B] / [B, S] (either may
 * be NULL), the config's values when no per-env rates are set. */
int lbsim_set_env_rates(lbsim_t* h, const float* arrival_rate, const float* server_rate,
                        void* stream);
int lbsim_clear_env_rates(lbsim_t* h);
int lbsim_get_env_rates(lbsim_t* h, float* arrival_rate_out, float* server_rate_out,
                        void* stream);

/* ---- rate schedules (non-stationary workloads) ----
 * A handle may carry a rate schedule: `phases` (P) phases, each held for `steps_per_phase` (H)
 * agent steps, cyclic (wrap != 0) or clamped at the last phase (wrap == 0).
 * Phase rule: with k = the steps env b has completed in its current episode (its episode step at
 * the launch of a step) and j = k / H, the step's dynamics use phase j % P (cyclic) or
 * min(j, P - 1) (clamped) of env b's rows.  A reset always runs at phase 0: the first arrival
 * draw, every warm-up step, and the in-launch reset of a next_step_reset handle.  A phase change
 * acts exactly as a mid-run lbsim_set_env_rates: the arrival already drawn keeps its time and
 * work, every later gap and service time uses the new phase's rates.
 * lbsim_set_rate_schedule: arrival_rate [rows, P] and / or server_rate [rows, P, S], f32 DEVICE
 * pointers, flows/s; rows = 1 (every env the same schedule) or B.  NULL: that quantity keeps, per
 * env, the rate that was in force before the call (what lbsim_get_env_rates would have returned),
 * constant over the phases.  Conversion, ranges and validation are lbsim_set_env_rates's: the call
 * waits on `stream`; any value out of range returns LBSIM_EINVAL (the count in lbsim_last_error)
 * and leaves the previous schedule or rates in force.  LBSIM_EINVAL: phases outside [1, 4096] or
 * steps_per_phase < 1.  LBSIM_ESHAPE: rows neither 1 nor B.  LBSIM_ENOMEM: a table of more than
 * 2^31 - 1 elements (B * P * S), or a failed allocation.  LBSIM_ENOTSUP: a non-NULL arrival_rate
 * on a lost-FIN or TRACE handle (as lbsim_set_env_rates); server schedules are allowed on both.
 * The handle stores the tables expanded to B rows, gap[B, P] and scale[B, P, S]: B * P * (S + 1)
 * * 4 bytes, twice with the rates as given (what lbsim_get_env_rates returns), and all of it twice
 * with the staging copies.  A scheduled handle's lbsim_step / lbsim_reset launch one small kernel
 * in front of the dynamics that gathers each env's row at its phase.  The tables are allocated by
 * the first call for a given P and never moved by later calls with the same P, which rewrite them
 * in place: a step captured into a hipGraph after the first call sees the new values on replay.
 * P, H and wrap are kernel arguments: changing any of them (a new P also moves the tables), or
 * dropping the schedule, needs a new capture.  lbsim_step / lbsim_reset gain no allocation and no
 * synchronisation.  The schedule is NOT part of the snapshot; the episode step is, so a scheduled
 * handle that loads a state continues at that state's phase.
 * On a scheduled handle lbsim_get_env_rates returns, per env, the rates its next step launch will
 * use, and lbsim_set_env_rates / lbsim_clear_env_rates drop the schedule first (the per-env rates
 * in force before the schedule are then the ones a NULL argument of lbsim_set_env_rates leaves as
 * they are).
 * lbsim_clear_rate_schedule: drops the schedule and goes back to the config's shared rates, as
 * lbsim_clear_env_rates (the tables stay allocated and take the config's values).
 * lbsim_rate_phase: phase_out[B] (int32 DEVICE) = the phase each env's next step launch will use
 * (zeros on a handle without a schedule). */
int lbsim_set_rate_schedule(lbsim_t* h, const float* arrival_rate, const float* server_rate,
                            int32_t rows, int32_t phases, int32_t steps_per_phase, int32_t wrap,
                            void* stream);
int lbsim_clear_rate_schedule(lbsim_t* h);
int lbsim_rate_phase(lbsim_t* h, int32_t* phase_out, void* stream);

/* ---- trace banks (per-env trace selection and trace schedules) ----
 * The TRACE counterpart of the two sections above.  One handle holds a bank of n_traces (T)
 * traces, back to back in one device buffer: trace t is rows [row_begin[t], row_begin[t + 1]),
 * R_t >= 1 of them.  Each env replays the trace its own id names: with env gid on trace t, the
 * k-th arrival of its episode e reads bank row
 *     row_begin[t] + ((gid * 7919 + (e - 1) * 1000003 + k) mod R_t),
 * which is what a handle given trace t alone by lbsim_set_trace reads.
 * lbsim_set_trace_bank replaces loading one of the reference's per-load files
 * (data/trace/poisson_for_loop/rate_*.csv, the rows of src/client/replay_fork_io.py:95-121) per
 * run: gap_us / work are DEVICE arrays of row_begin[n_traces] rows (lbsim_set_trace's columns),
 * row_begin a HOST array of n_traces + 1 ascending offsets with row_begin[0] = 0.  1 <= T <= 4096,
 * every R_t >= 1, fewer than 2^31 rows in all (LBSIM_EINVAL otherwise, and on a non-TRACE handle).
 * lbsim_set_trace is the case T = 1.  Either call drops any selection or schedule: every env is
 * back on trace 0.  A bank of the size (rows, T) of the one it replaces is rewritten in place; any
 * other moves the buffer, and a captured graph needs a new capture.
 * lbsim_set_trace_schedule replaces the reference's replay of one file per traffic level over a
 * day (src/client/replay_fork_io.py:95-121 started once per data/trace/poisson_for_loop/rate_*.csv):
 * trace_id [rows, P] int32 DEVICE, rows = 1 (every env the same schedule) or B, P phases each held
 * for steps_per_phase agent steps, cyclic (wrap != 0) or clamped.  The phase rule and the reset
 * rule are those of the rate schedules above, verbatim: phase (k / H) % P or min(k / H, P - 1)
 * with k the env's episode step at the launch; phase 0 for lbsim_reset, its warm-up steps and the
 * in-launch reset of a next_step_reset handle.  P = 1 is a constant per-env trace.  A change of
 * trace between two launches keeps the arrival already drawn (its time and work), the arrival
 * index and the episode; every later arrival reads the new trace at the row rule's index.
 * The call waits on `stream`.  LBSIM_EINVAL: a non-TRACE handle, no trace set yet, P outside
 * [1, 4096], steps_per_phase < 1, or an id outside [0, T) (the count in lbsim_last_error; the
 * selection in force stays untouched).  LBSIM_ESHAPE: rows neither 1 nor B.  LBSIM_ENOTSUP: a
 * lost-FIN handle (lost_fin_prob > 0: the bucket-wait mean is derived from the handle's one
 * arrival rate); a bank whose envs all stay on trace 0 is allowed there.  A trace schedule and a
 * server-rate schedule may be in force together, each with its own P, H and wrap.
 * A handle with a selection launches one small kernel in front of each dynamics launch; the
 * tables are allocated by the first call for a given P and rewritten in place by later calls with
 * the same P, so a step captured into a hipGraph after the first call sees the new ids on replay.
 * P, H and wrap are kernel arguments: a change of them, or dropping the schedule, needs a new
 * capture.  lbsim_step / lbsim_reset gain no allocation and no synchronisation.  The selection is
 * NOT part of the snapshot; the episode step is.
 * lbsim_clear_trace_schedule: every env back to trace 0 (waits for the device; the tables stay
 * allocated and take id 0).
 * lbsim_env_trace: per env, the trace (trace_id_out[B]) and the phase (phase_out[B]) its next step
 * launch will use, int32 DEVICE, either may be NULL; zeros on a handle without a selection. */
int lbsim_set_trace_bank(lbsim_t* h, const uint32_t* gap_us, const float* work,
                         const int64_t* row_begin, int n_traces, void* stream);
int lbsim_set_trace_schedule(lbsim_t* h, const int32_t* trace_id, int rows, int P,
                             int steps_per_phase, int wrap, void* stream);
int lbsim_clear_trace_schedule(lbsim_t* h);
int lbsim_env_trace(lbsim_t* h, int32_t* trace_id_out, int32_t* phase_out, void* stream);

/* ---- workload tables (per-env gap and flow-size distributions) ----
 * A Poisson handle draws, for each arrival, a gap -ln(u0) * mean_gap and a work -ln(u1).  With
 * workload tables in force it looks both up instead: a table is LBSIM_TABLE_BINS f32 quantile
 * levels of a mean-1 distribution, indexed by the raw 32-bit Philox word v of the draw (small v =
 * the tail, as for -ln u):
 *     bin(v) = v for v < 32, else with e = floor(log2 v): 32 (e - 4) + ((v >> (e - 5)) & 31)
 * (bins 0..31 hold one word each; bin k >= 32 holds 2^(k / 32 - 1) words: 32 levels per octave of
 * tail probability, down to 2^-32).  The arrival with Philox block d of env b gets
 *     gap  = max(1, (int32)(table[gap_id[b]][bin(d.x)] * mean_gap_b))   us
 *     work = table[work_id[b]][bin(d.y)]
 * with mean_gap_b the env's mean gap exactly as without tables (the config's, lbsim_set_env_rates'
 * or a schedule's); d.z and d.w are used as before.  A pure lookup: no interpolation.
 * lbsim_set_workload_tables: tables [T, LBSIM_TABLE_BINS] f32, gap_id / work_id int32 [rows] with
 * rows = 1 (every env the same pair) or B, all DEVICE pointers; 1 <= T <= 1024.  From the next
 * launch on (step, reset, warm-up) every arrival drawn uses the tables; the arrival already drawn
 * keeps its time and work.  The call validates on the device, waits on `stream`, and on any
 * offender leaves what was in force untouched.  LBSIM_EINVAL: a TRACE handle (the trace supplies
 * gap and work); T out of range; an id outside [0, T); an entry that is not finite or < 0; a
 * table some env uses for gaps with an entry > 64 or a mass-weighted mean < 2^-4; a table some env
 * uses for work whose largest entry wmax breaks  wmax * (1e6 / mu_min) * queue_capacity <= 2^30
 * (mu_min: the smallest server rate in force: the config's, the per-env arrays' or a schedule's
 * tables'; this keeps the 32-bit relative times safe).  LBSIM_ESHAPE: rows neither 1 nor B.
 * While tables are in force lbsim_set_env_rates / lbsim_set_rate_schedule reject a server rate
 * below wmax * queue_capacity * 1e6 / 2^30 (their lower bound, 1 without tables).
 * lbsim_set_env_workload: new ids [B] for the bank in force (either NULL = unchanged), validated
 * the same way; LBSIM_EINVAL without tables.  lbsim_get_env_workload: the ids in force into int32
 * DEVICE arrays [B] (either NULL); LBSIM_EINVAL without tables.  lbsim_clear_workload_tables: back
 * to the closed form (the buffers stay allocated).
 * The first call allocates the bank and the id array; later calls with the same T rewrite both in
 * place, so a step captured into a hipGraph after the first call sees them on replay; a new T, or
 * clearing, needs a new capture.  A handle with tables in force is a full handle, as one with flow
 * statistics: its steps run dynamics_group_full_kernel in two launches, whatever dyn_mapping /
 * step_kernel ask for (the lookups are compiled into that kernel alone).  lbsim_step / lbsim_reset gain no allocation and no
 * synchronisation.  Tables and ids are NOT part of the snapshot: a restored or forked env draws
 * from the tables of the slot it is loaded into.  Draws are keyed by global env id, so a shard
 * passes its own rows gap_id[lo:hi]. */
#define LBSIM_TABLE_BINS 896
int lbsim_set_workload_tables(lbsim_t* h, const float* tables, int n_tables, const int32_t* gap_id,
                              const int32_t* work_id, int rows, void* stream);
int lbsim_set_env_workload(lbsim_t* h, const int32_t* gap_id, const int32_t* work_id,
                           void* stream);
int lbsim_get_env_workload(lbsim_t* h, int32_t* gap_id_out, int32_t* work_id_out, void* stream);
int lbsim_clear_workload_tables(lbsim_t* h);

/*
 * Exact flow-completion-time statistics, opt-in per handle.  A handle with
 * them on counts every flow that completes during a STEP of an env, once, with its true
 * fct = completion - arrival in integer us (a lost-FIN handle counts the real value, not VPP's
 * guess; duration_mode SERVICE still counts completion - arrival).  Not counted: completions
 * inside a reset's warm-up steps (lbsim_reset, and the step that resets an env under next-step
 * auto-reset), flows dropped at full queues, flows lost when a server fails.  Per (env, server):
 * count (u32), sum_us (u64), max_us (u32) and hist[LBSIM_FLOW_STATS_BINS] (u32), cumulative over
 * steps and episodes until cleared: a reset does not touch them (per-episode statistics: clear
 * with the done mask a step returned).  Not part of the snapshot; a shard has its own rows.
 * Bins: v = min(fct_us, 2^26 - 1); bin = v for v < 8, else with e = floor(log2 v)
 * bin = 8 (e - 2) + ((v >> (e - 3)) & 7): lower edge (8 + bin % 8) << (bin / 8 - 1), at most 1/8
 * of it wide; bin 191 is open-ended.
 *
 * lbsim_flow_stats_enable: allocates and zeroes the arrays (784 bytes per server; never moved)
 * and makes the handle a full one: its steps run dynamics_group_full_kernel in two launches,
 * whatever dyn_mapping / step_kernel ask for; results are unchanged.  Before the handle's first
 * lbsim_reset (LBSIM_EINVAL after it, the handle stays as it was); a second call is a no-op.
 * lbsim_step / lbsim_reset gain no allocation and no synchronisation.
 * lbsim_flow_stats_get: asynchronous copies on `stream` into device buffers [B, S] /
 * [B, S, LBSIM_FLOW_STATS_BINS]; any may be NULL.
 * lbsim_flow_stats_quantiles: q_ppm[nq] (device, 1 <= nq <= 16) quantiles in parts per million,
 * clamped to [1, 10^6], into out_us [B, nq] (per_server 0: an env's histograms and counts summed
 * over its servers, the maximum over them) or [B, S, nq] (per_server 1); one kernel on `stream`,
 * no host synchronisation.  With n the row's count, r = max(1, ceil(q_ppm n / 10^6)) and k the
 * first bin whose cumulative count reaches r, the result is min(lower(k + 1) - 1, max_us), max_us
 * for k = 191 and 0 for n = 0: at or above the exact nearest-rank quantile, less than 1/8 above
 * it, exact for q = 1 and below 8 us.
 * lbsim_flow_stats_clear: zeroes the rows of the envs with env_mask[b] != 0 (device mask, NULL =
 * all); one kernel on `stream`, capturable.
 * get / quantiles / clear return LBSIM_ENOTSUP on a handle without statistics. */
#define LBSIM_FLOW_STATS_BINS 192
int lbsim_flow_stats_enable(lbsim_t* h);
int lbsim_flow_stats_get(lbsim_t* h, uint32_t* count, uint64_t* sum_us, uint32_t* max_us,
                         uint32_t* hist, void* stream);
int lbsim_flow_stats_quantiles(lbsim_t* h, const uint32_t* q_ppm, int nq, int per_server,
                               uint32_t* out_us, void* stream);
int lbsim_flow_stats_clear(lbsim_t* h, const uint8_t* env_mask, void* stream);

/* ---- scripted server availability (cluster sizes and outage schedules) ----
 * The server side of a scenario, per env and on the device: which servers of env b are up at
 * each phase of its episode.  A table is up[rows, P, S] bytes (DEVICE pointer), nonzero = up,
 * rows = 1 (every env the same table) or B, 1 <= P <= 4096, each phase held for steps_per_phase
 * (H >= 1) agent steps, cyclic (wrap != 0) or clamped at the last phase.  The phase rule is
 * lbsim_set_rate_schedule's on k = ep_step[b].  P = 1 is a static per-env cluster.
 * The table is applied at the START of every step launch, from the state as it is: one small
 * kernel in front of the step compares, per (env, server), the wanted bit with the down section.
 * up -> down is exactly the failure of fail_prob: the server's queued flows
 * count as dropped, its queue and reservoirs are emptied (hc = head, last_tc = none, res_count =
 * 0, lost_on = 0, a lost-FIN handle's duration count and pending guesses dropped,
 * reservoir_mode VPP's bins zeroed), its cached features are zeroed, down = 1; its flow
 * statistics are kept.  down -> up writes down = 0 and nothing else.  A down server shows as a
 * zero row, is left out of the reward by the active rule, and takes no flows: SED / LSQ never
 * pick it; under ALIAS an arrival sent to it is dropped, so the policy must give it weight 0.
 * Resets are untouched: every server starts up, the warm-up and the reset observation have all
 * S servers, and the first step of the episode applies phase 0.  On a next_step_reset handle an
 * env with ep_step >= max_steps is skipped (that launch resets it) and served at its next step
 * with k = 0.
 * lbsim_server_avail_enable: before the handle's first lbsim_reset (LBSIM_EINVAL after it; a
 * second call is a no-op).  Allocates the down section (zeroed) where the config did not, at the
 * position a fail_prob > 0 handle has it, so the snapshot layout equals such a handle's, and
 * plans the handle as one with failures (no one-wave kernel).  LBSIM_ENOTSUP on a handle with
 * fail_prob > 0: a random recovery would bring a scripted-down server back.
 * lbsim_set_server_avail: LBSIM_ENOTSUP without enable; LBSIM_EINVAL: P outside [1, 4096] or
 * H < 1; LBSIM_ESHAPE: rows neither 1 nor B; LBSIM_ENOMEM: more than 2^31 - 1 entries
 * (B * P * S), or a failed allocation.  The handle stores the table expanded to B rows (B * P * S
 * bytes), allocated by the first call for a given P and rewritten in place, on `stream`, by later
 * calls with the same P: a step captured into a hipGraph after the first call sees later tables
 * on replay; a new P, H or wrap needs a new capture.  Any nonzero byte is up: nothing is
 * validated on the device, and apart from the first allocation the call does not wait.
 * lbsim_clear_server_avail: no table; the next step brings every server up (an allocated table
 * takes all-up values, for the graphs that still read it).
 * lbsim_get_server_avail: want_out[B, S] (u8: the set the next step launch will enforce; all 1
 * for an env that launch resets), up_now_out[B, S] (u8: the current !down) and phase_out[B]
 * (i32), DEVICE pointers, any may be NULL; the same kernel pointed at the outputs, on `stream`.
 * lbsim_step / lbsim_reset gain no allocation and no synchronisation.  down is a state section,
 * so snapshots, forks and lbsim_get_state carry it; the table is NOT in the snapshot: a restored
 * or forked env is reconciled with its slot's table at its next step, by the rule above. */
int lbsim_server_avail_enable(lbsim_t* h);
int lbsim_set_server_avail(lbsim_t* h, const uint8_t* up, int32_t rows, int32_t phases,
                           int32_t steps_per_phase, int32_t wrap, void* stream);
int lbsim_clear_server_avail(lbsim_t* h);
int lbsim_get_server_avail(lbsim_t* h, uint8_t* want_out, uint8_t* up_now_out, int32_t* phase_out,
                           void* stream);

/* ---- hidden cross traffic (flows the agent's balancer did not forward) ----
 * On an enabled handle each arrival is, with probability share[b], a flow of another balancer:
 * it goes to a server drawn from the hidden weights of its env (the action is ignored), occupies
 * the FIFO and is served like any flow, and is seen nowhere: not in observation column 0, the
 * SED / LSQ scores, assign counts, the reservoirs, the reward or the flow statistics.  A hidden
 * flow that meets a full or down server is dropped and counted in `dropped`.  The decision is a
 * hash of (seed, global env id, episode, arrival index): independent of kernel form and sharding.
 * The visible arrival rate is (1 - share) * arrival_rate.
 * lbsim_cross_traffic_enable: before the handle's first lbsim_reset (LBSIM_EINVAL after it; a
 * second call is a no-op).  LBSIM_ENOTSUP on a handle with lost_fin_prob > 0.  Allocates the
 * lost_on section (zeroed) at the position an n_flow_on_mode VPP lost-FIN handle has it -- on
 * such a handle lost_on[b, s] is, as an int32, minus the hidden flows queued at the server -- and
 * makes the handle a full one (dynamics_group_full_kernel, two launches).  Every share starts 0:
 * results equal a handle without cross traffic.
 * lbsim_set_cross_traffic: share[rows] f32 in [0, 1] and weight[rows, S] f32 (finite, >= 0, each
 * row's sum > 0; NULL = uniform), DEVICE pointers, rows = 1 (every env the same) or B
 * (LBSIM_ESHAPE otherwise).  Stored as thr[b] = rint(share * 2^24) and the 24-bit edges
 * cum[b, s] = floor(2^24 c_s / c_{S-1}), c the sequential f64 prefix sum of the weights,
 * cum[b, S-1] = 2^24.  Converted into a staging copy on `stream`, and the call waits for it: with
 * any value out of range (NaN included) it returns LBSIM_EINVAL and what was in force stays.  The
 * arrays are allocated by the first call and rewritten in place: a step captured into a hipGraph
 * sees later values.  New values apply to arrivals assigned from the next launch on (a reset's
 * warm-up included); queued flows keep their flag.  Not part of the snapshot.
 * lbsim_get_cross_traffic: thr_out[B] and cum_out[B, S] (u32, DEVICE pointers, either may be
 * NULL), asynchronous on `stream`.  lbsim_clear_cross_traffic: every share 0, in place.
 * set / get / clear return LBSIM_ENOTSUP on a handle that was not enabled. */
int lbsim_cross_traffic_enable(lbsim_t* h);
int lbsim_set_cross_traffic(lbsim_t* h, const float* share, const float* weight, int32_t rows,
                            void* stream);
int lbsim_get_cross_traffic(lbsim_t* h, uint32_t* thr_out, uint32_t* cum_out, void* stream);
int lbsim_clear_cross_traffic(lbsim_t* h, void* stream);

/* ---- multi-worker servers (per-server worker counts) ----
 * On an enabled handle server s of env b has c = workers[b, s] identical workers, 1 <= c <= 64,
 * behind one FCFS queue; server_rate stays the rate of ONE worker (capacity c * mu).  The queue
 * entries are kept in non-decreasing completion order (a new entry after every equal or smaller
 * one); an arrival at ta that finds n flows queued starts at ta if n < c, else at
 * max(ta, completion of the entry at sorted position n - c).  c = 1 is the single FIFO pipe, bit
 * for bit.  Column 0, assign counts, dropped, eligibility and the flow statistics are defined as
 * before (flows in the system, in service included); a server's reservoir receives, per launch,
 * its carried-in completions in completion order and then the flows that arrive and complete in
 * the step in arrival order.
 * lbsim_server_workers_enable: before the handle's first lbsim_reset (LBSIM_EINVAL after it; a
 * second call is a no-op).  LBSIM_ENOTSUP on a handle with lost_fin_prob > 0 or duration_mode
 * SERVICE.  Allocates workers[B, S] (every count 1; never moved) and makes the handle a full one
 * (dynamics_group_full_kernel, two launches).  With every count 1 results equal a handle that was
 * not enabled.
 * lbsim_set_server_workers: workers[rows, S] int32, a DEVICE pointer, rows = 1 (every env the
 * same) or B (LBSIM_ESHAPE otherwise).  Validated on the device into a staging copy; the call
 * waits on `stream`, and with any count outside [1, 64] returns LBSIM_EINVAL (the count of
 * offenders in lbsim_last_error) and leaves what was in force untouched.  The array is rewritten
 * in place: a step captured into a hipGraph sees later values.  New counts apply to arrivals
 * assigned from the next launch on (a reset's warm-up included); queued flows keep their
 * completion times, and the c queued flows with the latest completions are taken to hold the
 * workers (exact while c is constant since a reset, an approximation after a change).  Not part
 * of the snapshot; a shard passes its own rows.
 * lbsim_get_server_workers: workers_out[B, S] int32 (DEVICE), asynchronous on `stream`.
 * lbsim_clear_server_workers: every count 1, in place, asynchronous on `stream`.
 * set / get / clear return LBSIM_EINVAL on a handle that was not enabled.  lbsim_step and
 * lbsim_reset gain no allocation and no synchronisation. */
int lbsim_server_workers_enable(lbsim_t* h);
int lbsim_set_server_workers(lbsim_t* h, const int32_t* workers, int32_t rows, void* stream);
int lbsim_get_server_workers(lbsim_t* h, int32_t* workers_out, void* stream);
int lbsim_clear_server_workers(lbsim_t* h, void* stream);

/* ---- ground-truth server state (for a centralised critic or mixer) ----
 * What the simulator knows about each server between two launches and the observation does not
 * show, one row of LBSIM_TRUTH_COLS f32 per (env, server).  With n the flows in the server's
 * queue (in service included), c its worker count (1 without server workers) and q(pos) the
 * completion time, in us from the start of the next step, of the queued flow at position pos in
 * completion order:
 *   0 n_total    (float)n
 *   1 n_hidden   hidden cross-traffic flows among them; 0 on a handle without cross traffic
 *   2 busy       (float)min(n, c)
 *   3 cpu        busy / (float)c
 *   4 wait_s     n < c ? 0 : max(0, q(n - c)): until a worker is free for a flow arriving now
 *   5 backlog_s  n == 0 ? 0 : max(0, q(n - 1)): until the server drains with no further arrival
 *   6 up         0 while the server is down (random failures or scripted availability: the
 *                up_now of lbsim_get_server_avail), else 1
 *   7 capacity   (float)c * mu, mu the server rate lbsim_get_env_rates reports: that of the env's
 *                next step, rate schedules included
 * Times are (float)us * 1e-6f seconds.  Every value is >= 0, and each is an exact conversion or
 * one correctly rounded f32 operation.  The rows describe the state as it stands: after a
 * lbsim_reset of done envs, the new episode.  Utilisation averaged over a step is not included.
 * lbsim_ground_truth: truth_out[B, S, LBSIM_TRUTH_COLS] f32, a DEVICE pointer aligned to 16
 * bytes; one small kernel on `stream` that reads the state and writes truth_out only: no
 * allocation, no synchronisation, capturable into a hipGraph.  Works on every handle, without an
 * enable call, from the point where lbsim_step does: after a lbsim_reset of every env, a
 * lbsim_set_state or a lbsim_state_load of every env.  LBSIM_EINVAL: a NULL or misaligned
 * truth_out, or a handle before that point. */
#define LBSIM_TRUTH_COLS 8
int lbsim_ground_truth(lbsim_t* h, float* truth_out, void* stream);
size_t lbsim_ground_truth_cols(void);

/* ---- action latency (per-env control delay applied inside the step) ----
 * On an enabled handle the weights derived from an action come into force delay_us[b] after the
 * start of the step they were passed to, 0 <= delay_us <= M * dt (dt = step_interval in us, M =
 * max_delay_steps).  With m = delay_us / dt, r = delay_us % dt, k = ep_step[b] as the step's
 * dynamics launch reads it, and W(j) the f32 weight row of the action passed to the step with
 * ep_step = j of the current episode (W(j < 0) = 1.0 on every server: the warm-up's weights), an
 * arrival at ta us from the step's start is assigned under W(k - m) if ta >= r and under
 * W(k - m - 1) if ta < r.  Only the choice reads the weights (SED / SED2 scores, the ALIAS table,
 * rebuilt at the switch; LSQ / LSQ2 ignore them).  Resets and warm-ups run at 1.0 as before, the
 * in-launch reset of a next_step_reset handle included (its action is ignored and stored nowhere).
 * lbsim_action_delay_enable: before the handle's first lbsim_reset (LBSIM_EINVAL after it, and
 * for max_delay_steps outside [1, 8]; a second call with the same value is a no-op).  Allocates
 * the weight ring wring[B, max_delay_steps + 2, S] f32 and delay_us[B] (every delay 0; never
 * moved) and makes the handle a full one whose steps launch dynamics_group_delay_kernel, the full
 * form with the delay code, in two launches (no other handle's kernels contain that code).  With
 * every delay 0 results equal a handle that was not enabled.  Composes with every other feature.
 * lbsim_set_action_delay: delay_s[rows] f32 seconds, a DEVICE pointer, rows = 1 (every env the
 * same) or B (LBSIM_ESHAPE otherwise); delay_us = (uint32_t)rint((double)delay_s * 1e6).
 * Validated on the device into a staging copy; the call waits on `stream`, and with any NaN,
 * negative value or value above M * dt returns LBSIM_EINVAL (the count of offenders in
 * lbsim_last_error) and leaves what was in force untouched.  The array is rewritten in place: a
 * step captured into a hipGraph sees later values.  A new delay applies from the next launch on,
 * the rule evaluated with the current value: shortening a delay can skip an action, lengthening
 * one can re-apply an older one.  Not part of any snapshot; a shard passes its own rows.
 * lbsim_get_action_delay: delay_us_out[B] uint32 (DEVICE), asynchronous on `stream`.
 * lbsim_clear_action_delay: every delay 0, in place, asynchronous on `stream`.
 * The weight ring is dynamic state that travels BESIDE a snapshot (lbsim_state_size and the
 * layout of lbsim_get_state are unchanged; lbsim_get_state / lbsim_set_state do not carry it):
 * lbsim_action_delay_size: the bytes of the ring, B * (max_delay_steps + 2) * S * 4.
 * lbsim_action_delay_save: the ring rows of the envs with env_mask[b] != 0 (NULL: all) into
 * dev_buf (DEVICE, [B, max_delay_steps + 2, S] f32), asynchronous on `stream`.
 * lbsim_action_delay_load: row src_env[b] of dev_buf into env b's rows where 0 <= src_env[b] < B
 * (any other index: env b keeps its rows; NULL: row b), asynchronous on `stream`.  A wrong
 * `bytes` is LBSIM_ESHAPE.  Call them beside lbsim_state_save / lbsim_state_load with the same
 * mask / indices: a restored env replays the same pending actions, a forked env inherits its
 * source's.
 * All but enable return LBSIM_EINVAL on a handle that was not enabled.  lbsim_step and
 * lbsim_reset gain no allocation and no synchronisation. */
int lbsim_action_delay_enable(lbsim_t* h, int32_t max_delay_steps);
int lbsim_set_action_delay(lbsim_t* h, const float* delay_s, int32_t rows, void* stream);
int lbsim_get_action_delay(lbsim_t* h, uint32_t* delay_us_out, void* stream);
int lbsim_clear_action_delay(lbsim_t* h, void* stream);
int lbsim_action_delay_size(const lbsim_t* h, size_t* bytes_out);
int lbsim_action_delay_save(lbsim_t* h, void* dev_buf, size_t bytes, const uint8_t* env_mask,
                            void* stream);
int lbsim_action_delay_load(lbsim_t* h, const void* dev_buf, size_t bytes, const int32_t* src_env,
                            void* stream);

/* Shared server pools: several balancers in front of ONE set of servers.
 * A = `balancers` consecutive envs of the handle form a pool: pool c is envs cA .. cA + A - 1,
 * and its members share one physical set of S FIFO servers.  Every env stays one balancer with
 * its own arrival stream (exactly the one it would have alone), action row, (S, 11) observation,
 * reward, reservoirs, drops and assign counts; only the queues are shared.  One event loop per
 * pool: the earliest completion due no later than the pool's next arrival goes first, else the
 * next arrival, the smallest next_arr over the members (ties: the lowest member).  Member a's
 * arrival is assigned by its own weight row and its OWN flows in flight n_own[a][s] (SED / SED2
 * scores, LSQ / LSQ2 counts; the hashes from its own words), a server is eligible while its
 * PHYSICAL queue is below queue_capacity, and a flow with no eligible server counts in member
 * a's `dropped`.  A flow starts at max(ta, tc of the last queued flow, whoever owns it); its
 * sample tc - ta goes into its owner's reservoir (gid_owner, s) under the unchanged rule.
 * Observation column 0 of member a is n_own[a][s]: bits 16-31 of its hc[b, s] hold its own count
 * and bit 15 its own big flag.  lbsim_reset resets a pool iff any member's mask byte is set, and
 * then every member of it (so ep_step, clock and done are equal across a pool).  With balancers
 * = 1 results equal a handle that was not enabled, bit for bit.
 * lbsim_server_pool_enable: before the handle's first lbsim_reset (LBSIM_EINVAL after it; a
 * second call with the same value is a no-op).  LBSIM_EINVAL for balancers outside [1, 8],
 * num_envs % balancers != 0 or env_id_offset % balancers != 0 (a pool never straddles a shard).
 * LBSIM_ENOTSUP, the message naming the option, with num_servers > 16, assign_policy ALIAS,
 * arrival_source TRACE, lost_fin_prob > 0, fail_prob > 0, reservoir_mode VPP, n_flow_on_mode
 * VPP, duration_mode SERVICE or next_step_reset, and on a handle with flow statistics, workload
 * tables, server availability, cross traffic, server workers, action delay, a rate or trace
 * schedule, or per-env rates in force (they may hold per-env server rates: call
 * lbsim_clear_env_rates, enable, then set the arrival rates again).  On an enabled handle those
 * opt-ins, a non-NULL server_rate in lbsim_set_env_rates, and lbsim_state_save /
 * lbsim_state_load (a per-env fork would tear a pool apart) return LBSIM_ENOTSUP.  Per-env
 * arrival rates (unequal ECMP splits),
 * normalize_obs, both action types, lbsim_step_ex's outputs, lbsim_episode_stats,
 * lbsim_vpp_export, lbsim_get_state / lbsim_set_state and hipGraph capture of lbsim_step work as
 * on any handle.  The steps launch dynamics_pool_kernel (lbsim_dynamics_kernel:
 * LBSIM_DYN_KERNEL_POOL) and the handle's ordinary observe; no allocation or synchronisation is
 * added to lbsim_step or lbsim_reset.
 * The state gains two sections after all the others (lbsim_state_size counts them): pool_hc
 * [C, S] u32, the physical FIFO's ring head | count << 16, and pool_owner [C, S, Q] u8, the
 * member that owns each ring entry; the entries {tc, ta} are the first member's ring rows.
 * lbsim_ground_truth on an enabled handle describes the physical server in every member's row:
 * n_total the physical queue length, n_hidden that minus the member's own count (what the other
 * balancers put there), busy / cpu / wait_s / backlog_s of the physical FIFO, up 1, capacity mu.
 * lbsim_server_pool_size: A, or 0 on a handle that was not enabled. */
int lbsim_server_pool_enable(lbsim_t* h, int32_t balancers);
int lbsim_server_pool_size(const lbsim_t* h);

/* Processor-sharing servers, opt-in per handle: every server has one
 * worker that the n flows queued on it share equally, instead of serving them first come first
 * served.  All quantities are integer us.  A server keeps a virtual clock V, a carry acc and the
 * time t_last of its last update; advance(t): with n > 0 queued, acc += t - t_last, V += acc / n,
 * acc %= n (else acc = 0), then t_last = t.  An arrival at ta assigned to the server advances it
 * to ta, takes svc = max(1, (int)(work * 1e6 / mu)) as on a FIFO server and the tag V + svc, and
 * is queued in tag order after every equal tag.  The head completes at t_last + (tag_head - V) *
 * n - acc; its sample fct = tc - ta is stamped as every sample is and always drawn from the
 * reservoir stream.  Everything else -- arrivals, the SED / LSQ scores on the queued counts,
 * eligibility n < queue_capacity, drops, the pop rule (completions due no later than the next
 * arrival first), the rebase, clock -- is the FIFO simulator's.  At a step's end every server is
 * advanced to dt; the ring then holds {tag - V, ta - dt} in tag order and the server's last_tc
 * word holds acc: the state layout and lbsim_state_size are those of any handle.
 * lbsim_processor_sharing_enable: before the handle's first lbsim_reset (LBSIM_EINVAL after it; a
 * second call is a no-op).  LBSIM_ENOTSUP, the message naming the option, with assign_policy
 * ALIAS, arrival_source TRACE, lost_fin_prob > 0, fail_prob > 0, reservoir_mode VPP,
 * n_flow_on_mode VPP, duration_mode SERVICE or next_step_reset, and on a handle with server
 * availability, cross traffic, server workers, action delay or server pools; on an enabled handle
 * those opt-ins and lbsim_ground_truth (its wait and backlog columns are FIFO quantities) return
 * LBSIM_ENOTSUP.  Per-env rates, rate schedules, workload tables, flow statistics, masked resets,
 * lbsim_state_save / lbsim_state_load, lbsim_get_state / lbsim_set_state, lbsim_vpp_export and
 * hipGraph capture of lbsim_step work as on any handle.  The steps launch dynamics_ps_kernel
 * (lbsim_dynamics_kernel: LBSIM_DYN_KERNEL_PS) and the handle's ordinary observe; no allocation
 * or synchronisation is added to lbsim_step or lbsim_reset.
 * lbsim_processor_sharing: 1 on an enabled handle, else 0. */
int lbsim_processor_sharing_enable(lbsim_t* h);
int lbsim_processor_sharing(const lbsim_t* h);

/* Duration samples at every data ACK, opt-in per handle: the data plane
 * records a flow_duration sample on every pure ACK after the handshake, so a flow offers its
 * server's duration reservoir one sample per data ACK instead of one at its completion.  All
 * quantities are integer us.  A flow on server s that arrived at ta starts service at t0 =
 * max(ta, tc of its predecessor on s), completes at tc = t0 + svc and emits k = min(max_acks,
 * max(1, svc / ack_us)) ACKs, ACK j = 1..k at t_j = t0 + (svc * j) / k (so t_k = tc); each offers
 * the flow's age t_j - ta, stamped (clock * dt + t_j) / 1000 ms, to the duration reservoir of s,
 * in the step whose (0, dt] holds t_j -- the warm-up steps of a reset included.  The duration
 * reservoir has its own count and {us, ts} records (state sections res_dur, 1024 S bytes per env,
 * and res_count_dur, 4 S bytes per env: lbsim_state_size grows, lbsim_set_state rejects a plain
 * handle's snapshot by size) and draws every sample from the reservoir stream under the word
 * (2 << 24) | (1 << 17) | s.  The fct reservoir, the queues, the counters and observation columns
 * 0-5 are bit for bit those of a handle without the option; columns 6-10 are the features of the
 * duration reservoir.
 * lbsim_ack_samples_enable: max_acks in [1, 32] (LBSIM_EINVAL otherwise), before the handle's
 * first lbsim_reset (LBSIM_EINVAL after it; a second call with the same value is a no-op, with
 * another LBSIM_EINVAL).  LBSIM_ENOTSUP, the message naming the option, with lost_fin_prob > 0,
 * fail_prob > 0, duration_mode SERVICE, reservoir_mode VPP, n_flow_on_mode VPP or
 * next_step_reset, and on a handle with server availability, cross traffic, server workers,
 * action delay, server pools, processor sharing, flow statistics, workload tables, a trace bank of
 * several traces or a trace schedule; on an enabled handle those opt-ins return LBSIM_ENOTSUP.
 * The five assignment policies, Poisson arrivals and a single trace, per-env rates, rate
 * schedules, normalize_obs, masked resets, lbsim_get_state / lbsim_set_state, lbsim_state_save /
 * lbsim_state_load, lbsim_ground_truth and hipGraph capture of lbsim_step work as on any handle.
 * The steps and resets launch dynamics_group_ack_kernel (lbsim_dynamics_kernel:
 * LBSIM_DYN_KERNEL_ACK) and the general observe; no allocation or synchronisation is added to
 * lbsim_step or lbsim_reset.
 * lbsim_ack_samples: max_acks of an enabled handle, else 0.
 * lbsim_set_ack_interval: us[rows] host int32 in [1, 2^30], rows = 1 (every env) or num_envs; in
 * force from the next launch on (a flow in service then places its remaining ACKs by the new
 * interval).  A value out of range: LBSIM_EINVAL, the previous intervals stay in force.  The call
 * copies synchronously into a device array that never moves, so a captured graph sees it.
 * lbsim_get_ack_interval: us_out[num_envs] host int32.  lbsim_clear_ack_interval: every env back
 * to 1000 us, the value after the enable.  All three return LBSIM_ENOTSUP on a handle without the
 * option.  The intervals are not part of the state. */
int lbsim_ack_samples_enable(lbsim_t* h, int32_t max_acks);
int lbsim_ack_samples(const lbsim_t* h);
int lbsim_set_ack_interval(lbsim_t* h, const int32_t* us, int rows);
int lbsim_get_ack_interval(lbsim_t* h, int32_t* us_out);
int lbsim_clear_ack_interval(lbsim_t* h);

/* Cores of processor-sharing servers, on a handle with
 * lbsim_processor_sharing_enable (LBSIM_ENOTSUP on any other): server s of env b has c = cores[b, s]
 * cores, each of rate server_rate, and its n flows are served at rate min(1, c / n) each: with
 * n <= c every flow has a core to itself, above c the cores are shared equally.  The rule, integer
 * us: advance(t) with d = t - t_last: n = 0: acc = 0; 1 <= n <= c: V += d, acc = 0; n > c: acc +=
 * c d, V += acc / n, acc %= n; then t_last = t.  The head completes at t_last + (tag_head - V) with
 * n <= c, else at t_last + ceil(((tag_head - V) n - acc) / c) (t_last where that is not positive),
 * where V reaches tag_head exactly and acc is left in [0, c).  c = 1 is section 3.22's rule bit for
 * bit; c >= queue_capacity makes fct = svc for every flow.  Everything else is section 3.22's; the
 * state layout is unchanged (acc stays in the last_tc word) and the counts are not part of it, nor
 * of a snapshot: a shard passes its own rows.
 * lbsim_set_ps_cores: `cores` is int32 [rows, S] on the device, rows = 1 (every env) or num_envs
 * (LBSIM_ESHAPE otherwise).  Converted into a staging copy and validated on `stream`, and the call
 * waits for that stream: a count outside [1, 64] returns LBSIM_EINVAL and what was in force stays.
 * The array is allocated by the first call, which therefore precedes a graph capture, never moves
 * afterwards and is rewritten in place: replays of a captured lbsim_step see new counts.  They
 * apply from the next launch on (step, reset, warm-up); queued flows keep their remaining tags.
 * Until the first call the handle launches what it launched before, with the same results.
 * lbsim_get_ps_cores: the counts in force into cores_out, int32 [num_envs, S] on the device (all 1
 * before the first set call), asynchronous on `stream`.
 * lbsim_clear_ps_cores: every count 1, in place, asynchronous on `stream`.
 * lbsim_ps_server_state: the privileged view of the servers as they stand after the last
 * lbsim_reset or lbsim_step (LBSIM_EINVAL before the first reset) into state_out, float32
 * [num_envs, S, LBSIM_PS_STATE_COLS] on the device, aligned to 16 bytes: column 0 the flows n on
 * the server, 1 the busy cores min(n, c), 2 the unfinished work in seconds of one core (the sum of
 * the remaining tags, less acc where n > c), 3 the seconds until the server is empty with no
 * further arrival, the last completion time the rule gives over the queued entries.  With c = 1
 * columns 2 and 3 are equal.  One kernel on `stream`, no allocation, no synchronisation: it can
 * be captured after lbsim_step.  (lbsim_ground_truth stays refused on these handles.) */
#define LBSIM_PS_STATE_COLS 4
int lbsim_set_ps_cores(lbsim_t* h, const int32_t* cores, int32_t rows, void* stream);
int lbsim_get_ps_cores(lbsim_t* h, int32_t* cores_out, void* stream);
int lbsim_clear_ps_cores(lbsim_t* h, void* stream);
size_t lbsim_ps_server_state_cols(void);
int lbsim_ps_server_state(lbsim_t* h, float* state_out, void* stream);

/* Shared server pools of processor-sharing servers: the discipline of a
 * pool's servers is a property of the pool.  lbsim_server_pool_enable_ps is
 * lbsim_server_pool_enable -- the same checks, allocations, messages and state sections -- and
 * marks the pool's S physical servers processor-sharing ones of c cores each (section 3.23's rule;
 * c = 1 until lbsim_set_pool_ps_cores).  Per (pool, server): the clock words V, acc, t_last and n
 * entries {tag, ta, owner} in non-decreasing tag order, a new entry after every equal tag.  The
 * pool's next arrival, the assignment by the member's own weight row and own counts, eligibility
 * by the physical n < queue_capacity and the drop rule are section 3.21's; on the chosen server
 * the completions due by ta go first, then advance(s, ta), tag = V + svc and the sorted insert,
 * moved entries carrying their owner.  A completion pops the head: its sample tc - ta goes into
 * the owner's reservoir (gid_owner, s), always drawn from the owner's reservoir stream at the
 * owner's count, stamped with the pool's clock.  No new state section: the entries {tag - V, ta}
 * are the first member's ring rows in tag order from the physical head, the owners pool_owner, the
 * physical head | n << 16 pool_hc, acc the last_tc word of every member's row of that server, and
 * a member's hc word the physical head, its own big flag and its own count.  balancers = 1 equals
 * a lbsim_processor_sharing_enable handle with the same cores bit for bit.
 * Calling lbsim_server_pool_enable_ps or lbsim_server_pool_enable on a handle whose pools were
 * enabled the other way returns LBSIM_EINVAL.  Such a handle is a pool handle, not a
 * lbsim_processor_sharing_enable one: lbsim_processor_sharing stays 0, lbsim_set_ps_cores and
 * lbsim_ps_server_state keep refusing, every refusal of a pool handle holds, and
 * lbsim_ground_truth returns LBSIM_ENOTSUP (lbsim_pool_ps_state is its view).  The steps launch
 * dynamics_pool_ps_kernel (lbsim_dynamics_kernel: LBSIM_DYN_KERNEL_POOL_PS) and the handle's
 * ordinary observe; no allocation or synchronisation is added to lbsim_step or lbsim_reset.
 * lbsim_server_pool_discipline: 1 on such a handle, 0 with FIFO pools or none.
 * lbsim_set_pool_ps_cores / lbsim_get_pool_ps_cores / lbsim_clear_pool_ps_cores: as the
 * lbsim_*_ps_cores calls, with one row per POOL: `cores` is int32 [rows, S], rows = 1 or C =
 * num_envs / balancers; cores_out int32 [C, S].  On any other handle LBSIM_ENOTSUP.
 * lbsim_pool_ps_state: state_out float32 [num_envs, S, LBSIM_POOL_PS_STATE_COLS] on the device,
 * each member's row describing the physical server: column 0 its flows n, 1 n minus the member's
 * own count (what the other balancers put there), 2 the busy cores min(n, c), 3 the unfinished
 * work in seconds of one core, 4 the seconds to drain (columns 2 and 3 of lbsim_ps_server_state
 * on the physical entries).  LBSIM_EINVAL before the first reset.  One kernel on `stream`, no
 * allocation, no synchronisation. */
#define LBSIM_POOL_PS_STATE_COLS 5
int lbsim_server_pool_enable_ps(lbsim_t* h, int32_t balancers);
int lbsim_server_pool_discipline(const lbsim_t* h);
int lbsim_set_pool_ps_cores(lbsim_t* h, const int32_t* cores, int32_t rows, void* stream);
int lbsim_get_pool_ps_cores(lbsim_t* h, int32_t* cores_out, void* stream);
int lbsim_clear_pool_ps_cores(lbsim_t* h, void* stream);
size_t lbsim_pool_ps_state_cols(void);
int lbsim_pool_ps_state(lbsim_t* h, float* state_out, void* stream);

/* Stateless: n Vose alias tables of S weights each (device pointers), the O(n) build of
 * problem-07's realtime VPP plugin (realtime-mode/problem-07-realtime-deployment/vpp-plugin/
 * alias_table.h:82-158, alias_table_build, rebuilt by lb_rl_node.c:92-111 from the weights the
 * controller writes): weights[n, S] f32 -> prob_out[n, S] f32, alias_out[n, S] u32, in the
 * float32 arithmetic of the C (a row summing to <= 0 gets the identity table). */
int lbsim_vose_tables(const float* weights, int64_t n, int S, float* prob_out,
                      uint32_t* alias_out, void* stream);

/* Stateless: k draws of alias_table_sample (alias_table.h:195-209, the per-packet pick of
 * lb_rl_node.c:246-288) from each of n tables (prob[n, S], alias[n, S] as lbsim_vose_tables
 * writes them) with the table's xorshift32 state (alias_table.h:163-172; state_io[n] u32, the
 * C's random_state, advanced in place).  idx_out[n, k] i32 (may be NULL) gets the picks;
 * hist_out[n, S] u64 (may be NULL) the per-server counts of this call
 * (alias_table_test_distribution, :221-237).  k <= INT32_MAX. */
int lbsim_vose_sample(const float* prob, const uint32_t* alias, int64_t n, int S,
                      uint32_t* state_io, int64_t k, int32_t* idx_out, uint64_t* hist_out,
                      void* stream);

/* ---- the VPP LB plugin's shared-memory view (src/vpp/lb/shm.h:14-91, marllb_amd/vpp_shm.py) ----
 * lbsim_vpp_export: envs [env_begin, env_begin + n_envs) of the handle as the data plane's raw
 * per-AS reservoirs (reservoir_as_t, shm.h:35-37; written by lbhash.h:116-135):
 *   tv_out [n_envs, S, 2, 128, 2] f32 = per server {fct[128], flow_duration[128]} of (t, v)
 *   pairs, t = the sample's completion time and v = the sample, both in seconds (slots past
 *   min(count, 128) are (0, 0), VPP's zeroed shm); n_flow_on_out [n_envs, S] i32 (as_stat_t
 *   n_flow_on, may be NULL); ts_out [n_envs] f32 frame time = simulated seconds since reset
 *   (msg_out_t ts, may be NULL).
 * lbsim_vpp_features: Shm_Manager.process_reservoir (src/lb/shm_proxy.py:518-543) of n raw
 *   reservoirs tv[n, 128, 2] (t, v) f32, reservoir r at frame time ts[r / res_per_ts] ->
 *   feats_out[n, 5] f64 {avg, 90, std, avg_decay, 90_decay} over all 128 bins, the decayed value
 *   v * decay^(ts - t) (numpy order; everything but the f64 pow bit-identical). */
int lbsim_vpp_export(lbsim_t* h, int64_t env_begin, int64_t n_envs, float* tv_out,
                     int32_t* n_flow_on_out, float* ts_out, void* stream);
int lbsim_vpp_features(const float* tv, const float* ts, int64_t res_per_ts, int64_t n,
                       double decay, double* feats_out, void* stream);

/*
 * Kernel timing: between lbsim_profile_begin and lbsim_profile_end every kernel launch of this
 * handle is bracketed by hipEvents recorded on the launch stream (at most max_launches launches
 * are timed; inside lbsim_step the event that closes the dynamics launch also opens the observe
 * launch, so a step records three events, not four).  lbsim_profile_end synchronises, and returns per kernel class
 * {0: dynamics step, 1: observe step, 2: dynamics reset, 3: observe reset} the summed event time
 * in ms (ms_out[4]) and the number of timed launches (count_out[4]).  lbsim_profile_end_ex
 * returns the first n_classes (<= LBSIM_PROFILE_CLASSES) classes, class 4 being the fused step
 * kernel.  Used by bench.py.  The events are created with hipEventDisableSystemFence (no cache
 * writeback / invalidate between the bracketed launches): read the times only after synchronising the device, as lbsim_profile_end's callers do.
 */
#define LBSIM_PROFILE_CLASSES 5
/* (lbsim_profile_end reports the first 4 classes only: a handle whose steps are one launch --
 * step_wave_kernel under AUTO, or FUSED -- times them in class 4, so its callers need
 * lbsim_profile_end_ex(..., 5).) */
int lbsim_profile_begin(lbsim_t* h, int max_launches);
int lbsim_profile_end(lbsim_t* h, double* ms_out, int64_t* count_out);
int lbsim_profile_end_ex(lbsim_t* h, double* ms_out, int64_t* count_out, int n_classes);

/* The kernels the last lbsim_step_ex (which = 0) or lbsim_reset_ex (which = 1) of this handle
 * launched, in launch order, as "class=name;class=name" (class as in the profiler above; name the
 * kernel's template signature as rocprofv3 reports it, e.g. "0=dynamics_group_kernel<4, 0, 0,
 * false, 1>;1=observe_kernel<4, 0, false>").  bench.py keys its committed PMC counter files by
 * these names.  LBSIM_ESHAPE if buf_len is too short.  Measurement labels; no reference
 * counterpart. */
int lbsim_launch_names(lbsim_t* h, int which, char* buf, size_t buf_len);

/* Snapshot: total bytes of the device state, and copies to/from a HOST buffer of that size.
 * Layout: DESIGN.md §4 (used by the parity tests to compare every state word with oracle/).  A
 * handle whose duration samples can differ from its fct samples (duration_mode SERVICE, or
 * lost_fin_prob > 0) keeps a duration plane and has a larger snapshot: lbsim_set_state rejects a
 * snapshot of the other record format by its size (LBSIM_ESHAPE). */
int lbsim_state_size(const lbsim_t* h, size_t* bytes_out);
int lbsim_get_state(lbsim_t* h, void* host_buf, size_t bytes);
int lbsim_set_state(lbsim_t* h, const void* host_buf, size_t bytes);

/* ---- on-device snapshots: save, restore and fork env states ----
 * The same snapshot as above, in a caller-owned DEVICE buffer of lbsim_state_size bytes laid out
 * exactly as lbsim_get_state lays out its host buffer (DESIGN.md §4, B envs): a buffer written by
 * lbsim_state_save of all envs and copied to the host is byte-identical to lbsim_get_state at the
 * same point.  Both calls are one kernel launch on `stream`: asynchronous, no allocation, no
 * synchronisation, no host copy, so both can be captured into a hipGraph (the buffer and index
 * pointers are then part of the capture; their contents are read at every replay).
 * lbsim_state_save: copies the state of the envs with env_mask[b] != 0 (device u8[B]; NULL: all)
 *   into dev_buf; bytes of envs outside the mask are left as they were.
 * lbsim_state_load: env b takes the state that dev_buf holds for env src_env[b] (device
 *   int32[B]); src_env NULL = identity, every env its own saved state.  An entry < 0 or >= B
 *   leaves env b untouched: indices are never rejected on the device (a raise would need a host
 *   synchronisation), out of range means "keep".  One source may feed many envs (a fork): they
 *   share the queues, reservoirs and the one arrival already drawn, and since every later draw is
 *   keyed by the env's own global id their futures are independent; an env loaded with its OWN
 *   saved state replays exactly the arrivals, work, failures and reservoir draws it had from there.
 *   A load with src_env == NULL marks the handle initialised, as lbsim_set_state does; with a
 *   src_env the handle must have been reset or loaded before (LBSIM_EINVAL otherwise: the envs it
 *   keeps would have no state).
 * Errors: NULL handle or buffer, or a dev_buf that is not 16-byte aligned: LBSIM_EINVAL; bytes
 *   other than lbsim_state_size: LBSIM_ESHAPE.
 * Outside the snapshot, as for lbsim_get_state: the seed, the per-env rates and rate schedules,
 *   the flow statistics and the trace.  A load leaves all of them as they are: a restored or
 *   forked env runs at the rates (and schedule rows) of the SLOT it is loaded into, and its
 *   slot's flow statistics go on counting. */
int lbsim_state_save(lbsim_t* h, void* dev_buf, size_t bytes, const uint8_t* env_mask,
                     void* stream);
int lbsim_state_load(lbsim_t* h, const void* dev_buf, size_t bytes, const int32_t* src_env,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LBSIM_H */
