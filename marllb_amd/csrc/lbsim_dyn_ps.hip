// lbsim_dyn_ps.hip -- the dynamics of a handle with processor-sharing servers:
// dynamics_ps_kernel, one group of G lanes per env, lane s owning server s, 64 / G envs per wave;
// one object per mode: built with -DLBSIM_DYN_MODE=0 (kModeStep, launch_dynamics_ps_step) and =1
// (kModeReset, launch_dynamics_ps_reset).  Objects of their own, as lbsim_dyn_pool.hip's are: no
// other kernel gains code.
//
// A lane keeps its server's virtual clock V, the carry acc, the time t_last of the last update,
// the count n and the head entry's tag in registers, and the entries {tag, ta}, sorted by tag, in
// its HBM ring row (lbsim_ps.h's rule over PsRing).  One event loop per env: every lane completes
// its own server's flows due by the env's next arrival -- servers do not interact, so the order of
// two servers' completions leaves no trace: the samples of a server enter its own reservoir in its
// own completion order -- then the group assigns that arrival, and the chosen lane advances its
// clock to the arrival and inserts the entry by its tag.  Arrivals are drawn G at a time, lane j
// drawing arrival k + j, as dynamics_group_kernel draws them; a PS handle may have workload
// tables, per-env rates and flow statistics, so the draws go through the table rule when the
// handle has tables and the statistics' arrays travel as a kernel argument (§3.11), as do the
// servers' core counts (§3.23: a null pointer until lbsim_set_ps_cores, every server one core).
#include "lbsim_internal.h"
#include "lbsim_dyn_group.h"
#include "lbsim_ps.h"

#if !defined(LBSIM_DYN_MODE) || (LBSIM_DYN_MODE != 0 && LBSIM_DYN_MODE != 1)
#error "build with -DLBSIM_DYN_MODE=0 (step) or 1 (reset)"
#endif

namespace lbk {
namespace {

constexpr int MODE = LBSIM_DYN_MODE == 0 ? kModeStep : kModeReset;

// A server's ring row in HBM by queue position (lbsim_ps.h's accessor).
struct PsRing {
  int2* ring;
  int head, Q;
  __device__ __forceinline__ int2 get(int pos) const {
    return ring[(uint32_t)ps_ring_index(head, pos, Q)];
  }
  __device__ __forceinline__ void set(int pos, const int2& e) const {
    ring[(uint32_t)ps_ring_index(head, pos, Q)] = e;
  }
};

template <int G, int MODE, int POLICY>
__global__ void __launch_bounds__(64)
    dynamics_ps_kernel(DevState st, SimParams p, const void* action, int action_dtype,
                       int32_t* assign_out, const uint8_t* reset_mask, FlowStats fs,
                       const int32_t* cores) {
  static_assert(G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64,
                "group = a power of two lanes of the wave");
  static_assert(POLICY >= 0 && POLICY <= 3, "SED, SED2, LSQ, LSQ2");
  constexpr bool two_choice = (POLICY == 1 || POLICY == 3);
  constexpr bool lsq = (POLICY == 2 || POLICY == 3);
  __shared__ int4 acache[64];  // draw-ahead arrival slots, [group][G]

  const int lane = (int)threadIdx.x;
  const int s = lane & (G - 1);
  const int gbase = lane & ~(G - 1);
  const int S = p.S, Q = p.Q;
  const int32_t dt = p.dt_us;
  const uint32_t b = blockIdx.x * (uint32_t)(64 / G) + (uint32_t)(lane / G);
  if (b >= (uint32_t)p.B) return;  // whole groups leave together
  if (MODE == kModeReset && reset_mask != nullptr && reset_mask[b] == 0) return;

  const bool act = s < S;
  const uint32_t gid = p.env_id_offset + b;
  const uint32_t sb = b * (uint32_t)S + (uint32_t)(act ? s : 0);  // this lane's (env, server) row
  const float mean_gap = env_mean_gap(st, p, b);
  const WorkSel ws = env_work_sel(st, b);  // the env's workload tables, if the handle has any
  float scale = p.svc_scale[0];
#pragma unroll
  for (int k = 1; k < G; ++k) scale = (k == s) ? p.svc_scale[k] : scale;
  if (st.env_scale != nullptr) scale = st.env_scale[sb];

  // ---- the env's words (the same in every lane of the group)
  int32_t next_arr;
  float next_work;
  uint32_t u2, u3, arr_idx, dropped, episode, clock;
  // ---- server s, in lane s
  PsClock ck{0, 0, 0};
  PsRing ring{st.ring + (size_t)sb * (size_t)Q, 0, Q};
  int32_t n = 0, head_tag = 0, assigned = 0;
  uint32_t rcnt = 0u;
  bool big = false;
  uint32_t cw[4] = {0u, 0u, 0u, 0u};  // the reservoir slots written this launch (DevState::chg)
  float wgt = 1.0f;
  // the server's cores (§3.23; nullptr, wave-uniform: every server has one)
  int32_t cr = 1;
  if (cores != nullptr) cr = cores[sb];
  // flow statistics: a step's completions count, a reset's warm-up is not the policy's doing
  const bool fs_on = MODE == kModeStep && act && fs.hist != nullptr;
  uint32_t fs_cnt = 0u, fs_max = 0u;
  unsigned long long fs_sum = 0ull;
  uint32_t* const fs_row = fs_on ? fs.hist + (size_t)sb * kFlowBins : nullptr;

  if constexpr (MODE == kModeReset) {
    // a new episode: its first arrival, empty servers, weights 1.0
    episode = st.episode[b] + 1u;
    clock = 0u;
    dropped = 0u;
    arr_idx = 0u;
    const u32x4 d = philox4x32_10(u32x4{0u, gid, episode, kStreamArrival << 24}, p.key0, p.key1);
    arrival_from_draw(mean_gap, d, 0, next_arr, next_work, u2, u3, ws);
    cw[0] = 1u;  // emptied reservoirs: slot 0 marked written, so the next observe recomputes the row
  } else {
    episode = st.episode[b];
    clock = st.clock[b];
    dropped = st.dropped[b];
    arr_idx = st.arr_idx[b];
    next_arr = st.next_arr[b];
    next_work = st.next_work[b];
    u2 = st.next_u2[b];
    u3 = st.next_u3[b];
    if (act) {
      const uint32_t hc = st.hc[sb];
      int head = (int)(hc & kHcHead);
      int cnt = (int)(hc >> 16);
      // (only lbsim_set_state could load words outside the ring)
      ring.head = head < Q ? head : 0;
      n = cnt <= Q ? cnt : Q;
      big = (hc & kHcBig) != 0u;
      // the carry lives in the server's last_tc word, which PS does not otherwise use: in [0, n)
      const int32_t a = st.last_tc[sb];
      ck.acc = (n > 0 && a > 0 && a < n) ? a : 0;
      rcnt = st.res_count[sb];
      wgt = action_weight_sel(p, action, action_dtype, (size_t)sb);
      if (n > 0) head_tag = ring.get(0).x;
      if (fs_on) {
        fs_cnt = fs.count[sb];
        fs_max = fs.max_us[sb];
        fs_sum = fs.sum[sb];
      }
    }
  }
  // the draw-ahead slots hold arrivals [cb, cb + G): none yet
  uint32_t cb = arr_idx + 1u + 0x80000000u;

  // ---- one step of the env (a reset runs warmup_steps of them at weights 1.0)
  auto sim_step = [&]() {
    const uint64_t base_us = (uint64_t)clock * (uint64_t)dt;
    const uint32_t base_ms = (uint32_t)(base_us / 1000u);
    const uint32_t base_rem = (uint32_t)(base_us - (uint64_t)base_ms * 1000u);
    const double den = (double)wgt + 1e-9;

    for (;;) {
      const bool arrival_due = next_arr < dt;  // the same in every lane of the group
      const int32_t th = arrival_due ? next_arr : dt;
      // ---- this server's completions due no later than it, each at its own time: the clock
      //      reaches the head's tag, the head leaves, its sample is drawn from the reservoir stream
      while (act && n > 0) {
        const PsDue due = ps_next_completion(ck, n, cr, head_tag);
        const int32_t tc = due.tc;
        if (tc > th) break;
        ps_complete(ck, due, head_tag);
        const int32_t ta = ring.get(0).y;
        ring.head = ring.head + 1 == Q ? 0 : ring.head + 1;
        n -= 1;
        if (n > 0) head_tag = ring.get(0).x;
        const uint32_t fct = (uint32_t)(tc - ta);
        int slot = (int)rcnt;
        if (rcnt >= (uint32_t)K) {
          const u32x4 d = philox4x32_10(
              u32x4{rcnt >> 1, gid, episode, (kStreamReservoir << 24) | (uint32_t)s}, p.key0,
              p.key1);
          slot = reservoir_slot(rcnt, d);
        }
        if (slot >= 0) {
          big |= big_record(fct, fct);
          st.res[(size_t)sb * K + (uint32_t)slot] =
              make_uint2(fct, base_ms + (base_rem + (uint32_t)tc) / 1000u);
#pragma unroll
          for (int w = 0; w < 4; ++w) cw[w] |= (w == (slot >> 5)) ? 1u << (slot & 31) : 0u;
        }
        rcnt = count_inc(rcnt);
        if (fs_on) {
          fs_cnt += 1u;
          fs_sum += fct;
          fs_max = fct > fs_max ? fct : fs_max;
          fs_row[flow_bin(fct)] += 1u;  // the lane owns its server's row for the whole launch
        }
      }
      if (!arrival_due) break;  // group-uniform

      // ---- the arrival: choose a server by the queued counts (§3.3); full servers not eligible
      const int32_t ta = next_arr;
      float score = 0.0f;
      if (act) {
        if constexpr (lsq) score = (float)n;
        else score = (float)((double)(n + 1) / den);
      }
      const bool elig = act && n < Q;
      const uint64_t em = group_bits<G>(__ballot(elig), gbase);
      int chosen = -1;
      if constexpr (two_choice) {
        const int h1 = two_choice_h1(u2, S), h2 = two_choice_h2(u2, S);
        const uint32_t bits = __float_as_uint(score);
        const float s1 = __uint_as_float(group_or<G>(s == h1 ? bits : 0u));
        const float s2 = __uint_as_float(group_or<G>(s == h2 ? bits : 0u));
        const bool ok1 = (em >> h1) & 1u, ok2 = (em >> h2) & 1u;
        chosen = (ok1 && ok2) ? ((s2 < s1) ? h2 : h1) : (ok1 ? h1 : (ok2 ? h2 : -1));
      } else {  // the scan from the hashed server h, replaced on a strictly lower score (§3.3)
        const bool num = elig && score == score;
        const float m = key_f32(group_min_i32<G>(num ? f32_key(score) : 0x7f800000));
        const int h = (int)__umulhi(u2, (uint32_t)S);
        const int c0 = ((em >> h) & 1u) ? h : (em ? __builtin_ctzll(em) : -1);
        const uint64_t tie = group_bits<G>(__ballot(num && score == m), gbase);
        const uint64_t nan = group_bits<G>(__ballot(score != score), gbase);
        chosen = c0 < 0 ? -1 : ((((tie | nan) >> c0) & 1u) ? c0 : (tie ? __builtin_ctzll(tie) : -1));
      }
      dropped += chosen < 0 ? 1u : 0u;
      if (act && s == chosen) {
        // the clock up to the arrival, then the entry by its tag: after every equal one
        ps_advance(ck, n, cr, ta);
        int32_t svc = (int32_t)(next_work * scale);
        svc = svc < 1 ? 1 : svc;
        const int32_t tag = ck.V + svc;
        const int at = ps_insert(ring, n, make_int2(tag, ta));
        head_tag = at == 0 ? tag : head_tag;
        n += 1;
        assigned += 1;
      }

      // ---- the next arrival, from the draw-ahead slots; refilled by the whole group when they
      //      are used up: lane j draws arrival knext + j
      const uint32_t knext = arr_idx + 1u;
      if (knext - cb >= (uint32_t)G) {  // group-uniform
        const u32x4 d = philox4x32_10(u32x4{knext + (uint32_t)s, gid, episode, kStreamArrival << 24},
                                      p.key0, p.key1);
        int32_t gap;
        float wk;
        if (ws.tab != nullptr) {  // wave-uniform: the handle's workload tables
          table_arrival(ws, d.x, d.y, mean_gap, gap, wk);
        } else {
          gap = (int32_t)(-lb_logf(u01_open0(d.x)) * mean_gap);
          wk = -lb_logf(u01_open0(d.y));
        }
        __builtin_amdgcn_wave_barrier();  // (the slots' last reads are done)
        acache[lane] = make_int4(gap, __float_as_int(wk), (int)d.z, (int)d.w);
        __builtin_amdgcn_wave_barrier();
        cb = knext;
      }
      const int4 nx = acache[gbase + (int)(knext - cb)];
      arr_idx = knext;
      next_arr = ta + nx.x;
      next_work = __int_as_float(nx.y);
      u2 = (uint32_t)nx.z;
      u3 = (uint32_t)nx.w;
    }

    // ---- step end: every clock up to dt, then the rebase to the next step's start: the stored
    //      tags become the remaining service, V = 0; the carry stays
    next_arr -= dt;
    if (act) {
      ps_advance(ck, n, cr, dt);
      head_tag -= ck.V;
      ps_rebase(ring, n, ck, dt);
    }
    clock += 1u;
  };

  if constexpr (MODE == kModeReset) {
    for (int k = 0; k < p.warmup_steps; ++k) sim_step();
  } else {
    sim_step();
  }

  // ---- back to HBM: the server's words (the ring's entries are where they belong), the env's
  if (act) {
    st.hc[sb] = (uint32_t)ring.head | (big ? kHcBig : 0u) | ((uint32_t)n << 16);
    st.last_tc[sb] = ck.acc;
    st.res_count[sb] = rcnt;
    *reinterpret_cast<uint4*>(st.chg + (size_t)sb * 4) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
    if (fs_on) {
      fs.count[sb] = fs_cnt;
      fs.max_us[sb] = fs_max;
      fs.sum[sb] = fs_sum;
    }
    // (a reset's warm-up assignments are not a step's)
    if (MODE != kModeReset && assign_out != nullptr) assign_out[sb] = assigned;
  }
  if (s == 0) {
    st.episode[b] = episode;
    st.clock[b] = clock;
    st.dropped[b] = dropped;
    st.arr_idx[b] = arr_idx;
    st.next_arr[b] = next_arr;
    st.next_work[b] = next_work;
    st.next_u2[b] = u2;
    st.next_u3[b] = u3;
    if (MODE == kModeReset) {
      st.ep_step[b] = 0;
      st.ep_return[b] = 0.0;
    }
  }
}

void launch_ps_t(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                 const uint8_t* mask, const int32_t* cores, hipStream_t stream) {
  const DynPlan& d = MODE == kModeReset ? L.plan.reset_dyn : L.plan.dyn;
  const dim3 grid(d.grid), block(d.block);
  pick<2, 4, 8, 16, 32, 64>(d.width, [&](auto GG) { pick<0, 1, 2, 3>(L.prm.policy, [&](auto P) {
    LBSIM_LAUNCH((dynamics_ps_kernel<decltype(GG)::value, MODE, decltype(P)::value>), grid, block,
                 0, stream, L.st, L.prm, action, dtype, assign, mask, L.flow, cores);
  }); });
}

}  // namespace

#if LBSIM_DYN_MODE == 0
void launch_dynamics_ps_step(const LaunchCtx& L, const void* action, int dtype, int32_t* assign,
                             const int32_t* cores, hipStream_t s) {
  launch_ps_t(L, action, dtype, assign, nullptr, cores, s);
}
#else
void launch_dynamics_ps_reset(const LaunchCtx& L, const uint8_t* mask, const int32_t* cores,
                              hipStream_t s) {
  launch_ps_t(L, nullptr, 0, nullptr, mask, cores, s);
}
#endif

}  // namespace lbk
