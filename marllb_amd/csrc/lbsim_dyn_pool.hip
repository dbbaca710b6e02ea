// lbsim_dyn_pool.hip -- the dynamics of a handle with shared server pools:
// dynamics_pool_kernel, one group of G lanes per pool of A balancers in front of S physical FIFO
// servers, one object per mode: built with -DLBSIM_DYN_MODE=0 (kModeStep,
// launch_dynamics_pool_step) and =1 (kModeReset, launch_dynamics_pool_reset; this object also
// holds the two small kernels of a pool handle, the reset mask widened to whole pools and the
// ground truth of the physical servers).  Objects of their own, as lbsim_dyn_delay.hip's are: no
// other kernel gains code.
//
// Lane s of a group owns physical server s (its FIFO word, head entry and tail in registers, the
// entries in the first member's HBM ring rows, their owners in PoolArrays::owner); lane a also
// carries member a's arrival words.  What a lane keeps per member -- n_own[a][s], the reservoir
// count of (member a, server s), member a's weight for s, its assignments -- are LDS words
// [a][lane], A * 2 KiB of dynamic LDS per wave with the members' draw-ahead slots.  One event loop
// per pool: every lane pops its own server's completions due by the pool's next arrival (a
// group-min over (time, member)), then the group assigns that arrival by its owner's weights and
// own counts, against the physical queue lengths.  A member's arrivals are drawn G at a time, lane
// j drawing the owner's arrival k + j, as dynamics_group_kernel draws its env's.
#include "lbsim_internal.h"
#include "lbsim_dyn_group.h"
#include "lbsim_pool.h"
#include "lbsim_truth.h"

#if !defined(LBSIM_DYN_MODE) || (LBSIM_DYN_MODE != 0 && LBSIM_DYN_MODE != 1)
#error "build with -DLBSIM_DYN_MODE=0 (step) or 1 (reset)"
#endif

namespace lbk {
namespace {

constexpr int MODE = LBSIM_DYN_MODE == 0 ? kModeStep : kModeReset;

// A server's ring slots in HBM (lbsim_pool.h's accessor).  An owner byte is clamped below A: it
// indexes LDS rows (only lbsim_set_state could load another).
struct PoolRing {
  int2* ring;
  uint8_t* own;
  int A;
  __device__ __forceinline__ int2 entry(int i) const { return ring[(uint32_t)i]; }
  __device__ __forceinline__ int owner(int i) const {
    const int o = (int)own[(uint32_t)i];
    return o < A ? o : 0;
  }
  __device__ __forceinline__ void put(int i, int32_t tc, int32_t ta, int o) const {
    ring[(uint32_t)i] = make_int2(tc, ta);
    own[(uint32_t)i] = (uint8_t)o;
  }
};

// Dynamic LDS of one wave, rows [member][lane]: A * (16 + 4 * 4) * 64 bytes.
__host__ __device__ constexpr unsigned pool_lds_bytes(int A) { return (unsigned)A * 64u * 32u; }

template <int G, int MODE, int POLICY>
__global__ void __launch_bounds__(64)
    dynamics_pool_kernel(DevState st, SimParams p, PoolArrays pa, const void* action,
                         int action_dtype, int32_t* assign_out, const uint8_t* reset_mask) {
  static_assert(G == 2 || G == 4 || G == 8 || G == 16, "a pool's group is one DPP row at most");
  static_assert(POLICY >= 0 && POLICY <= 3, "SED, SED2, LSQ, LSQ2");
  constexpr bool two_choice = (POLICY == 1 || POLICY == 3);
  constexpr bool lsq = (POLICY == 2 || POLICY == 3);
  extern __shared__ __align__(16) unsigned char pool_smem[];
  const int A = pa.A;
  int4* const acache = reinterpret_cast<int4*>(pool_smem);             // draw-ahead slots
  int32_t* const nown = reinterpret_cast<int32_t*>(acache + A * 64);   // own flows in flight
  uint32_t* const rcnt = reinterpret_cast<uint32_t*>(nown + A * 64);   // reservoir counts
  float* const wgt = reinterpret_cast<float*>(rcnt + A * 64);          // the members' weights
  int32_t* const asg = reinterpret_cast<int32_t*>(wgt + A * 64);       // assignments this launch

  const int lane = (int)threadIdx.x;
  const int s = lane & (G - 1);
  const int gbase = lane & ~(G - 1);
  const int S = p.S, Q = p.Q;
  const int32_t dt = p.dt_us;
  const uint32_t C = (uint32_t)p.B / (uint32_t)A;
  const uint32_t c = blockIdx.x * (uint32_t)(64 / G) + (uint32_t)(lane / G);
  if (c >= C) return;  // whole groups leave together
  const uint32_t b0 = c * (uint32_t)A;  // the pool's first member
  const bool mem = s < A, act = s < S;
  // (the mask of a reset is already widened to whole pools, launch_pool_mask: every member's byte
  // says whether the pool resets)
  if (MODE == kModeReset && reset_mask != nullptr && reset_mask[b0] == 0) return;

  // ---- member a's words, in lane a
  const uint32_t bm = b0 + (uint32_t)(mem ? s : 0);
  const uint32_t gid0 = p.env_id_offset + b0;
  const float mean_gap = env_mean_gap(st, p, bm);
  int32_t m_next = 0x7FFFFFFF;  // (a lane without a member never holds the minimum)
  float m_work = 0.0f;
  uint32_t m_u2 = 0u, m_u3 = 0u, m_idx = 0u, m_drop = 0u;
  uint32_t episode, clock;

  // ---- server s, in lane s: the physical FIFO; the per-member words are LDS rows
  const uint32_t ps = c * (uint32_t)S + (uint32_t)(act ? s : 0);  // the (pool, server) row
  const PoolRing ring{st.ring + ((size_t)b0 * (uint32_t)S + (uint32_t)(act ? s : 0)) * (size_t)Q,
                      pa.owner + (size_t)ps * (size_t)Q, A};
  auto row = [&](int a) -> uint32_t {  // member a's (env, server) row
    return (b0 + (uint32_t)a) * (uint32_t)S + (uint32_t)(act ? s : 0);
  };
  PoolFifo F{0, 0, 0, 0, 0};
  int32_t last = kLastNone;
  uint32_t big = 0u;  // bit a: member a's sticky kHcBig flag for this server
  float scale = p.svc_scale[0];
#pragma unroll
  for (int k = 1; k < G; ++k) scale = (k == s) ? p.svc_scale[k] : scale;
  // (a handle with per-env arrival rates holds the config's server rates in its per-env array)
  if (st.env_scale != nullptr) scale = st.env_scale[(size_t)b0 * (uint32_t)S + (uint32_t)(act ? s : 0)];

  auto mark = [&](int a, int slot) {  // the slot's bit in (member a, server s)'s written-slot mask:
    // a plain read-modify-write, the lane owns the row for the whole launch
    if (act) st.chg[(size_t)row(a) * 4 + ((uint32_t)slot >> 5)] |= 1u << (slot & 31);
  };

  if constexpr (MODE == kModeReset) {
    // a new episode for every member: its first arrival, empty servers, weights 1.0
    episode = st.episode[b0] + 1u;
    clock = 0u;
    if (mem) {
      const u32x4 d = philox4x32_10(u32x4{0u, gid0 + (uint32_t)s, episode, kStreamArrival << 24},
                                    p.key0, p.key1);
      arrival_from_draw(mean_gap, d, 0, m_next, m_work, m_u2, m_u3);
    }
    for (int a = 0; a < A; ++a) {
      nown[a * 64 + lane] = 0;
      rcnt[a * 64 + lane] = 0u;
      wgt[a * 64 + lane] = 1.0f;
      asg[a * 64 + lane] = 0;
      // emptied reservoirs: slot 0 marked written, so the next observe recomputes the row
      if (act) *reinterpret_cast<uint4*>(st.chg + (size_t)row(a) * 4) = make_uint4(1u, 0u, 0u, 0u);
    }
  } else {
    episode = st.episode[b0];
    clock = st.clock[b0];
    if (mem) {
      m_next = st.next_arr[bm];
      m_work = st.next_work[bm];
      m_u2 = st.next_u2[bm];
      m_u3 = st.next_u3[bm];
      m_idx = st.arr_idx[bm];
      m_drop = st.dropped[bm];
    }
    for (int a = 0; a < A; ++a) {
      const uint32_t hc = st.hc[row(a)];
      nown[a * 64 + lane] = act ? (int32_t)(hc >> 16) : 0;
      big |= (act && (hc & kHcBig) != 0u) ? 1u << a : 0u;
      rcnt[a * 64 + lane] = act ? st.res_count[row(a)] : 0u;
      wgt[a * 64 + lane] = act ? action_weight_sel(p, action, action_dtype, (size_t)row(a)) : 1.0f;
      asg[a * 64 + lane] = 0;
      if (act) *reinterpret_cast<uint4*>(st.chg + (size_t)row(a) * 4) = make_uint4(0u, 0u, 0u, 0u);
    }
    if (act) {
      F = pool_fifo_load(pa.hc[ps], ring, Q);
      last = st.last_tc[row(0)];
    }
  }
  // the member's draw-ahead slots hold arrivals [m_cb, m_cb + G): none yet
  uint32_t m_cb = m_idx + 1u + 0x80000000u;

  // ---- one step of the pool (a reset runs warmup_steps of them at weights 1.0)
  auto sim_step = [&]() {
    const uint64_t base_us = (uint64_t)clock * (uint64_t)dt;
    const uint32_t base_ms = (uint32_t)(base_us / 1000u);
    const uint32_t base_rem = (uint32_t)(base_us - (uint64_t)base_ms * 1000u);

    // 1. this lane's carried-in flows that complete in this step: samples in FIFO order, each into
    //    its owner's reservoir (§3.4: slot = count below K, else the owner's reservoir stream)
    if (act && pool_due(F, dt)) {
      int pos = F.head;
      for (int i = 0; i < F.cnt; ++i) {
        const int2 e = ring.entry(pos);
        if (e.x > dt) break;
        const int a = ring.owner(pos);
        const uint32_t rc = rcnt[a * 64 + lane];
        int slot = (int)rc;
        if (rc >= (uint32_t)K) {
          const u32x4 d = philox4x32_10(u32x4{rc >> 1, gid0 + (uint32_t)a, episode,
                                              (kStreamReservoir << 24) | (uint32_t)s},
                                        p.key0, p.key1);
          slot = reservoir_slot(rc, d);
        }
        if (slot >= 0) {
          const uint32_t fct = (uint32_t)(e.x - e.y);
          big |= big_record(fct, fct) ? 1u << a : 0u;
          st.res[(size_t)row(a) * K + (uint32_t)slot] =
              make_uint2(fct, base_ms + (base_rem + (uint32_t)e.x) / 1000u);
          mark(a, slot);
        }
        rcnt[a * 64 + lane] = count_inc(rc);
        pos = pool_ring_next(pos, Q);
      }
    }

    // 2. the event loop
    for (;;) {
      // the pool's next arrival: the smallest time over the members, ties to the lowest member
      const int32_t tmin = group_min_i32<G>(m_next);
      const int owner = group_min_i32<G>((mem && m_next == tmin) ? s : 0xFF);
      const bool arrival_due = tmin < dt;  // the same in every lane of the group
      const int32_t th = arrival_due ? tmin : dt;
      // completions due no later than it go first: every lane its own server's, each one out of its
      // owner's count (servers do not interact, so their order among servers leaves no trace)
      while (act && pool_due(F, th)) {
        last = F.head_tc;
        const int a = pool_pop(F, ring, Q);
        nown[a * 64 + lane] -= 1;
      }
      if (!arrival_due) break;  // group-uniform

      // ---- member `owner`'s arrival: its words from its lane, its weights and own counts
      const int ol = gbase + owner;
      const int32_t ta = tmin;
      const float work = __shfl(m_work, ol, 64);
      const uint32_t u2 = (uint32_t)__shfl((int)m_u2, ol, 64);
      const uint32_t u3 = (uint32_t)__shfl((int)m_u3, ol, 64);
      float score = 0.0f;
      if (act) {
        const int32_t n = nown[owner * 64 + lane];
        if constexpr (lsq) score = (float)n;
        else score = (float)((double)(n + 1) / ((double)wgt[owner * 64 + lane] + 1e-9));
      }
      const bool elig = act && pool_eligible(F, Q);  // the physical queue against Q
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
      if (s == owner) m_drop += chosen < 0 ? 1u : 0u;  // no eligible server: the member's drop
      if (act && s == chosen) {
        const int32_t tc = pool_push(F, ring, Q, ta, pool_service(work, scale), owner);
        nown[owner * 64 + lane] += 1;
        asg[owner * 64 + lane] += 1;
        if (tc <= dt) {  // completes in this step: its sample now, drawn by its arrival's word r
          const uint32_t rc = rcnt[owner * 64 + lane];
          const int slot = reservoir_slot_r32(rc, u3);
          if (slot >= 0) {
            st.res[(size_t)row(owner) * K + (uint32_t)slot] =
                make_uint2((uint32_t)(tc - ta), base_ms + (base_rem + (uint32_t)tc) / 1000u);
            mark(owner, slot);
          }
          rcnt[owner * 64 + lane] = count_inc(rc);
        }
      }

      // ---- the owner's next arrival, from its draw-ahead slots; refilled by the whole group when
      //      they are used up: lane j draws the owner's arrival knext + j
      const uint32_t knext = (uint32_t)__shfl((int)m_idx, ol, 64) + 1u;
      uint32_t cb = (uint32_t)__shfl((int)m_cb, ol, 64);
      if (knext - cb >= (uint32_t)G) {  // group-uniform
        const float ogap = __shfl(mean_gap, ol, 64);
        const u32x4 d = philox4x32_10(u32x4{knext + (uint32_t)s, gid0 + (uint32_t)owner, episode,
                                            kStreamArrival << 24},
                                      p.key0, p.key1);
        const int32_t gap = (int32_t)(-lb_logf(u01_open0(d.x)) * ogap);
        const float wk = -lb_logf(u01_open0(d.y));
        acache[owner * 64 + lane] = make_int4(gap, __float_as_int(wk), (int)d.z, (int)d.w);
        __builtin_amdgcn_wave_barrier();
        cb = knext;
      }
      const int4 nx = acache[owner * 64 + gbase + (int)(knext - cb)];
      if (s == owner) {
        m_idx = knext;
        m_cb = cb;
        m_next = ta + nx.x;
        m_work = __int_as_float(nx.y);
        m_u2 = (uint32_t)nx.z;
        m_u3 = (uint32_t)nx.w;
      }
    }

    // ---- rebase to the next step's start
    if (mem) m_next -= dt;
    if (act) {
      int pos = F.head;
      for (int i = 0; i < F.cnt; ++i) {
        int2 e = ring.ring[(uint32_t)pos];
        e.x -= dt;
        e.y -= dt;
        ring.ring[(uint32_t)pos] = e;
        pos = pool_ring_next(pos, Q);
      }
      F.head_tc -= dt;
      F.tail -= dt;
      last = (last < kLastNone + dt) ? kLastNone : last - dt;
    }
    clock += 1u;
  };

  if constexpr (MODE == kModeReset) {
    for (int k = 0; k < p.warmup_steps; ++k) sim_step();
  } else {
    sim_step();
  }

  // ---- back to HBM: the physical FIFO's word, every member's row of this server, the members
  if (act) {
    pa.hc[ps] = pool_hc_word(F);
    if (p.big_in_step) {  // the in-step records this launch wrote (big_written)
      __builtin_amdgcn_s_waitcnt(0);
      __asm__ volatile("" ::: "memory");
      for (int a = 0; a < A; ++a) {
        const uint4 m = *reinterpret_cast<const uint4*>(st.chg + (size_t)row(a) * 4);
        const uint32_t cw[4] = {m.x, m.y, m.z, m.w};
        big |= big_written(st, row(a), cw, rcnt[a * 64 + lane]) ? 1u << a : 0u;
      }
    }
    for (int a = 0; a < A; ++a) {
      const uint32_t r = row(a);
      // the member's word: the physical head, its own flag and its own count (observation column 0)
      st.hc[r] = (uint32_t)F.head | (((big >> a) & 1u) ? kHcBig : 0u) |
                 ((uint32_t)nown[a * 64 + lane] << 16);
      st.last_tc[r] = last;
      st.res_count[r] = rcnt[a * 64 + lane];
      // (a reset's warm-up assignments are not a step's)
      if (MODE != kModeReset && assign_out != nullptr) assign_out[r] = asg[a * 64 + lane];
    }
  }
  if (mem) {
    st.episode[bm] = episode;
    st.clock[bm] = clock;
    st.dropped[bm] = m_drop;
    st.arr_idx[bm] = m_idx;
    st.next_arr[bm] = m_next;
    st.next_work[bm] = m_work;
    st.next_u2[bm] = m_u2;
    st.next_u3[bm] = m_u3;
    if (MODE == kModeReset) {
      st.ep_step[bm] = 0;
      st.ep_return[bm] = 0.0;
    }
  }
}

void launch_pool_t(const LaunchCtx& L, const PoolArrays& pa, const void* action, int dtype,
                   int32_t* assign, const uint8_t* mask, hipStream_t stream) {
  const DynPlan& d = MODE == kModeReset ? L.plan.reset_dyn : L.plan.dyn;
  const dim3 grid(d.grid), block(d.block);
  const unsigned lds = pool_lds_bytes(pa.A);
  pick<2, 4, 8, 16>(d.width, [&](auto GG) { pick<0, 1, 2, 3>(L.prm.policy, [&](auto P) {
    LBSIM_LAUNCH((dynamics_pool_kernel<decltype(GG)::value, MODE, decltype(P)::value>), grid,
                 block, lds, stream, L.st, L.prm, pa, action, dtype, assign, mask);
  }); });
}

#if LBSIM_DYN_MODE == 1
// out[b] = whether any member of b's pool has its byte set.
__global__ void __launch_bounds__(256)
    pool_mask_kernel(const uint8_t* mask, uint8_t* out, int B, int A) {
  const int b = (int)(blockIdx.x * 256u + threadIdx.x);
  if (b >= B) return;
  const int b0 = b - b % A;
  uint8_t any = 0;
  for (int a = 0; a < A; ++a) any |= mask[b0 + a];
  out[b] = any != 0 ? 1 : 0;
}

struct PoolTruthArgs {
  const uint32_t* hc;       // the members' words: their own counts
  const uint32_t* pool_hc;  // the physical FIFOs' words
  const int2* ring;
  int32_t B, S, Q, A;
  float mu[kPoolMaxServers];
};

struct PoolTruthRing {  // (lbsim_truth.h's accessor; the index stays inside the ring)
  const int2* ring;
  int head, Q;
  __device__ __forceinline__ int2 get(int pos) const {
    const uint32_t r = (uint32_t)workers_ring_index(head, pos, Q);
    return ring[r < (uint32_t)Q ? r : (uint32_t)Q - 1u];
  }
};

// lbsim_ground_truth on a pool handle, one lane per (env, server): the physical server's row
// (truth_row at c = 1 on the pool's FIFO) with n_hidden = the physical length minus the member's
// own count.
__global__ void __launch_bounds__(256) pool_truth_kernel(PoolTruthArgs a, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.S) return;
  const int64_t b = i / a.S;
  const int s = (int)(i - b * a.S);
  const int64_t c = pool_of(b, a.A);
  uint32_t phc = a.pool_hc[c * a.S + s];
  int n = truth_count(phc), head = truth_head(phc);
  n = n <= a.Q ? n : a.Q;
  head = head < a.Q ? head : 0;
  phc = (uint32_t)head | (uint32_t)n << 16;
  const PoolTruthRing q{a.ring + (size_t)(pool_env(c, a.A, 0) * a.S + s) * (size_t)a.Q, head, a.Q};
  float r[kTruthCols];
  truth_row(q, phc, 1, -pool_hidden(n, truth_count(a.hc[i])), false, a.mu[s], r);
  float4* const o = reinterpret_cast<float4*>(out) + 2 * i;
  o[0] = make_float4(r[0], r[1], r[2], r[3]);
  o[1] = make_float4(r[4], r[5], r[6], r[7]);
}
#endif

}  // namespace

#if LBSIM_DYN_MODE == 0
void launch_dynamics_pool_step(const LaunchCtx& L, const PoolArrays& pa, const void* action,
                               int dtype, int32_t* assign, hipStream_t s) {
  launch_pool_t(L, pa, action, dtype, assign, nullptr, s);
}
#else
void launch_dynamics_pool_reset(const LaunchCtx& L, const PoolArrays& pa, const uint8_t* mask,
                                hipStream_t s) {
  launch_pool_t(L, pa, nullptr, 0, nullptr, mask, s);
}
void launch_pool_mask(const PoolArrays& pa, const uint8_t* mask, int B, hipStream_t s) {
  hipLaunchKernelGGL(pool_mask_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, mask,
                     pa.mask, B, (int)pa.A);
}
void launch_pool_truth(const LaunchCtx& L, const PoolArrays& pa, const float* mu, float* out,
                       hipStream_t s) {
  PoolTruthArgs a{};
  a.hc = L.st.hc;
  a.pool_hc = pa.hc;
  a.ring = L.st.ring;
  a.B = L.prm.B, a.S = L.prm.S, a.Q = L.prm.Q, a.A = pa.A;
  for (int k = 0; k < kPoolMaxServers; ++k) a.mu[k] = k < L.prm.S ? mu[k] : 1.0f;
  const size_t n = (size_t)a.B * (size_t)a.S;
  hipLaunchKernelGGL(pool_truth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, out);
}
#endif

}  // namespace lbk
