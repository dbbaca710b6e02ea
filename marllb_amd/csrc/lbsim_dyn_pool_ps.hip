// lbsim_dyn_pool_ps.hip -- the dynamics of a handle whose shared server pools have
// processor-sharing servers: dynamics_pool_ps_kernel, one group of G lanes per
// pool of A balancers in front of S physical PS servers of c cores each, one object per mode:
// built with -DLBSIM_DYN_MODE=0 (kModeStep, launch_dynamics_pool_ps_step) and =1 (kModeReset,
// launch_dynamics_pool_ps_reset; this object also holds the small kernel of lbsim_pool_ps_state).
// Objects of their own, as lbsim_dyn_pool.hip's and lbsim_dyn_ps.hip's are: no other kernel gains
// code.
//
// The skeleton is dynamics_pool_kernel's: lane s of a group owns physical server s, lane a also
// carries member a's arrival words; what a lane keeps per member -- n_own[a][s], the reservoir
// count of (member a, server s), member a's weight for s, its assignments -- are LDS words
// [a][lane] beside the members' draw-ahead slots; the pool's next arrival is a group-min over
// (time, member).  The server is dynamics_ps_kernel's: the clock words V, acc, t_last, the count n,
// the head entry's tag and the cores c in the owning lane's registers, the entries {tag, ta, owner}
// sorted by tag in the first member's HBM ring rows with their owners in PoolArrays::owner
// (lbsim_ps.h's rule over PoolPsRing).  Every lane completes its own server's flows due by the
// pool's next arrival, each sample into its owner's reservoir through the LDS count row and drawn
// from the owner's reservoir stream; then the group assigns that arrival by its owner's weights and
// own counts against the physical n < Q, and the chosen lane advances its clock to the arrival and
// inserts the entry by its tag.  The cores travel as a kernel argument (a null pointer: one each).
#include "lbsim_internal.h"
#include "lbsim_dyn_group.h"
#include "lbsim_pool.h"
#include "lbsim_ps.h"
#include "lbsim_truth.h"

#if !defined(LBSIM_DYN_MODE) || (LBSIM_DYN_MODE != 0 && LBSIM_DYN_MODE != 1)
#error "build with -DLBSIM_DYN_MODE=0 (step) or 1 (reset)"
#endif

namespace lbk {
namespace {

constexpr int MODE = LBSIM_DYN_MODE == 0 ? kModeStep : kModeReset;

// An entry of a PS pool's server: .x the tag, .y t_arrival (lbsim_ps.h reads these two), .o the
// member that forwarded the flow.
struct PoolPsEntry {
  int32_t x, y, o;
};

// A server's ring row in HBM by queue position (lbsim_ps.h's accessor), the owner bytes beside it.
// An owner byte is clamped below A: it indexes LDS rows (only lbsim_set_state could load another).
struct PoolPsRing {
  int2* ring;
  uint8_t* own;
  int head, Q, A;
  __device__ __forceinline__ PoolPsEntry get(int pos) const {
    const uint32_t i = (uint32_t)ps_ring_index(head, pos, Q);
    const int2 e = ring[i];
    const int o = (int)own[i];
    return PoolPsEntry{e.x, e.y, o < A ? o : 0};
  }
  __device__ __forceinline__ void set(int pos, const PoolPsEntry& e) const {
    const uint32_t i = (uint32_t)ps_ring_index(head, pos, Q);
    ring[i] = make_int2(e.x, e.y);
    own[i] = (uint8_t)e.o;
  }
};

// Dynamic LDS of one wave, rows [member][lane]: A * (16 + 4 * 4) * 64 bytes (dynamics_pool_kernel's).
__host__ __device__ constexpr unsigned pool_ps_lds_bytes(int A) { return (unsigned)A * 64u * 32u; }

template <int G, int MODE, int POLICY>
__global__ void __launch_bounds__(64)
    dynamics_pool_ps_kernel(DevState st, SimParams p, PoolArrays pa, const void* action,
                            int action_dtype, int32_t* assign_out, const uint8_t* reset_mask,
                            const int32_t* cores) {
  static_assert(G == 2 || G == 4 || G == 8 || G == 16, "a pool's group is one DPP row at most");
  static_assert(POLICY >= 0 && POLICY <= 3, "SED, SED2, LSQ, LSQ2");
  constexpr bool two_choice = (POLICY == 1 || POLICY == 3);
  constexpr bool lsq = (POLICY == 2 || POLICY == 3);
  extern __shared__ __align__(16) unsigned char pool_ps_smem[];
  const int A = pa.A;
  int4* const acache = reinterpret_cast<int4*>(pool_ps_smem);          // draw-ahead slots
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
  // (the mask of a reset is already widened to whole pools, launch_pool_mask)
  if (MODE == kModeReset && reset_mask != nullptr && reset_mask[b0] == 0) return;

  // ---- member a's words, in lane a
  const uint32_t bm = b0 + (uint32_t)(mem ? s : 0);
  const uint32_t gid0 = p.env_id_offset + b0;
  const float mean_gap = env_mean_gap(st, p, bm);
  int32_t m_next = 0x7FFFFFFF;  // (a lane without a member never holds the minimum)
  float m_work = 0.0f;
  uint32_t m_u2 = 0u, m_u3 = 0u, m_idx = 0u, m_drop = 0u;
  uint32_t episode, clock;

  // ---- server s, in lane s: the physical PS server; the per-member words are LDS rows
  const uint32_t ps = c * (uint32_t)S + (uint32_t)(act ? s : 0);  // the (pool, server) row
  PoolPsRing ring{st.ring + ((size_t)b0 * (uint32_t)S + (uint32_t)(act ? s : 0)) * (size_t)Q,
                  pa.owner + (size_t)ps * (size_t)Q, 0, Q, A};
  auto row = [&](int a) -> uint32_t {  // member a's (env, server) row
    return (b0 + (uint32_t)a) * (uint32_t)S + (uint32_t)(act ? s : 0);
  };
  PsClock ck{0, 0, 0};
  int32_t n = 0, head_tag = 0;
  uint32_t big = 0u;  // bit a: member a's sticky kHcBig flag for this server
  // the server's cores (§3.23; nullptr, wave-uniform: every server has one)
  int32_t cr = 1;
  if (cores != nullptr) cr = cores[ps];
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
      // (own counts that lbsim_set_state loaded at odds with the owners of the physical entries
      // can fall below 0 at a completion: the word written back is then garbage in its count
      // bits, as on a FIFO pool; the count indexes nothing)
      nown[a * 64 + lane] = act ? (int32_t)(hc >> 16) : 0;
      big |= (act && (hc & kHcBig) != 0u) ? 1u << a : 0u;
      rcnt[a * 64 + lane] = act ? st.res_count[row(a)] : 0u;
      wgt[a * 64 + lane] = act ? action_weight_sel(p, action, action_dtype, (size_t)row(a)) : 1.0f;
      asg[a * 64 + lane] = 0;
      if (act) *reinterpret_cast<uint4*>(st.chg + (size_t)row(a) * 4) = make_uint4(0u, 0u, 0u, 0u);
    }
    if (act) {
      const uint32_t phc = pa.hc[ps];
      const int head = (int)(phc & kHcHead), cnt = (int)(phc >> 16);
      // (only lbsim_set_state could load words outside the ring)
      ring.head = head < Q ? head : 0;
      n = cnt <= Q ? cnt : Q;
      // the carry lives in the last_tc word of every member's row of this server: in [0, n)
      const int32_t w = st.last_tc[row(0)];
      ck.acc = (n > 0 && w > 0 && w < n) ? w : 0;
      if (n > 0) head_tag = ring.get(0).x;
    }
  }
  // the member's draw-ahead slots hold arrivals [m_cb, m_cb + G): none yet
  uint32_t m_cb = m_idx + 1u + 0x80000000u;

  // ---- one step of the pool (a reset runs warmup_steps of them at weights 1.0)
  auto sim_step = [&]() {
    const uint64_t base_us = (uint64_t)clock * (uint64_t)dt;
    const uint32_t base_ms = (uint32_t)(base_us / 1000u);
    const uint32_t base_rem = (uint32_t)(base_us - (uint64_t)base_ms * 1000u);

    for (;;) {
      // the pool's next arrival: the smallest time over the members, ties to the lowest member
      const int32_t tmin = group_min_i32<G>(m_next);
      const int owner = group_min_i32<G>((mem && m_next == tmin) ? s : 0xFF);
      const bool arrival_due = tmin < dt;  // the same in every lane of the group
      const int32_t th = arrival_due ? tmin : dt;
      // ---- this server's completions due no later than it, each at its own time: the clock
      //      reaches the head's tag, the head leaves, its sample goes into its owner's reservoir,
      //      drawn from the owner's reservoir stream at the owner's count
      while (act && n > 0) {
        const PsDue due = ps_next_completion(ck, n, cr, head_tag);
        const int32_t tc = due.tc;
        if (tc > th) break;
        ps_complete(ck, due, head_tag);
        const PoolPsEntry e = ring.get(0);
        ring.head = ring.head + 1 == Q ? 0 : ring.head + 1;
        n -= 1;
        if (n > 0) head_tag = ring.get(0).x;
        const int a = e.o;
        const uint32_t fct = (uint32_t)(tc - e.y);
        const uint32_t rc = rcnt[a * 64 + lane];
        int slot = (int)rc;
        if (rc >= (uint32_t)K) {
          const u32x4 d = philox4x32_10(u32x4{rc >> 1, gid0 + (uint32_t)a, episode,
                                              (kStreamReservoir << 24) | (uint32_t)s},
                                        p.key0, p.key1);
          slot = reservoir_slot(rc, d);
        }
        if (slot >= 0) {
          big |= big_record(fct, fct) ? 1u << a : 0u;
          st.res[(size_t)row(a) * K + (uint32_t)slot] =
              make_uint2(fct, base_ms + (base_rem + (uint32_t)tc) / 1000u);
          mark(a, slot);
        }
        rcnt[a * 64 + lane] = count_inc(rc);
        nown[a * 64 + lane] -= 1;
      }
      if (!arrival_due) break;  // group-uniform

      // ---- member `owner`'s arrival: its words from its lane, its weights and own counts
      const int ol = gbase + owner;
      const int32_t ta = tmin;
      const float work = __shfl(m_work, ol, 64);
      const uint32_t u2 = (uint32_t)__shfl((int)m_u2, ol, 64);
      float score = 0.0f;
      if (act) {
        const int32_t no = nown[owner * 64 + lane];
        if constexpr (lsq) score = (float)no;
        else score = (float)((double)(no + 1) / ((double)wgt[owner * 64 + lane] + 1e-9));
      }
      const bool elig = act && n < Q;  // the physical queue against Q
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
        // the clock up to the arrival, then the entry by its tag: after every equal one; the
        // entries it moves carry their owners with them
        ps_advance(ck, n, cr, ta);
        const int32_t tag = ck.V + pool_service(work, scale);
        const int at = ps_insert(ring, n, PoolPsEntry{tag, ta, owner});
        head_tag = at == 0 ? tag : head_tag;
        n += 1;
        nown[owner * 64 + lane] += 1;
        asg[owner * 64 + lane] += 1;
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
        __builtin_amdgcn_wave_barrier();  // (the slots' last reads are done)
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

    // ---- step end: every clock up to dt, then the rebase to the next step's start: the stored
    //      tags become the remaining service, V = 0; the carry and the owners stay
    if (mem) m_next -= dt;
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

  // ---- back to HBM: the physical server's word, every member's row of this server, the members
  if (act) {
    pa.hc[ps] = (uint32_t)ring.head | ((uint32_t)n << 16);
    for (int a = 0; a < A; ++a) {
      const uint32_t r = row(a);
      // the member's word: the physical head, its own flag and its own count (observation column 0)
      st.hc[r] = (uint32_t)ring.head | (((big >> a) & 1u) ? kHcBig : 0u) |
                 ((uint32_t)nown[a * 64 + lane] << 16);
      st.last_tc[r] = ck.acc;
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

void launch_pool_ps_t(const LaunchCtx& L, const PoolArrays& pa, const void* action, int dtype,
                      int32_t* assign, const uint8_t* mask, const int32_t* cores,
                      hipStream_t stream) {
  const DynPlan& d = MODE == kModeReset ? L.plan.reset_dyn : L.plan.dyn;
  const dim3 grid(d.grid), block(d.block);
  const unsigned lds = pool_ps_lds_bytes(pa.A);
  pick<2, 4, 8, 16>(d.width, [&](auto GG) { pick<0, 1, 2, 3>(L.prm.policy, [&](auto P) {
    LBSIM_LAUNCH((dynamics_pool_ps_kernel<decltype(GG)::value, MODE, decltype(P)::value>), grid,
                 block, lds, stream, L.st, L.prm, pa, action, dtype, assign, mask, cores);
  }); });
}

#if LBSIM_DYN_MODE == 1
struct PoolPsStateArgs {
  const uint32_t* hc;       // the members' words: their own counts
  const uint32_t* pool_hc;  // the physical servers' words
  const int2* ring;
  const int32_t* acc;       // the last_tc words
  const int32_t* cores;     // [C, S]; nullptr: one core each
  int32_t B, S, Q, A;
};

struct PoolPsStateRing {  // (lbsim_ps.h's accessor, read-only; the index stays inside the ring)
  const int2* ring;
  int head, Q;
  __device__ __forceinline__ int2 get(int pos) const {
    const uint32_t r = (uint32_t)ps_ring_index(head, pos, Q);
    return ring[r < (uint32_t)Q ? r : (uint32_t)Q - 1u];
  }
};

// lbsim_pool_ps_state, one lane per (env, server) as ps_state_kernel: the physical server's row
// in every member's, column 1 the flows the member did not forward itself.  n, head and acc are
// read as the dynamics prologue reads them.
__global__ void __launch_bounds__(256) pool_ps_state_kernel(PoolPsStateArgs a, float* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.S) return;
  const int64_t b = i / a.S;
  const int s = (int)(i - b * a.S);
  const int64_t c = pool_of(b, a.A);
  const uint32_t phc = a.pool_hc[c * a.S + s];
  const int head = truth_head(phc), cnt = truth_count(phc);
  const int n = cnt <= a.Q ? cnt : a.Q;
  const int32_t cr = a.cores != nullptr ? a.cores[c * a.S + s] : 1;
  const int32_t w = a.acc[i];
  const int32_t acc = (n > 0 && w > 0 && w < n) ? w : 0;
  const PoolPsStateRing q{a.ring + (size_t)(pool_env(c, a.A, 0) * a.S + s) * (size_t)a.Q,
                          head < a.Q ? head : 0, a.Q};
  int32_t work = 0, drain = 0;
  ps_server_state(q, n, cr, acc, work, drain);
  float* const o = out + 5 * i;
  o[0] = (float)n;
  o[1] = (float)pool_hidden(n, truth_count(a.hc[i]));
  o[2] = (float)(n < cr ? n : cr);
  o[3] = truth_seconds(work);
  o[4] = truth_seconds(drain);
}
#endif

}  // namespace

#if LBSIM_DYN_MODE == 0
void launch_dynamics_pool_ps_step(const LaunchCtx& L, const PoolArrays& pa, const void* action,
                                  int dtype, int32_t* assign, const int32_t* cores, hipStream_t s) {
  launch_pool_ps_t(L, pa, action, dtype, assign, nullptr, cores, s);
}
#else
void launch_dynamics_pool_ps_reset(const LaunchCtx& L, const PoolArrays& pa, const uint8_t* mask,
                                   const int32_t* cores, hipStream_t s) {
  launch_pool_ps_t(L, pa, nullptr, 0, nullptr, mask, cores, s);
}
void launch_pool_ps_state(const LaunchCtx& L, const PoolArrays& pa, const int32_t* cores,
                          float* out, hipStream_t s) {
  PoolPsStateArgs a{};
  a.hc = L.st.hc;
  a.pool_hc = pa.hc;
  a.ring = L.st.ring;
  a.acc = L.st.last_tc;
  a.cores = cores;
  a.B = L.prm.B, a.S = L.prm.S, a.Q = L.prm.Q, a.A = pa.A;
  const size_t n = (size_t)a.B * (size_t)a.S;
  hipLaunchKernelGGL(pool_ps_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a,
                     out);
}
#endif

}  // namespace lbk
