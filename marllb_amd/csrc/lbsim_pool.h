// lbsim_pool.h — shared server pools: A consecutive envs of a handle are A
// balancers in front of one physical set of S FIFO servers.  The rule -- which envs form a pool,
// what lbsim_server_pool_enable accepts, the lanes of a pool's group, the pool's next arrival, and
// the physical FIFO of one server whose entries carry their owner -- as plain __host__ __device__
// functions (tests/pool_probe.cpp compiles them as host C++ with no HIP header, on heap arrays of
// exactly Q entries standing for the ring); dynamics_pool_kernel (lbsim_dyn_pool.hip) runs them
// with one lane per server.
//
// A ring accessor R gives a server's Q ring slots by index:  R::entry(i) -> {.x t_complete,
// .y t_arrival},  R::owner(i) -> the member that forwarded the flow,  R::put(i, tc, ta, owner).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LBP_HD __host__ __device__ inline
#else
#define LBP_HD inline
#endif

namespace lbk {

constexpr int kPoolMaxBalancers = 8;  // members of a pool (their per-server counters live in LDS)
constexpr int kPoolMaxServers = 16;   // one DPP row holds a pool's group

// The arrays of a pool handle (null pointers: the handle has no pools): the physical FIFO's word
// per (pool, server), hc[C*S] = ring head | count << 16; the owner of every ring entry,
// owner[C*S*Q] (the entries themselves are the first member's ring rows); A; and mask[B], the
// reset mask of a call widened to whole pools.  An argument of the pool kernels alone, not a part
// of DevState (§3.11).
struct PoolArrays {
  uint32_t* hc;
  uint8_t* owner;
  int32_t A;
  uint8_t* mask;
};

// lbsim_server_pool_enable's argument check: 0 fine, 1 balancers outside [1, kPoolMaxBalancers],
// 2 num_envs no multiple of it, 3 env_id_offset no multiple of it (a pool would straddle a shard).
LBP_HD int pool_enable_check(int64_t num_envs, int64_t env_id_offset, int64_t balancers) {
  if (balancers < 1 || balancers > kPoolMaxBalancers) return 1;
  if (num_envs % balancers != 0) return 2;
  if (env_id_offset % balancers != 0) return 3;
  return 0;
}

// Pool c is envs cA .. cA + A - 1.
LBP_HD int64_t pool_of(int64_t env, int A) { return env / A; }
LBP_HD int64_t pool_env(int64_t pool, int A, int member) { return pool * A + member; }

// Lanes of a pool's group: pow2 >= max(S, A), at least 2; `forced` (LBSIM_DYN_GROUP_LANES) where
// it is 4, 8 or 16 and holds both.
LBP_HD int pool_group_lanes(int S, int A, int forced) {
  const int need = S > A ? S : A;
  if ((forced == 4 || forced == 8 || forced == 16) && forced >= need) return forced;
  int g = 2;
  while (g < need) g <<= 1;
  return g;
}

// The member whose arrival is the pool's next: the smallest time, ties to the lowest member.
LBP_HD int pool_next_member(const int32_t* next_arr, int A) {
  int m = 0;
  for (int a = 1; a < A; ++a) m = next_arr[a] < next_arr[m] ? a : m;
  return m;
}

LBP_HD int pool_ring_next(int i, int Q) { return i + 1 == Q ? 0 : i + 1; }
LBP_HD int pool_ring_index(int head, int pos, int Q) {  // head < Q, pos <= Q
  const int r = head + pos;
  return r >= Q ? r - Q : r;
}

// The physical FIFO of one server as its lane holds it: the ring word's two fields, the head
// entry's completion time and owner (valid while cnt > 0), and the completion time of the last
// queued flow.
struct PoolFifo {
  int32_t head, cnt, head_tc, head_owner, tail;
};

LBP_HD uint32_t pool_hc_word(const PoolFifo& f) { return (uint32_t)f.head | (uint32_t)f.cnt << 16; }
LBP_HD bool pool_eligible(const PoolFifo& f, int Q) { return f.cnt < Q; }  // the PHYSICAL length
LBP_HD bool pool_due(const PoolFifo& f, int32_t t) { return f.cnt > 0 && f.head_tc <= t; }

// The fifo of a ring word: the head entry and the tail's completion time read through r.
template <class R>
LBP_HD PoolFifo pool_fifo_load(uint32_t hc, const R& r, int Q) {
  PoolFifo f;
  f.head = (int32_t)(hc & 0x7FFFu);
  f.cnt = (int32_t)(hc >> 16);
  f.head = f.head < Q ? f.head : 0;    // (only lbsim_set_state could load such a word: no read
  f.cnt = f.cnt <= Q ? f.cnt : Q;      //  outside the ring whatever it holds)
  f.head_tc = 0, f.head_owner = 0, f.tail = 0;
  if (f.cnt > 0) {
    f.head_tc = r.entry(f.head).x;
    f.head_owner = r.owner(f.head);
    f.tail = r.entry(pool_ring_index(f.head, f.cnt - 1, Q)).x;
  }
  return f;
}

// start = max(ta, tc of the last queued flow, whoever owns it); svc = max(1, (int)(work * 1e6/mu)).
LBP_HD int32_t pool_start(const PoolFifo& f, int32_t ta) {
  return f.cnt > 0 && f.tail > ta ? f.tail : ta;
}
LBP_HD int32_t pool_service(float work, float scale) {
  const int32_t v = (int32_t)(work * scale);
  return v < 1 ? 1 : v;
}

// The head leaves (pool_due held): returns its owner; the next entry becomes the head.
template <class R>
LBP_HD int pool_pop(PoolFifo& f, const R& r, int Q) {
  const int own = f.head_owner;
  f.head = pool_ring_next(f.head, Q);
  f.cnt -= 1;
  if (f.cnt > 0) {
    f.head_tc = r.entry(f.head).x;
    f.head_owner = r.owner(f.head);
  }
  return own;
}

// A flow of `owner` arriving at ta joins (pool_eligible held): returns its completion time.
template <class R>
LBP_HD int32_t pool_push(PoolFifo& f, const R& r, int Q, int32_t ta, int32_t svc, int owner) {
  const int32_t tc = pool_start(f, ta) + svc;
  r.put(pool_ring_index(f.head, f.cnt, Q), tc, ta, owner);
  if (f.cnt == 0) {
    f.head_tc = tc;
    f.head_owner = owner;
  }
  f.tail = tc;
  f.cnt += 1;
  return tc;
}

// lbsim_ground_truth on a pool handle: what the other balancers put on a server.
LBP_HD int32_t pool_hidden(int32_t physical, int32_t own) { return physical - own; }

}  // namespace lbk
