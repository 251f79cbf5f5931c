// coalescer.h -- request coalescing behind the single-query entries (search.cpp: nrtgpu_search_bm25_coalesced, vectors.cpp:
// nrtgpu_knn_exact_coalesced): concurrent callers (the SEARCH pool's threads) are merged into device batches leader/follower
// style -- no extra thread.  The first caller to find no leader becomes one: it waits by its entry's rule, takes every pending
// request that may travel with its own (up to a cap), runs them as one batch outside the lock and wakes their callers.  The oldest
// request it leaves behind is promoted in the middle of its wait and leads the next batch, so two batches can be in flight and the
// host work of one hides behind the kernels of the other.
//
// The mechanism only: what travels together, when a leader leaves and how a batch is run are the entry's.  Standard library only
// (no HIP, no runtime_internal.h), so it can be driven -- and run under a thread sanitizer -- without a device
// (tests/standalone/coalescer_stress.cpp).
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

namespace nrtgpu {
namespace rt {

// What every queued caller is: the entry's request type derives from it and lives on its caller's stack.
struct CoQueued {
  int64_t deadline_ns = 0;   // the calling thread's (nrtgpu_set_thread_deadline_ns)
  int rc = 0;
  bool done = false;   // results (or the error) are in place
  bool lead = false;   // promoted: this caller waits for and runs the next batch
  std::string err;
  // Every caller sleeps on its own condition variable AND its own mutex: a finished batch wakes hundreds of callers, and if they
  // all had to re-acquire the coalescer's lock to leave their wait (and again to submit their next request) the lock handoffs
  // alone would cost more than the batch's kernels.  done / lead are written under `m`; the waiting leader is the one waiter that
  // uses `cv` with the coalescer's lock.
  std::mutex m;
  std::condition_variable cv;
};

enum class CoWait { leave, until_woken, until_linger_end };   // what a leader's rule answers (Coalescer::leader_wait)

struct Coalescer {
  std::mutex mu;
  std::vector<CoQueued*> pending;   // waiting for a leader
  CoQueued* leader = nullptr;       // the caller waiting for / about to run the next batch
  int inflight = 0;                 // batches executing right now
  int inflight_queries = 0;         // ... and how many requests they hold (read by the BM25 leave rule; the kNN rule does not use it)
  int last_batch = 0;               // size of the batch formed last
  bool hold = false;                // test hook: the entries' leave rules let no leader go with less than a full batch while set

  // Join: queue `me`.  true: this caller leads, `lk` holds the coalescer's lock.  false: it travelled in somebody's batch (or
  // expired in the queue): rc / err and the entry's results are in place, `lk` is released.  wake(waiting): what a follower's
  // arrival tells a waiting leader at once (the queue is full, the cohort is back); the leader's own rule decides.
  template <class Wake>
  bool join(std::unique_lock<std::mutex>& lk, CoQueued* me, Wake wake) {
    lk = std::unique_lock<std::mutex>(mu);
    pending.push_back(me);
    if (!leader) {
      leader = me;
      return true;
    }
    if (wake((int32_t)pending.size())) leader->cv.notify_one();
    lk.unlock();
    {
      std::unique_lock<std::mutex> mine(me->m);
      me->cv.wait(mine, [&] { return me->done || me->lead; });
    }
    if (me->done) return false;
    lk.lock();   // promoted: continue as the leader
    return true;
  }

  // The leader's wait (lock held): rule(waiting, late) says leave, sleep until woken, or sleep until woken but no longer than the
  // linger's end -- late: linger_us have passed since the wait began (from then on every sleep is until woken).  Woken by a
  // follower's arrival (join), a finishing batch (retire) and the test hook.
  template <class Rule>
  void leader_wait(std::unique_lock<std::mutex>& lk, CoQueued* me, int64_t linger_us, Rule rule) {
    const auto linger_end = std::chrono::steady_clock::now() + std::chrono::microseconds(linger_us);
    for (;;) {
      const bool late = std::chrono::steady_clock::now() >= linger_end;
      const CoWait w = rule((int32_t)pending.size(), late);
      if (w == CoWait::leave) return;
      if (w == CoWait::until_woken || late) me->cv.wait(lk);
      else me->cv.wait_until(lk, linger_end);
    }
  }

  // Form the leader's batch (lock held): `me` first, then every pending request that is compatible(r), up to cap.  A request whose
  // deadline passed in the queue leaves without being searched (expired_rc, expired_text); the others stay pending, and the
  // oldest of them is handed the lead.  The batch counts as in flight from here to retire().
  template <class Compatible>
  std::vector<CoQueued*> form(CoQueued* me, int32_t cap, Compatible compatible, bool (*deadline_passed)(int64_t), int expired_rc,
                              const char* expired_text) {
    std::vector<CoQueued*> batch{me}, rest;
    for (CoQueued* r : pending) {
      if (r == me) continue;
      if (deadline_passed(r->deadline_ns)) finish(r, expired_rc, expired_text, [] {});
      else if ((int32_t)batch.size() < cap && compatible(r)) batch.push_back(r);
      else rest.push_back(r);
    }
    pending.swap(rest);
    leader = pending.empty() ? nullptr : pending.front();
    if (leader) {
      std::lock_guard<std::mutex> theirs(leader->m);
      leader->lead = true;
      leader->cv.notify_one();
    }
    inflight++;
    inflight_queries += (int)batch.size();
    last_batch = (int)batch.size();
    return batch;
  }

  // Finish one member: fill() puts the entry's results in place, then the caller is told.  All of it under the request's own lock:
  // the woken caller cannot return -- and free its request -- before we are done with it, and it contends with nobody but us.
  template <class Fill>
  static void finish(CoQueued* r, int rc, const std::string& err, Fill fill) {
    std::lock_guard<std::mutex> theirs(r->m);
    fill();
    r->rc = rc;
    if (rc != 0) r->err = err;
    r->done = true;
    r->cv.notify_one();
  }

  // The batch has left the device: a waiting leader may have been waiting for that.
  void retire(size_t batch_size) {
    std::lock_guard<std::mutex> lk(mu);
    inflight--;
    inflight_queries -= (int)batch_size;
    if (leader) leader->cv.notify_one();
  }

  // test hooks (nrtgpu_debug_hold_coalescers, nrtgpu_debug_coalescer_pending)
  void set_hold(bool h) {
    std::lock_guard<std::mutex> lk(mu);
    hold = h;
    if (leader) leader->cv.notify_one();   // (the leader looks at its rule again: on release it may leave, on hold it sleeps again)
  }
  int pending_count() {
    std::lock_guard<std::mutex> lk(mu);
    return (int)pending.size();
  }
};

}  // namespace rt
}  // namespace nrtgpu
