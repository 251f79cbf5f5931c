// tests/standalone/coalescer_stress.cpp -- the request coalescer (nrtsearch_amd/csrc/coalescer.h) on its own, without HIP and
// without the library: 32 closed-loop callers with mixed compatibility keys, some of them with a deadline shorter than a batch,
// against a "device" that sleeps 200 us per batch.  Every call must return exactly once with its own answer (or with the
// expired-in-the-queue error, untouched), and nothing may be left pending.  A program of its own so that it can be built with
// -fsanitize=thread or -fsanitize=address,undefined:
//   clang++ -std=c++17 -O1 -g -pthread [-fsanitize=thread] tests/standalone/coalescer_stress.cpp -o coalescer_stress && ./coalescer_stress [seconds]
// (the thread sanitizer of g++ before 12 does not intercept pthread_cond_clockwait, which is what wait_until on the steady clock
// calls: it believes the leader keeps the coalescer's lock through its wait and reports a double lock that is none.)
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>

#include "../../nrtsearch_amd/csrc/coalescer.h"

using namespace nrtgpu::rt;

static int64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static bool deadline_passed(int64_t deadline_ns) { return deadline_ns != 0 && now_ns() >= deadline_ns; }

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      abort();                                                             \
    }                                                                      \
  } while (0)

struct Request : CoQueued {
  int key;             // requests travel together only under one key
  int64_t question;
  int64_t answer = 0;
  int delivered = 0;   // times a leader put an answer here
};

constexpr int kThreads = 32, kCap = 16, kExpired = -6;
static Coalescer co;
static std::atomic<int64_t> n_calls{0}, n_expired{0}, n_batches{0}, n_members{0};

static int call(int key, int64_t question, int64_t deadline_ns, int64_t* answer) {
  Request me;
  me.key = key;
  me.question = question;
  me.deadline_ns = deadline_ns;
  std::vector<CoQueued*> batch;
  {
    std::unique_lock<std::mutex> lk;
    if (!co.join(lk, &me, [&](int32_t waiting) { return waiting >= kCap; })) {
      CHECK(me.done && !lk.owns_lock());
      CHECK(me.rc == 0 ? me.delivered == 1 : me.rc == kExpired && me.err == "expired" && me.delivered == 0 && me.answer == 0);
      if (me.rc == 0) *answer = me.answer;
      return me.rc;
    }
    CHECK(lk.owns_lock() && co.leader == &me);
    co.leader_wait(lk, &me, 150, [&](int32_t waiting, bool late) {
      if (waiting >= kCap || (late && (co.inflight == 0 || (co.inflight == 1 && waiting >= 2 * co.inflight_queries)))) return CoWait::leave;
      return co.inflight >= 2 ? CoWait::until_woken : CoWait::until_linger_end;   // (both forms of sleep take part)
    });
    batch = co.form(&me, kCap, [&](const CoQueued* r) { return static_cast<const Request*>(r)->key == me.key; }, deadline_passed, kExpired,
                    "expired");
    CHECK(co.inflight >= 1 && co.leader != &me);   // (a full queue leaves whatever is in flight: no upper bound here)
  }
  CHECK(batch[0] == &me && (int)batch.size() <= kCap);
  std::this_thread::sleep_for(std::chrono::microseconds(200));   // the "device"
  for (size_t i = 1; i < batch.size(); ++i) {
    Request* r = static_cast<Request*>(batch[i]);
    CHECK(r->key == me.key);
    Coalescer::finish(r, 0, std::string(), [&] {
      r->answer = 2 * r->question + 1;
      r->delivered++;
    });
  }
  co.retire(batch.size());
  n_batches++;
  n_members += (int64_t)batch.size();
  CHECK(me.delivered == 0 && !me.done);
  *answer = 2 * me.question + 1;
  return 0;
}

int main(int argc, char** argv) {
  const double seconds = argc > 1 ? atof(argv[1]) : 3.0;
  const int64_t t_end = now_ns() + (int64_t)(seconds * 1e9);
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([t, t_end] {
      std::mt19937 rng(1234u + (unsigned)t);
      for (int64_t i = 0; now_ns() < t_end; ++i) {
        const int key = (int)(rng() % 3u);
        const int64_t question = (int64_t)t * 1000000007 + i;
        const int64_t deadline = rng() % 8u == 0 ? now_ns() + 100000 : 0;   // (half a batch away: most of these expire in the queue)
        int64_t answer = -1;
        const int rc = call(key, question, deadline, &answer);
        if (rc == 0) CHECK(answer == 2 * question + 1);
        else {
          CHECK(rc == kExpired && deadline != 0 && answer == -1);
          n_expired++;
        }
        n_calls++;
      }
    });
  for (std::thread& th : threads) th.join();
  CHECK(co.pending_count() == 0 && co.leader == nullptr && co.inflight == 0 && co.inflight_queries == 0);
  CHECK(n_members + n_expired == n_calls && n_batches > 0 && n_members > n_batches);   // (every call is accounted for; there was company)
  printf("coalescer_stress ok: %lld calls, %lld batches of %.1f on average, %lld expired in the queue\n", (long long)n_calls, (long long)n_batches,
         (double)n_members / (double)n_batches, (long long)n_expired);
  return 0;
}
