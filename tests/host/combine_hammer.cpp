// Drives the request combiner of ehx_knn / ehx_set (csrc/ehx_combine.h) with no device: 64 threads x 200 requests, a take
// like the kNN one (the oldest request's k, arrival order, a cap on the group's total size, other k left queued), a serve that
// sleeps a few microseconds and fails every 17th group with a text of its own.  Built by a plain host compiler
// (tests/test_combine_host.py); also the program to run under -fsanitize=thread and -fsanitize=address,undefined.
#include "ehx_combine.h"

#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>

using ehx_impl::CombineReq;
using ehx_impl::Combiner;

struct Req : CombineReq {
  unsigned k = 0, n = 0;   // the group key, and the request's size towards the cap
  int group = -1;          // written by take (lock held), read by serve and, after submit, by the owner
  int served = 0;          // written by serve
};
typedef Combiner<Req>::Group Group;

constexpr int kThreads = 64, kPerThread = 200, kFailEvery = 17;
constexpr unsigned kCap = 16;

static thread_local char t_err[512];   // the calling thread's error text, as the library's g_err
static Combiner<Req> combiner;
static int n_groups = 0;               // take's: under the combiner's lock
static std::atomic<int> in_serve{0}, n_served{0}, n_failed_groups{0}, n_shared_groups{0}, n_bad{0};

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "combine_hammer: %s (line %d)\n", #cond, __LINE__); \
      n_bad += 1;                                                      \
    }                                                                  \
  } while (0)

static bool fails(int group) { return group % kFailEvery == kFailEvery - 1; }

static Group take(Group& queue) {
  Group g;
  const unsigned gk = queue.front()->k;
  unsigned total = 0;
  for (auto it = queue.begin(); it != queue.end();) {
    if ((*it)->k == gk && total + (*it)->n <= kCap) {
      total += (*it)->n;
      (*it)->group = n_groups;
      g.push_back(*it);
      it = queue.erase(it);
    } else {
      ++it;
    }
  }
  n_groups += 1;
  return g;
}

static int serve(const Group& g) {
  CHECK(in_serve.fetch_add(1) == 0);   // one leader at a time
  CHECK(!g.empty());
  unsigned total = 0;
  for (Req* r : g) {
    CHECK(r->k == g[0]->k && r->group == g[0]->group);
    CHECK(r->served == 0 && !r->done);
    r->served += 1;
    total += r->n;
  }
  CHECK(total <= kCap);
  n_served += (int)g.size();
  n_shared_groups += g.size() > 1;
  std::this_thread::sleep_for(std::chrono::microseconds(3));
  int rc = 0;
  if (fails(g[0]->group)) {
    rc = 1000 + g[0]->group;
    snprintf(t_err, sizeof(t_err), "group %d failed", g[0]->group);
    n_failed_groups += 1;
  }
  in_serve -= 1;
  return rc;
}

static void caller(int t) {
  for (int i = 0; i < kPerThread; ++i) {
    Req me;
    me.k = (t + i) % 3 == 0 ? 7 : 3;
    me.n = 1 + (unsigned)(t * 31 + i * 7) % 5;
    snprintf(t_err, sizeof(t_err), "stale");
    const int rc = combiner.submit(me, take, serve, t_err, sizeof(t_err));
    CHECK(me.done && me.served == 1 && me.group >= 0 && rc == me.rc);
    if (fails(me.group)) {   // every request of a failed group sees that group's rc and text ...
      char want[64];
      snprintf(want, sizeof(want), "group %d failed", me.group);
      CHECK(rc == 1000 + me.group);
      CHECK(strcmp(me.err, want) == 0 && strcmp(t_err, want) == 0);
    } else {                 // ... and no other request does
      CHECK(rc == 0 && me.err[0] == 0);
    }
  }
}

int main() {
  alarm(120);   // a caller left waiting on an empty queue never returns: the program must end by itself
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t) th.emplace_back(caller, t);
  for (auto& t : th) t.join();
  CHECK(n_served == kThreads * kPerThread);
  CHECK(n_failed_groups == n_groups / kFailEvery && n_failed_groups > 0);
  CHECK(in_serve == 0);
  if (n_bad) return 1;
  printf("combine_hammer ok: %d requests in %d groups (%d of them shared, %d failed)\n", (int)n_served, n_groups,
         (int)n_shared_groups, (int)n_failed_groups);
  return 0;
}
