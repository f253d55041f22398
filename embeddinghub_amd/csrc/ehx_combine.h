// The leader/follower request combiner of ehx_knn (small searches become one device batch) and ehx_set (single-row Sets
// become one batch write).  Standard library only — tests/host/combine_hammer.cpp drives it with no device.
// A caller queues its request.  The first caller that finds no leader becomes one: it takes groups off the queue and serves
// them with the lock released until its OWN request has been answered, then gives the role up and wakes the waiters, one of
// whose requests may still be queued (a leader that kept serving while the queue refills would delay its own, already
// answered, caller without bound).  An uncontended call is a group of one and runs at once; under load the groups grow.
#pragma once
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <vector>

namespace ehx_impl {

struct CombineReq {   // what the combiner keeps per request: the base of a caller's request type
  int rc = 0;
  bool done = false;
  char err[256] = "";
};

template <class Req>   // Req: a CombineReq with the caller's arguments behind it, on its thread's stack until submit returns
class Combiner {
 public:
  typedef std::vector<Req*> Group;   // the queue (arrival order), and a group taken from it
  // take(queue) -> Group: removes the next group, at least one request, from the non-empty queue; called with the lock held.
  // serve(group) -> rc: answers all of it; called with the lock released, on the leader's thread.
  // err / err_cap: the CALLING thread's error text.  A serve that fails leaves its text there and every request of the group
  // gets a copy beside the rc; a request that failed leaves its copy there on return.
  template <class Take, class Serve>
  int submit(Req& me, Take&& take, Serve&& serve, char* err, size_t err_cap) {
    std::unique_lock<std::mutex> lk(mu_);
    queue_.push_back(&me);
    while (!me.done) {
      if (leader_) {  // somebody else is serving: wait for my result, or for the leadership to come free
        cv_.wait(lk, [&] { return me.done || !leader_; });
        continue;
      }
      leader_ = true;
      while (!me.done && !queue_.empty()) {
        const Group group = take(queue_);
        lk.unlock();
        const int rc = serve(group);
        lk.lock();
        for (Req* r : group) {
          r->rc = rc;
          if (rc) snprintf(r->err, sizeof(r->err), "%.255s", err);   // (cut to the request's 256 bytes)
          r->done = true;   // (last: its owner may return, and *r die, as soon as the lock is free)
        }
        cv_.notify_all();
      }
      leader_ = false;
      cv_.notify_all();  // a waiter whose request is still queued takes over
    }
    lk.unlock();
    if (me.rc) snprintf(err, err_cap, "%s", me.err);
    return me.rc;
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  Group queue_;
  bool leader_ = false;
};

}  // namespace ehx_impl
