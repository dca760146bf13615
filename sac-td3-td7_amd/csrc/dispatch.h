// How a built step program reaches the device (dispatch.cpp): the planner that turns a program's levels
// into its list of rle_level launches, the captured program, and the engine's AQL queue.
#pragma once
#include <hsa/hsa.h>

#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "host.h"

namespace rle {

// Appends one level's launches to `out`; no HIP or HSA call, no state of its own.
// d_ops / h_ops: the level's ops on the device (only its address is used) and on the host; nwg: its workgroups.
// A level of more than kLevelOps ops takes consecutive launches of kLevelOps (its ops are independent, so any
// split is correct).  next_ops / next_nops: the ops of the level launched after this one, which the
// last launch's 8 leading workgroups load into every XCD's L2 (0: none); a launch before the last
// prefetches the rest of its own level.  trace: the level's phase stamps (the launches are of the traced
// kernel) or null.  Throws Error (RLE_EHIP), `out` as it was, when a launch would exceed kMaxLevelWG workgroups.
void level_launches(const Op* d_ops, const Op* h_ops, int nops, int nwg, unsigned long long* trace, const Op* next_ops,
                    int next_nops, int ks, std::vector<LevelLaunch>& out);
// Plans one level and launches it on the stream (eager runs outside a captured program).
hipError_t launch_level(const Op* d_ops, const Op* h_ops, int nops, int nwg, hipStream_t st,
                        unsigned long long* trace = nullptr, const Op* next_ops = nullptr, int next_nops = 0,
                        int ks = KS_EXT);

// A captured program.  `launches` is the one description of what a replay runs: the hipGraph was captured
// from it, rle_plan dispatch 2 launches it on the stream, and dispatch 1 queues it as AQL packets whose
// kernel arguments are aql_ka's copies.
// Graph owns g and x: move-only, a move leaves the source without handles, the destructor destroys x then g.
// (The other fields point into the engine's device memory, which outlives every program.)
struct GraphFields {
  hipGraph_t g = nullptr;
  hipGraphExec_t x = nullptr;
  Op* d_ops = nullptr;
  unsigned long long* trace = nullptr;  // [total wg][4] when RLE_TRACE=1
  long long trace_n = 0;
  std::vector<int> nops, nwg, off;
  std::string desc;
  std::vector<LevelLaunch> launches;  // rle_level dispatches per replay (a level of > kLevelOps ops takes several)
  unsigned char* aql_ka = nullptr;    // (rle_plan dispatch 1, untraced) their kernel arguments in device memory, kAqlKaStride apart
  int levels() const { return (int)nops.size(); }
  int nlaunch() const { return (int)launches.size(); }
};
struct Graph : GraphFields {
  Graph() = default;
  Graph(const Graph&) = delete;
  Graph& operator=(const Graph&) = delete;
  Graph(Graph&& o) noexcept : GraphFields(std::move(o)) { o.g = nullptr, o.x = nullptr; }
  Graph& operator=(Graph&& o) noexcept {
    if (this != &o) {
      release();
      GraphFields::operator=(std::move(o));
      o.g = nullptr, o.x = nullptr;
    }
    return *this;
  }
  ~Graph() { release(); }

 private:
  void release() {
    if (x) (void)hipGraphExecDestroy(x);
    if (g) (void)hipGraphDestroy(g);
    x = nullptr, g = nullptr;
  }
};
constexpr size_t kAqlKaStride = 128;

// ---- Direct AQL dispatch (default; rle_plan.dispatch 0 for the hipGraph path): the step graphs' level
// launches written as kernel-dispatch packets into the engine's own HSA queue instead of hipGraph
// replays.  Fences as HIP's own: agent-scope acquire and release between dependent levels; the first
// packet of a flush acquires and its last releases at system scope (host-written inputs, host-read
// results).  tools/mbaql.cpp measured the same packets at 3.83 us per level against hipGraph's 4.08.
// One HSA queue of a device, shared by the engines aql_open hands it to (at most kAqlQueuesPerDevice
// per device and process: more user-mode queues than that oversubscribe the device's hardware queue
// slots, and every queue's dispatches slow down -- profiles/r05_seeds_aql.txt, r05_seeds_hwq.txt).
// mu: one burst's packets and doorbells at a time (engines driven from several threads).
struct AqlHw {
  hsa_agent_t agent{};
  hsa_queue_t* q = nullptr;
  uint64_t kobj[KS_COUNT] = {};  // rle_level<false, ks>
  uint32_t gseg[KS_COUNT] = {}, pseg[KS_COUNT] = {};
  std::atomic<bool> failed{false};  // a burst on this queue timed out: every engine sharing it fails fast
  std::mutex mu;
  ~AqlHw() {
    if (q) (void)hsa_queue_destroy(q);
  }
};
// An engine's view of its queue: its own completion signal, pending packets and timing.
struct AqlQueue {
  std::shared_ptr<AqlHw> hw;
  hsa_signal_t sig{};
  struct Pending {  // one replay of a program: packet i is (*launches)[i] with the arguments at ka + i * kAqlKaStride
    const std::vector<LevelLaunch>* launches;
    const unsigned char* ka;
  };
  std::vector<Pending> pending;
  // a LOWER bound on the time per packet: the fastest burst seen (>= kAqlMinBurst packets) x kAqlBoundFrac, 0 before
  // one was timed.  The wait sleeps only through this bound's share of a burst, so it wakes before the burst ends and
  // spins the rest: a mean-based estimate overslept short bursts (a 20-step bench burst woke 0.5 ms late, -17%).
  double us_per_launch = 0.0;
  bool failed = false;          // a flush timed out: its packets may still be queued, the queue takes no more
  size_t inflight = 0;          // packets submitted since the last aql_complete
  uint64_t last_idx = 0;        // queue index of the last packet this engine submitted
  bool timed_idle = false;      // the oldest burst in flight started on an idle queue (its wall time is its own)
  std::chrono::steady_clock::time_point t0{};  // first doorbell of the oldest burst in flight
  bool closed() const { return failed || (hw && hw->failed.load(std::memory_order_relaxed)); }
  ~AqlQueue() {
    if (sig.handle) (void)hsa_signal_destroy(sig);
  }
};
// The engine's queue on device `dev`, after HIP has loaded librle's code object (any rle_level launch).
std::unique_ptr<AqlQueue> aql_open(int dev);
// Writes every pending packet and rings the doorbell; bursts may be submitted back to back.
void aql_submit(AqlQueue& A);
// Waits until every submitted burst has retired (their host-side wall time added to *ms when given).
void aql_complete(AqlQueue& A, double* ms);
// The wait policy as a pure function (rle_aql_wait_plan).
enum AqlWaitAct : int { AQL_SPIN = 0, AQL_SLEEP = 1, AQL_TIMEOUT = 2 };
int aql_wait_step(double expected_us, double elapsed_us, double timeout_s, double* sleep_us);
// The failed-queue state machine and the doorbell groups without a device (rle_aql_selftest); throws Error.
void aql_selftest();

}  // namespace rle
