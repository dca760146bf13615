// The HBM replay buffer behind the rle_replay_* entries (replay.cpp).  It knows the engines bound to it only as
// opaque users: engine_drain and engine_unbind below are all it asks of them.
#pragma once
#include <utility>
#include <vector>

#include "memory.h"

namespace rle {

struct Engine;
// The engine's rle_step_async burst on its own queue retired (host wait; throws Error when the queue timed out).
void engine_drain(Engine& e);
// The engine's replay is going away: its steps fail with "no replay bound" from here on.
void engine_unbind(Engine& e);
struct Replay {
  int device;
  long long cap;
  int S, Sp, A, Ap, lap;
  long long ptr = 0, size = 0;
  float *state, *next_state, *action, *reward, *notdone, *priority;
  long long* size_d;
  // device copy of ptr, next to size_d and kept current wherever size_d is (push_cursor): the n-step gather stops
  // a walk at the write head (ops.h SampleArgs::ptr)
  long long* ptr_d;
  float* maxp_d;
  double* bsum;
  double* ssum;  // LAP sub-block sums (64 priorities each), nblk * 64
  int nblk;
  float* maxred_part;
  int maxred_nwg = 256;
  hipStream_t stream = nullptr;
  DevMem mem;
  Scratch scratch;  // eager entry points' temporaries
  // append staging
  float* stage = nullptr;
  long long stage_rows = 0;
  // bumped by every change of what sampling draws from (appends, priority writes):
  // an engine's batch prefetched under another version is stale
  unsigned long long version = 0;
  // engines bound to this replay, each with an event recorded on its stream after every
  // enqueued step: replay operations on `stream` wait for them first (an append after
  // rle_step_async must not race the step's priority scatter and block sums)
  std::vector<std::pair<Engine*, hipEvent_t>> users;
  // export / import staging (allocated at the first rle_replay_export / _import): two device images and two
  // pinned host images of kIoRows packed rows, the copies on a stream of their own so that the pack kernel of
  // chunk k+1 (on `stream`) runs under the copy of chunk k
  static constexpr long long kIoRows = 8192;
  PinMem pin;
  float* io_dev[2] = {nullptr, nullptr};
  float* io_host[2] = {nullptr, nullptr};
  hipStream_t io_stream = nullptr;
  hipEvent_t io_kernel_ev[2] = {nullptr, nullptr}, io_copy_ev[2] = {nullptr, nullptr};
  float* gather_host = nullptr;  // pinned image of a gather (grown on demand)
  size_t gather_host_floats = 0;
  size_t row_floats() const { return 2 * (size_t)S + A + 3; }
  void io_init();
  // The device copies of size and ptr from the host's, on `stream` (the caller synchronises).
  long long cursor_host[2] = {0, 0};  // the copy's source (a member: it outlives the asynchronous copy)
  void push_cursor();
  ReplayPackArgs pack_args() const {
    ReplayPackArgs a{};
    a.state = state, a.next_state = next_state, a.action = action;
    a.reward = reward, a.notdone = notdone, a.priority = priority;
    a.cap = cap, a.S = S, a.Sp = Sp, a.A = A, a.Ap = Ap;
    return a;
  }
  void wait_users();   // (also drains the users' direct-dispatch bursts)
  void drain_users();  // the users' rle_step_async bursts on their own queues retired (host wait)
  void remove_user(Engine* e);  // e no longer steps on this replay (no-op when it is not a user)
};

}  // namespace rle
