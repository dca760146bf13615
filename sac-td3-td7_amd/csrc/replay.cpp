// The HBM replay buffer: append, sampling and priority entry points run eagerly on the replay's own stream,
// export / import / gather through packed images, state statistics and normalisation; every rle_replay_* entry
// of include/rle.h.  The engines bound to a replay are reached through replay.h's two functions only.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "abi.h"
#include "dispatch.h"

namespace rle {

void Replay::drain_users() {
  for (auto& u : users) engine_drain(*u.first);
}
void Replay::wait_users() {
  drain_users();
  for (auto& u : users) HIPCHK(hipStreamWaitEvent(stream, u.second, 0));
}
void Replay::remove_user(Engine* e) {
  for (size_t i = 0; i < users.size(); ++i)
    if (users[i].first == e) {
      users.erase(users.begin() + i);
      break;
    }
}
void Replay::push_cursor() {
  // (size_d and ptr_d are one allocation, {size, ptr}: one copy)
  cursor_host[0] = size, cursor_host[1] = ptr;
  HIPCHK(hipMemcpyAsync(size_d, cursor_host, sizeof cursor_host, hipMemcpyHostToDevice, stream));
}
void Replay::io_init() {
  if (io_stream) return;
  const size_t n = (size_t)std::min(kIoRows, cap) * row_floats();  // (a chunk never has more rows than the ring)
  for (int b = 0; b < 2; ++b) {
    if (!io_dev[b]) io_dev[b] = mem.make<float>(n);
    if (!io_host[b]) io_host[b] = static_cast<float*>(pin.alloc(n * sizeof(float)));
    if (!io_kernel_ev[b]) HIPCHK(hipEventCreateWithFlags(&io_kernel_ev[b], hipEventDisableTiming));
    if (!io_copy_ev[b]) HIPCHK(hipEventCreateWithFlags(&io_copy_ev[b], hipEventDisableTiming));
  }
  HIPCHK(hipStreamCreateWithFlags(&io_stream, hipStreamNonBlocking));
}

// The packed image of c rows (ops.h ReplayPackArgs) with the fields the caller asked for, in the order
// state, next_state, action, reward, notdone, priority (`user`: the caller's six arrays, null = not wanted).
struct PackImage {
  size_t off[6], w[6], total = 0;
  long long c;
  bool want[6];
  template <class P>
  PackImage(const Replay& r, long long rows, P* const* user) : c(rows) {
    const size_t width[6] = {(size_t)r.S, (size_t)r.S, (size_t)r.A, 1, 1, 1};
    for (int f = 0; f < 6; ++f) {
      w[f] = width[f];
      want[f] = user[f] != nullptr;
      off[f] = total;
      if (want[f]) total += (size_t)c * w[f];
    }
  }
  void point(ReplayPackArgs& a, float* img) const {
    float** p[6] = {&a.p_state, &a.p_next_state, &a.p_action, &a.p_reward, &a.p_notdone, &a.p_priority};
    for (int f = 0; f < 6; ++f) *p[f] = want[f] ? img + off[f] : nullptr;
  }
  void to_user(const float* img, float* const* user, long long row0) const {
    for (int f = 0; f < 6; ++f)
      if (want[f]) std::memcpy(user[f] + (size_t)row0 * w[f], img + off[f], (size_t)c * w[f] * sizeof(float));
  }
  void from_user(float* img, const float* const* user, long long row0) const {
    for (int f = 0; f < 6; ++f)
      if (want[f]) std::memcpy(img + off[f], user[f] + (size_t)row0 * w[f], (size_t)c * w[f] * sizeof(float));
  }
};

}  // namespace rle

// ====================================================================== C ABI: the replay entries

using rle::Error;
using rle::guard;
using rle::PackImage;
using rle::Replay;

extern "C" {

int rle_replay_create(int device, long long capacity, int state_dim, int action_dim, int lap, rle_replay** out) {
  return guard([&] {
    REQUIRE(out && capacity > 0 && state_dim > 0 && action_dim > 0, "rle_replay_create: bad args");
    REQUIRE(state_dim <= 1024 && action_dim <= 128, "rle_replay_create: state_dim <= 1024, action_dim <= 128");
    REQUIRE(capacity <= 2048LL * 4096, "rle_replay_create: capacity > 8M transitions");
    HIPCHK(hipSetDevice(device));
    auto* h = new rle_replay();
    Replay& r = h->r;
    r.device = device;
    r.cap = capacity;
    r.S = state_dim;
    r.Sp = rle::r16(state_dim);
    r.A = action_dim;
    r.Ap = rle::r16(action_dim);
    r.lap = lap ? 1 : 0;
    try {
      HIPCHK(hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking));
      r.state = r.mem.make<float>((size_t)capacity * r.Sp);
      r.next_state = r.mem.make<float>((size_t)capacity * r.Sp);
      r.action = r.mem.make<float>((size_t)capacity * r.Ap);
      r.reward = r.mem.make<float>(capacity);
      r.notdone = r.mem.make<float>(capacity);
      r.priority = r.mem.make<float>(capacity);
      r.size_d = r.mem.make<long long>(2);  // {size, ptr} (zero from the allocation: an empty ring)
      r.ptr_d = r.size_d + 1;
      r.maxp_d = r.mem.make<float>(1);
      const float one = 1.f;  // lap.py:29 max_priority = 1
      HIPCHK(hipMemcpy(r.maxp_d, &one, 4, hipMemcpyHostToDevice));
      r.nblk = rle::cdiv(capacity, 4096);
      REQUIRE(!lap || capacity <= 64LL * 16 * 4096, "LAP replay capacity above 4M rows");  // (sampler: 16 blocks per lane)
      r.bsum = r.mem.make<double>(r.nblk);
      r.ssum = r.mem.make<double>((size_t)r.nblk * 64);
      r.maxred_part = r.mem.make<float>(r.maxred_nwg);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int rle_replay_destroy(rle_replay* r) {
  return guard([&] {
    if (!r) return;
    try {
      r->r.drain_users();
    } catch (const Error&) {  // (a timed-out burst: the engine's queue is closed; unbind anyway)
    }
    for (auto& u : r->r.users) {  // engines still bound: unbind (their steps now fail: "no replay bound")
      (void)hipEventSynchronize(u.second);
      rle::engine_unbind(*u.first);
    }
    (void)hipStreamSynchronize(r->r.stream);
    (void)hipStreamDestroy(r->r.stream);
    if (r->r.io_stream) {
      (void)hipStreamSynchronize(r->r.io_stream);
      (void)hipStreamDestroy(r->r.io_stream);
    }
    for (int b = 0; b < 2; ++b) {
      if (r->r.io_kernel_ev[b]) (void)hipEventDestroy(r->r.io_kernel_ev[b]);
      if (r->r.io_copy_ev[b]) (void)hipEventDestroy(r->r.io_copy_ev[b]);
    }
    delete r;
  });
}

int rle_replay_append(rle_replay* h, const float* state, const float* action, const float* reward,
                      const float* next_state, const float* notdone, long long count) {
  return guard([&] {
    REQUIRE(h && count >= 0, "append: bad args");
    Replay& r = h->r;
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    long long done = 0;
    // a chunk never wraps onto itself (rows i and i+cap would race; the later must win)
    const long long chunk_max = std::min<long long>(65536, r.cap);
    while (done < count) {
      const long long c = std::min(chunk_max, count - done);
      const size_t per = 2 * (size_t)r.Sp + r.Ap + 2;
      if (c > r.stage_rows) {
        r.stage = r.mem.make<float>((size_t)c * per);
        r.stage_rows = c;
      }
      std::vector<float> host((size_t)c * per, 0.f);
      float* hs = host.data();
      float* hns = hs + (size_t)c * r.Sp;
      float* ha = hns + (size_t)c * r.Sp;
      float* hr = ha + (size_t)c * r.Ap;
      float* hd = hr + c;
      for (long long i = 0; i < c; ++i) {
        const long long k = done + i;
        std::memcpy(hs + i * r.Sp, state + k * r.S, sizeof(float) * r.S);
        std::memcpy(hns + i * r.Sp, next_state + k * r.S, sizeof(float) * r.S);
        std::memcpy(ha + i * r.Ap, action + k * r.A, sizeof(float) * r.A);
        hr[i] = reward[k];
        hd[i] = notdone[k];
      }
      float* ds = r.stage;
      HIPCHK(hipMemcpyAsync(ds, hs, host.size() * sizeof(float), hipMemcpyHostToDevice, r.stream));
      HIPCHK(rle::launch_append(r.state, r.next_state, r.action, r.reward, r.notdone, r.priority, ds,
                                ds + (size_t)c * r.Sp, ds + 2 * (size_t)c * r.Sp, ds + 2 * (size_t)c * r.Sp + c * r.Ap,
                                ds + 2 * (size_t)c * r.Sp + c * r.Ap + c, r.ptr, r.cap, (int)c, r.Sp, r.Ap, r.maxp_d,
                                r.lap, r.bsum, r.ssum, r.size, r.stream));
      r.ptr = (r.ptr + c) % r.cap;
      r.size = std::min(r.size + c, r.cap);
      ++r.version;
      r.push_cursor();
      HIPCHK(hipStreamSynchronize(r.stream));
      done += c;
    }
  });
}

int rle_replay_state(rle_replay* h, long long* ptr, long long* size, float* max_priority) {
  return guard([&] {
    REQUIRE(h, "state: null");
    Replay& r = h->r;
    if (ptr) *ptr = r.ptr;
    if (size) *size = r.size;
    if (max_priority) {
      r.drain_users();
      HIPCHK(hipDeviceSynchronize());
      HIPCHK(hipMemcpy(max_priority, r.maxp_d, 4, hipMemcpyDeviceToHost));
    }
  });
}

static void recompute_bsum(Replay& r);

int rle_replay_fill_random(rle_replay* h, long long count, unsigned long long seed) {
  return guard([&] {
    Replay& r = h->r;
    REQUIRE(count > 0 && count <= r.cap, "fill: bad count");
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    HIPCHK(rle::launch_fill(r.state, r.next_state, r.action, r.reward, r.notdone, r.priority, count, r.S, r.Sp, r.A,
                            r.Ap, seed, r.stream));
    r.size = std::max(r.size, count);
    r.ptr = count % r.cap;
    ++r.version;
    r.push_cursor();
    HIPCHK(hipStreamSynchronize(r.stream));
    if (r.lap) recompute_bsum(r);
  });
}

int rle_replay_get_priority(rle_replay* h, float* out, long long n) {
  return guard([&] {
    REQUIRE(n <= h->r.cap, "get_priority: n > capacity");
    h->r.drain_users();
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->r.priority, n * 4, hipMemcpyDeviceToHost));
  });
}

int rle_replay_set_priority(rle_replay* h, const float* p, long long n, float max_priority) {
  return guard([&] {
    REQUIRE(n <= h->r.cap, "set_priority: n > capacity");
    h->r.drain_users();
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->r.priority, p, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->r.maxp_d, &max_priority, 4, hipMemcpyHostToDevice));
    if (h->r.lap) recompute_bsum(h->r);
    ++h->r.version;
  });
}

// Runs a small op program eagerly on the replay's stream (test hooks).
static void run_eager(Replay& r, std::vector<std::vector<rle::Op>> levels, int ks = rle::KS_EXT) {
  for (size_t l = 0; l < levels.size(); ++l) {
    auto& lv = levels[l];
    int wg = 0;
    for (auto& op : lv) {
      op.wg_begin = wg;
      wg += op.wg_count;
    }
    rle::Op* d = r.scratch.get<rle::Op>("ops" + std::to_string(l), lv.size());
    HIPCHK(hipMemcpy(d, lv.data(), lv.size() * sizeof(rle::Op), hipMemcpyHostToDevice));
    HIPCHK(rle::launch_level(d, lv.data(), (int)lv.size(), wg, r.stream, nullptr, nullptr, 0, ks));
  }
  HIPCHK(hipStreamSynchronize(r.stream));
}

// Full recompute of the LAP block sums (after bulk priority writes).  In-step and
// eager priority scatters and appends keep them exact incrementally.
static void recompute_bsum(Replay& r) {
  rle::Op a{};
  a.kind = rle::OP_SAMPLE_REDUCE;
  a.sample.priority = r.priority;
  a.sample.size = r.size_d;
  a.sample.bsum = r.bsum;
  a.sample.ssum = r.ssum;
  a.wg_count = r.nblk;
  run_eager(r, {{a}});
}

int rle_replay_sample_indices(rle_replay* h, int n, const float* u, long long* ind_out) {
  return guard([&] {
    Replay& r = h->r;
    REQUIRE(n > 0 && r.size > 0, "sample_indices: bad args / empty replay");
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    rle::Scratch& tmp = r.scratch;
    rle::SampleArgs s{};
    s.state = r.state;
    s.next_state = r.next_state;
    s.action = r.action;
    s.reward = r.reward;
    s.notdone = r.notdone;
    s.priority = r.priority;
    s.S = r.S;
    s.Sp = r.Sp;
    s.A = r.A;
    s.Ap = r.Ap;
    s.size = r.size_d;
    s.cap = r.cap;
    s.lap = r.lap;
    s.B = n;
    s.nq = n;
    s.bsum = r.bsum;
    s.ssum = r.ssum;
    s.nblk = r.nblk;
    auto timg = [&](const char* name, int rows, int cols) {  // scratch T image (outputs are not read back)
      rle::Mat m{};
      m.rbs = rle::r16(rows) / 16;
      m.cbn = cols / 16;
      m.t = tmp.get<float>(name, (size_t)rle::r16(rows) * cols);
      return m;
    };
    s.ss = timg("ss", 2 * n, r.Sp);
    s.a = timg("a", n, r.Ap);
    s.r = tmp.get<float>("r", n);
    s.nd = tmp.get<float>("nd", n);
    long long* dind = tmp.get<long long>("ind", n);
    s.ind = dind;
    s.u_out = tmp.get<float>("u_out", n);
    s.eps = timg("eps", n, r.Ap);
    // [0] rng step = 0, [1] tape position = 0 (zero from allocation, only read), [2] tape mode
    long long* cnt = tmp.get<long long>("ctl", 3);
    const long long ctl[3] = {0, 0, rle::kTapeU};
    float* du = tmp.get<float>("u", n);
    HIPCHK(hipMemcpyAsync(cnt, ctl, sizeof ctl, hipMemcpyHostToDevice, r.stream));
    HIPCHK(hipMemcpyAsync(du, u, n * 4, hipMemcpyHostToDevice, r.stream));
    s.ctrl_rng = cnt;
    s.tape_pos = cnt + 1;
    s.tape_mode = (const int*)(cnt + 2);
    s.tape_u = du;
    s.tape_eps = tmp.get<float>("tape_eps", (size_t)n * r.A);
    std::vector<std::vector<rle::Op>> lv;
    rle::Op b{};
    b.kind = rle::OP_SAMPLE_GATHER;
    b.sample = s;
    b.wg_count = rle::cdiv(n, 4);
    lv.push_back({b});
    run_eager(r, lv);
    HIPCHK(hipMemcpy(ind_out, dind, n * sizeof(long long), hipMemcpyDeviceToHost));
  });
}

int rle_replay_update_priority(rle_replay* h, int n, const long long* ind, const float* p) {
  return guard([&] {
    Replay& r = h->r;
    REQUIRE(n > 0 && n <= 1024, "update_priority: 0 < n <= 1024");
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    for (int i = 0; i < n; ++i) REQUIRE(ind[i] >= 0 && ind[i] < r.cap, "update_priority: index out of range");
    // The incremental fp64 block-sum update is exact for priorities >= 1 (integer multiples of
    // 2^-23 summing below 2^30); any smaller value -> full recompute of the block sums instead.
    bool small = false;
    for (int i = 0; i < n; ++i) small = small || !(p[i] >= 1.f);
    long long* di = r.scratch.get<long long>("prio_ind", n);
    float* dp = r.scratch.get<float>("prio_p", n);
    HIPCHK(hipMemcpyAsync(di, ind, n * 8, hipMemcpyHostToDevice, r.stream));
    HIPCHK(hipMemcpyAsync(dp, p, n * 4, hipMemcpyHostToDevice, r.stream));
    rle::Op op{};
    op.kind = rle::OP_PRIORITY;
    op.prio.priority = r.priority;
    op.prio.ind = di;
    op.prio.p = dp;
    op.prio.B = n;
    op.prio.max_priority = r.maxp_d;
    op.prio.bsum = r.lap && !small ? r.bsum : nullptr;
    op.prio.ssum = r.ssum;
    op.wg_count = 1;
    run_eager(r, {{op}});
    if (r.lap && small) recompute_bsum(r);
    ++r.version;
  });
}

int rle_replay_reset_max_priority(rle_replay* h) {
  return guard([&] {
    Replay& r = h->r;
    REQUIRE(r.size > 0, "reset_max_priority: empty");
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    rle::Op a{};
    a.kind = rle::OP_MAXRED;
    a.flat.src = r.priority;
    a.flat.size = r.size_d;
    a.flat.partial = r.maxred_part;
    a.flat.nwg = r.maxred_nwg;
    a.flat.stage = 0;
    a.wg_count = r.maxred_nwg;
    rle::Op b = a;
    b.flat.stage = 1;
    b.flat.out = r.maxp_d;
    b.wg_count = 1;
    run_eager(r, {{a}, {b}});
  });
}

int rle_replay_gather(rle_replay* h, int n, const long long* ind, float* state, float* action, float* reward,
                      float* next_state, float* notdone) {
  return guard([&] {
    REQUIRE(h && n >= 0 && (ind || n == 0), "gather: bad args");
    Replay& r = h->r;
    for (int i = 0; i < n; ++i) REQUIRE(ind[i] >= 0 && ind[i] < r.cap, "gather: index out of range");
    if (n == 0) return;
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    // one index-mode pack per chunk of kIoRows rows into a device image, one copy of the image into pinned
    // memory, then host copies into the caller's arrays (no per-row device copy)
    float* user[6] = {state, next_state, action, reward, notdone, nullptr};
    const long long cmax = std::min<long long>(n, Replay::kIoRows);
    long long* dind = r.scratch.get<long long>("gather_ind", n);
    float* dimg = r.scratch.get<float>("gather_img", (size_t)cmax * r.row_floats());
    if (r.gather_host_floats < (size_t)cmax * r.row_floats()) {
      r.gather_host_floats = (size_t)cmax * r.row_floats();
      r.gather_host = static_cast<float*>(r.pin.alloc(r.gather_host_floats * sizeof(float)));
    }
    HIPCHK(hipMemcpyAsync(dind, ind, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, r.stream));
    for (long long row0 = 0; row0 < n; row0 += cmax) {
      const long long c = std::min<long long>(cmax, n - row0);
      const PackImage L(r, c, user);
      rle::ReplayPackArgs a = r.pack_args();
      a.ind = dind + row0;
      a.n = (int)c;
      L.point(a, dimg);
      HIPCHK(rle::launch_replay_pack(a, r.stream));
      HIPCHK(hipMemcpyAsync(r.gather_host, dimg, L.total * sizeof(float), hipMemcpyDeviceToHost, r.stream));
      HIPCHK(hipStreamSynchronize(r.stream));
      L.to_user(r.gather_host, user, row0);
    }
  });
}

// The n-step host batch of rle.h's law: the sampler's own gather (OP_SAMPLE_GATHER on the KS_NSTEP instance, the
// op the step runs) with the caller's indices as its index tape, into N and T batch images as a step's are, read
// back and unpacked here.  The T images pass through the op's LDS-staged stores where the row shape takes them, the
// N images through its direct ones: both must hold the same rows.
int rle_replay_gather_nstep(rle_replay* h, int n, const long long* ind, int n_step, float discount, float* state,
                            float* action, float* reward, float* next_state, float* notdone, int* hops) {
  return guard([&] {
    REQUIRE(h && n >= 0 && (ind || n == 0), "gather_nstep: bad args");
    REQUIRE(n_step >= 1 && n_step <= rle::kMaxNStep, "gather_nstep: n_step outside 1 .. RLE_MAX_N_STEP");
    REQUIRE(std::isfinite(discount), "gather_nstep: discount must be finite");
    Replay& r = h->r;
    REQUIRE(n == 0 || r.size > 0, "gather_nstep: empty replay");
    for (int i = 0; i < n; ++i) REQUIRE(ind[i] >= 0 && ind[i] < r.size, "gather_nstep: index outside 0 .. size-1");
    if (n == 0) return;
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    rle::Scratch& tmp = r.scratch;
    constexpr int kChunk = 1024;  // queries per launch (a step's largest batch)
    const int Bmax = rle::r16(std::min(n, kChunk));
    auto img = [&](const char* name, int rows, int cols) {  // N + T images of [rows][cols], rows % 16 == 0
      rle::Mat m{};
      m.rbs = rows / 16;
      m.cbn = cols / 16;
      m.n = tmp.get<float>(std::string(name) + "_n", (size_t)rows * cols);
      m.t = tmp.get<float>(std::string(name) + "_t", (size_t)rows * cols);
      return m;
    };
    const rle::Mat ss_all = img("ns_ss", 2 * Bmax, r.Sp), a_all = img("ns_a", Bmax, r.Ap);
    float* d_r = tmp.get<float>("ns_r", Bmax);
    float* d_nd = tmp.get<float>("ns_nd", Bmax);
    float* d_hops = tmp.get<float>("ns_hops", Bmax);
    long long* d_ind = tmp.get<long long>("ns_ind", Bmax);
    long long* d_tape = tmp.get<long long>("ns_tape", Bmax);
    long long* cnt = tmp.get<long long>("ns_ctl", 3);  // [0] rng step, [1] tape position, [2] tape mode
    const long long ctl[3] = {0, 0, rle::kTapeInd};
    HIPCHK(hipMemcpyAsync(cnt, ctl, sizeof ctl, hipMemcpyHostToDevice, r.stream));
    auto n_at = [](int cbn, int row, int c) {
      return ((size_t)(row >> 4) * cbn + (c >> 4)) * 256 + ((c >> 2) & 3) * 64 + (row & 15) * 4 + (c & 3);
    };
    auto t_at = [](int rbs, int row, int c) {
      return ((size_t)(c >> 4) * rbs + (row >> 4)) * 256 + ((row >> 2) & 3) * 64 + (c & 15) * 4 + (row & 3);
    };
    std::vector<float> hn, ht, hv((size_t)Bmax * 3);
    for (int row0 = 0; row0 < n; row0 += kChunk) {
      const int c = std::min(kChunk, n - row0), B = rle::r16(c);
      rle::SampleArgs s{};
      s.state = r.state, s.next_state = r.next_state, s.action = r.action;
      s.reward = r.reward, s.notdone = r.notdone, s.priority = r.priority;
      s.S = r.S, s.Sp = r.Sp, s.A = r.A, s.Ap = r.Ap;
      s.size = r.size_d;
      s.cap = r.cap;
      s.lap = 0;
      s.B = B;
      s.nq = c;
      s.ss = ss_all;
      s.ss.rbs = 2 * B / 16;
      s.a = a_all;
      s.a.rbs = B / 16;
      s.r = d_r, s.nd = d_nd, s.ind = d_ind;
      s.ctrl_rng = cnt;
      s.tape_pos = cnt + 1;
      s.tape_mode = (const int*)(cnt + 2);
      s.tape_ind = d_tape;
      s.n_step = n_step;
      s.gamma = discount;
      s.ptr = r.ptr_d;
      s.hops_out = d_hops;
      HIPCHK(hipMemcpyAsync(d_tape, ind + row0, (size_t)c * sizeof(long long), hipMemcpyHostToDevice, r.stream));
      rle::Op op{};
      op.kind = rle::OP_SAMPLE_GATHER;
      op.sample = s;
      op.wg_count = rle::cdiv(c, 4);
      run_eager(r, {{op}}, rle::KS_NSTEP);
      auto unpack = [&](const rle::Mat& m, int rows, int cols, int src_row0, int width, float* out) {
        if (!out) return;
        hn.resize((size_t)rows * cols), ht.resize((size_t)rows * cols);
        HIPCHK(hipMemcpy(hn.data(), m.n, hn.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ht.data(), m.t, ht.size() * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < c; ++b)
          for (int j = 0; j < width; ++j) {
            const float vn = hn[n_at(m.cbn, src_row0 + b, j)], vt = ht[t_at(m.rbs, src_row0 + b, j)];
            if (std::memcmp(&vn, &vt, 4) != 0)
              throw Error{RLE_EHIP, "gather_nstep: the batch's N and T images differ"};
            out[((size_t)row0 + b) * width + j] = vt;
          }
      };
      unpack(s.ss, 2 * B, r.Sp, 0, r.S, state);
      unpack(s.ss, 2 * B, r.Sp, B, r.S, next_state);
      unpack(s.a, B, r.Ap, 0, r.A, action);
      HIPCHK(hipMemcpy(hv.data(), d_r, (size_t)c * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hv.data() + Bmax, d_nd, (size_t)c * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hv.data() + 2 * Bmax, d_hops, (size_t)c * 4, hipMemcpyDeviceToHost));
      for (int b = 0; b < c; ++b) {
        if (reward) reward[row0 + b] = hv[b];
        if (notdone) notdone[row0 + b] = hv[Bmax + b];
        if (hops) hops[row0 + b] = (int)hv[2 * Bmax + b];
      }
    }
  });
}

int rle_replay_io_rows(void) { return (int)Replay::kIoRows; }

int rle_replay_export(rle_replay* h, long long first, long long count, float* state, float* action, float* reward,
                      float* next_state, float* notdone, float* priority) {
  return guard([&] {
    REQUIRE(h, "export: null replay");
    Replay& r = h->r;
    REQUIRE(first >= 0 && count >= 0 && first + count <= r.cap, "export: slots first .. first+count-1 outside the ring");
    REQUIRE(!priority || r.lap, "export: priority of a replay without LAP");
    if (count == 0) return;
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    r.io_init();
    float* user[6] = {state, next_state, action, reward, notdone, priority};
    const long long R = Replay::kIoRows, nchunk = (count + R - 1) / R;
    auto finish = [&](long long k) {  // chunk k: its copy done, then out of the pinned image
      HIPCHK(hipEventSynchronize(r.io_copy_ev[k & 1]));
      PackImage(r, std::min(R, count - k * R), user).to_user(r.io_host[k & 1], user, k * R);
    };
    for (long long k = 0; k < nchunk; ++k) {
      const int b = (int)(k & 1);  // (image b is free: chunk k-2 left it in finish(k-2), an iteration ago)
      const long long c = std::min(R, count - k * R);
      const PackImage L(r, c, user);
      rle::ReplayPackArgs a = r.pack_args();
      a.first = first + k * R;
      a.n = (int)c;
      L.point(a, r.io_dev[b]);
      HIPCHK(rle::launch_replay_pack(a, r.stream));
      HIPCHK(hipEventRecord(r.io_kernel_ev[b], r.stream));
      HIPCHK(hipStreamWaitEvent(r.io_stream, r.io_kernel_ev[b], 0));
      HIPCHK(hipMemcpyAsync(r.io_host[b], r.io_dev[b], L.total * sizeof(float), hipMemcpyDeviceToHost, r.io_stream));
      HIPCHK(hipEventRecord(r.io_copy_ev[b], r.io_stream));
      if (k > 0) finish(k - 1);  // (under the kernel and copy of chunk k)
    }
    finish(nchunk - 1);
  });
}

int rle_replay_import(rle_replay* h, long long first, long long count, const float* state, const float* action,
                      const float* reward, const float* next_state, const float* notdone, const float* priority) {
  return guard([&] {
    REQUIRE(h, "import: null replay");
    Replay& r = h->r;
    REQUIRE(first >= 0 && count >= 0 && first + count <= r.cap, "import: slots first .. first+count-1 outside the ring");
    REQUIRE(!priority || r.lap, "import: priority of a replay without LAP");
    if (count == 0) return;
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    r.io_init();
    const float* user[6] = {state, next_state, action, reward, notdone, priority};
    const long long R = Replay::kIoRows, nchunk = (count + R - 1) / R;
    ++r.version;
    for (long long k = 0; k < nchunk; ++k) {
      const int b = (int)(k & 1);
      const long long c = std::min(R, count - k * R);
      const PackImage L(r, c, user);
      if (k >= 2) HIPCHK(hipEventSynchronize(r.io_copy_ev[b]));  // pinned image b: the copy of chunk k-2 has read it
      L.from_user(r.io_host[b], user, k * R);
      if (k >= 2) HIPCHK(hipStreamWaitEvent(r.io_stream, r.io_kernel_ev[b], 0));  // device image b: unpack k-2 done
      HIPCHK(hipMemcpyAsync(r.io_dev[b], r.io_host[b], L.total * sizeof(float), hipMemcpyHostToDevice, r.io_stream));
      HIPCHK(hipEventRecord(r.io_copy_ev[b], r.io_stream));
      HIPCHK(hipStreamWaitEvent(r.stream, r.io_copy_ev[b], 0));
      rle::ReplayPackArgs a = r.pack_args();
      a.first = first + k * R;
      a.n = (int)c;
      L.point(a, r.io_dev[b]);
      HIPCHK(rle::launch_replay_unpack(a, r.stream));
      HIPCHK(hipEventRecord(r.io_kernel_ev[b], r.stream));
    }
    HIPCHK(hipStreamSynchronize(r.stream));
  });
}

int rle_replay_set_state(rle_replay* h, long long ptr, long long size, float max_priority) {
  return guard([&] {
    REQUIRE(h, "set_state: null replay");
    Replay& r = h->r;
    REQUIRE(size >= 0 && size <= r.cap, "set_state: size outside 0..capacity");
    REQUIRE(ptr >= 0 && ptr < r.cap, "set_state: ptr outside 0..capacity-1");
    REQUIRE(std::isfinite(max_priority) && max_priority > 0.f, "set_state: max_priority must be finite and > 0");
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    r.ptr = ptr;
    r.size = size;
    r.push_cursor();
    HIPCHK(hipMemcpyAsync(r.maxp_d, &max_priority, sizeof(float), hipMemcpyHostToDevice, r.stream));
    HIPCHK(hipStreamSynchronize(r.stream));
    if (r.lap) recompute_bsum(r);  // (rows at or past size count as 0)
    ++r.version;
  });
}

// The stats launch shape of a replay's `state` over rows [0, size) (ops.h ReplayStatArgs)
static rle::ReplayStatArgs stat_args(Replay& r, const float* x) {
  rle::ReplayStatArgs a{};
  a.x = x;
  a.size = r.size;
  a.Sp = r.Sp;
  a.rows_wg = rle::stat_rows_wg(r.size, r.Sp);
  a.nwg = rle::stat_nwg(r.size, r.Sp);
  return a;
}

int rle_replay_state_stats(rle_replay* h, float* mean, float* std_out) {
  return guard([&] {
    REQUIRE(h && mean && std_out, "state_stats: null argument");
    Replay& r = h->r;
    if (r.size <= 0) throw Error{RLE_ESTATE, "state_stats: empty replay"};
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    rle::ReplayStatArgs a = stat_args(r, r.state);
    a.part = r.scratch.get<double>("stat_part", (size_t)a.nwg * r.Sp);
    double* md = r.scratch.get<double>("stat_mean_d", r.Sp);
    double* sd = r.scratch.get<double>("stat_std_d", r.Sp);
    float* mf = r.scratch.get<float>("stat_mean_f", r.Sp);
    float* sf = r.scratch.get<float>("stat_std_f", r.Sp);
    // pass 1: the means; pass 2: the centred squares (each: per-workgroup partials, then their sum in order)
    HIPCHK(rle::launch_replay_colsum(a, r.stream));
    a.out_d = md;
    a.out_f = mf;
    HIPCHK(rle::launch_replay_colfin(a, r.stream));
    a.center = md;
    HIPCHK(rle::launch_replay_colsum(a, r.stream));
    a.out_d = sd;
    a.out_f = sf;
    a.sq = 1;
    HIPCHK(rle::launch_replay_colfin(a, r.stream));
    HIPCHK(hipMemcpyAsync(mean, mf, (size_t)r.S * 4, hipMemcpyDeviceToHost, r.stream));
    HIPCHK(hipMemcpyAsync(std_out, sf, (size_t)r.S * 4, hipMemcpyDeviceToHost, r.stream));
    HIPCHK(hipStreamSynchronize(r.stream));
  });
}

int rle_replay_normalize_states(rle_replay* h, const float* shift, const float* scale) {
  return guard([&] {
    REQUIRE(h && shift && scale, "normalize_states: null argument");
    Replay& r = h->r;
    for (int j = 0; j < r.S; ++j) {
      REQUIRE(std::isfinite(shift[j]), "normalize_states: shift must be finite");
      REQUIRE(std::isfinite(scale[j]) && scale[j] != 0.f, "normalize_states: scale must be finite and non-zero");
    }
    if (r.size <= 0) throw Error{RLE_ESTATE, "normalize_states: empty replay"};
    HIPCHK(hipSetDevice(r.device));
    r.wait_users();
    // padded to Sp: a pad column computes (0 - 0) / 1, so it keeps the zero every first-layer GEMM relies on
    std::vector<float> hp(2 * (size_t)r.Sp, 0.f);
    for (int j = 0; j < r.Sp; ++j) hp[r.Sp + j] = 1.f;
    std::memcpy(hp.data(), shift, (size_t)r.S * 4);
    std::memcpy(hp.data() + r.Sp, scale, (size_t)r.S * 4);
    float* dp = r.scratch.get<float>("norm_vec", 2 * (size_t)r.Sp);
    HIPCHK(hipMemcpyAsync(dp, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, r.stream));
    rle::ReplayNormArgs a{};
    a.x[0] = r.state;
    a.x[1] = r.next_state;
    a.size = r.size;
    a.Sp = r.Sp;
    a.rows_wg = rle::stat_rows_wg(r.size, r.Sp);
    a.nwg = rle::stat_nwg(r.size, r.Sp);
    a.shift = dp;
    a.scale = dp + r.Sp;
    HIPCHK(rle::launch_replay_normalize(a, r.stream));
    HIPCHK(hipStreamSynchronize(r.stream));
    ++r.version;  // (bound engines redraw their prefetched batch, as after rle_replay_set_state)
  });
}

int rle_replay_copy(rle_replay* hd, rle_replay* hs) {
  return guard([&] {
    REQUIRE(hd && hs, "copy: null replay");
    Replay &d = hd->r, &s = hs->r;
    REQUIRE(d.cap == s.cap && d.S == s.S && d.A == s.A && d.lap == s.lap,
            "copy: replays differ in capacity, state_dim, action_dim or lap");
    if (hd == hs) return;
    // the source quiescent (its users' steps and its own stream), then every array on the destination's stream
    HIPCHK(hipSetDevice(s.device));
    s.wait_users();
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipSetDevice(d.device));
    d.wait_users();
    auto cp = [&](void* dst, const void* src, size_t bytes) {
      if (d.device == s.device) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, d.stream));
      else HIPCHK(hipMemcpyPeerAsync(dst, d.device, src, s.device, bytes, d.stream));
    };
    const size_t cap = (size_t)s.cap;
    cp(d.state, s.state, cap * s.Sp * sizeof(float));
    cp(d.next_state, s.next_state, cap * s.Sp * sizeof(float));
    cp(d.action, s.action, cap * s.Ap * sizeof(float));
    cp(d.reward, s.reward, cap * sizeof(float));
    cp(d.notdone, s.notdone, cap * sizeof(float));
    cp(d.priority, s.priority, cap * sizeof(float));
    cp(d.bsum, s.bsum, (size_t)s.nblk * sizeof(double));
    cp(d.ssum, s.ssum, (size_t)s.nblk * 64 * sizeof(double));
    cp(d.maxp_d, s.maxp_d, sizeof(float));
    d.ptr = s.ptr;
    d.size = s.size;
    d.push_cursor();  // (from the host's values: the source's device copies are these same two)
    HIPCHK(hipStreamSynchronize(d.stream));
    ++d.version;
  });
}

}  // extern "C"
