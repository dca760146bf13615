// The launch path of the MI355X off-policy update engine: a program's levels planned into its list of
// rle_level launches (level_launches), and the engine's direct AQL dispatch of such lists.  The three
// consumers of a list are Engine::capture (stream capture into the hipGraph), Engine::launch_graph
// (rle_plan dispatch 2: launch_packet on the stream) and aql_submit (dispatch 1).
#include "dispatch.h"

#include <hsa/hsa_ext_amd.h>
#include <hsa/hsa_ven_amd_loader.h>

#include <algorithm>
#include <map>
#include <thread>

namespace rle {

void level_launches(const Op* d_ops, const Op* h_ops, int nops, int nwg, unsigned long long* trace, const Op* next_ops,
                    int next_nops, int ks, std::vector<LevelLaunch>& out) {
  const size_t out0 = out.size();
  const int lines_per_op = (int)(sizeof(Op) / 64);
  for (int q0 = 0; q0 < nops; q0 += kLevelOps) {
    const int n = std::min(nops - q0, kLevelOps);
    const bool last = q0 + n >= nops;
    const int w0 = h_ops[q0].wg_begin;
    const int w1 = last ? nwg : h_ops[q0 + n].wg_begin;
    if (w1 - w0 + 8 > kMaxLevelWG) {
      out.resize(out0);
      throw Error{RLE_EHIP, std::string("level_launches: a launch of more than kMaxLevelWG - 8 workgroups: ") +
                                hipGetErrorString(hipErrorInvalidValue)};
    }
    LevelLaunch L{};
    L.ks = ks;
    L.traced = trace != nullptr;
    L.ka.ops = d_ops + q0;
    L.ka.trace = trace ? trace + (size_t)w0 * trace_stride() : nullptr;
    // the following launch's ops: the rest of this level, then the next level's
    const int nn = std::min(last ? next_nops : nops - q0 - n, kLevelOps);
    L.ka.next = last ? next_ops : d_ops + q0 + n;
    L.ka.next_lines = (unsigned)std::min(nn * lines_per_op, 2 * kThreads);
    for (int q = 0; q < kLevelOps; ++q) {
      if (q < n) {
        const Op& o = h_ops[q0 + q];
        const unsigned vid = o.kind == OP_GEMM ? (unsigned)o.gemm.vid : (unsigned)o.kind >> 4;
        L.ka.entry[q] = (unsigned)(o.wg_begin - w0) | (((unsigned)o.kind & 0xfu) << 16) | (vid << 20);
      } else {
        L.ka.entry[q] = 0xffffu;
      }
    }
    const int npf = L.ka.next_lines ? 8 : 0;  // leading prefetch workgroups (entry 0 bit 31)
    if (npf) L.ka.entry[0] |= 0x80000000u;
    L.grid = (unsigned)(w1 - w0 + npf);
    out.push_back(L);
  }
}

hipError_t launch_level(const Op* d_ops, const Op* h_ops, int nops, int nwg, hipStream_t st, unsigned long long* trace,
                        const Op* next_ops, int next_nops, int ks) {
  std::vector<LevelLaunch> launches;
  level_launches(d_ops, h_ops, nops, nwg, trace, next_ops, next_nops, ks, launches);
  for (const LevelLaunch& L : launches) {
    const hipError_t e = launch_packet(L, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- Direct AQL dispatch (dispatch.h)
constexpr int kAqlQueuesPerDevice = 4;
#define HSACHK(x)                                                                              \
  do {                                                                                         \
    hsa_status_t s_ = (x);                                                                     \
    if (s_ != HSA_STATUS_SUCCESS) throw Error{RLE_EHIP, std::string(#x) + ": hsa status " + std::to_string((int)s_)}; \
  } while (0)

static hsa_status_t aql_find_gpu(hsa_agent_t a, void* data) {
  auto* want = static_cast<std::pair<uint32_t, hsa_agent_t>*>(data);
  hsa_device_type_t t;
  if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU)
    return HSA_STATUS_SUCCESS;
  uint32_t bdf = 0;
  if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
  if (bdf == want->first) {
    want->second = a;
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}
struct AqlFind {
  hsa_agent_t agent;
  const char* name;
  uint64_t kobj;
  uint32_t gseg, pseg;
};
static hsa_status_t aql_find_kernel(hsa_executable_t exe, void* data) {
  auto* f = static_cast<AqlFind*>(data);
  hsa_executable_symbol_t sym;
  if (hsa_executable_get_symbol_by_name(exe, f->name, &f->agent, &sym) == HSA_STATUS_SUCCESS) {
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &f->kobj);
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &f->gseg);
    hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &f->pseg);
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}

// The queue of device `dev`, after HIP has loaded librle's code object (any rle_level launch).
static std::shared_ptr<AqlHw> aql_hw_create(int dev) {
  auto A = std::make_shared<AqlHw>();
  HSACHK(hsa_init());
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  std::pair<uint32_t, hsa_agent_t> want{(uint32_t)((prop.pciBusID << 8) | (prop.pciDeviceID << 3)), {}};
  hsa_iterate_agents(aql_find_gpu, &want);
  REQUIRE(want.second.handle, "aql: no HSA agent for the HIP device");
  A->agent = want.second;
  hsa_ven_amd_loader_1_03_pfn_t tbl;
  HSACHK(hsa_system_get_major_extension_table(HSA_EXTENSION_AMD_LOADER, 1, sizeof(tbl), &tbl));
  for (int x = 0; x < KS_COUNT; ++x) {
    AqlFind f{A->agent, level_kernel_symbol(x), 0, 0, 0};
    tbl.hsa_ven_amd_loader_iterate_executables(aql_find_kernel, &f);
    REQUIRE(f.kobj, "aql: rle_level's kernel object is not loaded");
    A->kobj[x] = f.kobj;
    A->gseg[x] = f.gseg;
    A->pseg[x] = f.pseg;
  }
  uint32_t qmax = 0;
  HSACHK(hsa_agent_get_info(A->agent, HSA_AGENT_INFO_QUEUE_MAX_SIZE, &qmax));
  HSACHK(hsa_queue_create(A->agent, std::min<uint32_t>(qmax, 16384), HSA_QUEUE_TYPE_SINGLE, nullptr, nullptr,
                          UINT32_MAX, UINT32_MAX, &A->q));
  return A;
}
// The engine's queue: a new HSA queue while the device has fewer than kAqlQueuesPerDevice live ones,
// else the live one with the fewest engines (its bursts then run in submission order with theirs).
std::unique_ptr<AqlQueue> aql_open(int dev) {
  static std::mutex pool_mu;
  static std::map<int, std::vector<std::weak_ptr<AqlHw>>> pool;
  auto A = std::make_unique<AqlQueue>();
  {
    std::lock_guard<std::mutex> lk(pool_mu);
    auto& live = pool[dev];
    live.erase(std::remove_if(live.begin(), live.end(), [](const std::weak_ptr<AqlHw>& w) { return w.expired(); }),
               live.end());
    if ((int)live.size() < kAqlQueuesPerDevice) {
      A->hw = aql_hw_create(dev);
      live.push_back(A->hw);
    } else {
      for (auto& w : live) {
        auto h = w.lock();
        if (h && (!A->hw || h.use_count() < A->hw.use_count())) A->hw = h;
      }
    }
  }
  HSACHK(hsa_signal_create(0, 0, nullptr, &A->sig));  // (bursts in flight: aql_submit)
  return A;
}

// How the host waits for a flush without holding its core (MuJoCo stepping runs on the host cores beside
// the engine, north_star): while more than kAqlSpinUs of the expected duration remain it sleeps (slices of
// at most kAqlSliceUs, the signal checked between them), then spins on the signal; past timeout_s it gives
// up.  expected_us = packets still to retire x a lower bound on the queue's time per packet (AqlQueue::us_per_launch).
constexpr double kAqlSpinUs = 150.0, kAqlSliceUs = 2000.0, kAqlTimeoutS = 60.0;
constexpr size_t kAqlMinBurst = 32;   // bursts timed for the per-packet bound (AqlQueue::us_per_launch)
constexpr double kAqlBoundFrac = 0.92;
int aql_wait_step(double expected_us, double elapsed_us, double timeout_s, double* sleep_us) {
  *sleep_us = 0.0;
  if (elapsed_us > timeout_s * 1e6) return AQL_TIMEOUT;
  const double left = expected_us - elapsed_us - kAqlSpinUs;
  if (left < 20.0) return AQL_SPIN;
  *sleep_us = std::min(left, kAqlSliceUs);
  return AQL_SLEEP;
}
// Waits until pred() holds, by aql_wait_step's policy; on timeout the engine's queue and the shared
// hardware queue are marked failed (every engine on it then fails fast instead of waiting 60 s again).
template <class Pred>
static void aql_wait(AqlQueue& A, Pred pred, double expected_us, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  while (!pred()) {
    const double el = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    double sl = 0.0;
    const int act = aql_wait_step(expected_us, el, kAqlTimeoutS, &sl);
    if (act == AQL_TIMEOUT) {
      A.failed = true;
      if (A.hw) A.hw->failed = true;
      A.pending.clear();
      A.inflight = 0;
      throw Error{RLE_EHIP, std::string("aql: ") + what + " did not complete within 60 s; the engine's queue is "
                            "closed (every later step fails; destroy the engine)"};
    }
    if (act == AQL_SLEEP) std::this_thread::sleep_for(std::chrono::duration<double, std::micro>(sl));
  }
}
static Error aql_closed_error() { return Error{RLE_EHIP, "aql: the engine's queue is closed after a timed-out dispatch"}; }

// Doorbell batching: the doorbell is rung after a packet whose queue index is the last of an aligned
// group of kAqlDoorbellEvery (and after a burst's last packet).  The groups are aligned to the ABSOLUTE
// index, so the packets one doorbell publishes never straddle the end of the ring (its size is a power
// of two >= kAqlDoorbellEvery).  Queue interceptors (rocprofv3's kernel tracing wraps the queue) copy
// the packets of one doorbell as one contiguous run of the ring: a run that crossed the ring's end read
// past it (profiles/r05_prof_crash.txt: SIGSEGV at the 1 MB ring's end, 16384 x 64 B).
constexpr uint64_t kAqlDoorbellEvery = 64;
static bool aql_doorbell_after(uint64_t idx, bool last) { return last || (idx & (kAqlDoorbellEvery - 1)) == kAqlDoorbellEvery - 1; }

// Writes every pending packet and rings the doorbell; the completion signal counts the submitted bursts
// still in flight (each burst's last packet decrements it), so bursts may be submitted back to back
// (rle_step_async) and aql_complete waits for all of them.  A slot is reserved only once the ring has
// room for it (the wait happens before hsa_queue_add_write_index, under hw.mu, so a timed-out wait never
// leaves a reserved slot unwritten for the packet processor to stall on).
void aql_submit(AqlQueue& A) {
  size_t n = 0;  // packets of this burst
  for (const AqlQueue::Pending& p : A.pending) n += p.launches->size();
  if (!n) return;
  if (A.closed()) {
    A.pending.clear();
    throw aql_closed_error();
  }
  AqlHw& hw = *A.hw;
  std::lock_guard<std::mutex> lk(hw.mu);
  hsa_queue_t* q = hw.q;
  const uint64_t mask = q->size - 1;
  if (!A.inflight) {
    A.timed_idle = hsa_queue_load_read_index_scacquire(q) == hsa_queue_load_write_index_relaxed(q);
  }
  hsa_signal_add_relaxed(A.sig, 1);
  bool rung = false;
  uint64_t since_bell = 0;  // packets written since the last doorbell
  auto bell = [&](uint64_t idx) {
    hsa_signal_store_screlease(q->doorbell_signal, idx);
    since_bell = 0;
    if (!A.inflight && !rung) A.t0 = std::chrono::steady_clock::now();
    rung = true;
  };
  // packet i is launch L of the pending program before `prog`, its kernel arguments at ka
  auto prog = A.pending.begin();
  const LevelLaunch *L = nullptr, *L_end = nullptr;
  const unsigned char* ka = nullptr;
  for (size_t i = 0; i < n; ++i, ++L, ka += kAqlKaStride) {
    for (; L == L_end; ++prog) {
      L = prog->launches->data();
      L_end = L + prog->launches->size();
      ka = prog->ka;
    }
    const uint64_t next = hsa_queue_load_write_index_relaxed(q);
    if (next - hsa_queue_load_read_index_scacquire(q) >= q->size) {
      // (bursts of > q->size packets) publish what is written, wait until half the queue has drained, then
      // write on: the host sleeps through most of it instead of tracking the device one packet at a time
      if (since_bell) bell(next - 1);
      const uint64_t half = q->size / 2;
      const double ahead = (double)(next - hsa_queue_load_read_index_scacquire(q) - half + 1);
      try {
        aql_wait(A, [&] { return next - hsa_queue_load_read_index_scacquire(q) < half; }, ahead * A.us_per_launch,
                 "a queue slot");
      } catch (...) {
        hsa_signal_subtract_relaxed(A.sig, 1);  // (this burst's last packet will never be written)
        throw;
      }
    }
    const uint64_t idx = hsa_queue_add_write_index_relaxed(q, 1);
    auto* pk = (hsa_kernel_dispatch_packet_t*)q->base_address + (idx & mask);
    pk->workgroup_size_x = kThreads;
    pk->workgroup_size_y = 1;
    pk->workgroup_size_z = 1;
    pk->reserved0 = 0;
    pk->grid_size_x = L->grid * kThreads;
    pk->grid_size_y = 1;
    pk->grid_size_z = 1;
    const int x = L->ks;
    pk->private_segment_size = hw.pseg[x];
    pk->group_segment_size = hw.gseg[x];
    pk->kernel_object = hw.kobj[x];
    pk->kernarg_address = const_cast<unsigned char*>(ka);
    pk->reserved2 = 0;
    const bool last = i + 1 == n;
    pk->completion_signal = last ? A.sig : hsa_signal_t{0};
#ifndef RLE_EXP_ACQ  // (timing-only variant builds: make variant-engine; the product uses agent / agent)
#define RLE_EXP_ACQ HSA_FENCE_SCOPE_AGENT
#define RLE_EXP_REL HSA_FENCE_SCOPE_AGENT
#endif
    const int a = i == 0 ? HSA_FENCE_SCOPE_SYSTEM : RLE_EXP_ACQ;
    const int r = last ? HSA_FENCE_SCOPE_SYSTEM : RLE_EXP_REL;
    const uint16_t hdr = (HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
                         (a << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (r << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
    __atomic_store_n((uint32_t*)pk, (uint32_t)hdr | (1u << 16), __ATOMIC_RELEASE);  // header | setup (1 dim)
    ++since_bell;
    if (last) A.last_idx = idx;
    if (aql_doorbell_after(idx, last)) bell(idx);
  }
  A.inflight += n;
  A.pending.clear();
}
// Waits until every submitted burst has retired (host-side wall time from the first doorbell of the
// oldest burst in flight to completion added to *ms when given).  The sleep estimate counts only the
// packets up to this engine's last one (other engines' later bursts on a pooled queue are not its
// wait), and the per-packet bound is refreshed only from bursts that started on an idle queue.
void aql_complete(AqlQueue& A, double* ms) {
  if (!A.inflight) return;
  if (A.closed()) {
    A.inflight = 0;
    throw aql_closed_error();
  }
  hsa_queue_t* q = A.hw->q;
  const uint64_t rd = hsa_queue_load_read_index_scacquire(q);
  const double left = A.last_idx + 1 > rd ? (double)(A.last_idx + 1 - rd) : 0.0;
  aql_wait(A, [&] { return hsa_signal_load_scacquire(A.sig) < 1; }, left * A.us_per_launch, "a dispatch");
  const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - A.t0).count();
  if (A.inflight >= kAqlMinBurst && A.timed_idle) {
    const double per = kAqlBoundFrac * wall_ms * 1e3 / (double)A.inflight;
    A.us_per_launch = A.us_per_launch > 0.0 ? std::min(A.us_per_launch, per) : per;
  }
  A.inflight = 0;
  if (ms) *ms += wall_ms;
}


void aql_selftest() {
  auto hw = std::make_shared<AqlHw>();
  AqlQueue a, b;
  a.hw = hw;
  b.hw = hw;
  REQUIRE(!a.closed() && !b.closed(), "selftest: fresh queues closed");
  a.failed = true;
  hw->failed = true;  // (as aql_wait's timeout leaves them)
  const std::vector<LevelLaunch> one(1);
  a.pending.push_back({&one, nullptr});
  a.inflight = 7;
  int refused = 0;
  try {
    aql_submit(a);
  } catch (const Error&) {
    ++refused;
  }
  REQUIRE(refused == 1 && a.pending.empty(), "selftest: a closed queue took a burst");
  try {
    aql_complete(a, nullptr);
  } catch (const Error&) {
    ++refused;
  }
  REQUIRE(refused == 2 && a.inflight == 0, "selftest: a closed queue waited for its burst");
  aql_complete(a, nullptr);  // (nothing in flight: returns)
  b.pending.push_back({&one, nullptr});
  try {
    aql_submit(b);
  } catch (const Error&) {
    ++refused;
  }
  REQUIRE(refused == 3, "selftest: an engine sharing a failed hardware queue took a burst");
  // doorbell groups: for every start index, the packets between two doorbells lie in one pass of the ring
  for (uint64_t size : {64ull, 1024ull, 16384ull})
    for (uint64_t start = size - 130; start < size + 130; ++start)
      for (uint64_t n : {1ull, 5ull, 64ull, 200ull}) {
        uint64_t first = start;
        for (uint64_t i = start; i < start + n; ++i)
          if (aql_doorbell_after(i, i + 1 == start + n)) {
            REQUIRE(first / size == i / size, "selftest: a doorbell group straddles the ring's end");
            first = i + 1;
          }
        REQUIRE(first == start + n, "selftest: packets left without a doorbell");
      }
}

}  // namespace rle
