// The program planner (plan.cpp): what turns a step program -- a list of ops with read / write resource
// sets -- into dependency levels, and the checks that guard it.  GEMM layout checks and finalisation, the
// host replay of the GEMM's address arithmetic (RLE_AUDIT), the byte-level conflict check of every level
// (RLE_HAZARD), the traffic model (RLE_TRAFFIC) and struct Prog with its scheduler.
//
// No HIP or HSA call, and no state of its own: nothing global or thread-local, no environment variable
// read.  Everything a program is planned with arrives in its PlanOptions.
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "host.h"

namespace rle {

inline int r4(int x) { return (x + 3) & ~3; }
inline int r16(int x) { return (x + 15) & ~15; }
inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// byte offset of the 16 x 16 block holding (r, c) in an N image of cbn column blocks / a T image of rbs row blocks
inline long long h_nblk(int cbn, int r, int c) { return ((long long)(r >> 4) * cbn + (c >> 4)) * 1024; }
inline long long h_tblk(int rbs, int r, int c) { return ((long long)(c >> 4) * rbs + (r >> 4)) * 1024; }

// Live allocations (address -> bytes) for the RLE_AUDIT=1 operand-range check and the RLE_HAZARD=1 level
// check.  Engines and replays on other host threads allocate concurrently (ctypes drops the GIL), so every
// method locks.
class AllocRegistry {
 public:
  void add(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(mu_);
    m_[(uintptr_t)p] = bytes;
  }
  void drop(const void* p) {
    std::lock_guard<std::mutex> lk(mu_);
    m_.erase((uintptr_t)p);
  }
  // every allocation that starts in [p, p + bytes): the buffers carved out of one block
  void drop_range(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(mu_);
    const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
    for (auto it = m_.lower_bound(lo); it != m_.end() && it->first < hi;) it = m_.erase(it);
  }
  // the allocation holding address a: true, with its [*lo, *hi)
  bool containing(uintptr_t a, uintptr_t* lo, uintptr_t* hi) const {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = m_.upper_bound(a);
    if (it == m_.begin()) return false;
    --it;
    if (a >= it->first + it->second) return false;
    *lo = it->first;
    *hi = it->first + it->second;
    return true;
  }
  // the end of the allocation holding p (p + 4 when none does)
  uintptr_t end_of(const void* p) const {
    uintptr_t lo, hi;
    return containing((uintptr_t)p, &lo, &hi) ? hi : (uintptr_t)p + 4;
  }

 private:
  mutable std::mutex mu_;
  std::map<uintptr_t, size_t> m_;
};

// How a program is planned: the scheduling knobs of rle_plan (resolved, no field "default") and the
// diagnostic switches.  The engine fills one per program built (Engine::prog_options).
struct PlanOptions {
  int balance = 0;  // 0 off, 1 any item, 2 no Adam items, 3 no Adam items + only into levels
                    // whose longest op is at least twice as long
  // weight of the step-end op (RLE_TINY_W, A/B; 0 = no tiny-op moves)
  // (rle_plan tiny_w / uni_w / tiny_wg; A/B tiny_w 0 / 20 / 30: TD7 8021 / 8050 / 8054, SAC 12249 /
  // 12235 / 12328; uni_w 60 as the LAP sampler, 12 with tiny_wg 64: SAC +-0, TD3 -0.5%)
  int tiny_w = 30, uni_w = 60, tiny_wg = 2;
  int pl_w = 0;  // (rle_plan pl_w) added to GEMMs whose workgroups run an in-tile prologue (has_pre 3-5)
  int lap_w = 60, head_w = 60, adam_w = 8;  // (rle_plan lap_w / head_w / adam_w)
  int lpt = 0;                              // (rle_plan lpt: longest-first op order in each level)
  int rb = 0;                               // register-blocked wide weight-gradient tiles (rle_plan rb)
  int xcd = 1;                              // XCD-aware tile order (rle_plan xcd)
  bool audit = false;    // RLE_AUDIT: every GEMM added is replayed against `allocs`
  bool hazard = false;   // RLE_HAZARD: schedule() checks every level's byte ranges
  bool crit = false;     // RLE_DESC_CRIT: schedule() marks the ops on a longest dependency chain
  bool traffic = false;  // RLE_TRAFFIC: graph descriptions carry level_traffic's figures
  const AllocRegistry* allocs = nullptr;  // the live allocations (audit, hazard and traffic read it)
  // The same options for a pass that wants the dependency levels alone: no rebalance, program order
  PlanOptions asap() const {
    PlanOptions o = *this;
    o.balance = o.lpt = 0;
    return o;
  }
};

void check_gemm(const GemmArgs& g);
// (ks < 0: in any kernel set)
bool gemm_variant_compiled(int vid, int ks = -1);
// Device-side dispatch fields of a GEMM op: compiled variant, split count, tile-row
// reciprocal (kernels.hip gemm_v); xcd: the XCD-aware tile order (rle_plan xcd).
void gemm_finalize(GemmArgs& g, bool xcd);

// A byte range an op touches.
struct Access {
  uintptr_t lo, hi;
  int w;  // 1: the op stores (or atomically updates) these bytes
  const char* what;
  int t = -1;  // (GEMM ranges) the op's workgroup that touches them; -1: the op as a whole
};
// Where audit_gemm's ranges go: appended to `out` with their workgroup index when it is set, else each is
// checked to lie inside one allocation of `allocs` (Error when one does not).
struct AuditSink {
  const AllocRegistry* allocs = nullptr;
  std::vector<Access>* out = nullptr;
};
void audit_gemm(const GemmArgs& g, const AuditSink& sink);

// The conflict sweep of the hazard check as a pure function: ranges [lo, hi) of op `op`, w: it stores them;
// item[op]: the program item the op came from.  Returns the first pair of overlapping ranges (indices into
// recs; in address order of the later range's start, the earlier-starting range first) of different ops of
// different items of which at least one stores, or {-1, -1}.
struct HazardRec {
  uintptr_t lo, hi;
  int w, op;
};
std::pair<int, int> hazard_scan(const std::vector<HazardRec>& recs, const std::vector<int>& item);
// ops: one level's ops; item[i]: the program item op i came from.  Throws on a conflict.
void level_hazards(const std::vector<Op>& ops, const std::vector<int>& item, int level, const AllocRegistry& allocs);

// ---- RLE_TRAFFIC=1: the bytes each level must move (the union of its ops' byte ranges, so a range
// several tiles read counts once), by kind: activations read / written, weights read, Adam state
// (p, m, v read and written, N image written).  Graph descriptions carry it (tools/pmc_levels.py
// sets it against the PMC counters: traffic above these bytes is re-reads, e.g. one copy per XCD).
struct LevelTraffic {
  double act_r = 0, act_w = 0, w_r = 0, adam = 0, other = 0;
  // Per-XCD read model: every XCD's L2 fetches its own copy of what its workgroups read (round-robin dispatch:
  // workgroup w of a launch runs on XCD w mod 8, the 8 descriptor-prefetch workgroups first), so a GEMM
  // operand that tiles on several XCDs read is fetched once per XCD; reads of non-GEMM ops count once.
  double xcd_r = 0, adam_w = 0;  // (adam_w: the Adam stores alone -- adam counts its reads and stores)
};
// (P, nP: the engine's parameter block, whose reads count as weights)
LevelTraffic level_traffic(const std::vector<Op>& ops, const float* P, size_t nP, const AllocRegistry& allocs);

// A step program: items in program order, each one op or a group of ops, with the resources it reads and writes.
struct Prog {
  struct Item {
    std::vector<Op> ops;  // one op, or a group writing disjoint parts of the same buffers
    std::vector<int> rd, wr;
    int level = 0;
  };
  explicit Prog(const PlanOptions& o) : opt(o) {}
  PlanOptions opt;
  std::vector<Item> items;
  // ops per level: one launch each (kLevelOps preloaded entries)
  static constexpr int max_ops = kLevelOps;
  // (Engine::norm_fin) the finalized AvgL1Norm row means of this program: producer partials -> (means, resource)
  std::map<const float*, std::pair<float*, int>> norm_fins;
  static bool rb_eligible(const GemmArgs& g);
  void add(const Op& op, std::vector<int> rd, std::vector<int> wr) { add_group({op}, std::move(rd), std::move(wr)); }
  // (GEMM ops are finalised with the program's rb / xcd, checked, and audited when opt.audit)
  void add_group(std::vector<Op> ops, std::vector<int> rd, std::vector<int> wr);
  // A GEMM of this program whose epilogue was changed after it was added: its dispatch fields again
  void refinalize(GemmArgs& g) const { gemm_finalize(g, opt.xcd != 0); }
  // Relative per-workgroup duration of an item (its longest op): a GEMM workgroup's
  // dependent MFMA chain grows with reduction length x tile width (4 waves share it); Adam
  // epilogues, the loss head and the sampler are long for their size (level traces).
  int tiny_weight() const { return opt.tiny_w ? opt.tiny_w : 8; }
  int uniform_weight() const { return opt.uni_w; }
  bool tiny_moves() const { return opt.tiny_w != 0; }
  int op_weight(const Op& op) const;
  int item_weight(const Item& it) const;
  // RAW / WAW / WAR successors of every item (program order)
  std::vector<std::vector<int>> successors() const;
  // (describe, RLE_DESC_CRIT=1) items on a longest dependency chain of the ASAP placement: their
  // level + the longest chain after them = the last level (every dependence edge is one level)
  std::vector<char> crit;
  void mark_critical(int maxl);
  // After the ASAP pass: in reverse program order, move each item with slack (every
  // successor at least two levels later) to the lightest level of its window where it is
  // not the longest op, so wide ASAP levels (contended CUs) shed work into thin levels of
  // the critical chain.  Dependencies are the RAW / WAW / WAR edges of the ASAP pass.
  void rebalance(int maxl, std::vector<int>& nops, std::vector<int>& nwg, int wg_cap);
  std::vector<std::vector<char>> crit_lv;  // (describe) per level, per op: on a longest chain
  // Lowest level respecting RAW / WAR / WAW against all earlier ops (program order), and
  // (wg_cap) holding no more workgroups than are resident on the device at once unless
  // the op alone exceeds that: a second dispatch wave costs more than a later level.
  // Returns the levels' ops in launch order, wg_begin assigned.
  std::vector<std::vector<Op>> schedule(int wg_cap = 1 << 30);
};

}  // namespace rle
