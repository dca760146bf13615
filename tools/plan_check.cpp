// Stand-alone check of the program planner (csrc/plan.cpp) for a sanitizer build on the host:
//   make -C sac-td3-td7_amd plan-check
// compiles this file and plan.cpp with -fsanitize=address,undefined and runs it.  No GPU, no Python.  It feeds
// Prog::schedule and hazard_scan the made-up programs and byte ranges of tests/test_plan_host.py (the expected
// values are derived there) and a few thousand random ones, for the sanitizers' sake, whose results are only
// checked for consistency.  Exit status 0 and "plan-check: ... ok" when every check holds.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>

#include "plan.h"

using namespace rle;

static std::atomic<int> g_checks{0}, g_failed{0};  // (random_cases runs on two threads)
#define CHECK(c)                                               \
  do {                                                         \
    ++g_checks;                                                \
    if (!(c)) {                                                \
      ++g_failed;                                              \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                          \
  } while (0)

static Op gemm(int wg, int weight, int tn = 64, int epi = EPI_STORE, int pre = 0) {
  Op op{};
  op.kind = OP_GEMM;
  op.wg_count = wg;
  op.gemm.R = weight * 1024 / tn;
  op.gemm.tn = tn;
  op.gemm.epi = epi;
  op.gemm.has_pre = pre;
  return op;
}
static Op plain(int kind, int wg) {
  Op op{};
  op.kind = kind;
  op.wg_count = wg;
  return op;
}
static Op copy(int wg) { return plain(OP_COPY, wg); }
static Op step_end(int mode) {
  Op op = plain(OP_STEP_END, 1);
  op.end.mode = mode;
  return op;
}
static Op gather(int wg, int lap) {
  Op op = plain(OP_SAMPLE_GATHER, wg);
  op.sample.lap = lap;
  return op;
}

struct Placed {
  int level, pos, wg_begin;
  bool operator==(const Placed& o) const { return level == o.level && pos == o.pos && wg_begin == o.wg_begin; }
};
// Items filled directly (the GEMMs have no operands to finalise), ops numbered in program order through Op::seq.
struct Synth {
  Prog pg;
  int nops = 0;
  explicit Synth(const PlanOptions& o) : pg(o) {}
  void add(std::vector<Op> ops, std::vector<int> rd, std::vector<int> wr) {
    Prog::Item it;
    for (Op& op : ops) op.seq = nops++;
    it.ops = std::move(ops), it.rd = std::move(rd), it.wr = std::move(wr);
    pg.items.push_back(std::move(it));
  }
  std::vector<Placed> run(int wg_cap = 1 << 30) {
    std::vector<Placed> out((size_t)nops, Placed{-1, -1, -1});
    const auto levels = pg.schedule(wg_cap);
    for (size_t l = 0; l < levels.size(); ++l)
      for (size_t k = 0; k < levels[l].size(); ++k) out[levels[l][k].seq] = {(int)l, (int)k, levels[l][k].wg_begin};
    return out;
  }
};
static std::vector<int> levels_of(const std::vector<Placed>& p) {
  std::vector<int> l;
  for (const Placed& x : p) l.push_back(x.level);
  return l;
}
static PlanOptions knobs(int balance = 0, int lpt = 0) {
  PlanOptions o;
  o.balance = balance;
  o.lpt = lpt;
  return o;
}
using V = std::vector<int>;

// chain c0 -> c1 -> c2 -> c3 (levels 0 .. 3), x beside c0 with its consumer on level 4 (test_plan_host.py window_prog)
static std::vector<int> window(const PlanOptions& o, Op x, int w2 = 64, int n2 = 1) {
  Synth s(o);
  s.add({gemm(100, 64)}, {}, {1});
  s.add({x}, {}, {9});
  s.add({gemm(20, 64)}, {1}, {2});
  s.add(std::vector<Op>((size_t)n2, gemm(n2 == 1 ? 10 : 1, w2)), {2}, {3});
  s.add({gemm(50, 64)}, {3}, {4});
  s.add({copy(5)}, {9, 4}, {});
  return levels_of(s.run());
}
static std::vector<int> tiny(PlanOptions o, int mode) {
  Synth s(o);
  s.add({gemm(1, 16)}, {}, {1});
  s.add({step_end(mode)}, {}, {9});
  s.add({gemm(1, 16)}, {1}, {2});
  s.add({gemm(1, 64)}, {2}, {3});
  s.add({gemm(1, 64)}, {3}, {4});
  s.add({copy(1)}, {9, 4}, {});
  return levels_of(s.run());
}

static void scheduler_cases() {
  {  // dependencies
    Synth s(knobs());
    s.add({copy(1)}, {}, {1}), s.add({copy(1)}, {1}, {2}), s.add({copy(1)}, {1, 2}, {}), s.add({copy(1)}, {}, {1});
    s.add({copy(1)}, {-1}, {-1});
    CHECK(levels_of(s.run()) == (V{0, 1, 2, 3, 0}));
  }
  {  // 12 ops per level, groups deferred whole
    Synth s(knobs());
    for (int i = 0; i < 10; ++i) s.add({copy(1)}, {}, {});
    s.add({copy(1), copy(1), copy(1)}, {}, {});
    s.add({copy(1), copy(1)}, {}, {});
    const auto p = s.run();
    CHECK((p[10] == Placed{1, 0, 0}) && (p[12] == Placed{1, 2, 2}) && (p[13] == Placed{0, 10, 10}) && (p[14] == Placed{0, 11, 11}));
  }
  {  // wg_cap
    Synth s(knobs());
    s.add({copy(60)}, {}, {}), s.add({copy(50)}, {}, {}), s.add({copy(40)}, {}, {});
    const auto p = s.run(100);
    CHECK((p[0] == Placed{0, 0, 0}) && (p[1] == Placed{1, 0, 0}) && (p[2] == Placed{0, 1, 60}));
    Synth b(knobs());
    b.add({copy(500)}, {}, {}), b.add({copy(10)}, {}, {}), b.add({copy(500)}, {}, {});
    CHECK(levels_of(b.run(100)) == (V{0, 1, 2}));
  }
  // balance
  CHECK(window(knobs(0), copy(30)) == (V{0, 0, 1, 2, 3, 4}));
  CHECK(window(knobs(1), copy(30)) == (V{0, 2, 1, 2, 3, 4}));
  CHECK(window(knobs(1), copy(30), 4)[1] == 1);
  CHECK(window(knobs(1), copy(30), 64, 12)[1] == 1);
  CHECK(window(knobs(1), gemm(30, 1, 16, EPI_ADAM))[1] == 2);
  CHECK(window(knobs(2), gemm(30, 1, 16, EPI_ADAM))[1] == 0);
  CHECK(window(knobs(2), copy(30), 15)[1] == 2);
  CHECK(window(knobs(3), copy(30), 15)[1] == 1);
  CHECK(window(knobs(3), copy(30), 16)[1] == 2);
  // tiny-op move
  CHECK(tiny(knobs(1), 0) == (V{0, 2, 1, 2, 3, 4}));
  CHECK(tiny(knobs(0), 0)[1] == 0 && tiny(knobs(1), 1)[1] == 0);
  {
    PlanOptions o = knobs(1);
    o.tiny_w = 0;
    CHECK(tiny(o, 0)[1] == 0);
    o = knobs(1);
    o.tiny_wg = 0;
    CHECK(tiny(o, 0)[1] == 0);
  }
  {  // lpt
    Synth s(knobs(0, 1));
    for (const Op& op : {copy(3), gemm(5, 64), plain(OP_HEAD, 2), copy(7), gemm(4, 16, 32), gather(6, 1)}) s.add({op}, {}, {});
    const std::vector<Placed> want{{0, 4, 17}, {0, 0, 0}, {0, 1, 5}, {0, 5, 20}, {0, 3, 13}, {0, 2, 7}};
    CHECK(s.run() == want);
  }
}

static void scan_cases() {
  using Recs = std::vector<HazardRec>;
  using P = std::pair<int, int>;
  const P none{-1, -1};
  CHECK(hazard_scan(Recs{{0x1000, 0x2000, 0, 0}, {0x1800, 0x2800, 0, 1}}, {0, 1}) == none);
  CHECK(hazard_scan(Recs{{0x1000, 0x2000, 1, 0}, {0x1800, 0x2800, 0, 1}}, {0, 1}) == (P{0, 1}));
  CHECK(hazard_scan(Recs{{0x1800, 0x2800, 1, 0}, {0x1000, 0x2000, 1, 1}}, {0, 1}) == (P{1, 0}));
  CHECK(hazard_scan(Recs{{0x1000, 0x2000, 1, 0}, {0x1800, 0x2800, 1, 1}}, {3, 3}) == none);
  CHECK(hazard_scan(Recs{{0x1000, 0x2000, 1, 0}, {0x2000, 0x3000, 1, 1}}, {0, 1}) == none);
  Recs act{{0x100, 0x200, 0, 3},   {0x300, 0x400, 0, 3},   {0x1000, 0x9000, 1, 0}, {0x2000, 0x2100, 0, 1},
           {0x3000, 0x3100, 0, 1}, {0x4000, 0x4100, 0, 1}, {0x8000, 0x8100, 0, 2}, {0x9000, 0x9100, 0, 3}};
  const std::vector<int> item{0, 0, 1, 2};
  std::mt19937 rng(5);
  for (int rep = 0; rep < 50; ++rep) {
    const P hit = hazard_scan(act, item);
    CHECK(hit.first >= 0 && act[hit.first].op == 0 && act[hit.second].op == 2);
    std::shuffle(act.begin(), act.end(), rng);
  }
  CHECK(hazard_scan({}, {}) == none);
}

// Random programs and ranges: every op placed once, dependencies and the op bound respected, wg_begin a prefix
// sum; a reported pair really conflicts, and brute force finds a conflict exactly when the sweep does.
static void random_cases(unsigned seed, int rounds) {
  std::mt19937 rng(seed);
  auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
  for (int r = 0; r < rounds; ++r) {
    PlanOptions o = knobs(pick(4), pick(2));
    o.tiny_w = pick(2) * 30;
    Synth s(o);
    const int nitems = 1 + pick(40);
    for (int i = 0; i < nitems; ++i) {
      std::vector<Op> ops;
      for (int k = 1 + pick(3); k > 0; --k) {
        const int kind = pick(4);
        ops.push_back(kind == 0 ? gemm(1 + pick(200), 1 + pick(64), 64, pick(2)) : kind == 1 ? step_end(pick(3))
                      : kind == 2 ? gather(1 + pick(8), pick(2)) : copy(1 + pick(300)));
      }
      std::vector<int> rd, wr;
      for (int k = pick(3); k > 0; --k) rd.push_back(pick(12) - 1);
      for (int k = pick(3); k > 0; --k) wr.push_back(pick(12) - 1);
      s.add(std::move(ops), rd, wr);
    }
    const int cap = pick(2) ? 1 << 30 : 64 + pick(512);
    const auto p = s.run(cap);
    bool ok = true;
    for (const Placed& x : p) ok = ok && x.level >= 0 && x.pos >= 0 && x.pos < Prog::max_ops && x.wg_begin >= 0;
    const auto succ = s.pg.successors();
    for (size_t i = 0; i < succ.size(); ++i)
      for (int j : succ[i]) ok = ok && s.pg.items[i].level < s.pg.items[j].level;
    CHECK(ok);
  }
  for (int r = 0; r < rounds; ++r) {
    const int nops = 1 + pick(6), n = pick(30);
    std::vector<int> item((size_t)nops);
    for (int& i : item) i = pick(4);
    std::vector<HazardRec> recs;
    for (int k = 0; k < n; ++k) {
      const uintptr_t lo = 0x1000 + 16 * (uintptr_t)pick(64);
      recs.push_back({lo, lo + 16 * (uintptr_t)(1 + pick(8)), pick(4) == 0, pick(nops)});
    }
    bool brute = false;
    for (int a = 0; a < n; ++a)
      for (int b = a + 1; b < n; ++b)
        brute = brute || (recs[a].lo < recs[b].hi && recs[b].lo < recs[a].hi && (recs[a].w || recs[b].w) &&
                          recs[a].op != recs[b].op && item[recs[a].op] != item[recs[b].op]);
    const auto hit = hazard_scan(recs, item);
    CHECK((hit.first >= 0) == brute);
    if (hit.first >= 0) {
      const HazardRec &x = recs[hit.first], &y = recs[hit.second];
      CHECK(x.lo < y.hi && y.lo < x.hi && (x.w || y.w) && item[x.op] != item[y.op]);
    }
  }
}

int main() {
  scheduler_cases();
  scan_cases();
  random_cases(1, 2000);
  std::thread a(random_cases, 2, 500), b(random_cases, 3, 500);  // (re-entrancy: nothing shared between calls)
  a.join();
  b.join();
  std::printf("plan-check: %d checks, %d failed: %s\n", g_checks.load(), g_failed.load(), g_failed ? "FAILED" : "ok");
  return g_failed ? 1 : 0;
}
