// Host side of the MI355X off-policy update engine: device memory, the
// per-agent step programs (built as op DAGs), hipGraph capture and the C ABI
// declared in include/rle.h.
//
// A step program is written in the reference's order (td7.py:287-332,
// td3.py:206-242, sac.py:251-295) as a list of ops with read/write resource
// sets.  `Prog::schedule` (plan.cpp) assigns every op the lowest dependency
// level that respects RAW, WAR and WAW hazards; each level becomes one launch
// of the device dispatch kernel, and the whole step is captured into a hipGraph.
//
// The planner -- struct Prog and its scheduler, the GEMM layout checks and gemm_finalize, the RLE_AUDIT
// address replay, the RLE_HAZARD level check and the RLE_TRAFFIC model -- lives in plan.cpp / plan.h and makes
// no HIP call; Engine::prog_options is the one place that hands it its knobs and switches.
// How a captured program reaches the device -- its launch list, the AQL queue (aql_open, aql_submit,
// aql_wait_step, ...) and struct Graph -- lives in dispatch.cpp / dispatch.h; Error, HIPCHK, REQUIRE and
// the kernel launchers' prototypes in host.h.
// The replay buffer and its entries: replay.cpp / replay.h; device and pinned memory: memory.h; what the files that
// define extern "C" entries share: abi.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "abi.h"
#include "dispatch.h"
#include "plan.h"

namespace rle {
thread_local std::string g_err;  // (abi.h: one per thread for the whole library)

static int host_fkey(float f) {
  int i;
  std::memcpy(&i, &f, 4);
  return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
static float host_unkey(int k) {
  int i = k >= 0 ? k : k ^ 0x7FFFFFFF;
  float f;
  std::memcpy(&f, &i, 4);
  return f;
}

// ------------------------------------------------------------------ programs

// A tensor of the step program: fragment images (ops.h "tensor images") for
// anything a GEMM touches, or a plain vector for 1-column tensors outside GEMMs.
struct View {
  Mat m{};                      // images (m.n / m.t may be null)
  float* p = nullptr;           // plain vector data (1-column tensors), else null
  int rows = 0, cols = 0;       // rows (16-multiple for images), padded columns
  int id = -1;
  const float* norm = nullptr;  // AvgL1Norm partials (producer |x| column-tile sums)
  int norm_ld = 0, norm_row0 = 0, nparts = 0, width = 0, norm_id = -1;
  // EPI_NBDOT output (the gradient g of an AvgL1Norm output whose backward is deferred
  // into the consuming DW, kDwNb): row partials of sum_j g x
  const float* nbdot = nullptr;
  int nbdot_ld = 0, nbdot_n = 0, nbdot_id = -1;
  // EPI_QDOT output: row partials [qd_n][qd_ld] of sum_j y_j w_j (a critic's q before its bias)
  const float* qd = nullptr;
  int qd_ld = 0, qd_n = 0, qd_id = -1;
  View sub(int r0, int n) const {
    View v = *this;
    if (m.n || m.t) {
      if (r0 % 16) throw Error{RLE_EINVAL, "sub-view of an image must start at a 16-row boundary"};
      if (m.n) v.m.n = m.n + (size_t)(r0 / 16) * m.cbn * 256;
      if (m.t) v.m.t = m.t + (size_t)(r0 / 16) * 256;
    }
    if (p) v.p = p + r0;
    v.rows = n;
    v.norm_row0 += r0;
    return v;
  }
  NormRef nref() const {
    NormRef r{};
    if (norm) {
      r.part = norm;
      r.ld = norm_ld;
      r.row0 = norm_row0;
      r.nparts = nparts;
      r.width = width;
    }
    return r;
  }
};

// GEMM tile width: the narrowest tile (more workgroups, reduction split across the
// 4 waves) while the output has at most 640 16x16 blocks per width step.
static int pick_tn(int M, int N) {
  const int blocks = cdiv(M, 16) * cdiv(N, 16);
  if (blocks <= 640) return 16;
  if (blocks <= 1280) return 32;
  return 64;
}

struct Layer {
  std::string wname, bname;
  int out = 0, K = 0;
  std::vector<int> seg_w, seg_p;  // logical / padded widths of input segments
  int rb = 0, cb = 0;             // 16-blocks of out rows / K columns
  size_t wn_off = 0, wt_off = 0, b_off = 0;  // N image, T image, bias [16 rb]
  int res = -1;
};

struct Net {
  std::string name, kind;  // kind: sale_enc / sale_actor / sale_critic / mlp
  std::vector<Layer> layers;
  size_t off = 0, size = 0;
  int res = -1;  // whole-net resource (polyak / copy)
};

enum Res : int {
  R_CNT = 1,
  R_VKEYS,
  R_VT,
  R_INFO,
  R_LA,
  R_PRIO,
  R_MAXP,
  R_REPLAY,
  R_ADAMSC,  // Ctrl::adam_step / adam_bc2s (Adam bias corrections of this step)
  R_ADAMSC1, // their copy for steps on batch set 1 (two steps in one graph: g_pair)
  R_FIRST_DYNAMIC = 100,
};

// The planner's knobs of a resolved plan (no field "default"); the diagnostic switches stay off.
static PlanOptions plan_knobs(const rle_plan& plan) {
  PlanOptions o;
  o.balance = plan.balance;  // (rle_plan balance, A/B)
  // measured on MI355X (tools/abk.sh, RLE_BALANCE 0/1/2/3): TD3 HalfCheetah 15481/16050/15911/
  // 15637, SAC Humanoid 7674/8025/7997/7801, TD7 Humanoid 6532/6478/6498/6517 steps/s (round 1);
  // TD7 after the guarded operand rings: 7744/7774/7720/7754 (4-step graphs), and 6-step
  // graphs with mode 1: 7822 (tools/abenv.sh)
  o.tiny_w = plan.tiny_w;
  o.uni_w = plan.uni_w;
  o.tiny_wg = plan.tiny_wg;
  o.pl_w = plan.pl_w;
  o.lap_w = plan.lap_w;
  o.head_w = plan.head_w;
  o.adam_w = plan.adam_w;
  o.lpt = plan.lpt;
  o.rb = plan.rb;
  o.xcd = plan.xcd;
  return o;
}

// The default plan: every field "default" (resolved per engine by Engine::resolve_plan).
static rle_plan plan_defaults() {
  rle_plan p{};
  p.steps_per_graph = -1;
  p.balance = -1;
  p.tiny_w = p.uni_w = p.tiny_wg = -1;
  p.rb = -1;
  p.pl_w = -1;
  p.lap_w = p.head_w = p.adam_w = -1;
  p.wide = -1;
  p.lpt = -1;
  p.dispatch = p.dpf = p.xcd = -1;
  return p;
}

// The engine's stream, destroyed with the holder (Engine's member block says why its place matters).
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  operator hipStream_t() const { return s; }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

struct Engine {
  rle_config cfg;
  rle_plan plan = plan_defaults();  // (resolved: no field left "default")
  // Defaults of the fields left at "default" for this engine's algorithm (rle.h rle_plan).
  // The extended kernel instance runs this engine's programs when its plan uses what only that
  // instance compiles: register-blocked weight-gradient tiles, the fused priority sampler.
  // the rle_level instance this engine's programs run on (ops.h KernelSet): the agent's own set, or the
  // extended instance when the plan asks for its opt-in paths
  int kernel_set() const {
    // (LayerNorm critics: OP_LN / OP_LN_BWD are KS_LN's alone; it holds KS_CLIP's code, so they compose with
    // clipping, every activation and both offline modes)
    // (n-step returns: the sampler's multi-hop gather is KS_NSTEP's alone -- KS_DROP's code with it, so every
    // setting below composes with it: LnArgs p == 0, no OP_LN and no OP_CLIP run on it as on their own instances)
    if (n_step > 1) return KS_NSTEP;
    // (critic dropout: the row ops' dropout path is KS_DROP's alone -- KS_LN's code with it)
    if (ln_on() && drop_p > 0.f) return KS_DROP;
    if (ln_on()) return KS_LN;
    // (gradient clipping: EPI_GSQ, the scaled Adam pass over normed operands and OP_CLIP are KS_CLIP's alone; it
    // holds KS_ACT's code, so every activation and offline mode clips)
    if (clip_on()) return KS_CLIP;
    // (LeakyReLU / SiLU / GELU: the ELU variants' second dispatch is KS_ACT's alone, ops.h act_vslot)
    if (std::max({actP, actC, actE}) > ACT_TANH) return KS_ACT;
    if (!acts_default) return KS_EXT;  // (the activation variants outside the agent's own set)
    // (offline TD3: OP_BC modes 2 / 3, the kDwGs variant, the |min| slot and the info kinds are the extended
    // instance's alone, so the TD3 / SAC instance is byte for byte what the online programs ran on before)
    if (offline3()) return KS_EXT;
    if (offline_sac()) return KS_EXT;  // (OP_AWAC is the extended instance's alone, for the same reason)
    if (algo == RLE_TD7 && plan.wide && !(plan.fuse_on & RLE_FUSE_PRIOSAMPLE)) return KS_TD7W;  // (rb compiled in)
    if (plan.rb || (plan.fuse_on & RLE_FUSE_PRIOSAMPLE) || plan.wide) return KS_EXT;
    return algo == RLE_TD7 ? KS_TD7 : KS_MLP;
  }
  // Gradient clipping (rle_set_grad_clip): 0 = off.  clip_buf: per optimizer (0 critics, 1 policy, 2 TD7 encoder)
  // {total, coef, the Adam passes' scalar, -}, written by OP_CLIP; clip_id: their scheduler resources.
  float clip_max = 0.f;
  float* clip_buf = nullptr;
  int clip_id[3] = {-1, -1, -1};
  bool clip_on() const { return clip_max > 0.f; }
  // LayerNorm critics (rle_set_layer_norm): parameter-free LayerNorm, eps 1e-5, after every hidden Linear of q1, q2
  // and their targets, before the activation (TD3 / SAC)
  bool ln_critic = false;
  bool ln_on() const { return ln_critic; }
  // Critic dropout (rle_set_critic_dropout): inverted dropout on every hidden Linear's output of the critics, ahead
  // of the LayerNorm, inside OP_LN / OP_LN_BWD (ops.h LnArgs p).  0: off.  Needs ln_on().  A pass of a gradient step
  // hands its number to the row ops (drop_site); rle_eval hands none and runs without dropout.
  float drop_p = 0.f;
  enum DropPass : int { DROP_TARGET = 0, DROP_ONLINE = 1, DROP_POLICY = 2, DROP_AWAC_DATA = 3, DROP_NONE = -1 };
  static int drop_site(int pass, int twin, int layer) { return (pass * 2 + twin) * 8 + layer; }
  // n-step returns (rle_set_n_step): the sampler's gather walks up to n_step rows from the sampled slot and hands the
  // step the n-step reward, the last hop's next_state and gamma^(hops-1) notdone in the batch's one-step places
  // (ops.h SampleArgs), so no op downstream changes.  1: off.  TD3 / SAC.  hops: per batch set, the rows' hop
  // counts for the info row's replay/hops (allocated by the setter: n_step == 1 allocates nothing).
  int n_step = 1;
  void ensure_hops() {
    for (BatchSet& b : bsets)
      if (!b.hops.p) b.hops = vec(B);
    use_set(0);
  }
  void resolve_plan() {
    if (plan.steps_per_graph < 0) plan.steps_per_graph = algo == RLE_TD3 ? 16 : algo == RLE_SAC ? 8 : 6;
    // (SAC's target critics' raw-head pre-GEMM consumers: 32 measured +1.0% over 64, 2 pairs)
    if (plan.pre_tn == 0) plan.pre_tn = algo == RLE_TD3 ? 64 : 32;
    plan.pre_tn = plan.pre_tn == 32 || plan.pre_tn == 64 ? plan.pre_tn : 16;
    // (SAC pl_tn 32: its 64-workgroup actor-DX pre-layer level; with uni_w 30, A/B 2 pairs: 14.40k -> 14.55k;
    // TD3 32: -5%)
    if (plan.pl_tn == 0) plan.pl_tn = algo == RLE_SAC ? 32 : 64;
    plan.pl_tn = plan.pl_tn == 16 || plan.pl_tn == 32 ? plan.pl_tn : 64;
    plan.tn_min = plan.tn_min == 32 || plan.tn_min == 64 ? plan.tn_min : 16;
    if (plan.flat_div <= 0) plan.flat_div = 4;
    // (TD7: mode 3, no Adam items moved and only under a twice-longer op -- interleaved A/B, 4 pairs: TD7 Humanoid
    // 8,295-8,306 -> 8,328-8,341 steps/s, Ant +0.1%, B = 1024 +-0; TD3 -5%, SAC -2% at 3, so they keep 1;
    // profiles/r06_ab_balance.txt)
    // (SAC: mode 2, 4 pairs 14.75k -> 14.78k, profiles/r06_ab_plan_mlp.txt; TD3 keeps 1)
    if (plan.balance < 0) plan.balance = algo == RLE_TD7 ? 3 : algo == RLE_SAC ? 2 : 1;
    if (plan.tiny_w < 0) plan.tiny_w = 30;
    // (uniform sampler weight, A/B 2 pairs, SAC Humanoid uni_w 60 / 45 / 30 / 15 -> 14.10k / 14.13k / 14.40k /
    // 14.39k; TD3 HalfCheetah 60 / 30 / 20 / 15 / 8 / 1 -> 25.40k / 25.42k / 25.30k / 25.81k / 25.84k / 25.76k: a
    // lighter sampler is moved off the level it would bound)
    if (plan.uni_w < 0) plan.uni_w = algo == RLE_SAC ? 30 : algo == RLE_TD3 ? 8 : 60;
    if (plan.tiny_wg < 0) plan.tiny_wg = 2;
    plan.sched_cap = plan.sched_cap ? 1 : 0;
    // (64-row LDS-staged tiles: the 16-row tiles' per-workgroup fixed cost and 2 KB of operand loads per 4
    // MFMAs bound the B >= 512 levels, DESIGN round 5; with them the register-blocked weight-gradient tiles, the
    // batch split over the 4 waves, where a 16 x 64 weight-gradient tile's waves would each reduce all B rows)
    if (plan.wide < 0) plan.wide = 0;  // (opt-in: slower at B = 1024 than the 16-row tiles, DESIGN round 5)
    // (longest first: interleaved A/B on the round-6 tree, TD7 Humanoid +0.5% (4 pairs), Ant +1.1%, B = 1024 +0.2%,
    // TD3 HalfCheetah +1.9%, SAC Humanoid +0.9%; profiles/r06_ab_lpt.txt.  Round 5 measured it at +-0)
    if (plan.lpt < 0) plan.lpt = 1;
    plan.lpt = plan.lpt ? 1 : 0;
    plan.rb = plan.rb < 0 ? (plan.wide ? 1 : 0) : (plan.rb ? 1 : 0);
    // (A/B, 2 pairs: SAC Humanoid pl_w 0 / 8 / 16 / 24 -> 14.09k / 14.09k / 14.11k / 14.15k; TD3 HalfCheetah
    // 25.37k / 25.33k / 25.38k / 25.36k)
    if (plan.pl_w < 0) plan.pl_w = algo == RLE_SAC ? 24 : 0;
    if (plan.lap_w < 0) plan.lap_w = 60;
    if (plan.head_w < 0) plan.head_w = 60;
    // (A/B 2 pairs, SAC Humanoid adam_w 0 / 8 / 12 / 16 / 24 / 32 -> 14.38k / 14.56k / 14.67k / 14.67k / 14.64k /
    // 14.67k; TD3 HalfCheetah 0 / 8 / 16 -> 25.81k / 25.84k / 25.00k; TD7 Humanoid 0 / 8 / 16 -> 8.17k / 8.25k /
    // 8.24k, B = 1024 flat: profiles/r04_ab_weights.txt)
    if (plan.adam_w < 0) plan.adam_w = algo == RLE_SAC ? 16 : 8;
    if (plan.level_cap < 0) plan.level_cap = 0;
    plan.wide = plan.wide == 32 || plan.wide == 0 ? plan.wide : 64;  // (the tile width; 1 = 64)
    plan.dispatch = plan.dispatch < 0 ? 1 : std::min(plan.dispatch, 2);
    plan.dpf = plan.dpf < 0 ? 1 : (plan.dpf ? 1 : 0);
    plan.xcd = plan.xcd < 0 ? 1 : (plan.xcd ? 1 : 0);
  }
  int S, Sp, A, Ap, H, Hp, B;
  int Bv = 0;  // batch rows (rle_config.batch, any 1..1024); B = Bv padded to 16: the padded rows are zero and
               // every mean, loss, priority and value bound counts the Bv batch rows only
  int Z = 0, Zp = 0;    // TD7: SALE embedding width zs_dim (sale.py:23), padded
  std::vector<int> HS;  // TD3 / SAC: hidden widths of make_mlp (mlp.py:10-35), input side first
  // hidden activations (ops.h Act) of the actor, the critics and TD7's encoders (rle_config act_*)
  int actP = ACT_RELU, actC = ACT_ELU, actE = ACT_ELU;
  bool acts_default = true;
  // The derivative source of a hidden activation for an input-gradient GEMM: ELU' = exp(z), and LeakyReLU', SiLU',
  // GELU' likewise (ops.h act_zsaved), read the pre-activation z (as autograd's backward does), ReLU' the output,
  // identity none.
  static const View* dsrc_of(int act, const View& y, const View& z) {
    return act_zsaved(act) ? &z : act == ACT_RELU ? &y : nullptr;
  }
  int algo;
  // What the engine owns.  THE ORDER OF THESE FOUR, AND THAT EVERY PROGRAM IS DECLARED AFTER THEM, IS LOAD-BEARING:
  // members are destroyed in reverse order of declaration, after ~Engine() has (1) drained the AQL burst, ignoring a
  // closed queue, (2) synchronised the stream, (3) unbound from the replay and (4) destroyed done_ev.  Then (5) the
  // captured programs (every Graph member and map of programs below) release their graph execs and graphs, (6) the
  // stream is destroyed, (7) then aql, pin and, last of all, the device memory every program and buffer points into.
  DevMem mem;
  PinMem pin;
  std::unique_ptr<AqlQueue> aql;  // (rle_plan dispatch 1) direct dispatch of the step graphs
  Stream stream;
  ~Engine() {
    try {
      aql_drain();
    } catch (const Error&) {  // (a timed-out burst closed the engine's queue: destroy anyway)
    }
    (void)hipStreamSynchronize(stream);
    if (replay) replay->remove_user(this);
    if (done_ev) (void)hipEventDestroy(done_ev);
  }
  float* P = nullptr;
  size_t nP = 0;
  std::vector<Net> nets;
  Ctrl* ctrl = nullptr;
  float* info = nullptr;
  int info_cap = 4096;
  std::vector<float> info_host;
  Replay* replay = nullptr;
  hipEvent_t done_ev = nullptr;  // recorded after every enqueued step (Replay::users)
  int next_id = R_FIRST_DYNAMIC;
  // Graphs per batch-buffer parity p: g_prime[p] samples batch p (draws of the next
  // step); g_pol[p] / g_pln[p] run a (policy / plain) step on batch p and, once its
  // priority update is done, prefetch the next step's batch into 1 - p.
  Graph g_prime[2], g_pol[2], g_pln[2], g_hard;
  Graph g_slot0;  // info slot := 0 as a level of its own (rle_step_async bursts on the AQL queue)
  // g_pair[p]: multi_k consecutive steps as ONE program, starting on batch p (policy,
  // plain, policy, ... with policy_freq 2; SAC: every step), so the scheduler overlaps
  // each step's early levels (encoder phase, fixed encoders, online critic forward) with
  // the previous step's policy-phase tail and last Adam level.  Steps on the two batch
  // sets keep their own Adam scalars (asc_set) so only true data dependencies order them.
  Graph g_pair[2];
  int multi_k = 0;
  // g_rem[r][p]: kRemK[r] steps as one program (a burst's tail shorter than multi_k: the driver's 20-step bench
  // burst is 3 x 6 + 2), built when kRemK[r] < multi_k
  static constexpr int kRemK[2] = {4, 2};
  Graph g_rem[2][2];
  int asc_set = 0;
  float* adamsc1 = nullptr;  // [step[4], bc2s[4]] of steps built on set 1
  float* adam_step_of(int set) { return set ? adamsc1 : ctrl->adam_step; }
  float* adam_bc2s_of(int set) { return set ? adamsc1 + 4 : ctrl->adam_bc2s; }
  // (diagnostics: the parity that last ran; with policy_freq 2 policy and plain steps
  // alternate, so each kind always runs on the same parity)
  int pol_set = 0, pln_set = 0;
  const Graph& policy_graph() const { return g_pol[pol_set]; }
  const Graph& plain_graph() const { return algo == RLE_SAC ? g_pol[pol_set] : g_pln[pln_set]; }  // SAC: every step
  // rle_graph_describe / rle_graph_trace `which`: 0 policy, 1 plain, 3 the multi-step program, else the hard update
  const Graph& graph_by(int which) const {
    return which == 0 ? policy_graph() : which == 1 ? plain_graph() : which == 3 ? g_pair[pol_set] : g_hard;
  }
  bool built = false;
  long long n_runs = 0;  // host mirror of the agent's step counter
  int cur_set = 0, last_set = 0;       // batch the next step runs on / the last step ran on
  bool primed = false;                 // batch cur_set holds the next step's draws
  unsigned long long primed_ver = 0;   // replay version it was drawn under
  // step buffers: two batch sets (the running step's and the prefetched next one)
  struct BatchSet {
    View ss, act_in, rw, nd, eps, eps2;
    View hops;  // (n-step returns only: ensure_hops)
    long long* ind = nullptr;
    float* u_buf = nullptr;
    int ind_id = -1;
  };
  BatchSet bsets[2];
  View ss, act_in, rw, nd, eps, eps2;  // the set a program is being built on (use_set)
  View hops;
  long long* ind = nullptr;
  float* u_buf = nullptr;
  double* bsum = nullptr;
  void use_set(int k) {
    const BatchSet& b = bsets[k];
    ss = b.ss;
    act_in = b.act_in;
    rw = b.rw;
    nd = b.nd;
    eps = b.eps;
    eps2 = b.eps2;
    hops = b.hops;
    ind = b.ind;
    u_buf = b.u_buf;
    ind_id = b.ind_id;
  }
  // tapes
  float *t_u = nullptr, *t_eps = nullptr, *t_eps2 = nullptr;
  long long* t_ind = nullptr;
  long long tape_cap = 0, tape_left = 0;
  // act programs (cached per n)
  std::map<int, std::pair<Graph, View>> act_graphs;  // n -> graph, output view
  std::map<int, View> act_inputs;
  // act-sample programs (rle_act_sample): environment action straight into pinned memory
  struct ActSample {
    Graph G;
    View in;
    float* img = nullptr;  // pinned staging of the input image (N image, M rows)
    int* ctl = nullptr;    // pinned: mode, Philox counter lo / hi
    float* eps = nullptr;  // pinned [n][A] noise tape
    float* out = nullptr;  // pinned [n][A] actions
  };
  std::map<int, ActSample> act_samplers;
  // B = 1 act chain (one launch, in-kernel hand-offs): built on first use when it fits
  bool chain_tried = false, chain_ok = false;
  ActChainArgs chain{};
  unsigned chain_tag = 0;
  volatile unsigned* done_host = nullptr;  // pinned [64]: head workgroups' completion tags
  float* act_map = nullptr;  // [scale A | bias A | exploration_noise] (rle_set_action_map)
  unsigned long long act_counter = 0;  // Philox counter of the exploration draws
  // The rle_act_chain program of this engine's actor (ops.h ActChainArgs), or false when it does
  // not fit (observation wider than 384, hidden wider than 256, LDS).
  bool build_chain(const ActArgs& ao) {
    ActChainArgs& c = chain;
    c = ActChainArgs{};
    if (Sp > 384) return false;
    auto layer = [&](const Layer& L, int act, int in0, int in1, int norm, int dst, int sync) {
      ActLayer& x = c.L[c.nl++];
      x.wn = P + L.wn_off;
      x.bias = P + L.b_off;
      x.cbn = L.cb;
      x.rbs = L.rb;
      x.out = L.out;
      x.act = act;
      x.in0 = in0;
      x.in1 = in1;
      x.k0 = L.seg_p.empty() ? 0 : L.seg_p[0];
      x.norm = norm;
      x.dst = dst;
      x.sync = sync;
      return L.K <= kActVec || in1 >= 0;
    };
    bool ok = true;
    if (algo == RLE_TD7) {  // td7.py:158-162: zs = fixed_encoder(s); policy(s, zs)
      Net& fe = net("fixed_encoder");
      Net& pi = net("policy");
      ok &= layer(fe.layers[0], actE, 0, -1, 0, 1, 0);
      ok &= layer(pi.layers[0], ACT_NONE, 0, -1, 1, 2, 1);
      ok &= layer(fe.layers[1], actE, 1, -1, 0, 3, 1);
      ok &= layer(fe.layers[2], ACT_NONE, 3, -1, 1, 4, 1);
      ok &= layer(pi.layers[1], actP, 2, 4, 0, 5, 1);
      ok &= layer(pi.layers[2], actP, 5, -1, 0, 6, 1);
      ok &= layer(pi.layers[3], ACT_TANH, 6, -1, 0, 7, 0);
    } else {  // mlp.py:55-68
      Net& pi = net("policy");
      const int D = (int)HS.size();  // (hidden layer i -> slot i + 1; the output -> slot 7)
      for (int i = 0; i < D; ++i) ok &= layer(pi.layers[i], actP, i, -1, 0, i + 1, 1);
      ok &= layer(pi.layers[D], algo == RLE_SAC ? ACT_NONE : ACT_TANH, D, -1, 0, 7, 0);
      c.sac = algo == RLE_SAC;
    }
    c.nwg = 1;
    for (int l = 0; l < c.nl; ++l) {
      ok &= c.L[l].out <= kActVec && c.L[l].cbn <= 32;  // (kernels.hip act_load: <= 8 blocks per lane)
    ok &= A <= 32;  // ActChainArgs::eps, one output per thread
      if (l < c.nl - 1) c.nwg = std::max(c.nwg, c.L[l].rbs);
    }
    c.heads = c.sac ? 1 : c.L[c.nl - 1].rbs;
    ok &= c.heads <= c.nwg;
    for (int l = 0; l < c.nl - 1; ++l) ok &= c.L[l].rbs == c.nwg;  // (every workgroup in every hidden layer)
    if (!ok) return false;
    c.Sp = Sp;
    c.xbuf = mem.make<unsigned long long>((size_t)kActMaxL * kActVec);
    c.err = const_cast<int*>(ao.ctl) + 8;  // pinned (ActSample::ctl[8], [9]): read by the host directly
    done_host = (volatile unsigned*)pin.alloc(64 * sizeof(unsigned));
    HIPCHK(hipHostGetDevicePointer((void**)&c.done, (void*)done_host, 0));
    c.ao = ao;
    c.min_log_std = cfg.min_log_std;
    c.max_log_std = cfg.max_log_std;
    const char* fw = std::getenv("RLE_ACT_FAIL_WG");  // failure-path test, first call only
    c.fail_wg = fw ? std::atoi(fw) : -1;
    return true;
  }
  void ensure_action_map() {  // default: identity map, exploration_noise 0.1 (td7.py:41, td3.py:40)
    if (act_map) return;
    std::vector<float> m((size_t)2 * A + 1, 0.f);
    for (int j = 0; j < A; ++j) m[j] = 1.f;
    m[2 * A] = 0.1f;
    act_map = mem.make<float>(m.size());
    HIPCHK(hipMemcpy(act_map, m.data(), m.size() * 4, hipMemcpyHostToDevice));
  }

  // ---------------------------------------------------------------- params
  Net& net(const std::string& name) {
    for (auto& n : nets)
      if (n.name == name) return n;
    throw Error{RLE_EINVAL, "unknown net '" + name + "'"};
  }

  void add_layer(Net& n, const std::string& pre, int out, std::vector<int> segw) {
    Layer L;
    L.wname = pre + ".weight";
    L.bname = pre + ".bias";
    L.out = out;
    L.seg_w = segw;
    // every input segment padded to 16 so a 16-wide reduction chunk never straddles two
    for (int w : segw) L.seg_p.push_back(r16(w));
    L.K = 0;
    for (int p : L.seg_p) L.K += p;
    L.res = next_id++;
    n.layers.push_back(L);
  }

  Net make_net(const std::string& name, const std::string& kind) {
    Net n;
    n.name = name;
    n.kind = kind;
    n.res = next_id++;
    if (kind == "sale_enc") {  // rl/nn/sale.py:16-55 (zs_dim Z, hdim H)
      add_layer(n, "zs1", H, {S});
      add_layer(n, "zs2", H, {H});
      add_layer(n, "zs3", Z, {H});
      add_layer(n, "zsa1", H, {Z, A});
      add_layer(n, "zsa2", H, {H});
      add_layer(n, "zsa3", Z, {H});
    } else if (kind == "sale_actor") {  // sale.py:58-83
      add_layer(n, "l0", H, {S});
      add_layer(n, "l1", H, {H, Z});
      add_layer(n, "l2", H, {H});
      add_layer(n, "l3", A, {H});
    } else if (kind == "sale_critic") {  // sale.py:86-121
      add_layer(n, "q01", H, {S, A});
      add_layer(n, "q1", H, {H, Z, Z});
      add_layer(n, "q2", H, {H});
      add_layer(n, "q3", 1, {H});
    } else {  // mlp_actor (mlp.py:38-55) / mlp_critic (mlp.py:75-101): Linear / ReLU pairs, nn.Sequential
      // indices 0, 2, 4, ... (make_mlp, mlp.py:24-35)
      const bool actor = kind == "mlp_actor";
      const int D = (int)HS.size();
      for (int i = 0; i <= D; ++i) {
        const int out = i < D ? HS[i] : !actor ? 1 : algo == RLE_SAC ? 2 * A : A;
        std::vector<int> in{i ? HS[i - 1] : S};
        if (!i && !actor) in.push_back(A);
        add_layer(n, "mlp." + std::to_string(2 * i), out, in);
      }
    }
    return n;
  }

  // Per layer: weight N image | weight T image | bias (padded to 16 rows); the
  // Adam m / v arenas mirror the layout at +nP / +2nP (m, v live at the T offsets).
  void layout_params() {
    size_t off = 0;
    for (auto& n : nets) {
      n.off = off;
      for (auto& L : n.layers) {
        L.rb = cdiv(L.out, 16);
        L.cb = L.K / 16;
        const size_t img = (size_t)L.rb * L.cb * 256;
        L.wn_off = off;
        L.wt_off = off + img;
        L.b_off = off + 2 * img;
        off += 2 * img + (size_t)L.rb * 16;
      }
      n.size = off - n.off;
    }
    nP = off + 4;  // + SAC log_alpha slot
    P = mem.make<float>(3 * nP);  // params | m | v
  }

  Mat wmat(const Layer& L, int which = 0) {
    Mat m{};
    m.n = P + (size_t)which * nP + L.wn_off;
    m.t = P + (size_t)which * nP + L.wt_off;
    m.cbn = L.cb;
    m.rbs = L.rb;
    return m;
  }
  float* bias(const Layer& L) { return P + L.b_off; }

  static size_t h_nidx(int cbn, int r, int c) {
    return ((size_t)(r >> 4) * cbn + (c >> 4)) * 256 + ((c >> 2) & 3) * 64 + (r & 15) * 4 + (c & 3);
  }
  static size_t h_tidx(int rbs, int r, int c) {
    return ((size_t)(c >> 4) * rbs + (r >> 4)) * 256 + ((r >> 2) & 3) * 64 + (c & 15) * 4 + (r & 3);
  }

  // locate (net, torch param name) -> (layer, is_bias)
  std::pair<Layer*, bool> find_param(const std::string& netn, const std::string& name) {
    Net& n = net(netn);
    for (auto& L : n.layers) {
      if (L.wname == name) return {&L, false};
      if (L.bname == name) return {&L, true};
    }
    throw Error{RLE_EINVAL, "unknown param '" + netn + "." + name + "'"};
  }

  long long numel(const std::string& netn, const std::string& name) {
    if (netn == "tmp") return 1;
    auto pr = find_param(netn, name);
    const Layer& L = *pr.first;
    if (pr.second) return L.out;
    long long k = 0;
    for (int w : L.seg_w) k += w;
    return (long long)L.out * k;
  }

  // copy between logical [out][sum seg_w] host layout and padded device layout
  void xfer_param(const std::string& netn, const std::string& name, float* host, long long n, bool to_dev,
                  int which) {
    REQUIRE(n == numel(netn, name), "size mismatch for " + netn + "." + name);
    const size_t base = (size_t)which * nP;
    HIPCHK(hipStreamSynchronize(stream));
    if (to_dev) fold_dirty = true;
    if (netn == "tmp") {
      float* d = P + base + (nP - 4);
      if (to_dev) HIPCHK(hipMemcpy(d, host, 4, hipMemcpyHostToDevice));
      else HIPCHK(hipMemcpy(host, d, 4, hipMemcpyDeviceToHost));
      return;
    }
    auto pr = find_param(netn, name);
    const Layer& L = *pr.first;
    if (pr.second) {
      float* d = P + base + L.b_off;
      if (to_dev) HIPCHK(hipMemcpy(d, host, sizeof(float) * L.out, hipMemcpyHostToDevice));
      else HIPCHK(hipMemcpy(host, d, sizeof(float) * L.out, hipMemcpyDeviceToHost));
      return;
    }
    // weights: both images written from the logical [out][sum seg_w] array (params);
    // read back from the T image (Adam m / v live only there)
    const size_t img = (size_t)L.rb * L.cb * 256;
    std::vector<float> tim(img, 0.f), nim(img, 0.f);
    float* dt = P + base + L.wt_off;
    float* dn = P + base + L.wn_off;
    int klog = 0;
    for (int w : L.seg_w) klog += w;
    if (!to_dev) HIPCHK(hipMemcpy(tim.data(), dt, img * 4, hipMemcpyDeviceToHost));
    for (int o = 0; o < L.out; ++o) {
      int lc = 0, pc = 0;
      for (size_t s = 0; s < L.seg_w.size(); ++s) {
        for (int c = 0; c < L.seg_w[s]; ++c) {
          float& hv = host[(size_t)o * klog + lc + c];
          const size_t ti = h_tidx(L.rb, o, pc + c);
          if (to_dev) {
            tim[ti] = hv;
            nim[h_nidx(L.cb, o, pc + c)] = hv;
          } else {
            hv = tim[ti];
          }
        }
        lc += L.seg_w[s];
        pc += L.seg_p[s];
      }
    }
    if (to_dev) {
      HIPCHK(hipMemcpy(dt, tim.data(), img * 4, hipMemcpyHostToDevice));
      if (which == 0) HIPCHK(hipMemcpy(dn, nim.data(), img * 4, hipMemcpyHostToDevice));
    }
  }

  // ---------------------------------------------------------------- packed state (rle_state_*)
  // Table of contents of the packed state of a mask of RLE_STATE_* (rle.h), and the tables the pack kernels
  // run from (ops.h StateDesc / StateTile), built once per mask from nets / Layer.  Host only until
  // state_io_init uploads them.
  struct StateToc {
    std::vector<rle_state_entry> entries;
    std::vector<StateDesc> desc;
    std::vector<StateTile> tiles;
    long long total = 0;  // floats of the packed state
    StateDesc* d_desc = nullptr;
    StateTile* d_tiles = nullptr;
  };
  std::map<int, StateToc> state_tocs;
  float* state_dev = nullptr;   // packed image of the full mask (device / pinned)
  float* state_host = nullptr;
  static bool has_optimizer(const std::string& n) { return n == "policy" || n == "q1" || n == "q2" || n == "encoder"; }

  StateToc& state_toc(int what) {
    REQUIRE(what > 0 && what <= RLE_STATE_ALL, "state: `what` must be a non-empty mask of RLE_STATE_PARAMS / _ADAM_M / _ADAM_V");
    auto it = state_tocs.find(what);
    if (it != state_tocs.end()) return it->second;
    StateToc t;
    auto add = [&](const std::string& netn, const std::string& name, int arena, StateDesc d, long long numel) {
      rle_state_entry en{};
      std::snprintf(en.net, sizeof en.net, "%s", netn.c_str());
      std::snprintf(en.name, sizeof en.name, "%s", name.c_str());
      en.arena = arena;
      en.offset = t.total;
      en.numel = numel;
      d.p_off = t.total;
      const size_t img = d.kind ? (size_t)d.n_img : (size_t)d.rb * d.cb * 256;
      REQUIRE((size_t)d.wt_off + img <= 3 * nP && (d.wn_off < 0 || (size_t)d.wn_off + img <= 3 * nP),
              "state: a tensor image outside the parameter arenas");
      const int nt = d.kind ? 1 : d.rb * cdiv(d.cb * 16, kStateCols);
      for (int s = 0; s < nt; ++s) t.tiles.push_back({(int)t.desc.size(), s});
      t.desc.push_back(d);
      t.entries.push_back(en);
      t.total += numel;
    };
    for (int arena = 0; arena < 3; ++arena) {
      if (!((what >> arena) & 1)) continue;
      const long long base = (long long)arena * (long long)nP;
      for (const Net& n : nets) {
        if (arena && !has_optimizer(n.name)) continue;
        for (const Layer& L : n.layers) {
          REQUIRE(L.seg_w.size() <= (size_t)kStateSegs, "state: a layer with more input segments than the pack kernels take");
          StateDesc w{};
          w.kind = 0;
          w.wt_off = base + (long long)L.wt_off;
          w.wn_off = arena == 0 ? (long long)L.wn_off : -1;  // (Adam m / v live at the T offsets only)
          w.rb = L.rb;
          w.cb = L.cb;
          w.out = L.out;
          w.nseg = (int)L.seg_w.size();
          for (int s = 0; s < w.nseg; ++s) {
            w.seg_w[s] = L.seg_w[s];
            w.seg_p[s] = L.seg_p[s];
            w.klog += L.seg_w[s];
          }
          add(n.name, L.wname, arena, w, (long long)L.out * w.klog);
          StateDesc b{};
          b.kind = 1;
          b.wt_off = base + (long long)L.b_off;
          b.wn_off = -1;
          b.out = L.out;
          b.n_img = 16 * L.rb;
          add(n.name, L.bname, arena, b, L.out);
        }
      }
      if (algo == RLE_SAC) {  // the log_alpha slot: one float
        StateDesc a{};
        a.kind = 1;
        a.wt_off = base + (long long)(nP - 4);
        a.wn_off = -1;
        a.out = a.n_img = 1;
        add("tmp", "log_alpha", arena, a, 1);
      }
    }
    return state_tocs.emplace(what, std::move(t)).first->second;
  }

  // the mask's tables on the device, and the staging images (sized once, for the full mask)
  void state_io_init(StateToc& t) {
    if (!state_dev) {
      const size_t n = (size_t)state_toc(RLE_STATE_ALL).total;
      state_dev = mem.make<float>(n);
      state_host = static_cast<float*>(pin.alloc(n * sizeof(float)));
    }
    if (t.d_desc) return;
    t.d_desc = mem.make<StateDesc>(t.desc.size());
    t.d_tiles = mem.make<StateTile>(t.tiles.size());
    HIPCHK(hipMemcpy(t.d_desc, t.desc.data(), t.desc.size() * sizeof(StateDesc), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t.d_tiles, t.tiles.data(), t.tiles.size() * sizeof(StateTile), hipMemcpyHostToDevice));
  }
  StatePackArgs state_args(const StateToc& t) const {
    StatePackArgs a{};
    a.P = P;
    a.packed = state_dev;
    a.desc = t.d_desc;
    a.tiles = t.d_tiles;
    a.ntiles = (int)t.tiles.size();
    return a;
  }
  // the same networks, layer by layer (the parameter layout depends on nothing else)
  bool same_shapes(const Engine& o) const {
    if (algo != o.algo || nP != o.nP || nets.size() != o.nets.size()) return false;
    for (size_t i = 0; i < nets.size(); ++i) {
      if (nets[i].name != o.nets[i].name || nets[i].layers.size() != o.nets[i].layers.size()) return false;
      for (size_t l = 0; l < nets[i].layers.size(); ++l) {
        const Layer &a = nets[i].layers[l], &b = o.nets[i].layers[l];
        if (a.wname != b.wname || a.out != b.out || a.seg_w != b.seg_w || a.wt_off != b.wt_off) return false;
      }
    }
    return true;
  }

  // ---------------------------------------------------------------- buffers
  // Zero-initialised tensor images (rows and columns padded to 16; padding stays
  // zero, which the GEMM reduction relies on), or a dense vector.
  View buf(int rows, int cols, bool want_n = true, bool want_t = true) {
    View v;
    v.rows = r16(rows);
    v.cols = r16(cols);
    const size_t img = (size_t)v.rows * v.cols;
    v.m.cbn = v.cols / 16;
    v.m.rbs = v.rows / 16;
    if (want_n) v.m.n = mem.make<float>(img);
    if (want_t) v.m.t = mem.make<float>(img);
    v.rows = rows;
    v.id = next_id++;
    return v;
  }
  View vec(int rows) {
    View v;
    v.rows = rows;
    v.cols = 1;
    v.p = mem.make<float>((size_t)rows + 4);
    v.id = next_id++;
    return v;
  }

  // ---------------------------------------------------------------- op builders
  // Operand segments: N image (x = tensor rows, reduction along columns) or
  // T image (x = tensor columns, reduction along rows).
  static Seg seg_n(const View& v, int r0, int r1) {
    Seg s{};
    s.p = v.m.n;
    s.xs = v.m.cbn;
    s.x0 = 0;
    s.x1 = v.rows;
    s.r0 = r0;
    s.r1 = r1;
    s.norm = v.nref();
    return s;
  }
  static Seg seg_t(const View& v, int x0, int r0, int r1) {
    Seg s{};
    s.p = v.m.t;
    s.xs = v.m.rbs;
    s.x0 = x0;
    s.x1 = x0 + v.cols;
    s.r0 = r0;
    s.r1 = r1;
    s.norm = v.nref();
    return s;
  }

  // Y = act(X W^T + b) over concatenated input segments (each a list of row pieces).
  // The GEMM kernel wants every A segment to span the op's whole row range, so
  // row pieces split the op into one sub-op per row range (same level, disjoint
  // output rows).
  // A weight block for fwd(): N image of a [out][segment width] matrix (a column block
  // of a layer's weights, or a folded product) and the resource it belongs to.
  struct WSeg {
    const float* p;
    int xs, res;
  };
  // A layer's whole weight matrix as a forward GEMM's B operand (N image)
  Seg wseg_n(const Layer& L) const {
    Seg w{};
    w.p = P + L.wn_off;
    w.xs = L.cb;
    w.x1 = L.out;
    w.r1 = L.K;
    return w;
  }
  WSeg wblock(const Layer& L, int col0) const {
    return {P + L.wn_off + (size_t)(col0 / 16) * 256, L.cb, L.res};
  }
  // Columns [col0, col0 + width) of a layer's weights as a GEMM A operand (N image).
  View wview_n(const Layer& L, int col0, int width) const {
    View v;
    v.m.n = P + L.wn_off + (size_t)(col0 / 16) * 256;
    v.m.cbn = L.cb;
    v.m.rbs = L.rb;
    v.rows = L.out;
    v.cols = r16(width);
    v.id = L.res;
    return v;
  }

  struct DxTerm {
    View dz;
    const Layer* L;  // weights of a layer (T image) ...
    int col0;
    const View* wv = nullptr;  // ... or of a derived [out][in] matrix (T image) when L is null
  };
  // W[:, col0 : col0 + ncols] of an input-gradient term through the T image, its rows at reduction offset roff
  Seg wseg_t(const DxTerm& tm, int ncols, int roff) const {
    Seg b{};
    if (tm.L) {
      b.p = P + tm.L->wt_off + (size_t)(tm.col0 / 16) * tm.L->rb * 256;
      b.xs = tm.L->rb;
    } else {
      b.p = tm.wv->m.t + (size_t)(tm.col0 / 16) * tm.wv->m.rbs * 256;
      b.xs = tm.wv->m.rbs;
    }
    b.x1 = ncols;
    b.r0 = roff;
    b.r1 = roff + (tm.L ? tm.L->out : tm.wv->rows);
    return b;
  }

  // A pre-GEMM (PreArgs) and the resources it reads, for fwd() / dx(): the consumer's A segment
  // a.seg is computed in-tile, so the view passed for that segment only gives its layout.
  struct PreUse {
    PreArgs a;
    std::vector<int> rd;
    int kind = 1;  // GemmArgs::has_pre: 1 pre-GEMM (actor output layer), 3 pre-layer, 4 pre-layer behind a2
    PreArgs a2{};  // (kind 4) the pre-GEMM computing the pre-layer's input segment a2.seg
  };
  // The critic loss head fused into the DX of critic n's last hidden layer (GemmArgs::has_pre 2)
  struct HeadUse {
    HeadArgs h;
    int n;
    std::vector<int> rd, wr;  // the head's resources (beyond the DX's own)
  };
  // The SAC actor rsample (OP_SAC_ACTOR) as the epilogue of its raw head GEMM (EPI_SACFWD)
  struct SacFwdUse {
    SacFwdArgs a;
    std::vector<int> rd, wr;
  };
  // The SAC actor backward (OP_SAC_ACTOR_BWD) as the epilogue of the DX producing da (EPI_SACBWD)
  struct SacBwdUse {
    SacBwdArgs a;
    std::vector<int> rd, wr;
  };
  // The actor's tanh output layer L over rows x (+ target smoothing noise) as a pre-GEMM
  // (sale.py:77-83 / mlp.py:55-62, td7.py:188-194, td3.py:154-158).
  PreUse pre_actor_fwd(const Layer& L, const View& x, const View* noise, int seg) {
    REQUIRE(L.out <= 32 && L.seg_p.size() == 1 && x.m.n && !x.norm, "pre: actor output layer operands");
    PreUse u{};
    PreArgs& p = u.a;
    p.mode = GEMM_FWD;
    p.A.seg[0] = seg_n(x, 0, L.K);
    p.A.nseg = 1;
    p.B.seg[0] = wseg_n(L);
    p.B.nseg = 1;
    p.N = L.out;
    p.R = L.K;
    p.seg = seg;
    p.bias = bias(L);
    u.rd = {x.id, L.res};
    if (noise) {
      p.noise = noise->m;
      p.noise_sigma = cfg.target_policy_noise;
      p.noise_clip = cfg.noise_clip;
      u.rd.push_back(noise->id);
    }
    return u;
  }
  // SAC's raw head L over rows x, then the target rsample a' = tanh(mean + exp(clamp(log_std)) eps)
  // (sac.py:132-152), as a pre-GEMM of the target critics' first layer (GemmArgs::has_pre 5): the target
  // branch does not wait a level for the standalone EPI_SACFWD op, which still runs for the policy rows,
  // log pi and the backward.  Both reduce the raw head in one order (kernels.hip sacraw_*).
  PreUse pre_sac_fwd(const Layer& L, const View& x, const View& eps, int seg) {
    REQUIRE(L.out == 2 * A && L.out <= 48 && L.K <= 256 && L.seg_p.size() == 1 && x.m.n && !x.norm && eps.m.t,
            "pre: SAC raw head operands");
    PreUse u{};
    u.kind = 5;
    PreArgs& p = u.a;
    p.mode = GEMM_FWD;
    p.A.seg[0] = seg_n(x, 0, L.K);
    p.A.nseg = 1;
    p.B.seg[0] = wseg_n(L);
    p.B.nseg = 1;
    p.N = L.out;
    p.R = L.K;
    p.seg = seg;
    p.sac_a = A;
    p.bias = bias(L);
    p.noise = eps.m;
    p.noise_sigma = cfg.min_log_std;
    p.noise_clip = cfg.max_log_std;
    u.rd = {x.id, L.res, eps.id};
    return u;
  }
  bool sac_pre() const { return fused(RLE_FUSE_SACPRE) && sac_fwd_fused() && 2 * A <= 48 && H <= 256; }
  // A small-K first layer L0 (ReLU, K <= 48: TD3 / SAC on low-dimensional observations) over the
  // input segments xs, recomputed in-tile by the layer after it (prelayer_fwd): one level fewer on
  // the critic and actor chains.  The standalone L0 output stays for its other readers (the
  // weight gradient, the ReLU mask of the input gradient).  RLE_NO_PRELAYER=1: off (tests, A/B).
  // minimum tile width of a pre-GEMM consumer: each tile recomputes the actor output layer for its
  // 16 rows, so wider tiles cut that redundant work (A/B, RLE_PRE_TN 16 / 32 / 64: TD3 HalfCheetah
  // 23.37k / 23.79k / 23.91k, TD7 Humanoid 8069 / 8094 / 8060 steps/s)
  int pre_tn() const { return plan.pre_tn; }
  int pl_tn() const { return plan.pl_tn; }
  // (fusions whose in-tile recomputations are compiled for the default activations only; the q-dot partials and the
  // loss head fused into the DX also for ReLU / ELU critics -- the extended instance holds both -- not for identity)
  static constexpr unsigned kActFusions = RLE_FUSE_PRELAYER | RLE_FUSE_PRE | RLE_FUSE_TWOSTAGE | RLE_FUSE_SACPRE;
  static constexpr unsigned kCriticActFusions = RLE_FUSE_QDOT | RLE_FUSE_HEADDX;
  bool fused(unsigned bit) const {
    // (clipped programs: the AvgL1Norm backward stays an op of its own, so kDwNb needs no norm-pass and no scaled form)
    if (clip_on() && (bit & RLE_FUSE_NBDEFER)) return false;
    // (LayerNorm critics: the rule of the non-default activations, wholesale -- no in-tile recomputation of a
    // layer, no q-dot partials, no head inside an input gradient; the norm sits between a Linear and its consumers)
    if (ln_on() && (bit & (kActFusions | kCriticActFusions))) return false;
    if (!acts_default && (bit & kActFusions)) return false;
    if (!acts_default && actC == ACT_NONE && (bit & kCriticActFusions)) return false;
    return (bit & RLE_FUSE_OPT_IN) ? (plan.fuse_on & bit) != 0 : !(plan.fuse_off & bit);
  }
  bool prelayer_shape(const Layer& L0, const Layer& L1) const {
    return L0.K <= 48 && L0.out <= 256 && L0.out % 16 == 0 && L1.seg_p.size() == 1 && L1.seg_p[0] == L0.out;
  }
  bool prelayer_ok(const Layer& L0, const Layer& L1) const {
    return fused(RLE_FUSE_PRELAYER) && prelayer_shape(L0, L1);
  }
  bool prelayer_ok_dx(const Layer& L, const Layer& Lprev) const {
    return fused(RLE_FUSE_PRELAYER) && r16(L.out) <= 48 && L.K <= 256 && L.K % 16 == 0 && Lprev.out == L.K &&
           Lprev.out <= 256;
  }
  // (lds_seg >= 0: input segment lds_seg is computed in-tile by a pre-GEMM -- its view gives the layout)
  PreUse pre_layer(const Layer& L0, const std::vector<View>& xs, int lds_seg = -1) {
    REQUIRE(xs.size() == L0.seg_p.size() && L0.K <= 48, "pre-layer: operands");
    PreUse u{};
    u.kind = 3;
    PreArgs& p = u.a;
    p.mode = GEMM_FWD;
    int koff = 0;
    for (size_t q = 0; q < xs.size(); ++q) {
      REQUIRE(xs[q].m.n && xs[q].cols == L0.seg_p[q] && !xs[q].norm, "pre-layer: input segment");
      p.A.seg[q] = seg_n(xs[q], koff, koff + L0.seg_p[q]);
      koff += L0.seg_p[q];
      if ((int)q != lds_seg) u.rd.push_back(xs[q].id);
    }
    p.A.nseg = (int)xs.size();
    p.B.seg[0] = wseg_n(L0);
    p.B.nseg = 1;
    p.N = L0.out;
    p.R = L0.K;
    p.seg = 0;
    p.act = ACT_RELU;
    p.bias = bias(L0);
    u.rd.push_back(L0.res);
    return u;
  }
  // The input gradient through layer L (small fan-out: L.out <= 48, e.g. SAC's raw head 2 x action
  // dims) masked by act'(saved), dZ W * act'(saved), recomputed in-tile by the input-gradient GEMM of
  // the layer before (prelayer_fwd, GEMM_DX).  The standalone op stays for the weight gradient.
  PreUse pre_layer_dx(const Layer& L, const View& dz, const View& saved) {
    REQUIRE(r16(L.out) <= 48 && dz.m.n && dz.cols == r16(L.out) && saved.m.t && L.K <= 256, "pre-layer dx: operands");
    PreUse u{};
    u.kind = 3;
    PreArgs& p = u.a;
    p.mode = GEMM_DX;
    p.A.seg[0] = seg_n(dz, 0, L.out);
    p.A.nseg = 1;
    Seg b{};
    b.p = P + L.wt_off;
    b.xs = L.rb;
    b.x1 = L.K;
    b.r1 = L.out;
    p.B.seg[0] = b;
    p.B.nseg = 1;
    p.N = L.K;
    p.R = r16(L.out);
    p.seg = 0;
    p.act = ACT_RELU;
    p.dsrc = saved.m;
    u.rd = {dz.id, L.res, saved.id};
    return u;
  }
  // The gradient wrt the actor's tanh input, sum_t dZ_t W_t[:, col0_t ..] * (1 - a^2), as a
  // pre-GEMM (the DX op dx(terms, ncols, ..., ACT_TANH, &a) would compute).
  PreUse pre_actor_dx(const std::vector<DxTerm>& terms, int ncols, const View& a, int seg) {
    REQUIRE(ncols <= 32 && a.m.t && (int)terms.size() <= kMaxSeg, "pre: actor output gradient operands");
    PreUse u{};
    PreArgs& p = u.a;
    p.mode = GEMM_DX;
    int roff = 0;
    for (size_t t = 0; t < terms.size(); ++t) {
      const DxTerm& tm = terms[t];
      REQUIRE(tm.dz.m.n && tm.col0 % 16 == 0 && (tm.L || (tm.wv && tm.wv->m.t)), "pre: dx term layout");
      const int wout = tm.L ? tm.L->out : tm.wv->rows;
      p.A.seg[t] = seg_n(tm.dz, roff, roff + wout);
      p.B.seg[t] = wseg_t(tm, ncols, roff);
      roff += r16(wout);
      u.rd.push_back(tm.dz.id);
      u.rd.push_back(tm.L ? tm.L->res : tm.wv->id);
    }
    p.A.nseg = p.B.nseg = (int)terms.size();
    p.N = ncols;
    p.R = roff;
    p.seg = seg;
    REQUIRE(a.m.t, "pre: the saved tanh output needs a T image");
    p.dsrc = a.m;
    u.rd.push_back(a.id);
    return u;
  }

  // Partial sums that an info-row entry (or a later op) reduces: the floats, how many, and the resource that
  // orders their readers after the producer
  struct LossPart {
    float* p = nullptr;
    int n = 0, id = -1;
  };

  // Per-call options of the op builders below.  The default value is a plain layer: its output in both images,
  // tiles as the planner picks them.  A call names what it uses (a null operand leaves that feature off), and a
  // run of layers built alike shares one const value, so no option outlives the calls it is meant for.
  struct FwdOpt {
    View* pre_out = nullptr;  // keep the pre-activation: T image (DX epilogue masks); N (pre_n) only where the
    bool pre_n = false;       // loss head reads the rows -- 4 scattered stores per lane saved everywhere else
    bool normed = false;      // AvgL1Norm row partials with the output (consumers apply the norm)
    const View* noise = nullptr;  // clipped target-policy noise on the rows from noise_row0 on
    int noise_row0 = 0;
    const std::vector<WSeg>* wsegs = nullptr;  // one weight block per input segment instead of L's matrix
    const View* bias_ovr = nullptr;
    const PreUse* pre = nullptr;    // an input segment computed in-tile (pre-GEMM / pre-layer)
    const Layer* qdot = nullptr;    // EPI_QDOT: row partials of this H -> 1 layer applied to the output
    const SacFwdUse* sfu = nullptr;  // EPI_SACFWD: SAC's rsample in the raw head's epilogue
    // The output's T image is the weight gradients' B operand: forward-only layers (fixed and target networks,
    // the policy pass through the critics) drop it -- one store per lane and the written-back bytes of each
    // such layer saved
    bool t = true;
    // This layer is also recomputed in-tile by a pre-layer consumer: at most 32-wide tiles keep its reduction
    // split, so the stored output (the ReLU mask of the input gradient, the weight gradient's operand) is the
    // same floats as the consumer's copy, whatever the planner widens
    bool pl_src = false;
    // EPI_MSE: the output is the gradient of mse_scale * sum (y - AvgL1Norm(mse_tgt))^2 over the batch rows; the
    // per-tile loss partials are allocated here and returned in *loss
    const View* mse_tgt = nullptr;
    float mse_scale = 0.f;
    // EPI_QHEAD: the output is dZ of this layer under a constant dL/dq = qhead_dq through the H -> 1 layer qhead;
    // per-tile sums of Q - b (+ B b on tile 0) into the caller's slot loss->p, resource loss->id
    const Layer* qhead = nullptr;
    float qhead_dq = 0.f;
    LossPart* loss = nullptr;  // (both: loss->n = the tiles written, one loss partial per 16-row block)
    FwdOpt() {}  // (user-provided, here and below: a default argument inside Engine cannot use the implicit one)
    FwdOpt& keep_pre(View* z, bool n_image = false) { return pre_out = z, pre_n = n_image, *this; }
    FwdOpt& norm() { return normed = true, *this; }
    FwdOpt& noised(const View* e, int row0) { return noise = e, noise_row0 = row0, *this; }
    FwdOpt& wblocks(const std::vector<WSeg>* w, const View* b) { return wsegs = w, bias_ovr = b, *this; }
    FwdOpt& pre_gemm(const PreUse* p) { return pre = p, *this; }
    FwdOpt& q_dot(const Layer* l) { return qdot = l, *this; }
    FwdOpt& sac_fwd(const SacFwdUse* s) { return sfu = s, *this; }
    FwdOpt& keep_t(bool on) { return t = on, *this; }
    FwdOpt& no_t() { return keep_t(false); }
    FwdOpt& pl_source(bool on) { return pl_src = on, *this; }
    FwdOpt& mse(const View* tgt, float scale, LossPart* out) { return mse_tgt = tgt, mse_scale = scale, loss = out, *this; }
    FwdOpt& q_head(const Layer* l, float dq, LossPart* slot) { return qhead = l, qhead_dq = dq, loss = slot, *this; }
  };
  struct DxOpt {
    const View* into = nullptr;    // the output view (default: a new buffer)
    const View* nb_x = nullptr;    // EPI_NBDOT: the output is g of AvgL1Norm(nb_x), its backward deferred to the DW
    const PreUse* pre = nullptr;   // a dZ segment computed in-tile
    const HeadUse* head = nullptr;  // the loss head fused in: A segment 0 is z, not dZ
    const SacBwdUse* sbu = nullptr;  // EPI_SACBWD: SAC's actor backward as the epilogue
    // Output images: N for the next input gradient / norm backward, T for the weight gradient.  An output
    // that only one kind of consumer reads drops the other (its stores and written-back bytes saved).
    bool n = true, t = true;
    bool pl_src = false;  // as FwdOpt::pl_src: the pre-layer consumer is the input gradient of the layer before
    DxOpt() {}
    DxOpt& out_into(const View* v) { return into = v, *this; }
    DxOpt& nb_defer(const View* x) { return nb_x = x, *this; }
    DxOpt& pre_gemm(const PreUse* p) { return pre = p, *this; }
    DxOpt& head_use(const HeadUse* h) { return head = h, *this; }
    DxOpt& sac_bwd(const SacBwdUse* s) { return sbu = s, *this; }
    DxOpt& images(bool n_image, bool t_image) { return n = n_image, t = t_image, *this; }
    DxOpt& no_t() { return t = false, *this; }
    DxOpt& pl_source(bool on) { return pl_src = on, *this; }
  };
  // One clipped optimizer update of a step: the per-tile partials its norm passes fill ([0, n): `used` of them
  // handed out, the rest stay zero), the resources they write, and the Adam passes waiting for OP_CLIP.
  struct ClipGroup {
    int opt = 0;             // 0 critics, 1 policy, 2 TD7 encoder (clip_buf / rle_grad_clip_stats order)
    float* part = nullptr;
    int n = 0, used = 0;
    std::vector<int> part_ids;
    const float* gin = nullptr;  // offline TD3's actor: lmbda, in the norm passes and in OP_CLIP's scalar
    int gin_id = -1;
    struct Pending {
      Op op;
      std::vector<int> rd, wr;
    };
    std::vector<Pending> adam;
  };
  // (null with clipping off: the builders then emit the unclipped program op for op)
  ClipGroup clip_group(int opt, const std::vector<const Layer*>& layers, float* part = nullptr) {
    ClipGroup c;
    c.opt = opt;
    for (const Layer* L : layers) c.n += dw_gsq_w(*L) + dw_gsq_b(*L);
    c.part = part ? part : mem.make<float>((size_t)c.n);
    return c;
  }
  void clip_close(Prog& pg, ClipGroup& c) {
    REQUIRE(clip_on() && !c.adam.empty() && c.used <= c.n, "clip_close: an empty or overfull clip group");
    Op op{};
    op.kind = OP_CLIP;
    op.wg_count = 1;
    ClipArgs& a = op.clip;
    a.part = c.part;
    a.n = c.n;
    a.max_norm = clip_max;
    a.gin = c.gin;
    a.out = clip_buf + 4 * c.opt;
    a.scale = clip_buf + 4 * c.opt + 2;
    std::vector<int> rd = c.part_ids;
    if (c.gin) rd.push_back(c.gin_id);
    pg.add(op, rd, {clip_id[c.opt]});
    for (ClipGroup::Pending& p : c.adam) pg.add(p.op, p.rd, p.wr);
    c.adam.clear();
  }
  struct DwOpt {
    float* gsq = nullptr;    // per-tile grad-square partials of the weights / the bias (dw_gsq_w / dw_gsq_b slots)
    float* gsq_b = nullptr;
    const View* nb_x = nullptr;  // kDwNb: dZ is the AvgL1Norm backward of (dz = g, nb_x), applied on load
    // (TD3 policy steps) tau of the self-aliased target-policy Polyak fused into the Adam epilogue
    // (AdamArgs::ptau), 0 elsewhere
    float ptau = 0.f;
    // (offline TD3 policy steps, kDwGs) lmbda, which the Adam epilogue multiplies the gradient by
    // (GemmArgs::gscale; OP_BC mode 3, or mode 2 behind the standalone head, writes it), and its resource
    const float* gscale = nullptr;
    int gscale_id = -1;
    DwOpt() {}
    DwOpt& gsq_parts(const std::pair<float*, float*>& p) { return gsq = p.first, gsq_b = p.second, *this; }
    DwOpt& nb_defer(const View* x) { return nb_x = x, *this; }
    DwOpt& polyak(float tau) { return ptau = tau, *this; }
    DwOpt& grad_scale(const float* s, int id) { return gscale = s, gscale_id = id, *this; }
    // (gradient clipping) the optimizer's clip group: dw() emits the norm pass and leaves the Adam pass with the
    // group, which clip_close() emits behind the group's OP_CLIP
    ClipGroup* clip = nullptr;
    DwOpt& clip_in(ClipGroup* g) { return clip = g, *this; }
  };
  // The row-norm ops of the LayerNorm critics (ln_fwd / ln_bwd).  Default: a forward-only layer -- the output in its
  // N image alone, nothing kept for a backward.
  struct LnOpt {
    bool t = false;          // the output's T image too (a weight gradient reads it)
    View* u = nullptr;       // ln_fwd: keep the normalised rows (N image) and their rstd ([rows]) for ln_bwd
    View* rstd = nullptr;
    LnOpt() {}
    LnOpt& keep_t(bool on) { return t = on, *this; }
    LnOpt& keep_bwd(View* u_out, View* rstd_out) { return u = u_out, rstd = rstd_out, *this; }
    // critic dropout on the op's rows: probability p (0: none) at mask site `site` (drop_site)
    float p = 0.f;
    int site = 0;
    LnOpt& drop(float p_, int site_) { return p = p_, site = site_, *this; }
  };
  struct NormBwdOpt {
    bool n = true, t = true;  // output images, as DxOpt's
    NormBwdOpt() {}
    NormBwdOpt& no_t() { return t = false, *this; }
  };

  // The tile plan of a forward or input-gradient GEMM, in one place for fwd() and dx().
  // 64-row LDS-staged tiles (rle_plan wide; returns the tile width, 0 = off): a plain op (no in-tile prologue,
  // fused head or row-wise epilogue), every row piece whole 64-row blocks, whole tile columns
  int wide_tiles(bool plain, int N, const std::vector<int>& cuts) const {
    bool wide = plan.wide && plain && N % plan.wide == 0;
    for (size_t ci = 0; wide && ci + 1 < cuts.size(); ++ci) wide = (cuts[ci + 1] - cuts[ci]) % 64 == 0;
    return wide ? plan.wide : 0;
  }
  // Tiles and workgroups of an M x N output in tn-wide tiles (wide: 64 rows per workgroup instead of 16)
  static void set_tiles(Op& op, int M, int N, int tn, int wide) {
    GemmArgs& g = op.gemm;
    g.tn = wide ? wide : tn;
    g.hot.wide = wide;
    g.tiles_m = cdiv(M, kTileM);
    g.tiles_n = cdiv(N, g.tn);
    op.wg_count = (wide ? g.tiles_m / 4 : g.tiles_m) * g.tiles_n;
  }

  View fwd(Prog& pg, const Layer& L, const std::vector<std::vector<View>>& ins, int M, int act, const FwdOpt& o = {}) {
    REQUIRE(ins.size() == L.seg_p.size(), "fwd: input segment count mismatch for " + L.wname);
    REQUIRE(M % kTileM == 0, "fwd: rows must be a multiple of 16");
    REQUIRE(!o.wsegs || o.wsegs->size() == ins.size(), "fwd: one weight block per input segment");
    std::vector<int> rd{L.res}, wr;
    if (o.wsegs)
      for (const WSeg& w : *o.wsegs) rd.push_back(w.res);
    if (o.bias_ovr) rd.push_back(o.bias_ovr->id);
    std::vector<int> cuts{0, M};
    for (size_t s = 0; s < ins.size(); ++s) {
      int xo = 0;
      for (const View& v : ins[s]) {
        REQUIRE(v.cols == L.seg_p[s] && v.m.n, "fwd: segment width / image mismatch for " + L.wname);
        xo += v.rows;
        if (xo < M) cuts.push_back(xo);
        if (o.pre && (int)s == o.pre->a.seg) continue;  // computed in-tile
        rd.push_back(v.id);
        if (v.norm) rd.push_back(v.norm_id);
      }
      REQUIRE(xo >= M, "fwd: input rows < M");
    }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    REQUIRE((int)ins.size() <= kMaxSeg, "fwd: too many operand segments");
    if (o.pre) {
      REQUIRE(cuts.size() == 2 && !o.noise, "fwd: a pre-GEMM consumer is one row piece");
      rd.insert(rd.end(), o.pre->rd.begin(), o.pre->rd.end());
    }
    const auto tq = choose_tn(M, L.out);
    // (EPI_SACFWD: one tile column holds whole rows; a pre-layer consumer recomputes the first layer
    // per tile, so wider tiles cut that redundant work: RLE_PL_TN, default 64)
    // (a pre-GEMM consumer that is also a pre-layer source: at most 32 wide, as any FwdOpt::pl_src)
    const int tn = o.sfu ? 64
                       : (o.pre && (o.pre->kind == 3 || o.pre->kind == 4) ? std::max(tq.first, pl_tn())
                          : o.pre && (o.pre->kind == 1 || o.pre->kind == 5)
                              ? (o.pl_src ? std::min(std::max(tq.first, pre_tn()), 32) : std::max(tq.first, pre_tn()))
                                                  : (o.pl_src ? std::min(tq.first, 32) : tq.first));
    const int wide = wide_tiles(!o.sfu && !o.pre && !o.noise, L.out, cuts);
    const int tiles_n = cdiv(L.out, wide ? wide : tn);
    View out = buf(M, L.out, true, o.t);
    if (o.sfu) {
      REQUIRE(!o.pre && !o.qdot && !o.normed && !o.noise && act == ACT_NONE && L.out <= 64, "fwd: SAC forward epilogue");
      rd.insert(rd.end(), o.sfu->rd.begin(), o.sfu->rd.end());
      wr.insert(wr.end(), o.sfu->wr.begin(), o.sfu->wr.end());
    }
    wr.push_back(out.id);
    if (o.pre_out) {
      *o.pre_out = buf(M, L.out, o.pre_n, true);
      wr.push_back(o.pre_out->id);
    }
    float* part = nullptr;
    if (o.normed) {
      part = mem.make<float>((size_t)tiles_n * M);
      out.norm = part;
      out.norm_ld = M;
      out.norm_row0 = 0;
      out.nparts = tiles_n;
      out.width = L.out;
      out.norm_id = next_id++;
      wr.push_back(out.norm_id);
    }
    float* qpart = nullptr;
    if (o.qdot) {  // EPI_QDOT: row partials of the H -> 1 layer qdot applied to this output
      // (qdot->K is the padded width: the kernel zeroes the weights of the columns past L.out, j < N)
      REQUIRE(!o.normed && o.qdot->out == 1 && o.qdot->K == r16(L.out) &&
                  (act_zsaved(act) || act == ACT_RELU || act == ACT_NONE),
              "fwd: q-dot partial layout");
      qpart = mem.make<float>((size_t)tiles_n * M);
      out.qd = qpart;
      out.qd_ld = M;
      out.qd_n = tiles_n;
      out.qd_id = next_id++;
      wr.push_back(out.qd_id);
      rd.push_back(o.qdot->res);
    }
    if (o.loss) {  // EPI_MSE / EPI_QHEAD: one row piece, per-tile loss partials
      REQUIRE(cuts.size() == 2 && !o.sfu && !o.pre && !o.qdot && !o.normed && !o.noise && !o.pre_out &&
                  !o.mse_tgt != !o.qhead,
              "fwd: a loss epilogue is a plain one-piece layer");
      o.loss->n = cdiv(M, kTileM) * tiles_n;  // (wide: one loss partial per 16-row block too)
      if (o.mse_tgt) {
        o.loss->p = mem.make<float>(o.loss->n);
        o.loss->id = next_id++;
        rd.insert(rd.end(), {o.mse_tgt->id, o.mse_tgt->norm_id});
      } else {
        REQUIRE(L.seg_p.size() == 1 && ins[0][0].cols == L.seg_p[0] && ins[0][0].m.n && o.qhead->out == 1,
                "qhead: operand layout");
        rd.push_back(o.qhead->res);
      }
      wr.push_back(o.loss->id);
    }
    if (o.noise) rd.push_back(o.noise->id);
    std::vector<Op> ops;
    for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
      const int ra = cuts[ci], rb = cuts[ci + 1], m = rb - ra;
      REQUIRE(ra % kTileM == 0, "fwd: row pieces must be 16-aligned");
      Op op{};
      op.kind = OP_GEMM;
      GemmArgs& g = op.gemm;
      g.mode = GEMM_FWD;
      int koff = 0;
      for (size_t s = 0; s < ins.size(); ++s) {
        int xo = 0;
        for (const View& v : ins[s]) {
          if (ra >= xo && ra < xo + v.rows) {
            g.A.seg[s] = seg_n(v.sub(ra - xo, m), koff, koff + L.seg_p[s]);
            break;
          }
          xo += v.rows;
        }
        koff += L.seg_p[s];
      }
      g.A.nseg = (int)ins.size();
      if (!o.wsegs) {
        g.B.seg[0] = wseg_n(L);
        g.B.nseg = 1;
      } else {  // one weight block per input segment, paired like a DX operand
        for (size_t q = 0; q < ins.size(); ++q) {
          Seg w{};
          w.p = (*o.wsegs)[q].p;
          w.xs = (*o.wsegs)[q].xs;
          w.x0 = 0;
          w.x1 = L.out;
          w.r0 = g.A.seg[q].r0;
          w.r1 = g.A.seg[q].r1;
          g.B.seg[q] = w;
        }
        g.B.nseg = (int)ins.size();
      }
      g.M = m;
      g.N = L.out;
      g.R = L.K;
      set_tiles(op, m, L.out, tn, wide);
      g.epi = EPI_STORE;
      g.act = act;
      g.out = out.sub(ra, m).m;
      g.bias = o.bias_ovr ? o.bias_ovr->p : bias(L);
      if (o.pre_out) g.pre = o.pre_out->sub(ra, m).m;
      if (o.normed) {
        g.norm_out = part + ra;
        g.norm_ld = M;
      }
      if (o.sfu) {
        REQUIRE(cuts.size() == 2, "fwd: SAC forward epilogue over one row piece");
        g.epi = EPI_SACFWD;
        g.sf = o.sfu->a;
      }
      if (o.qdot) {
        g.epi = EPI_QDOT;
        g.qw = P + o.qdot->wn_off;
        g.qw_cbn = o.qdot->cb;
        g.norm_out = qpart + ra;
        g.norm_ld = M;
      }
      if (o.loss) {
        g.loss_part = o.loss->p;
        g.mvalid = Bv;
      }
      if (o.mse_tgt) {
        g.epi = EPI_MSE;
        g.tgt = o.mse_tgt->m;
        g.tgt_norm = o.mse_tgt->nref();
        g.mse_scale = o.mse_scale;
      }
      if (o.qhead) {
        g.epi = EPI_QHEAD;
        g.qw = P + o.qhead->wn_off;
        g.qw_cbn = o.qhead->cb;
        g.qb = bias(*o.qhead);
        g.qscale = o.qhead_dq;
      }
      if (o.noise && rb > o.noise_row0) {
        const int first = std::max(ra, o.noise_row0);  // first noised row (global)
        g.noise = o.noise->sub(first - o.noise_row0, rb - first).m;
        g.noise_row0 = first - ra;
        g.noise_sigma = cfg.target_policy_noise;
        g.noise_clip = cfg.noise_clip;
      }
      if (o.pre) {
        g.has_pre = o.pre->kind;
        g.prea = o.pre->a;
        if (o.pre->kind == 4) g.prea2 = o.pre->a2;
      }
      op.seq = tq.second;
      ops.push_back(op);
    }
    pg.add_group(std::move(ops), rd, wr);
    return out;
  }

  // dX[:, 0:ncols] = sum_t dZ_t W_t[:, col0_t : col0_t + ncols]  (* act'(saved))
  View dx(Prog& pg, const std::vector<DxTerm>& terms, int ncols, int M, int dact, const View* saved,
          const DxOpt& o = {}) {
    if (dact == ACT_NONE && !o.pre && !o.head) saved = nullptr;  // (an identity layer's backward reads no derivative)
    Op op{};
    op.kind = OP_GEMM;
    GemmArgs& g = op.gemm;
    g.mode = GEMM_DX;
    std::vector<int> rd, wr;
    REQUIRE((int)terms.size() <= kMaxSeg, "dx: too many terms");
    int roff = 0;
    for (size_t t = 0; t < terms.size(); ++t) {
      const DxTerm& tm = terms[t];
      REQUIRE(tm.dz.m.n && tm.col0 % 16 == 0 && (tm.L || (tm.wv && tm.wv->m.t)), "dx: operand layout");
      const int wout = tm.L ? tm.L->out : tm.wv->rows;
      g.A.seg[t] = seg_n(tm.dz, roff, roff + wout);
      g.B.seg[t] = wseg_t(tm, ncols, roff);
      roff += r16(wout);
      if (!(o.pre && (int)t == o.pre->a.seg)) rd.push_back(tm.dz.id);  // (else computed in-tile)
      rd.push_back(tm.L ? tm.L->res : tm.wv->id);
    }
    g.A.nseg = g.B.nseg = (int)terms.size();
    g.M = M;
    g.N = ncols;
    g.R = roff;
    const auto tq = choose_tn(M, ncols);
    const int tn = o.pre && o.pre->kind == 3 ? std::max(tq.first, pl_tn())
                   : o.pre && o.pre->kind == 1 ? std::max(tq.first, pre_tn())
                                           : (o.pl_src ? std::min(tq.first, 32) : tq.first);
    op.seq = tq.second;
    // (wide: a plain or EPI_NBDOT input gradient)
    set_tiles(op, M, ncols, tn, wide_tiles(!o.pre && !o.head && !o.sbu, ncols, {0, M}));
    g.epi = EPI_STORE;
    g.act = ACT_NONE;
    View out = o.into ? *o.into : buf(M, ncols, o.n, o.t);
    if (o.nb_x) {  // out = g of AvgL1Norm(x): row partials of sum_j g x for the consuming DW (kDwNb)
      REQUIRE(!saved && o.nb_x->norm && o.nb_x->m.t && o.nb_x->rows == M && o.nb_x->cols == r16(ncols),
              "dx: deferred AvgL1Norm backward operands");
      g.epi = EPI_NBDOT;
      g.nbx = o.nb_x->m;
      // any tile plan fits (the row stride of the row-major layout: the partial count rounded up to 4)
      float* part = mem.make<float>((size_t)((cdiv(ncols, kTileM) + 3) & ~3) * M);
      // RLE_FUSE_NBROWS: row-major partials [row][rs], so the consuming weight gradient's workgroups read a row's
      // partials in rs / 4 loads (kernels.hip nb_rows_issue: one row per thread, the mean finalized, 16-row tiles)
      const int rs = (g.tiles_n + 3) & ~3;
      const bool rows = fused(RLE_FUSE_NBROWS) && fused(RLE_FUSE_NORMFIN) && kernel_set() == KS_TD7 &&
                        !g.hot.wide && M <= kThreads && rs <= 16;
      g.norm_out = part;
      g.norm_ld = rows ? -rs : M;
      out.nbdot = part;
      out.nbdot_ld = g.norm_ld;
      out.nbdot_n = g.tiles_n;
      out.nbdot_id = next_id++;
      wr.push_back(out.nbdot_id);
      rd.push_back(o.nb_x->id);
    }
    REQUIRE(!o.into || (o.into->rows == M && o.into->cols == r16(ncols)), "dx: output view shape");
    g.out = out.m;
    if (saved) {
      REQUIRE(saved->m.t, "dx: derivative source needs a T image");
      g.dact = dact;
      g.dsrc = saved->m;
      rd.push_back(saved->id);
    }
    wr.push_back(out.id);
    if (o.pre) {
      g.has_pre = o.pre->kind;
      g.prea = o.pre->a;
      rd.insert(rd.end(), o.pre->rd.begin(), o.pre->rd.end());
    }
    if (o.head) {  // A segment 0 is z of critic o.head->n's last hidden layer, not dZ
      g.has_pre = 2;
      g.hd = o.head->h;
      g.head_n = o.head->n;
      rd.insert(rd.end(), o.head->rd.begin(), o.head->rd.end());
      wr.insert(wr.end(), o.head->wr.begin(), o.head->wr.end());
    }
    if (o.sbu) {  // the output is o.sbu->a.dout (d / d(mean | log_std)), not da
      REQUIRE(!o.head && !o.pre && !o.nb_x && !saved, "dx: SAC backward epilogue is a plain DX");
      g.epi = EPI_SACBWD;
      g.out = Mat{};
      g.sb = o.sbu->a;
      rd.insert(rd.end(), o.sbu->rd.begin(), o.sbu->rd.end());
      wr.insert(wr.end(), o.sbu->wr.begin(), o.sbu->wr.end());
    }
    pg.add(op, rd, wr);
    return out;
  }
  // (through an identity layer: no derivative to read)
  View dx(Prog& pg, const std::vector<DxTerm>& terms, int ncols, int M, const DxOpt& o = {}) {
    return dx(pg, terms, ncols, M, ACT_NONE, nullptr, o);
  }

  // Tile width of the next GEMM op: from the plan of a previous build pass
  // (capture() widens tiles of levels that exceed one resident wave of
  // workgroups), else the per-op default.  Returns the op's creation index too.
  std::vector<int> tn_plan;
  int tn_seq = 0;
  std::pair<int, int> choose_tn(int M, int N) {
    const int seq = tn_seq++;
    const int t = seq < (int)tn_plan.size() ? tn_plan[seq] : pick_tn(M, N);
    return {t, seq};
  }
  // per-tile grad-square partial slots of a dW op (weights at the narrowest tile width,
  // so any plan fits; unused slots stay zero; bias)
  static int dw_gsq_w(const Layer& L) { return cdiv(L.out, kTileM) * cdiv(L.K, 16); }
  static int dw_gsq_b(const Layer& L) { return cdiv(L.out, kTileM); }

  // dW = dZ^T [X], db = sum dZ, fused Adam (torch.optim.Adam law).
  void dw(Prog& pg, const Layer& L, const View& dz, const std::vector<View>& X, int Brows, int cnt, float lr,
          const DwOpt& o = {}) {
    const View* const nb_x = o.nb_x;
    REQUIRE(X.size() == L.seg_p.size(), "dw: input count mismatch for " + L.wname);
    REQUIRE(dz.m.t, "dw: dZ needs a T image");
    Op op{};
    op.kind = OP_GEMM;
    GemmArgs& g = op.gemm;
    g.mode = GEMM_DW;
    std::vector<int> rd{dz.id, L.res, asc_set ? R_ADAMSC1 : R_ADAMSC}, wr{L.res};
    g.A.seg[0] = seg_t(dz, 0, 0, Brows);
    g.A.nseg = 1;
    int koff = 0;
    for (size_t s = 0; s < X.size(); ++s) {
      const View& v = X[s];
      REQUIRE(v.cols == L.seg_p[s] && v.rows >= Brows && v.m.t, "dw: input view mismatch for " + L.wname);
      g.B.seg[s] = seg_t(v, koff, 0, Brows);
      if (v.norm && fused(RLE_FUSE_NORMFIN)) {  // (the finalized row means, norm_fin)
        const auto f = norm_fin(pg, v);
        g.B.seg[s].norm = f.first;
        rd.push_back(f.second);
      } else if (v.norm) {
        rd.push_back(v.norm_id);
      }
      rd.push_back(v.id);
      koff += L.seg_p[s];
    }
    g.B.nseg = (int)X.size();
    g.M = L.out;
    g.N = L.K;
    g.R = Brows;
    const auto tq = choose_tn(L.out, L.K);
    g.tn = tq.first;
    op.seq = tq.second;
    g.tiles_m = cdiv(L.out, kTileM);
    g.tiles_n = cdiv(L.K, g.tn) + 1;
    g.epi = EPI_ADAM;
    AdamArgs& ad = g.adam;
    ad.w = wmat(L);
    ad.b = bias(L);
    ad.mo = (long long)nP;
    ad.vo = 2LL * (long long)nP;
    ad.step = adam_step_of(asc_set) + cnt;
    ad.bc2s = adam_bc2s_of(asc_set) + cnt;
    ad.lr = lr;
    ad.beta1 = 0.9f;
    g.gscale = o.gscale;
    if (o.gscale) {  // (the kDwGs variant: offline TD3's actor)
      REQUIRE(!nb_x, "dw: no gradient scale with a deferred AvgL1Norm backward");
      g.act = kDwGs;
      rd.push_back(o.gscale_id);
    }
    ad.beta2 = 0.999f;
    ad.omb1 = (float)(1.0 - 0.9);
    ad.omb2 = (float)(1.0 - 0.999);
    ad.eps = 1e-8f;
    ad.bias_col = cdiv(L.K, g.tn) * g.tn;
    ad.gsq = o.gsq;
    ad.gsq_b = o.gsq_b;
    ad.ptau = o.ptau;
    if (nb_x) {  // dZ = AvgL1Norm backward of (dz = g, x), applied on load (kDwNb)
      REQUIRE(dz.nbdot && nb_x->norm && nb_x->m.t && nb_x->rows >= Brows, "dw: deferred AvgL1Norm backward operands");
      g.act = kDwNb;
      g.nbx = nb_x->m;
      g.nbx_xs = nb_x->m.rbs;
      g.nbm = nb_x->nref();
      g.nbdot = dz.nbdot;
      g.nbdot_ld = dz.nbdot_ld;
      g.nbdot_n = dz.nbdot_n;
      rd.push_back(nb_x->id);
      if (fused(RLE_FUSE_NORMFIN)) {  // (the finalized row means, norm_fin; x's width for the sign term)
        const auto f = norm_fin(pg, *nb_x);
        g.nbm = f.first;
        g.nb_width = nb_x->width;
        rd.push_back(f.second);
      } else {
        rd.push_back(nb_x->norm_id);
      }
      rd.push_back(dz.nbdot_id);
    }
    op.wg_count = g.tiles_m * g.tiles_n;
    if (ClipGroup* const c = o.clip) {
      // Clipped: the norm pass now -- the same op (operands, tile plan, so the same accumulators) with the EPI_GSQ
      // epilogue, which reads no parameter and writes the tile partials alone -- and the Adam pass, in its kDwGs
      // form on the clip group's scalar, once clip_close() has emitted the group's OP_CLIP.
      REQUIRE(!nb_x, "dw: a clipped weight gradient takes no deferred AvgL1Norm backward");
      REQUIRE((o.gscale != nullptr) == (c->gin != nullptr), "dw: the clip group carries the gradient scale");
      Op np = op;
      GemmArgs& ng = np.gemm;
      ng.epi = EPI_GSQ;
      ng.adam.ptau = 0.f;
      if (!o.gsq) {  // (slots of the group's own array; the TD3 actor passes norm/policy's)
        const int nw = dw_gsq_w(L), nb = dw_gsq_b(L);
        REQUIRE(c->used + nw + nb <= c->n, "dw: clip group partial slots");
        ng.adam.gsq = c->part + c->used;
        ng.adam.gsq_b = c->part + c->used + nw;
        c->used += nw + nb;
      }
      std::vector<int> nrd;
      for (int r : rd)
        if (r != L.res && r != R_ADAMSC && r != R_ADAMSC1) nrd.push_back(r);
      const int pid = next_id++;
      c->part_ids.push_back(pid);
      pg.add(np, nrd, {pid});
      g.act = kDwGs;
      g.gscale = clip_buf + 4 * c->opt + 2;
      ad.gsq = ad.gsq_b = nullptr;
      std::vector<int> ard;
      for (int r : rd)
        if (!o.gscale || r != o.gscale_id) ard.push_back(r);
      ard.push_back(clip_id[c->opt]);
      c->adam.push_back({op, ard, wr});
      return;
    }
    pg.add(op, rd, wr);
  }

  // (DwOpt::ptau; plan without RLE_FUSE_PIPOLYAK: the standalone OP_POLYAK over the policy instead, tests, A/B)
  bool pi_polyak_fused() const { return fused(RLE_FUSE_PIPOLYAK); }

  // The AvgL1Norm means of a normed view's rows (sale.py:11-13: mean |x| before the 1e-8 clamp), computed once
  // from its producer's partials by a finalize op (OP_NORMBWD fwd 2, the level after the producer), for the
  // weight gradients: their tables cover every batch row and would otherwise sum every row's partials in every
  // workgroup (B = 1024: 4 rows per thread, 16 partials each, 3-7 us per workgroup).  Returned as a one-partial
  // NormRef of width 1 (the consumer's sum / 1 and clamp are the same floats) and its resource id; one op per
  // producer output per program.
  std::pair<NormRef, int> norm_fin(Prog& pg, const View& v) {
    REQUIRE(v.norm && v.norm_ld > 0, "norm_fin: not a normed view");
    auto it = pg.norm_fins.find(v.norm);
    if (it == pg.norm_fins.end()) {
      Op op{};
      op.kind = OP_NORMBWD;
      NormBwdArgs& a = op.nb;
      a.fwd = 2;
      a.rows = v.norm_ld;  // (the producer's rows: partials are [nparts][norm_ld])
      a.width = v.width;
      a.norm.part = v.norm;
      a.norm.ld = v.norm_ld;
      a.norm.row0 = 0;
      a.norm.nparts = v.nparts;
      a.norm.width = v.width;
      a.mout = mem.make<float>((size_t)v.norm_ld);
      op.wg_count = cdiv(v.norm_ld, kThreads);
      const int id = next_id++;
      pg.add(op, {v.norm_id}, {id});
      it = pg.norm_fins.emplace(v.norm, std::make_pair(a.mout, id)).first;
    }
    NormRef r{};
    r.part = it->second.first;
    r.ld = v.norm_ld;
    r.row0 = v.norm_row0;
    r.nparts = 1;
    r.width = 1;
    return {r, it->second.second};
  }

  View normbwd(Prog& pg, const View& gv, const View& x, const NormBwdOpt& o = {}) {
    REQUIRE(x.norm, "normbwd: x is not a normed view");
    REQUIRE(gv.m.n && x.m.n && gv.rows % 16 == 0, "normbwd: operand layout");
    Op op{};
    op.kind = OP_NORMBWD;
    NormBwdArgs& a = op.nb;
    View out = buf(gv.rows, x.width, o.n, o.t);
    a.g = gv.m;
    a.x = x.m;
    a.dx = out.m;
    a.rows = gv.rows;
    a.width = x.width;
    a.norm = x.nref();
    op.wg_count = cdiv(gv.rows, 4);
    pg.add(op, {gv.id, x.id, x.norm_id}, {out.id});
    return out;
  }

  // LayerNorm critics (ops.h LnArgs).  ln_fwd: h = act(LayerNorm(z)) of a hidden layer of `width` columns from its
  // Linear's output z (a fwd() with the identity epilogue); rows at or past nvalid come out zero.  ln_bwd: dz of
  // that Linear's output from dh, the gradient of h (an input gradient with no derivative mask, or the standalone
  // head's), and what ln_fwd kept.
  View ln_fwd(Prog& pg, const View& z, int width, int nvalid, int act, const LnOpt& o = {}) {
    REQUIRE(z.m.n && z.rows % 16 == 0 && width >= 4 && width <= 512 && width % 4 == 0 && z.cols == r16(width) &&
                nvalid >= 0 && nvalid <= z.rows && !o.u == !o.rstd,
            "ln_fwd: operand layout (widths 4 .. 512 in steps of 4)");
    Op op{};
    op.kind = OP_LN;
    LnArgs& a = op.ln;
    View out = buf(z.rows, width, true, o.t);
    std::vector<int> wr{out.id};
    a.x = z.m;
    a.y = out.m;
    if (o.u) {
      *o.u = buf(z.rows, width, true, false);
      *o.rstd = vec(z.rows);
      a.u = o.u->m;
      a.rstd = o.rstd->p;
      wr.insert(wr.end(), {o.u->id, o.rstd->id});
    }
    a.rows = z.rows;
    a.nvalid = nvalid;
    a.width = width;
    a.act = act;
    std::vector<int> rd{z.id};
    ln_drop(a, o, rd);
    op.wg_count = cdiv(z.rows, 4);  // (one row per wave)
    pg.add(op, rd, wr);
    return out;
  }
  View ln_bwd(Prog& pg, const View& dh, const View& u, const View& rstd, int width, int nvalid, int act,
              const LnOpt& o = {}) {
    REQUIRE(dh.m.n && u.m.n && rstd.p && dh.rows % 16 == 0 && u.rows == dh.rows && rstd.rows == dh.rows &&
                width >= 4 && width <= 512 && width % 4 == 0 && dh.cols == r16(width) && u.cols == dh.cols &&
                nvalid >= 0 && nvalid <= dh.rows,
            "ln_bwd: operand layout");
    Op op{};
    op.kind = OP_LN_BWD;
    LnArgs& a = op.ln;
    View out = buf(dh.rows, width, true, o.t);
    a.x = dh.m;
    a.y = out.m;
    a.u = u.m;
    a.rstd = rstd.p;
    a.rows = dh.rows;
    a.nvalid = nvalid;
    a.width = width;
    a.act = act;
    std::vector<int> rd{dh.id, u.id, rstd.id};
    ln_drop(a, o, rd);
    op.wg_count = cdiv(dh.rows, 4);
    pg.add(op, rd, {out.id});
    return out;
  }
  // Critic dropout's fields of a row op: the op then reads the RNG step counter, so it is ordered before the step
  // end that bumps it (R_CNT), as the noise ops are.  p == 0 leaves the descriptor and the reads as they were.
  void ln_drop(LnArgs& a, const LnOpt& o, std::vector<int>& rd) {
    if (!(o.p > 0.f)) return;
    REQUIRE(o.p < 1.f && o.site >= 0 && o.site < 64 && a.rows <= (1 << 25), "ln: dropout probability / site");
    a.p = o.p;
    a.s = 1.0f / (1.0f - o.p);
    a.site = o.site;
    a.step = &ctrl->counters[CNT_RNG];
    a.seed = cfg.seed;
    rd.push_back(R_CNT);
  }

  // AvgL1Norm itself (sale.py:11-13) applied to a normed view: out = x / m (OP_NORMBWD with
  // fwd = 1).  Only diagnostics read a normed tensor explicitly; the step defers the norm.
  View normfwd(Prog& pg, const View& x) {
    REQUIRE(x.norm && x.m.n && x.rows % 16 == 0, "normfwd: x is not a normed view");
    Op op{};
    op.kind = OP_NORMBWD;
    NormBwdArgs& a = op.nb;
    View out = buf(x.rows, x.width);
    a.g = x.m;
    a.x = x.m;
    a.dx = out.m;
    a.rows = x.rows;
    a.width = x.width;
    a.norm = x.nref();
    a.fwd = 1;
    op.wg_count = cdiv(x.rows, 4);
    pg.add(op, {x.id, x.norm_id}, {out.id});
    return out;
  }

  // SALEEncoder.encode_state (sale.py:41-46): a normed view (consumers apply the norm).
  View enc_zs(Prog& pg, Net& E, const View& s, int M) {
    View h1 = fwd(pg, E.layers[0], {{s}}, M, actE);
    View h2 = fwd(pg, E.layers[1], {{h1}}, M, actE);
    return fwd(pg, E.layers[2], {{h2}}, M, ACT_NONE, FwdOpt().norm());
  }
  // SALEEncoder.encode_state_action (sale.py:48-55).
  View enc_zsa(Prog& pg, Net& E, const View& zs, const View& a, int M) {
    View a1 = fwd(pg, E.layers[3], {{zs}, {a}}, M, actE);
    View a2 = fwd(pg, E.layers[4], {{a1}}, M, actE);
    return fwd(pg, E.layers[5], {{a2}}, M, ACT_NONE);
  }

  // make_mlp forward (mlp.py:24-35): `act` (action_fn) after every hidden layer, `last` after the output layer.
  View mlp_fwd(Prog& pg, Net& N, const std::vector<std::vector<View>>& in, int M, int last, int act) {
    View h;
    for (size_t i = 0; i < N.layers.size(); ++i)
      h = fwd(pg, N.layers[i], i ? std::vector<std::vector<View>>{{h}} : in, M, i + 1 == N.layers.size() ? last : act);
    return h;
  }

  // The policy forward of the engine's algorithm on the rows `in`; returns the head's output.  TD7: the fixed
  // encoder, then the policy on (s, zs) (td7.py:158-162).  TD3 / SAC: make_mlp, whose output layer gets `mlp_last`
  // (raw for rle_act and SAC's rsample, tanh for TD3's act-sample epilogue).
  View policy_fwd(Prog& pg, const View& in, int M, int mlp_last) {
    Net& pi = net("policy");
    if (algo != RLE_TD7) return mlp_fwd(pg, pi, {{in}}, M, mlp_last, actP);
    View zs = enc_zs(pg, net("fixed_encoder"), in, M);
    View p0 = fwd(pg, pi.layers[0], {{in}}, M, ACT_NONE, FwdOpt().norm());
    View p1 = fwd(pg, pi.layers[1], {{p0}, {zs}}, M, actP);
    View p2 = fwd(pg, pi.layers[2], {{p1}}, M, actP);
    return fwd(pg, pi.layers[3], {{p2}}, M, ACT_TANH);
  }
  // What every program of this engine is planned with: the plan's scheduling knobs and the diagnostic switches
  // of the environment, read here once per program built (tests set them before they create their engine).
  PlanOptions prog_options() const {
    auto on = [](const char* name) {
      const char* e = std::getenv(name);
      return e && e[0] == '1';
    };
    PlanOptions o = plan_knobs(plan);
    o.audit = std::getenv("RLE_AUDIT") != nullptr;  // (set to any value)
    o.hazard = on("RLE_HAZARD");
    o.crit = on("RLE_DESC_CRIT");
    o.traffic = on("RLE_TRAFFIC");
    o.allocs = &live_allocs();
    return o;
  }
  // A program outside plan_build: the prime / hard-update / fold programs, the forward entry points, the diagnostics.
  Prog aux_prog() const { return Prog(prog_options()); }
  // The ActArgs of an act-sample program over n rows: its pinned buffers, the action map, and a Philox stream
  // of its own, not the step's
  ActArgs act_args(const ActSample& as, int n) {
    ActArgs ao{};
    HIPCHK(hipHostGetDevicePointer((void**)&ao.out, as.out, 0));
    HIPCHK(hipHostGetDevicePointer((void**)&ao.ctl, as.ctl, 0));
    HIPCHK(hipHostGetDevicePointer((void**)&ao.eps, as.eps, 0));
    ao.scale = act_map;
    ao.bias = act_map + A;
    ao.sigma = act_map + 2 * A;
    ao.n = n;
    ao.A = A;
    ao.seed = cfg.seed * 0x9E3779B97F4A7C15ull + 0x5851F42D4C957F2Dull;
    return ao;
  }
  // An OP_SAC_ACTOR / OP_SAC_ACTOR_BWD op over `rows` rows of the raw head output (mean | log_std): the fields
  // every use shares.  The caller adds its eps, act and logpi (or gradient) operands.
  Op sac_actor_op(int kind, const Mat& raw, int rows) {
    Op op{};
    op.kind = kind;
    SacActorArgs& a = op.sac;
    a.out = raw;
    a.A = A;
    a.rows = rows;
    a.min_log_std = cfg.min_log_std;
    a.max_log_std = cfg.max_log_std;
    a.mean_off = 0;
    a.ls_off = A;
    op.wg_count = cdiv(rows, kThreads);
    return op;
  }

  // Host rows [n][w] into every kept image of v (rows past n and columns past w stay zero).
  void upload(const View& v, const float* host, int n, int w) {
    const size_t img = (size_t)v.m.rbs * 16 * v.m.cbn * 16;
    if (v.m.n) {
      std::vector<float> buf_n(img, 0.f);
      for (int i = 0; i < n; ++i)
        for (int c = 0; c < w; ++c) buf_n[h_nidx(v.m.cbn, i, c)] = host[(size_t)i * w + c];
      HIPCHK(hipMemcpyAsync(v.m.n, buf_n.data(), img * 4, hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    if (v.m.t) {
      std::vector<float> buf_t(img, 0.f);
      for (int i = 0; i < n; ++i)
        for (int c = 0; c < w; ++c) buf_t[h_tidx(v.m.rbs, i, c)] = host[(size_t)i * w + c];
      HIPCHK(hipMemcpyAsync(v.m.t, buf_t.data(), img * 4, hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
  }
  // Rows [n][w] of v's T image to the host (syncs the engine stream).
  void download(const View& v, float* host, int n, int w) {
    std::vector<float> res((size_t)v.m.rbs * 16 * v.m.cbn * 16);
    HIPCHK(hipMemcpyAsync(res.data(), v.m.t, res.size() * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < w; ++c) host[(size_t)i * w + c] = res[h_tidx(v.m.rbs, i, c)];
  }

  // Diagnostic forward programs (rle_eval, rle_sac_rsample), captured once per shape.
  struct EvalGraph {
    Graph G;
    View in0, in1, out;
    float* out_vec = nullptr;
    int width = 0;
  };
  std::map<std::string, EvalGraph> eval_graphs;

  // polyak / copy over a whole net range
  void flat(Prog& pg, int kind, Net& dst, Net* src, float tau, bool self_alias) {
    Op op{};
    op.kind = kind;
    FlatArgs& f = op.flat;
    f.dst = P + dst.off;
    f.src = src ? P + src->off : P + dst.off;
    f.n = (long long)dst.size;
    f.tau = tau;
    f.omt = 1.f - tau;  // fp32(1 - tau) as torch casts the python scalar (Q2)
    f.self_alias = self_alias ? 1 : 0;
    op.wg_count = cdiv(f.n, (long long)kThreads * 4);
    std::vector<int> rd{dst.res}, wr{dst.res};
    for (auto& L : dst.layers) {
      rd.push_back(L.res);
      wr.push_back(L.res);
    }
    if (src) {
      rd.push_back(src->res);
      for (auto& L : src->layers) rd.push_back(L.res);
    }
    pg.add(op, rd, wr);
  }

  // ---------------------------------------------------------------- step programs
  // The previous step's LAP priority update, applied by the sampler (SampleArgs::pend_*)
  struct PendUpd {
    const long long* ind;
    const float* p;
    int ind_id, p_id;
  };
  void add_sampling(Prog& pg, bool sac, int ahead, const PendUpd* pu = nullptr) {
    // LAP block sums are maintained by every priority write (OP_PRIORITY, appends)
    Op op{};
    op.kind = OP_SAMPLE_GATHER;
    fill_sample_args(op.sample, sac);
    op.sample.ahead = ahead;
    op.wg_count = cdiv(Bv, 4);  // one wave per query
    // reads the RNG step / tape position counters -> ordered before STEP_END (WAR)
    std::vector<int> rd{bsum_id, R_PRIO, R_REPLAY, R_CNT};
    if (pu) {
      op.sample.pend_ind = pu->ind;
      op.sample.pend_p = pu->p;
      op.sample.pend_n = Bv;
      rd.push_back(pu->ind_id);
      rd.push_back(pu->p_id);
    }
    std::vector<int> wr{ss.id, act_in.id, rw.id, nd.id, ind_id};
    if (n_step > 1) wr.push_back(hops.id);  // (the gather writes the rows' hop counts)
    pg.add(op, rd, wr);
    Op nz{};
    nz.kind = OP_NOISE;
    fill_sample_args(nz.sample, sac);
    nz.sample.ahead = ahead;
    nz.wg_count = cdiv(Bv * A, kThreads);
    pg.add(nz, {R_CNT}, {eps.id, sac ? eps2.id : -1});
  }
  int bsum_id = -1, ind_id = -1;

  void fill_sample_args(SampleArgs& s, bool sac) {
    Replay& rp = *replay;
    s.state = rp.state;
    s.next_state = rp.next_state;
    s.action = rp.action;
    s.reward = rp.reward;
    s.notdone = rp.notdone;
    s.priority = rp.priority;
    s.S = S;
    s.Sp = Sp;
    s.A = A;
    s.Ap = Ap;
    s.size = rp.size_d;
    s.cap = rp.cap;
    s.lap = rp.lap;
    s.B = B;
    s.nq = Bv;
    s.bsum = rp.bsum;
    s.ssum = rp.ssum;
    s.nblk = rp.nblk;
    s.ss = ss.m;
    s.a = act_in.m;
    s.r = rw.p;
    s.nd = nd.p;
    s.ind = ind;
    s.u_out = u_buf;
    s.eps = eps.m;
    if (sac) s.eps2 = eps2.m;
    s.ctrl_rng = &ctrl->counters[4];
    s.seed = cfg.seed;
    s.tape_mode = &ctrl->tape_mode;
    s.tape_pos = &ctrl->counters[5];
    s.tape_u = t_u;
    s.tape_eps = t_eps;
    s.tape_eps2 = t_eps2;
    s.tape_ind = t_ind;
    if (n_step > 1) {  // (n_step == 1: the fields stay zero, the descriptor is the one it was)
      REQUIRE(hops.p, "n-step returns: the hop buffers (rle_set_n_step allocates them)");
      s.n_step = n_step;
      s.gamma = cfg.discount;
      s.ptr = rp.ptr_d;
      s.hops_out = hops.p;
    }
  }

  Op head_op(int mode, int rows) {
    Op op{};
    op.kind = OP_HEAD;
    HeadArgs& h = op.head;
    h.mode = mode;
    h.rows = rows;
    h.H = H;
    h.gamma = cfg.discount;
    h.inv_b = 1.f / (float)Bv;
    h.nvalid = Bv;
    h.tgt_mode = -1;
    op.wg_count = cdiv(rows, 4);
    return op;
  }

  // The target twins' last layer fused into a *_LOSS head (HeadArgs::tgt_mode).
  void set_head_target(HeadArgs& h, int mode, const View& t1, const View& t2, const Layer& l1, const Layer& l2) {
    REQUIRE(t1.m.n && t2.m.n && l1.out == 1 && l2.out == 1 && l1.cb == h.w_cbn, "head: target operand layout");
    h.tgt_mode = mode;
    h.th[0] = t1.m;
    h.th[1] = t2.m;
    h.tw[0] = P + l1.wn_off;
    h.tw[1] = P + l2.wn_off;
    h.tb[0] = bias(l1);
    h.tb[1] = bias(l2);
  }

  void set_head_twin(HeadArgs& h, const View& h1, const View& h2, const Layer& l1, const Layer& l2) {
    REQUIRE(h1.m.n && h2.m.n && l1.out == 1 && l2.out == 1, "head: operand layout");
    h.h[0] = h1.m;
    h.h[1] = h2.m;
    h.w[0] = P + l1.wn_off;
    h.w[1] = P + l2.wn_off;
    h.w_cbn = l1.cb;
    h.b[0] = bias(l1);
    h.b[1] = bias(l2);
  }

  Op step_end_op() {
    Op op{};
    op.kind = OP_STEP_END;
    StepEndArgs& a = op.end;
    a.counters = ctrl->counters;
    a.info_slot = &ctrl->info_slot;
    a.info = info;
    a.info_cap = info_cap;
    a.inv_b = 1.f / (float)Bv;
    op.wg_count = 1;
    return op;
  }

  void info_sum(StepEndArgs& a, int k, const float* part, int n, int stride, float scale) {
    a.part[k] = part;
    a.npart[k] = n;
    a.stride[k] = stride;
    a.scale[k] = scale;
    a.kind[k] = INFO_SUM;
  }

  // STEP_END writes the info row and bumps the step counters; every reader of a
  // counter (Adam t, RNG step, tape position) is therefore scheduled before it.
  // Split in two (plan without RLE_FUSE_ENDSPLIT: one op): the counters (+ the SAC temperature update), which
  // the next step reads, at the step's end; the info row, which only the host reads, after it,
  // free to sit under a longer op (the rebalance pass's one-workgroup rule).
  float* sac_scr = nullptr;
  int sac_scr_id = -1;
  bool end_split() const { return fused(RLE_FUSE_ENDSPLIT); }
  void add_step_end(Prog& pg, Op op, std::vector<int> rd, const std::vector<int>& counters) {
    StepEndArgs& a = op.end;
    a.cmask = 0;
    for (int c : counters) a.cmask |= 1 << c;
    const std::vector<int> rd_info = rd;  // (the info op does not touch the counters)
    rd.push_back(R_CNT);
    if (!end_split()) {
      std::vector<int> wr{R_INFO, R_CNT};
      if (a.log_alpha) wr.push_back(R_LA);
      pg.add(op, rd, wr);
      return;
    }
    const bool sac_tmp = a.log_alpha && a.la_lr > 0.f;
    if (sac_tmp && !sac_scr) {
      sac_scr = mem.make<float>(4);
      sac_scr_id = next_id++;
    }
    Op c = op, i = op;
    c.end.mode = 1;
    c.end.sac_scratch = sac_tmp ? sac_scr : nullptr;
    std::vector<int> cw{R_CNT};
    if (a.log_alpha) cw.push_back(R_LA);
    if (sac_tmp) cw.push_back(sac_scr_id);
    pg.add(c, rd, cw);
    i.end.mode = 2;
    i.end.cmask = 0;
    i.end.sac_scratch = sac_tmp ? sac_scr : nullptr;
    std::vector<int> ir = rd_info;
    if (sac_tmp) ir.push_back(sac_scr_id);
    else if (a.log_alpha) ir.push_back(R_LA);  // (fixed temperature: read, never written)
    pg.add(i, ir, {R_INFO});
  }

  // TD7 (td7.py:287-332)
  // Next step's batch into the other buffer set, after this step's priority update
  // (RAW on the priorities) and before STEP_END bumps the counters (WAR).
  void add_prefetch(Prog& pg, bool sac, int set, const PendUpd* pu = nullptr) {
    use_set(1 - set);
    add_sampling(pg, sac, 1, pu);
    use_set(set);
  }
  // LAPReplayMemory.update_priority (lap.py:66-69) of this step's batch, then the next step's batch.
  // Fused (RLE_FUSE_PRIOSAMPLE): the sampler applies the update to what its search reads, and the
  // OP_PRIORITY that persists it runs after the sampler, off the step-to-step chain.
  bool prio_sample_fused() const {
    int ns = 64;  // (kernels.hip pend_prepare's LDS layout, within rle_level's 24 KB)
    while (ns < 2 * B) ns <<= 1;
    return fused(RLE_FUSE_PRIOSAMPLE) && replay->lap && B <= 1024 &&
           std::max(8 * ns, 20 * B) + 12 * replay->nblk <= 24 * 1024;
  }
  void add_update_and_prefetch(Prog& pg, bool sac, int set, bool lap, const View& prio) {
    Op op{};
    op.kind = OP_PRIORITY;
    op.prio.priority = replay->priority;
    op.prio.ind = ind;
    op.prio.p = prio.p;
    op.prio.B = Bv;
    op.prio.max_priority = replay->maxp_d;
    op.prio.bsum = replay->lap ? replay->bsum : nullptr;
    op.prio.ssum = replay->ssum;
    op.wg_count = 1;
    const std::vector<int> rd{prio.id, ind_id}, wr{R_PRIO, R_MAXP, bsum_id};
    if (!lap) {
      add_prefetch(pg, sac, set);
    } else if (prio_sample_fused()) {
      const PendUpd pu{ind, prio.p, ind_id, prio.id};
      add_prefetch(pg, sac, set, &pu);
      pg.add(op, rd, wr);
    } else {
      pg.add(op, rd, wr);
      add_prefetch(pg, sac, set);
    }
  }
  void build_prime(Prog& pg, bool sac, int set) {
    use_set(set);
    add_sampling(pg, sac, 0);
  }

  // What the phases of one step hand to each other.  build_td7 / build_mlp create one per step (begin_step) and
  // pass it by reference, so nothing of a program under construction lives on the engine; what only two
  // neighbouring phases share travels as a phase's return value instead.
  struct StepBuild {
    bool policy = false;
    int set = 0;                      // the batch buffer set the step runs on
    View s, s2;                       // its state and next-state rows
    LossPart enc_loss, qloss, ploss;  // info row: TD7's encoder loss, the critic loss, the policy objective
    int ploss_id2 = -1;               // (TD7: the second critic's q-head writes a loss resource of its own)
    // behaviour cloning of an offline policy step (add_bc): e = dL_bc / d pi and (q_abs ..) I for the action
    // gradient, the row blocks' sums of (pi - a)^2, the scalars {q_abs, lmbda}
    View bc_e, bc_eye;
    LossPart bc_part;
    float* bc_s = nullptr;
    int bc_s_id = -1;
    // TD3 policy steps: per-tile grad-square partials of the actor; tensor t owns tiles [gsq_offs[t], gsq_offs[t+1])
    float* gsq = nullptr;
    std::vector<int> gsq_offs;
  };
  // The one place that selects a step's buffer set and Adam scalars (asc_set: read by dw() and the step end)
  StepBuild begin_step(Prog& pg, bool policy, int set) {
    use_set(set);
    asc_set = set;
    add_adam_scalars(pg);
    StepBuild sb;
    sb.policy = policy;
    sb.set = set;
    sb.s = ss.sub(0, B);
    sb.s2 = ss.sub(B, B);
    return sb;
  }

  // The critic loss head of a step (HEAD_TD7_LOSS / HEAD_MLP_LOSS with the target twins' last layer fused in): the
  // buffers it writes and the fields and resources both algorithms share.  c / t: the last hidden layers of the
  // critics / the target critics, dsrc: the derivative source of c's activation.  The caller adds its own fields
  // and reads, then emits `op` or fuses it into the critics' input gradients (HeadUse).
  struct LossHead {
    Op op;
    View dz[2], dq[2], prio;
    std::vector<int> rd;
  };
  LossHead loss_head(StepBuild& sb, int mode, int tgt_mode, const View* c, const View* dsrc, const View* t,
                     const Layer* const* qo, const Layer* const* tqo, bool fused_dx, bool lap) {
    LossHead lh;
    // (dZ of the critics' last hidden layers: with the fused head only their weight gradients read it, in the T image)
    for (int n = 0; n < 2; ++n) lh.dz[n] = buf(B, H, !fused_dx, true);
    for (int n = 0; n < 2; ++n) lh.dq[n] = buf(B, 1, false, true);
    lh.prio = vec(B);
    sb.qloss.n = cdiv(B, 4) * 4;
    sb.qloss.p = mem.make<float>((size_t)sb.qloss.n);
    lh.op = head_op(mode, Bv);
    HeadArgs& h = lh.op.head;
    set_head_twin(h, c[0], c[1], *qo[0], *qo[1]);
    set_head_target(h, tgt_mode, t[0], t[1], *tqo[0], *tqo[1]);
    h.reward = rw.p;
    h.notdone = nd.p;
    h.dact = actC;
    h.lap = lap;
    for (int n = 0; n < 2; ++n) {
      h.dsrc[n] = dsrc[n].m;
      h.dz[n] = lh.dz[n].m;
      h.dq[n] = lh.dq[n].m;
    }
    h.loss_part = sb.qloss.p;
    h.prio = lh.prio.p;
    lh.rd = {c[0].id, c[1].id, qo[0]->res, qo[1]->res, t[0].id, t[1].id, tqo[0]->res, tqo[1]->res, rw.id, nd.id};
    sb.qloss.id = next_id++;
    return lh;
  }
  // The SAC fields of a head over the logpi rows from row0 on, and the two resources they read
  void set_head_sac(HeadArgs& h, const View& logpi, int row0, std::vector<int>& rd) {
    h.sac = 1;
    h.logpi = logpi.p + row0;
    h.log_alpha = alpha_src();
    h.alpha_lin = cfg.tmp >= 0.f;
    rd.push_back(logpi.id);
    rd.push_back(R_LA);
  }

  // OP_BC, the behaviour-cloning term of an offline policy step, in its two ops.
  // Mode 0 needs the actor output *v alone, so it runs many levels before the action gradient: e = dL_bc / d pi
  // per row (sb.bc_e, scaled by lambda) and the row blocks' sums of (pi - a)^2 (sb.bc_part).
  // The scalar op, one workgroup: q_abs into sb.bc_s[0] and its multiple of I into sb.bc_eye.  Mode 1 (TD7, reads no
  // lambda): mean |cat Q| from the twins' row partials v[0], v[1] and their head layers qo.  Offline TD3, with
  // lmbda = lambda / q_abs into sb.bc_s[1]: mode 3, mean |min Q| from the same operands, beside the fused policy
  // head; mode 2, from the standalone policy head's |min| partials (sb.ploss), a level after it.
  void add_bc(Prog& pg, StepBuild& sb, int mode, float lambda, const View* v, const Layer* const* qo = nullptr) {
    Op op{};
    op.kind = OP_BC;
    BcArgs& b = op.bc;
    b.mode = mode;
    b.nvalid = Bv;
    b.A = A;
    b.lambda = lambda;
    if (mode == 0) {
      REQUIRE(A <= kThreads && v->m.n && act_in.m.n, "bc: operand layout");
      sb.bc_e = buf(B, A, true, false);
      sb.bc_part.n = cdiv(Bv, 16);
      sb.bc_part.p = mem.make<float>((size_t)sb.bc_part.n);
      sb.bc_part.id = next_id++;
      b.pi = v->m;
      b.a = act_in.m;
      b.e = sb.bc_e.m;
      b.part = sb.bc_part.p;
      op.wg_count = sb.bc_part.n;
      pg.add(op, {v->id, act_in.id}, {sb.bc_e.id, sb.bc_part.id});
      return;
    }
    sb.bc_eye = buf(A, A, false, true);
    sb.bc_s = mem.make<float>(4);
    sb.bc_s_id = next_id++;
    b.eye = sb.bc_eye.m;
    b.out = sb.bc_s;
    op.wg_count = 1;
    if (mode == 2) {
      b.qp[0] = sb.ploss.p + 1;
      b.qp_n[0] = sb.ploss.n;
      b.qp_ld = 4;
      pg.add(op, {sb.ploss.id}, {sb.bc_eye.id, sb.bc_s_id});
      return;
    }
    for (int n = 0; n < 2; ++n) {
      b.qp[n] = v[n].qd;
      b.qp_n[n] = v[n].qd_n;
      b.qb[n] = bias(*qo[n]);
    }
    REQUIRE(v[0].qd && v[1].qd && v[0].qd_ld == v[1].qd_ld, "bc: q partial layout");
    b.qp_ld = v[0].qd_ld;
    pg.add(op, {v[0].qd_id, v[1].qd_id, qo[0]->res, qo[1]->res}, {sb.bc_eye.id, sb.bc_s_id});
  }
  // The offline tail of the info row, after the algorithm's three entries: TD7 [.., policy + bc term, bc, q_abs],
  // TD3 [.., policy + bc term, norm/policy, train/bc, train/lmbda]; NaN on plain steps
  void info_offline(StepEndArgs& a, std::vector<int>& rd, const StepBuild& sb) {
    a.ninfo = 5;
    if (!sb.policy) {
      a.kind[3] = a.kind[4] = INFO_NAN;
      return;
    }
    a.bcs = sb.bc_s;
    info_sum(a, 3, sb.bc_part.p, sb.bc_part.n, 1, 1.f / ((float)Bv * (float)A));
    if (algo == RLE_TD7) {
      a.kind[2] = INFO_SUM_BC;
      a.bc_lambda = cfg.bc_lambda;
      info_sum(a, 4, sb.bc_s, 1, 1, 1.f);
    } else {
      a.kind[1] = INFO_SUM_BC3;  // lmbda * -mean(min Q) + bc
      a.kind[4] = INFO_BCS1;
    }
    rd.push_back(sb.bc_s_id);
    rd.push_back(sb.bc_part.id);
  }
  // TD7 offline mode (rle_config bc_lambda > 0); offline TD3 (rle_config_ext bc_alpha > 0, TD3+BC)
  bool offline() const { return algo == RLE_TD7 && cfg.bc_lambda > 0.f; }
  float bc_alpha = 0.f;
  bool offline3() const { return algo == RLE_TD3 && bc_alpha > 0.f; }
  static std::vector<const Layer*> layer_ptrs(const Net& a, const Net* b = nullptr) {
    std::vector<const Layer*> v;
    for (const Layer& L : a.layers) v.push_back(&L);
    if (b)
      for (const Layer& L : b->layers) v.push_back(&L);
    return v;
  }
  // offline SAC (rle_config_ext awac_lambda > 0, AWAC; the temperature is fixed at 0)
  float awac_lambda = 0.f;
  bool offline_sac() const { return algo == RLE_SAC && awac_lambda > 0.f; }

  // ---- TD7 (td7.py:287-332): build_td7 below is the list of these phases.
  // Encoder update (td7.py:246-257): the online encoder on [s; s'] (one GEMM per layer), zsa3 with the MSE
  // gradient against the normed zs' as its epilogue, then backward + Adam (optim_encoder, lr = policy_lr).
  void td7_encoder_update(Prog& pg, StepBuild& sb) {
    Net& enc = net("encoder");
    const int B2 = 2 * B;
    View ez1, ez2;
    View eh1 = fwd(pg, enc.layers[0], {{ss}}, B2, actE, FwdOpt().keep_pre(&ez1));
    View eh2 = fwd(pg, enc.layers[1], {{eh1}}, B2, actE, FwdOpt().keep_pre(&ez2));
    View ex3 = fwd(pg, enc.layers[2], {{eh2}}, B2, ACT_NONE, FwdOpt().norm());
    View ezs = ex3.sub(0, B), ezs2 = ex3.sub(B, B);
    View ea1z, ea2z;
    View ea1 = fwd(pg, enc.layers[3], {{ezs}, {act_in}}, B, actE, FwdOpt().keep_pre(&ea1z));
    View ea2 = fwd(pg, enc.layers[4], {{ea1}}, B, actE, FwdOpt().keep_pre(&ea2z));
    const float mean = 1.f / (float)((long long)Bv * Z);  // (mean over the B x zs_dim zsa, td7.py:253)
    View ed3 = fwd(pg, enc.layers[5], {{ea2}}, B, ACT_NONE, FwdOpt().mse(&ezs2, mean, &sb.enc_loss));
    // (gradient clipping: optim_encoder's clip group; null when off, and every dw() below is then the op it was)
    ClipGroup cgs;
    if (clip_on()) cgs = clip_group(2, layer_ptrs(enc));
    const DwOpt eo = DwOpt().clip_in(clip_on() ? &cgs : nullptr);
    View d2 = dx(pg, {{ed3, &enc.layers[5], 0}}, H, B, actE, &ea2z);
    dw(pg, enc.layers[5], ed3, {ea2}, B, CNT_ADAM_ENC, cfg.policy_lr, eo);
    View d1 = dx(pg, {{d2, &enc.layers[4], 0}}, H, B, actE, &ea1z);
    dw(pg, enc.layers[4], d2, {ea1}, B, CNT_ADAM_ENC, cfg.policy_lr, eo);
    View gzs = dx(pg, {{d1, &enc.layers[3], 0}}, Z, B, DxOpt().no_t());  // (read by the norm backward only)
    dw(pg, enc.layers[3], d1, {ezs, act_in}, B, CNT_ADAM_ENC, cfg.policy_lr, eo);
    View dx3 = normbwd(pg, gzs, ex3.sub(0, B));
    View ez2s = ez2.sub(0, B), ez1s = ez1.sub(0, B);
    View dh2 = dx(pg, {{dx3, &enc.layers[2], 0}}, H, B, actE, &ez2s);
    dw(pg, enc.layers[2], dx3, {eh2.sub(0, B)}, B, CNT_ADAM_ENC, cfg.policy_lr, eo);
    View dh1 = dx(pg, {{dh2, &enc.layers[1], 0}}, H, B, actE, &ez1s);
    dw(pg, enc.layers[1], dh2, {eh1.sub(0, B)}, B, CNT_ADAM_ENC, cfg.policy_lr, eo);
    dw(pg, enc.layers[0], dh1, {sb.s}, B, CNT_ADAM_ENC, cfg.policy_lr, eo);
    if (clip_on()) clip_close(pg, cgs);
  }
  // Fixed encoder on s, fixed target encoder on s', and the actor on [s; s'] (the target policy aliases the
  // policy, Q1).  The later phases read:
  struct Td7Actor {
    View fzs, tzs, fzsa;         // zs of s (fixed encoder) and of s' (fixed target encoder); zsa of (s, a)
    View ap0, ap1, ap2;          // the actor's hidden layers on [s; s'] ...
    View ap1z, ap2z;             // ... and an ELU actor's pre-activations, for the policy backward: ELU' = exp(z)
    View a_pi, a_next;           // pi(s); the smoothed target action (pre: layout only)
    bool prea = false;           // a' is recomputed in-tile by the target branch's first layers (pre-GEMM pn1)
    PreUse pn1;
    const PreUse* pnext() const { return prea ? &pn1 : nullptr; }
  };
  Td7Actor td7_fixed_and_actor(Prog& pg, const StepBuild& sb) {
    Net& fe = net("fixed_encoder");
    Net& fet = net("fixed_encoder_target");
    Net& pi = net("policy");
    const int B2 = 2 * B;
    Td7Actor o;
    // forward-only outputs (no weight gradient reads them); fzs and fzsa, which the critics' and the actor's
    // weight gradients read, keep both images
    const FwdOpt fo = FwdOpt().no_t();
    View fh1 = fwd(pg, fe.layers[0], {{sb.s}}, B, actE, fo);
    View fh2 = fwd(pg, fe.layers[1], {{fh1}}, B, actE, fo);
    o.fzs = fwd(pg, fe.layers[2], {{fh2}}, B, ACT_NONE, FwdOpt().norm());
    View th1 = fwd(pg, fet.layers[0], {{sb.s2}}, B, actE, fo);
    View th2 = fwd(pg, fet.layers[1], {{th1}}, B, actE, fo);
    o.tzs = fwd(pg, fet.layers[2], {{th2}}, B, ACT_NONE, FwdOpt(fo).norm());
    View fa1 = fwd(pg, fe.layers[3], {{o.fzs}, {act_in}}, B, actE, fo);
    View fa2 = fwd(pg, fe.layers[4], {{fa1}}, B, actE, fo);
    o.fzsa = fwd(pg, fe.layers[5], {{fa2}}, B, ACT_NONE);
    o.ap0 = fwd(pg, pi.layers[0], {{ss}}, B2, ACT_NONE, FwdOpt().norm());
    const bool pz = act_zsaved(actP);
    o.ap1 = fwd(pg, pi.layers[1], {{o.ap0}, {o.fzs, o.tzs}}, B2, actP, FwdOpt().keep_pre(pz ? &o.ap1z : nullptr));
    o.ap2 = fwd(pg, pi.layers[2], {{o.ap1}}, B2, actP, FwdOpt().keep_pre(pz ? &o.ap2z : nullptr));
    // a' = clamp(pi(s', zs') + noise) only feeds the target branch's first layers, which
    // recompute it in-tile (pre-GEMM): the actor output layer runs on the s rows alone
    o.prea = actor_pre();
    View actv = o.prea ? fwd(pg, pi.layers[3], {{o.ap2.sub(0, B)}}, B, ACT_TANH)
                       : fwd(pg, pi.layers[3], {{o.ap2}}, B2, ACT_TANH, FwdOpt().noised(&eps, B));
    o.a_pi = actv.sub(0, B);
    o.a_next = o.prea ? o.a_pi : actv.sub(B, B);
    if (o.prea) o.pn1 = pre_actor_fwd(pi.layers[3], o.ap2.sub(B, B), &eps, 1);
    return o;
  }
  // Target branch (forward only): zsa' and the target critics' last hidden layers on (s', a')
  struct TwinViews {
    View v[2];
  };
  TwinViews td7_target(Prog& pg, const StepBuild& sb, const Td7Actor& ac) {
    Net& fet = net("fixed_encoder_target");
    Net* tq[2] = {&net("target_q1"), &net("target_q2")};
    const FwdOpt fo = FwdOpt().no_t();
    const PreUse* pnext = ac.pnext();
    View ta1 = fwd(pg, fet.layers[3], {{ac.tzs}, {ac.a_next}}, B, actE, FwdOpt(fo).pre_gemm(pnext));
    View ta2 = fwd(pg, fet.layers[4], {{ta1}}, B, actE, fo);
    // zsa' = zsa3(ta2) only feeds the target critics' first hidden layer, a linear map:
    // with `fold`, tq.q1[:, zsa block] x fet.zsa3 is precomputed (add_target_fold) and the
    // target critics read ta2 directly (one dependent level fewer)
    const bool fold = td7_fold();
    View tzsa;
    if (!fold) tzsa = fwd(pg, fet.layers[5], {{ta2}}, B, ACT_NONE, fo);
    TwinViews th;
    for (int n = 0; n < 2; ++n) {
      View t01 = fwd(pg, tq[n]->layers[0], {{sb.s2}, {ac.a_next}}, B, ACT_NONE, FwdOpt(fo).norm().pre_gemm(pnext));
      View t1;
      if (fold) {  // fixed_encoder_target.zsa3 folded into the zsa block (tfold_w / tfold_b)
        const Layer& L1 = tq[n]->layers[1];
        const std::vector<WSeg> ws{wblock(L1, 0), {tfold_w[n].m.n, tfold_w[n].m.cbn, tfold_w[n].id},
                                   wblock(L1, L1.seg_p[0] + L1.seg_p[1])};
        t1 = fwd(pg, L1, {{t01}, {ta2}, {ac.tzs}}, B, actC, FwdOpt(fo).wblocks(&ws, &tfold_b[n]));
      } else {
        t1 = fwd(pg, tq[n]->layers[1], {{t01}, {tzsa}, {ac.tzs}}, B, actC, fo);
      }
      th.v[n] = fwd(pg, tq[n]->layers[2], {{t1}}, B, actC, FwdOpt(fo).q_dot(td7_qdot() ? &tq[n]->layers[3] : nullptr));
    }
    return th;
  }
  // Online critics on (s, a, zsa_f, zs_f) and the loss head (td7.py:211-218; y per row from the target twins,
  // then the loss), the priority update and the next step's batch.  The backward reads:
  struct Td7Critics {
    View c01[2], c1[2], c2[2], c1z[2];  // the layers' outputs and the first hidden layer's pre-activation
    View dz2[2], dq[2];                 // the head's gradients: dZ of the last hidden layer, dq
    bool hdx = false;                   // the head ran inside the DX of each critic's second hidden layer, ...
    View d1f[2];                        // ... which gave dZ of the first
  };
  Td7Critics td7_critics(Prog& pg, StepBuild& sb, const Td7Actor& ac, const TwinViews& th) {
    Net* q[2] = {&net("q1"), &net("q2")};
    Net* tq[2] = {&net("target_q1"), &net("target_q2")};
    const bool qpart = td7_qdot();  // the loss head's q from EPI_QDOT partials
    Td7Critics o;
    View c2z[2];
    for (int n = 0; n < 2; ++n) {
      o.c01[n] = fwd(pg, q[n]->layers[0], {{sb.s}, {act_in}}, B, ACT_NONE, FwdOpt().norm());
      o.c1[n] = fwd(pg, q[n]->layers[1], {{o.c01[n]}, {ac.fzsa}, {ac.fzs}}, B, actC, FwdOpt().keep_pre(&o.c1z[n]));
      o.c2[n] = fwd(pg, q[n]->layers[2], {{o.c1[n]}}, B, actC,
                    FwdOpt().keep_pre(&c2z[n], true).q_dot(qpart ? &q[n]->layers[3] : nullptr));
    }
    o.hdx = td7_headdx() && qpart;  // (the fused head reads q partials only)
    const Layer *qo[2] = {&q[0]->layers[3], &q[1]->layers[3]}, *tqo[2] = {&tq[0]->layers[3], &tq[1]->layers[3]};
    LossHead lh = loss_head(sb, HEAD_TD7_LOSS, HEAD_TD7_TARGET, o.c2, c2z, th.v, qo, tqo, o.hdx, cfg.use_lap);
    HeadArgs& h = lh.op.head;
    h.vmax_key = &ctrl->vmax_key;
    h.vmin_key = &ctrl->vmin_key;
    h.vt = ctrl->vt;
    lh.rd.push_back(R_VT);
    if (qpart) {
      set_head_parts(h, o.c2, th.v, lh.rd);
      REQUIRE(h.qp_n[0] <= 64 && h.qp_n[1] <= 64 && h.tp_n[0] <= 64 && h.tp_n[1] <= 64, "head: q partial layout");
    }
    for (int n = 0; n < 2; ++n) o.dz2[n] = lh.dz[n], o.dq[n] = lh.dq[n];
    if (!o.hdx) {
      std::vector<int> rd = lh.rd;
      rd.insert(rd.end(), {c2z[0].id, c2z[1].id});
      pg.add(lh.op, rd, {lh.dz[0].id, lh.dz[1].id, lh.dq[0].id, lh.dq[1].id, lh.prio.id, sb.qloss.id, R_VKEYS});
    } else {
      // the head runs inside the DX of each critic's second hidden layer (one level fewer on
      // the critic chain); critic 0's op stores the priorities, loss partials and value bounds
      for (int n = 0; n < 2; ++n) {
        HeadUse hu{h, n, lh.rd, {lh.dz[n].id, lh.dq[n].id}};
        if (n == 0) hu.wr.insert(hu.wr.end(), {lh.prio.id, sb.qloss.id, R_VKEYS});
        o.d1f[n] = dx(pg, {{c2z[n], &q[n]->layers[2], 0}}, H, B, actC, &o.c1z[n], DxOpt().head_use(&hu));
      }
    }
    add_update_and_prefetch(pg, false, sb.set, cfg.use_lap, lh.prio);
    return o;
  }
  // Critic backward + Adam (optim_q_fns spans q1 + q2)
  void td7_critic_backward(Prog& pg, const StepBuild& sb, const Td7Actor& ac, const Td7Critics& cr) {
    const bool nbd = td7_nb_defer();
    ClipGroup cgs;  // (gradient clipping: optim_q_fns' clip group, q1 + q2 together)
    if (clip_on()) cgs = clip_group(0, layer_ptrs(net("q1"), &net("q2")));
    const DwOpt qo = DwOpt().clip_in(clip_on() ? &cgs : nullptr);
    for (int n = 0; n < 2; ++n) {
      Net& Q = net(n ? "q2" : "q1");
      dw(pg, Q.layers[3], cr.dq[n], {cr.c2[n]}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
      View d1 = cr.hdx ? cr.d1f[n] : dx(pg, {{cr.dz2[n], &Q.layers[2], 0}}, H, B, actC, &cr.c1z[n]);
      dw(pg, Q.layers[2], cr.dz2[n], {cr.c1[n]}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
      // (read by the weight gradient / the norm backward only: the T / the N image alone)
      View g01 = dx(pg, {{d1, &Q.layers[1], 0}}, H, B, DxOpt().nb_defer(nbd ? &cr.c01[n] : nullptr).images(!nbd, nbd));
      dw(pg, Q.layers[1], d1, {cr.c01[n], ac.fzsa, ac.fzs}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
      if (nbd) {  // AvgL1Norm backward deferred into the weight-gradient GEMM (kDwNb)
        dw(pg, Q.layers[0], g01, {sb.s, act_in}, B, CNT_ADAM_Q, cfg.critic_lr, DwOpt().nb_defer(&cr.c01[n]));
      } else {
        View dx01 = normbwd(pg, g01, cr.c01[n]);
        dw(pg, Q.layers[0], dx01, {sb.s, act_in}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
      }
    }
    if (clip_on()) clip_close(pg, cgs);
  }
  // Upper bound on the tiles of an EPI_QHEAD GEMM over B rows (its loss partial slots).
  int qhead_tiles(const Layer& L) const { return cdiv(B, kTileM) * cdiv(L.out, kTileM); }
  // Policy pass (td7.py:259-276) through the updated critics (no weight gradient of these layers), the actor's
  // backward + Adam
  void td7_policy(Prog& pg, StepBuild& sb, const Td7Actor& ac) {
    Net& fe = net("fixed_encoder");
    Net& pi = net("policy");
    Net* q[2] = {&net("q1"), &net("q2")};
    const Layer* qo[2] = {&q[0]->layers[3], &q[1]->layers[3]};
    const View &s = sb.s, &a_pi = ac.a_pi, &fzs = ac.fzs;
    const bool nbd = td7_nb_defer(), fold = td7_fold();
    const FwdOpt fo = FwdOpt().no_t();
    View pa1z, pa2z;
    View pa1 = fwd(pg, fe.layers[3], {{fzs}, {a_pi}}, B, actE, FwdOpt(fo).keep_pre(&pa1z));
    View pa2 = fwd(pg, fe.layers[4], {{pa1}}, B, actE, FwdOpt(fo).keep_pre(&pa2z));
    View pzsa = fwd(pg, fe.layers[5], {{pa2}}, B, ACT_NONE, fo);
    View p01[2], p1[2], p1z[2], dzp2[2];
    for (int n = 0; n < 2; ++n) {
      p01[n] = fwd(pg, q[n]->layers[0], {{s}, {a_pi}}, B, ACT_NONE, FwdOpt(fo).norm());
      p1[n] = fwd(pg, q[n]->layers[1], {{p01[n]}, {pzsa}, {fzs}}, B, actC, FwdOpt(fo).keep_pre(&p1z[n]));
    }
    // q2 + q3 + dL/dQ = -1/(2B) fused (EPI_QHEAD): dZ of q2 straight from the GEMM (read by the input-gradient
    // GEMM only: no weight update here).  One loss resource per critic: the two heads share a level
    sb.ploss.id = next_id++;
    sb.ploss_id2 = next_id++;
    sb.ploss.p = mem.make<float>((size_t)(qhead_tiles(q[0]->layers[2]) + qhead_tiles(q[1]->layers[2])));
    for (int n = 0; n < 2; ++n) {
      LossPart slot{sb.ploss.p + sb.ploss.n, 0, n ? sb.ploss_id2 : sb.ploss.id};
      dzp2[n] = fwd(pg, q[n]->layers[2], {{p1[n]}}, B, actC, FwdOpt(fo).q_head(qo[n], -0.5f / (float)Bv, &slot));
      sb.ploss.n += slot.n;
    }
    // ---- offline (rle_config bc_lambda): + lmbda * mean|cat Q|.detach() * mse(pi(s), a).  dL/dq stays
    // -1/(2B) (q_abs is detached), so the q-heads above are the online ones.  The per-row q for q_abs: the
    // same layers once more with the EPI_QDOT epilogue, beside the q-heads (same level, nothing waits for
    // them but OP_BC); OP_BC a level later forms q_abs, bc and e = dL_bc / d pi, which the action gradient
    // below reads several levels on.
    if (offline()) {
      add_bc(pg, sb, 0, cfg.bc_lambda, &a_pi);
      View pq[2];
      for (int n = 0; n < 2; ++n) pq[n] = fwd(pg, q[n]->layers[2], {{p1[n]}}, B, actC, FwdOpt(fo).q_dot(qo[n]));
      add_bc(pg, sb, 1, 0.f, pq, qo);
    }
    View dzp1[2], dxp01[2];
    const DxOpt po = DxOpt().no_t();  // (no weight gradient of the critics or the fixed encoder in the policy pass)
    for (int n = 0; n < 2; ++n) {
      dzp1[n] = dx(pg, {{dzp2[n], &q[n]->layers[2], 0}}, H, B, actC, &p1z[n], po);
      View g = dx(pg, {{dzp1[n], &q[n]->layers[1], 0}}, H, B, po);
      dxp01[n] = normbwd(pg, g, p01[n], NormBwdOpt().no_t());
    }
    // grad wrt zsa from both critics (q1 input columns [H, 2H))
    View dpa2;
    if (fold) {  // d zsa -> d pa2 through zsa3 folded: G_n = q_n.q1[:, zsa block] x fe.zsa3 (updated critics)
      View G[2];
      for (int n = 0; n < 2; ++n)
        G[n] = dx(pg, {{wview_n(q[n]->layers[1], Hp, H), &fe.layers[5], 0}}, H, H);  // (a T-image operand below)
      dpa2 = dx(pg, {{dzp1[0], nullptr, 0, &G[0]}, {dzp1[1], nullptr, 0, &G[1]}}, H, B, actE, &pa2z, po);
    } else {
      View gzsa = dx(pg, {{dzp1[0], &q[0]->layers[1], Hp}, {dzp1[1], &q[1]->layers[1], Hp}}, Z, B);
      dpa2 = dx(pg, {{gzsa, &fe.layers[5], 0}}, H, B, actE, &pa2z);
    }
    View dpa1 = dx(pg, {{dpa2, &fe.layers[4], 0}}, H, B, actE, &pa1z, po);
    // d action = sum of three paths, then tanh' (actor output)
    std::vector<DxTerm> t3{
        {dxp01[0], &q[0]->layers[0], Sp}, {dxp01[1], &q[1]->layers[0], Sp}, {dpa1, &fe.layers[3], Zp}};
    // (offline: e0 x (q_abs I), the behaviour-cloning gradient wrt pi, one more reduction segment ahead of
    // tanh' -- in the in-tile recomputation below as well, so RLE_FUSE_PRE stays)
    if (offline()) t3.push_back({sb.bc_e, nullptr, 0, &sb.bc_eye});
    View dl3 = dx(pg, t3, A, B, ACT_TANH, &a_pi);
    const PreUse p3 = ac.prea ? pre_actor_dx(t3, A, a_pi, 0) : PreUse{};  // dl2 recomputes dl3 in-tile
    // input-grads through a layer are emitted BEFORE its Adam update so the
    // scheduler orders them against the pre-update weights (as autograd does)
    View ap2s = ac.ap2.sub(0, B), ap1s = ac.ap1.sub(0, B);
    const View ap2zs = act_zsaved(actP) ? ac.ap2z.sub(0, B) : View{}, ap1zs = act_zsaved(actP) ? ac.ap1z.sub(0, B) : View{};
    View dl2 = dx(pg, {{dl3, &pi.layers[3], 0}}, H, B, actP, dsrc_of(actP, ap2s, ap2zs),
                  DxOpt().pre_gemm(ac.prea ? &p3 : nullptr));
    ClipGroup cgs;  // (gradient clipping: optim_policy's clip group)
    if (clip_on()) cgs = clip_group(1, layer_ptrs(pi));
    const DwOpt pio = DwOpt().clip_in(clip_on() ? &cgs : nullptr);
    dw(pg, pi.layers[3], dl3, {ap2s}, B, CNT_ADAM_PI, cfg.policy_lr, pio);
    View dl1 = dx(pg, {{dl2, &pi.layers[2], 0}}, H, B, actP, dsrc_of(actP, ap1s, ap1zs));
    dw(pg, pi.layers[2], dl2, {ap1s}, B, CNT_ADAM_PI, cfg.policy_lr, pio);
    const View ap0s = ac.ap0.sub(0, B);
    View gl0 = dx(pg, {{dl1, &pi.layers[1], 0}}, H, B, DxOpt().nb_defer(nbd ? &ap0s : nullptr).images(!nbd, nbd));
    dw(pg, pi.layers[1], dl1, {ap0s, fzs}, B, CNT_ADAM_PI, cfg.policy_lr, pio);
    if (nbd) {
      dw(pg, pi.layers[0], gl0, {s}, B, CNT_ADAM_PI, cfg.policy_lr, DwOpt().nb_defer(&ap0s));
    } else {
      View dl0 = normbwd(pg, gl0, ap0s);
      dw(pg, pi.layers[0], dl0, {s}, B, CNT_ADAM_PI, cfg.policy_lr, pio);
    }
    if (clip_on()) clip_close(pg, cgs);
  }
  // Step end: info row [encoder, q_fn, policy] (offline: + [bc, q_abs])
  void td7_step_end(Prog& pg, const StepBuild& sb) {
    Op op = step_end_op();
    StepEndArgs& a = op.end;
    info_sum(a, 0, sb.enc_loss.p, sb.enc_loss.n, 1, 1.f / (float)((long long)Bv * Z));
    info_sum(a, 1, sb.qloss.p, sb.qloss.n, 1, (cfg.use_lap ? 1.f : 0.5f) / (float)Bv);
    if (sb.policy) info_sum(a, 2, sb.ploss.p, sb.ploss.n, 1, -0.5f / (float)Bv);
    else a.kind[2] = INFO_NAN;
    a.ninfo = 3;
    std::vector<int> rd{sb.enc_loss.id, sb.qloss.id};
    if (sb.policy) rd.insert(rd.end(), {sb.ploss.id, sb.ploss_id2});
    if (offline()) info_offline(a, rd, sb);
    std::vector<int> cn{CNT_ADAM_Q, CNT_ADAM_ENC, 3, CNT_RNG, CNT_TAPE};
    if (sb.policy) cn.push_back(CNT_ADAM_PI);
    add_step_end(pg, op, rd, cn);
  }
  void build_td7(Prog& pg, bool policy, int set) {
    StepBuild sb = begin_step(pg, policy, set);
    td7_encoder_update(pg, sb);
    const Td7Actor ac = td7_fixed_and_actor(pg, sb);
    const TwinViews th = td7_target(pg, sb, ac);
    const Td7Critics cr = td7_critics(pg, sb, ac, th);
    td7_critic_backward(pg, sb, ac, cr);
    if (policy) td7_policy(pg, sb, ac);
    td7_step_end(pg, sb);
  }


  // Algebraic folds of TD7's linear zsa3 layer into its consumers (build_td7): on when
  // every block is 16-aligned and zs_dim = hdim (the folded block replaces the zsa block in place).
  // Without RLE_FUSE_FOLD: the unfolded programs (tests).
  bool td7_fold() const {
    return algo == RLE_TD7 && H % 16 == 0 && Z == H && fused(RLE_FUSE_FOLD);
  }
  // The actor's tanh output layer (N = act_dim <= 32) recomputed in-tile by the consumers on
  // the critical path (PreArgs).  Without RLE_FUSE_PRE: separate ops (tests).
  bool actor_pre() const { return A <= 32 && fused(RLE_FUSE_PRE); }
  // The critics' and target critics' last hidden layers emit EPI_QDOT row partials of q, so the
  // loss head reads 2 x 16 floats per row instead of 4 rows of H.  RLE_NO_QDOT=1: row loads (A/B).
  bool td7_qdot() const { return fused(RLE_FUSE_QDOT); }
  // The critic loss head fused into the DX of the critics' second hidden layers (HeadUse):
  // H <= 256, B a multiple of 16.  without RLE_FUSE_HEADDX: the standalone head (tests, A/B).
  bool td7_headdx() const {
    return algo == RLE_TD7 && H <= 256 && H % 16 == 0 && B % 16 == 0 && fused(RLE_FUSE_HEADDX);
  }
  // AvgL1Norm backwards that feed only a weight-gradient GEMM are applied inside it
  // (EPI_NBDOT producer + kDwNb consumer: one level fewer).  RLE_NO_NBDEFER=1: separate
  // OP_NORMBWD (tests).
  bool td7_nb_defer() const { return B <= 1024 && fused(RLE_FUSE_NBDEFER); }
  View tfold_w[2], tfold_b[2];  // per target critic: q1[:, zsa block] x fet.zsa3, folded q1 bias
  bool fold_dirty = true;       // parameters written from the host since the last fold
  Graph g_fold;
  void alloc_folds() {
    if (!td7_fold()) return;
    for (int n = 0; n < 2; ++n) {
      tfold_w[n] = buf(H, H);
      tfold_b[n] = vec(H);
    }
  }
  // tq_n.q1 applied to zsa3(x) = (W1[:, zsa] W3) x + (b1 + W1[:, zsa] b3): the target
  // critics and the fixed target encoder change only at hard updates (and host loads)
  void add_target_fold(Prog& pg) {
    Net& fet = net("fixed_encoder_target");
    for (int n = 0; n < 2; ++n) {
      const Layer& L1 = net(n ? "target_q2" : "target_q1").layers[1];
      const Layer& L3 = fet.layers[5];
      dx(pg, {{wview_n(L1, L1.seg_p[0], H), &L3, 0}}, H, H, DxOpt().out_into(&tfold_w[n]));
      Op op{};
      op.kind = OP_FOLDBIAS;
      FoldBiasArgs& f = op.fb;
      f.wn = P + L1.wn_off;
      f.cbn = L1.cb;
      f.col0 = L1.seg_p[0];
      f.H = H;
      f.bin = bias(L3);
      f.bbase = bias(L1);
      f.bout = tfold_b[n].p;
      op.wg_count = 1;
      pg.add(op, {L1.res, L3.res}, {tfold_b[n].id});
    }
  }

  void build_td7_hard(Prog& pg) {  // td7.py:278-285, 325-331
    flat(pg, OP_COPY, net("target_q1"), &net("q1"), 0.f, false);
    flat(pg, OP_COPY, net("target_q2"), &net("q2"), 0.f, false);
    flat(pg, OP_COPY, net("fixed_encoder_target"), &net("fixed_encoder"), 0.f, false);
    flat(pg, OP_COPY, net("fixed_encoder"), &net("encoder"), 0.f, false);
    if (td7_fold()) add_target_fold(pg);
    Op c{};
    c.kind = OP_CTRL;
    c.ctrl.mode = 0;
    c.ctrl.vmax_key = &ctrl->vmax_key;
    c.ctrl.vmin_key = &ctrl->vmin_key;
    c.ctrl.vt = ctrl->vt;
    c.wg_count = 1;
    pg.add(c, {R_VKEYS}, {R_VT});
    if (cfg.use_lap) add_reset_maxp(pg);
  }

  void add_reset_maxp(Prog& pg) {
    Replay& rp = *replay;
    Op a{};
    a.kind = OP_MAXRED;
    a.flat.src = rp.priority;
    a.flat.size = rp.size_d;
    a.flat.partial = rp.maxred_part;
    a.flat.nwg = rp.maxred_nwg;
    a.flat.stage = 0;
    a.wg_count = rp.maxred_nwg;
    int pid = next_id++;
    pg.add(a, {R_PRIO}, {pid});
    Op b = a;
    b.flat.stage = 1;
    b.flat.out = rp.maxp_d;
    b.wg_count = 1;
    pg.add(b, {pid}, {R_MAXP});
  }

  // MLP critic stack forward (mlp.py:98-101 over make_mlp's layers): hs[i] = hidden layer i's output
  // qd: the last hidden layer also emits EPI_QDOT row partials of q (a fused head reads them)
  // Behind a pre-GEMM (TD3's target critics: a' computed in-tile from the actor's last hidden layer),
  // the first layer is recomputed in-tile by the second too, its a' segment first (two-stage prologue,
  // GemmArgs::has_pre 4, whose epilogue is the q partials: two hidden layers only): the target branch's
  // first layer costs no level of its own.  Without the fusion it is its own level, in at most 32-wide
  // tiles (FwdOpt::pl_src), so both give the same floats.
  // hz: the pre-activations too when the backward needs them (ELU critics; the last layer's with an N image,
  // for the loss head's rows)
  // out_t: the outputs keep a T image (false: a forward-only pass, no weight gradient reads them)
  void mlp_critic_fwd(Prog& pg, Net& Q, const View& sv, const View& av, std::vector<View>& hs, bool out_t,
                      const PreUse* pre = nullptr, bool last_t = true, bool qd = false, std::vector<View>* hz = nullptr) {
    const int D = (int)Q.layers.size() - 1;
    hs.assign(D, View{});
    if (hz) hz->assign(D, View{});
    auto zp = [&](int i) { return hz && act_zsaved(actC) ? &(*hz)[i] : nullptr; };
    const bool shape = prelayer_shape(Q.layers[0], Q.layers[1]);
    // (the pre-GEMM's a' segment is one column block, kernels.hip PK 4 / gemm_finalize's two-stage REQUIRE)
    const bool two = pre && pre->kind == 1 && pre->a.mode == GEMM_FWD && pre->a.N <= 32 && r16(A) <= 16 && qd &&
                     D == 2 && prelayer_ok(Q.layers[0], Q.layers[1]) && fused(RLE_FUSE_TWOSTAGE);
    // (not behind a pre-GEMM: the first layer's own a segment is recomputed in-tile already)
    const bool use_pl = !pre && prelayer_ok(Q.layers[0], Q.layers[1]);
    if (two) {
      hs[0] = buf(B, Q.layers[0].out, true, false);  // (layout of the consumer's A operand only: never stored)
    } else {
      hs[0] = fwd(pg, Q.layers[0], {{sv}, {av}}, B, actC,
                  FwdOpt().keep_pre(zp(0), D == 1).pre_gemm(pre).keep_t(out_t).pl_source(use_pl || (pre && shape)));
    }
    for (int i = 1; i < D; ++i) {
      const bool last = i == D - 1;
      PreUse pl = i == 1 && (use_pl || two) ? pre_layer(Q.layers[0], {sv, av}, two ? pre->a.seg : -1) : PreUse{};
      if (i == 1 && two) {
        pl.kind = 4;
        pl.a2 = pre->a;
        pl.rd.insert(pl.rd.end(), pre->rd.begin(), pre->rd.end());
      }
      // (last_t = false: only the head reads the last layer, in the N image)
      hs[i] = fwd(pg, Q.layers[i], {{hs[i - 1]}}, B, actC,
                  FwdOpt().keep_pre(zp(i), last).pre_gemm(pl.kind >= 3 ? &pl : nullptr)
                      .q_dot(last && qd ? &Q.layers[D] : nullptr).keep_t(out_t && (!last || last_t)));
    }
  }
  // The stack with LayerNorm critics (rle_set_layer_norm): per hidden layer the Linear with the identity epilogue
  // (N image only: the norm is its one reader), then OP_LN -- one more level per layer.  M rows, the first nvalid
  // of them real.  us / rs: the normalised rows and rstd of every layer, for the backward (null: forward only).
  // pass2: critic dropout's pass * 2 + twin of this stack (DROP_*; negative: no dropout -- rle_eval).
  void mlp_critic_fwd_ln(Prog& pg, Net& Q, const View& sv, const View& av, int M, int nvalid, std::vector<View>& hs,
                         int pass2, bool out_t, bool last_t = true, std::vector<View>* us = nullptr,
                         std::vector<View>* rs = nullptr) {
    const int D = (int)Q.layers.size() - 1;
    hs.assign(D, View{});
    if (us) us->assign(D, View{}), rs->assign(D, View{});
    for (int i = 0; i < D; ++i) {
      const View z = i ? fwd(pg, Q.layers[i], {{hs[i - 1]}}, M, ACT_NONE, FwdOpt().no_t())
                       : fwd(pg, Q.layers[0], {{sv}, {av}}, M, ACT_NONE, FwdOpt().no_t());
      hs[i] = ln_fwd(pg, z, Q.layers[i].out, nvalid, actC,
                     LnOpt().keep_t(out_t && (i < D - 1 || last_t)).keep_bwd(us ? &(*us)[i] : nullptr, us ? &(*rs)[i] : nullptr)
                         .drop(pass2 < 0 ? 0.f : drop_p, pass2 < 0 ? 0 : pass2 * 8 + i));
    }
  }
  // rle_eval(RLE_EVAL_Q) on a LayerNorm critic: the stack above and the H -> 1 layer
  View mlp_critic_eval_ln(Prog& pg, Net& Q, const View& sv, const View& av, int M, int nvalid) {
    std::vector<View> hs;
    mlp_critic_fwd_ln(pg, Q, sv, av, M, nvalid, hs, /*pass2 (inference: no dropout)*/ DROP_NONE, /*out_t*/ false);
    return fwd(pg, Q.layers.back(), {{hs.back()}}, M, ACT_NONE);
  }
  // TD3 / SAC: the critic loss head and the actor objective's head fused into the DX of each
  // critic's last hidden layer (GemmArgs::has_pre 2; one level fewer on the critic chain and on
  // the policy chain).  without RLE_FUSE_HEADDX: the standalone heads (tests, A/B).
  // SAC: the rsample as the epilogue of the actor's raw head (without RLE_FUSE_SACFWD: OP_SAC_ACTOR, A/B)
  // (kernels.hip sacraw_*: three column blocks over R <= 256, gemm_finalize's REQUIRE; wider heads or larger
  // hidden layers take OP_SAC_ACTOR)
  bool sac_fwd_fused() const { return fused(RLE_FUSE_SACFWD) && 2 * A <= 48 && H <= 256; }
  // SAC: the actor backward as the epilogue of the da DX (without RLE_FUSE_SACBWD: OP_SAC_ACTOR_BWD, A/B)
  bool sac_bwd_fused() const { return fused(RLE_FUSE_SACBWD); }
  bool mlp_headdx() const { return fused(RLE_FUSE_HEADDX) && B % 16 == 0 && H <= 256 && H % 4 == 0; }
  // q partials of the twins (and target twins) into a head fused by headdx
  static void set_head_parts(HeadArgs& h, const View* q, const View* t, std::vector<int>& rd) {
    for (int n = 0; n < 2; ++n) {
      h.qp[n] = q[n].qd;
      h.qp_n[n] = q[n].qd_n;
      rd.push_back(q[n].qd_id);
      if (t) {
        h.tp[n] = t[n].qd;
        h.tp_n[n] = t[n].qd_n;
        rd.push_back(t[n].qd_id);
      }
    }
    h.qp_ld = q[0].qd_ld;
    h.tp_ld = t ? t[0].qd_ld : 0;
    REQUIRE(q[1].qd_ld == h.qp_ld && (!t || t[1].qd_ld == h.tp_ld), "head: q partial layout");
  }

  // SAC temperature operand of the heads and the actor backward: log_alpha (autotune, the
  // trained parameter), or fp32(tmp) itself for a fixed temperature -- the reference multiplies
  // by the Python float (sac.py:189, 227), so exp(log(tmp)) would be an ulp off
  float* alpha_fixed = nullptr;
  const float* alpha_src() {
    if (cfg.tmp < 0.f) return P + (nP - 4);
    if (!alpha_fixed) {
      alpha_fixed = mem.make<float>(1);
      HIPCHK(hipMemcpy(alpha_fixed, &cfg.tmp, 4, hipMemcpyHostToDevice));
    }
    return alpha_fixed;
  }

  // ---- TD3 (td3.py:206-242) and SAC (sac.py:251-295): build_mlp below is the list of these phases.
  // Actor on [s; s'] (the target policy aliases the policy, Q1; SAC's policy is unchanged until its step) with
  // the TD3 (tanh + target smoothing noise) or the SAC (rsample) head.  The later phases read:
  struct MlpActor {
    std::vector<View> h, hz;  // the hidden layers' outputs on [s; s'] (hz: an ELU actor's pre-activations)
    View raw, logpi;          // SAC: the raw head (mean | log_std) and log pi of the sampled actions
    View a_pi, a_next;        // the action on s; on s' (behind a pre-GEMM: layout only)
    bool prea = false;        // TD3: the target critics' first layer recomputes a' in-tile (pre-GEMM, as TD7)
    PreUse pn1, psac;         // that pre-GEMM; SAC's, from the raw head (has_pre 5)
    const PreUse* tpre() const { return prea ? &pn1 : (psac.kind == 5 ? &psac : nullptr); }
  };
  MlpActor mlp_actor(Prog& pg) {
    const bool sac = algo == RLE_SAC;
    const int B2 = 2 * B, D = (int)HS.size();  // make_mlp's depth (mlp.py:24-35): D hidden layers, then Lout
    Net& pi = net("policy");
    const Layer& Lout = pi.layers[D];
    MlpActor o;
    std::vector<View>&h = o.h, &hz = o.hz;
    h.resize(D), hz.resize(D);
    const bool pz = act_zsaved(actP);
    const bool pl01 = prelayer_ok(pi.layers[0], pi.layers[1]);  // (the second layer recomputes the first in-tile)
    h[0] = fwd(pg, pi.layers[0], {{ss}}, B2, actP, FwdOpt().keep_pre(pz ? &hz[0] : nullptr).pl_source(pl01));
    const PreUse pl0 = pl01 ? pre_layer(pi.layers[0], {ss}) : PreUse{};
    for (int i = 1; i < D; ++i)
      h[i] = fwd(pg, pi.layers[i], {{h[i - 1]}}, B2, actP,
                 FwdOpt().keep_pre(pz ? &hz[i] : nullptr).pre_gemm(i == 1 && pl0.kind == 3 ? &pl0 : nullptr));
    const View hl = h[D - 1];  // the last hidden layer's output
    View actv;
    o.prea = !sac && actor_pre();
    const View h1n = hl.sub(B, B);
    if (o.prea) o.pn1 = pre_actor_fwd(Lout, h1n, &eps, 1);
    if (!sac) {
      actv = o.prea ? fwd(pg, Lout, {{hl.sub(0, B)}}, B, ACT_TANH)
                    : fwd(pg, Lout, {{hl}}, B2, ACT_TANH, FwdOpt().noised(&eps, B));
    } else if (sac_fwd_fused()) {  // the rsample in the raw head's epilogue (one level fewer)
      actv = buf(B2, A);
      o.logpi = vec(B2);
      SacFwdUse sfu{};
      SacFwdArgs& a = sfu.a;
      a.eps = eps.m;
      a.eps2 = eps2.m;
      a.act = actv.m;
      a.logpi = o.logpi.p;
      a.min_log_std = cfg.min_log_std;
      a.max_log_std = cfg.max_log_std;
      a.A = A;
      a.mean_off = 0;
      a.ls_off = A;
      a.eps_row_split = B;
      sfu.rd = {eps.id, eps2.id};
      sfu.wr = {actv.id, o.logpi.id};
      o.raw = fwd(pg, Lout, {{hl}}, B2, ACT_NONE, FwdOpt().sac_fwd(&sfu));
    } else {
      o.raw = fwd(pg, Lout, {{hl}}, B2, ACT_NONE);
      actv = buf(B2, A);
      o.logpi = vec(B2);
      Op op = sac_actor_op(OP_SAC_ACTOR, o.raw.m, B2);
      SacActorArgs& a = op.sac;
      a.eps = eps.m;
      a.eps2 = eps2.m;
      a.eps_row_split = B;
      a.act = actv.m;
      a.logpi = o.logpi.p;
      pg.add(op, {o.raw.id, eps.id, eps2.id}, {actv.id, o.logpi.id});
    }
    o.a_pi = actv.sub(0, B);
    o.a_next = o.prea ? o.a_pi : actv.sub(B, B);
    if (sac && sac_pre()) o.psac = pre_sac_fwd(Lout, h1n, eps, 1);
    return o;
  }
  // Target critics (forward only) and y, the online critics and the loss head (td3.py:160-164, sac.py:188-193:
  // y per row, then the loss), the priority update and the next step's batch.  The backward reads:
  struct MlpCritics {
    std::vector<View> c[2], cz[2];  // the hidden layers' outputs and (ELU critics) pre-activations
    std::vector<View> crs[2];       // LayerNorm critics: cz holds the normalised rows u, crs their rstd
    View dz1[2], dq[2];             // the head's gradients: dZ of the last hidden layer, dq
    bool hdx = false;               // the head ran inside the DX of each critic's last hidden layer, ...
    View d0f[2];                    // ... which gave dZ of the layer before
  };
  MlpCritics mlp_critics(Prog& pg, StepBuild& sb, const MlpActor& ac) {
    const bool sac = algo == RLE_SAC;
    const int D = (int)HS.size();
    Net* q[2] = {&net("q1"), &net("q2")};
    Net* tq[2] = {&net("target_q1"), &net("target_q2")};
    const bool lap = cfg.use_lap && !sac;
    MlpCritics o;
    std::vector<View> th[2];
    o.hdx = mlp_headdx();
    const bool ln = ln_on();
    REQUIRE(!ln || !o.hdx, "LayerNorm critics: the heads run stand-alone");
    for (int n = 0; n < 2; ++n)  // (forward only)
      if (ln) mlp_critic_fwd_ln(pg, *tq[n], sb.s2, ac.a_next, B, Bv, th[n], DROP_TARGET * 2 + n, /*out_t*/ false);
      else mlp_critic_fwd(pg, *tq[n], sb.s2, ac.a_next, th[n], /*out_t*/ false, ac.tpre(), true, o.hdx);
    for (int n = 0; n < 2; ++n)
      if (ln) mlp_critic_fwd_ln(pg, *q[n], sb.s, act_in, B, Bv, o.c[n], DROP_ONLINE * 2 + n, /*out_t*/ true, true, &o.cz[n], &o.crs[n]);
      else mlp_critic_fwd(pg, *q[n], sb.s, act_in, o.c[n], /*out_t*/ true, nullptr, true, o.hdx, &o.cz[n]);
    // (the loss head's derivative rows: ELU' reads the pre-activation; ReLU' / identity the output.  LayerNorm
    // critics: the head leaves dh = dq w, no derivative -- OP_LN_BWD takes act' from u)
    const bool cze = act_zsaved(actC) && !ln;
    // (the last hidden layers and the heads' layers)
    const View c1[2] = {o.c[0][D - 1], o.c[1][D - 1]}, th1[2] = {th[0][D - 1], th[1][D - 1]};
    const View cz1[2] = {o.cz[0][D - 1], o.cz[1][D - 1]};
    const Layer *qo[2] = {&q[0]->layers[D], &q[1]->layers[D]}, *tqo[2] = {&tq[0]->layers[D], &tq[1]->layers[D]};
    LossHead lh = loss_head(sb, HEAD_MLP_LOSS, HEAD_MLP_TARGET, c1, cze ? cz1 : c1, th1, qo, tqo, o.hdx, lap);
    HeadArgs& h = lh.op.head;
    if (ln) h.dact = ACT_NONE;
    if (sac) set_head_sac(h, ac.logpi, B, lh.rd);  // (the next-state rows)
    if (cze) lh.rd.insert(lh.rd.end(), {cz1[0].id, cz1[1].id});
    for (int n = 0; n < 2; ++n) o.dz1[n] = lh.dz[n], o.dq[n] = lh.dq[n];
    if (!o.hdx) {
      pg.add(lh.op, lh.rd, {lh.dz[0].id, lh.dz[1].id, lh.dq[0].id, lh.dq[1].id, lh.prio.id, sb.qloss.id});
    } else {
      // the head runs inside the DX of each critic's last hidden layer; critic 0's op stores the
      // priorities and loss partials
      set_head_parts(h, c1, th1, lh.rd);
      for (int n = 0; n < 2; ++n) {
        HeadUse hu{h, n, lh.rd, {lh.dz[n].id, lh.dq[n].id}};
        if (n == 0) hu.wr.insert(hu.wr.end(), {lh.prio.id, sb.qloss.id});
        // (the head forms dZ = dq w act'(segment 0): an ELU critic's pre-activations, a ReLU critic's outputs)
        o.d0f[n] = dx(pg, {{cze ? cz1[n] : c1[n], &q[n]->layers[D - 1], 0}}, HS[D - 2], B, actC,
                      dsrc_of(actC, o.c[n][D - 2], o.cz[n][D - 2]), DxOpt().head_use(&hu));
      }
    }
    add_update_and_prefetch(pg, sac, sb.set, lap, lh.prio);
    return o;
  }
  // Critic backward + Adam (input gradients through a layer before its Adam update)
  void mlp_critic_backward(Prog& pg, const StepBuild& sb, const MlpCritics& cr) {
    const int D = (int)HS.size();
    ClipGroup cgs;  // (gradient clipping: the critics' optimizer, q1 + q2 together)
    if (clip_on()) cgs = clip_group(0, layer_ptrs(net("q1"), &net("q2")));
    const DwOpt qo = DwOpt().clip_in(clip_on() ? &cgs : nullptr);
    for (int n = 0; n < 2; ++n) {
      Net& Q = net(n ? "q2" : "q1");
      dw(pg, Q.layers[D], cr.dq[n], {cr.c[n][D - 1]}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
      if (ln_on()) {
        // dh of hidden layer i (the head's, then an input gradient with no mask) -> OP_LN_BWD -> dZ of its Linear,
        // which the layer's weight gradient (T image) and the next input gradient (N image) read
        View dh = cr.dz1[n];
        for (int i = D - 1; i >= 0; --i) {
          const View dzi = ln_bwd(pg, dh, cr.cz[n][i], cr.crs[n][i], Q.layers[i].out, Bv, actC,
                                  LnOpt().keep_t(true).drop(drop_p, drop_site(DROP_ONLINE, n, i)));
          if (i) dh = dx(pg, {{dzi, &Q.layers[i], 0}}, HS[i - 1], B, DxOpt().no_t());
          if (i) dw(pg, Q.layers[i], dzi, {cr.c[n][i - 1]}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
          else dw(pg, Q.layers[0], dzi, {sb.s, act_in}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
        }
        continue;
      }
      View d = cr.dz1[n];  // dZ of hidden layer i, from i = D - 1 down
      for (int i = D - 1; i >= 1; --i) {
        const View dp = cr.hdx && i == D - 1 ? cr.d0f[n]
                                              : dx(pg, {{d, &Q.layers[i], 0}}, HS[i - 1], B, actC,
                                                   dsrc_of(actC, cr.c[n][i - 1], cr.cz[n][i - 1]));
        dw(pg, Q.layers[i], d, {cr.c[n][i - 1]}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
        d = dp;
      }
      dw(pg, Q.layers[0], d, {sb.s, act_in}, B, CNT_ADAM_Q, cfg.critic_lr, qo);
    }
    if (clip_on()) clip_close(pg, cgs);
  }
  // Policy pass through the updated critics, the objective's head, the actor's backward + Adam
  void mlp_policy(Prog& pg, StepBuild& sb, const MlpActor& ac) {
    const bool sac = algo == RLE_SAC;
    const int D = (int)HS.size();
    Net* q[2] = {&net("q1"), &net("q2")};
    const Layer* qo[2] = {&q[0]->layers[D], &q[1]->layers[D]};
    const View &s = sb.s, &a_pi = ac.a_pi, &raw = ac.raw;
    const bool ln = ln_on();
    const bool hdx = mlp_headdx(), cze = act_zsaved(actC) && !ln;
    REQUIRE(!ln || !hdx, "LayerNorm critics: the heads run stand-alone");
    std::vector<View> pc[2], pcz[2], prs[2];  // (LayerNorm critics: pcz holds u, prs rstd)
    for (int n = 0; n < 2; ++n)
      // (LayerNorm critics: no T image at all -- no weight gradient here, and no input gradient reads a mask)
      if (ln) mlp_critic_fwd_ln(pg, *q[n], s, a_pi, B, Bv, pc[n], DROP_POLICY * 2 + n, /*out_t*/ false, false, &pcz[n], &prs[n]);
      else mlp_critic_fwd(pg, *q[n], s, a_pi, pc[n], /*out_t*/ true, nullptr, /*last_t*/ false, hdx, &pcz[n]);
    const View p1[2] = {pc[0][D - 1], pc[1][D - 1]};
    // (no weight gradient of the critics in the policy pass: the gradients keep N images only)
    const DxOpt po = DxOpt().no_t();
    View dzp1[2];
    if (!hdx) dzp1[0] = buf(B, H, true, false), dzp1[1] = buf(B, H, true, false);
    sb.ploss.n = cdiv(B, 4);  // (4 partials per head workgroup)
    sb.ploss.p = mem.make<float>((size_t)sb.ploss.n * 4);
    // the objective's head: inside the DX of each critic's last hidden layer (hdx: critic 0's op stores the loss
    // partials), or standalone, forming dZ of the last hidden layers (dzp1) itself
    Op op = head_op(HEAD_MLP_POLICY, Bv);
    HeadArgs& h = op.head;
    set_head_twin(h, p1[0], p1[1], *qo[0], *qo[1]);
    h.dact = ln ? ACT_NONE : actC;  // (LayerNorm critics: dzp1 is dh = dq w; OP_LN_BWD takes act' from u)
    h.loss_part = sb.ploss.p;
    std::vector<int> rd{p1[0].id, p1[1].id, qo[0]->res, qo[1]->res};
    if (!hdx) {
      for (int n = 0; n < 2; ++n) {
        h.dsrc[n] = (cze ? pcz[n][D - 1] : p1[n]).m;
        h.dz[n] = dzp1[n].m;
      }
      if (cze) rd.insert(rd.end(), {pcz[0][D - 1].id, pcz[1][D - 1].id});
    }
    if (sac) set_head_sac(h, ac.logpi, 0, rd);
    if (hdx) set_head_parts(h, p1, nullptr, rd);
    sb.ploss.id = next_id++;
    if (!hdx) pg.add(op, rd, {dzp1[0].id, dzp1[1].id, sb.ploss.id});
    View dzp0[2];
    for (int n = 0; n < 2 && !ln; ++n) {
      HeadUse hu{h, n, rd, {}};
      if (n == 0) hu.wr.push_back(sb.ploss.id);
      // (the fused head forms dZ = dq w act'(segment 0), as the loss head's)
      const View& z = hdx ? (cze ? pcz[n][D - 1] : p1[n]) : dzp1[n];
      dzp0[n] = dx(pg, {{z, &q[n]->layers[D - 1], 0}}, HS[D - 2], B, actC, dsrc_of(actC, pc[n][D - 2], pcz[n][D - 2]),
                   DxOpt(po).head_use(hdx ? &hu : nullptr));
    }
    // ---- offline (rle_config_ext bc_alpha): L = -lmbda mean(min Q) + mse(pi(s), a), lmbda = bc_alpha /
    // mean|min Q| (detached).  Scale at the end: the chain above and below stays the online one (dL/dq = -1/B),
    // so it carries the gradient of L / lmbda; the cloning term enters the action gradient as e0 x (q_abs /
    // bc_alpha) I (one more reduction segment ahead of tanh', TD7's construction), and the actor's Adam
    // epilogues multiply by lmbda.  OP_BC mode 0 needs the actor output alone (many levels earlier); q_abs
    // comes from the policy pass's row partials beside the fused head (mode 3) or from the standalone head's
    // |min| partials a level after it (mode 2): either way it is ready a level before the action gradient.
    if (offline3()) {
      add_bc(pg, sb, 0, 1.f, &a_pi);
      add_bc(pg, sb, hdx ? 3 : 2, bc_alpha, p1, qo);
    }
    // (LayerNorm critics: OP_LN_BWD, then the plain input gradient, per hidden layer down to dZ of the first)
    for (int n = 0; n < 2 && ln; ++n) {
      View dh = dzp1[n];
      for (int i = D - 1; i >= 0; --i) {
        dzp0[n] = ln_bwd(pg, dh, pcz[n][i], prs[n][i], q[n]->layers[i].out, Bv, actC,
                         LnOpt().drop(drop_p, drop_site(DROP_POLICY, n, i)));
        if (i) dh = dx(pg, {{dzp0[n], &q[n]->layers[i], 0}}, HS[i - 1], B, po);
      }
    }
    // (deeper critics: on down to the first hidden layer; no weight gradient reads these)
    for (int i = D - 2; i >= 1 && !ln; --i)
      for (int n = 0; n < 2; ++n)
        dzp0[n] = dx(pg, {{dzp0[n], &q[n]->layers[i], 0}}, HS[i - 1], B, actC,
                     dsrc_of(actC, pc[n][i - 1], pcz[n][i - 1]), po);
    const std::vector<DxTerm> ta0{{dzp0[0], &q[0]->layers[0], Sp}, {dzp0[1], &q[1]->layers[0], Sp}};
    View dout;
    PreUse pdout{};  // TD3: d1 recomputes dout in-tile
    if (!sac) {
      std::vector<DxTerm> ta = ta0;
      // (offline: the cloning gradient, in the in-tile recomputation as well, so RLE_FUSE_PRE stays)
      if (offline3()) ta.push_back({sb.bc_e, nullptr, 0, &sb.bc_eye});
      dout = dx(pg, ta, A, B, ACT_TANH, &a_pi);
      if (ac.prea) pdout = pre_actor_dx(ta, A, a_pi, 0);
    } else if (sac_bwd_fused()) {  // the backward in the epilogue of the DX that forms da (one level fewer)
      dout = buf(B, 2 * A);
      SacBwdUse sbu{};
      SacBwdArgs& a = sbu.a;
      a.raw = raw.m;
      a.eps2 = eps2.m;
      a.dout = dout.m;
      a.log_alpha = alpha_src();
      a.alpha_lin = cfg.tmp >= 0.f;
      a.inv_b = 1.f / (float)Bv;
      a.nvalid = Bv;
      a.min_log_std = cfg.min_log_std;
      a.max_log_std = cfg.max_log_std;
      a.mean_off = 0;
      a.ls_off = A;
      sbu.rd = {raw.id, eps2.id, R_LA};
      sbu.wr = {dout.id};
      dx(pg, ta0, A, B, DxOpt().sac_bwd(&sbu));
    } else {
      dout = buf(B, 2 * A);
      View da = dx(pg, ta0, A, B);
      Op op = sac_actor_op(OP_SAC_ACTOR_BWD, raw.m, Bv);  // (rows of the padded batch past Bv keep a zero gradient)
      SacActorArgs& a = op.sac;
      a.eps2 = eps2.m;
      a.da = da.m;
      a.dout = dout.m;
      a.log_alpha = alpha_src();
      a.alpha_lin = cfg.tmp >= 0.f;
      a.inv_b = 1.f / (float)Bv;
      pg.add(op, {raw.id, eps2.id, da.id, R_LA}, {dout.id});
    }
    mlp_actor_backward(pg, sb, ac, dout, pdout);
  }
  // Offline SAC (rle_config_ext awac_lambda, AWAC): the policy phase without a gradient through the critics.  The
  // updated critics run forward on (s, a) and on (s, a_pi) (two B-row passes each, no T images: no weight gradient
  // reads them) down to their H -> 1 layers; OP_AWAC forms adv, w and the gradient with respect to the raw head
  // (ops.h AwacArgs); the actor's backward from there is the online one.  No critic DX, no OP_SAC_ACTOR_BWD /
  // EPI_SACBWD, no policy loss head.  sb.ploss: OP_AWAC's {w logp, lp, adv, w} sums of each 4-row workgroup.
  void mlp_policy_awac(Prog& pg, StepBuild& sb, const MlpActor& ac) {
    const int D = (int)HS.size();
    Net* q[2] = {&net("q1"), &net("q2")};
    Op op{};
    op.kind = OP_AWAC;
    AwacArgs& a = op.awac;
    std::vector<int> rd{ac.raw.id, act_in.id, ac.logpi.id};
    for (int n = 0; n < 2; ++n) {
      std::vector<View> hd, hv;
      if (ln_on()) {
        mlp_critic_fwd_ln(pg, *q[n], sb.s, act_in, B, Bv, hd, DROP_AWAC_DATA * 2 + n, /*out_t*/ false);
        mlp_critic_fwd_ln(pg, *q[n], sb.s, ac.a_pi, B, Bv, hv, DROP_POLICY * 2 + n, /*out_t*/ false);
      } else {
        mlp_critic_fwd(pg, *q[n], sb.s, act_in, hd, /*out_t*/ false);
        mlp_critic_fwd(pg, *q[n], sb.s, ac.a_pi, hv, /*out_t*/ false);
      }
      const View qd = fwd(pg, q[n]->layers[D], {{hd[D - 1]}}, B, ACT_NONE, FwdOpt().no_t());
      const View qv = fwd(pg, q[n]->layers[D], {{hv[D - 1]}}, B, ACT_NONE, FwdOpt().no_t());
      a.qd[n] = qd.m;
      a.qv[n] = qv.m;
      rd.insert(rd.end(), {qd.id, qv.id});
    }
    const View dout = buf(B, 2 * A), adv = vec(B), w = vec(B);
    op.wg_count = cdiv(Bv, 4);  // (one row per wave)
    sb.ploss.n = op.wg_count;
    sb.ploss.p = mem.make<float>((size_t)sb.ploss.n * 4);
    sb.ploss.id = next_id++;
    a.raw = ac.raw.m;
    a.a = act_in.m;
    a.logpi = ac.logpi.p;
    a.dout = dout.m;
    a.adv = adv.p;
    a.w = w.p;
    a.part = sb.ploss.p;
    a.nvalid = Bv;
    a.A = A;
    a.mean_off = 0;
    a.ls_off = A;
    a.lambda = awac_lambda;
    a.min_log_std = cfg.min_log_std;
    a.max_log_std = cfg.max_log_std;
    pg.add(op, rd, {dout.id, adv.id, w.id, sb.ploss.id});
    mlp_actor_backward(pg, sb, ac, dout, PreUse{});
  }
  // The actor's backward + Adam from dout, the gradient with respect to its output layer's pre-activation
  // (pdout: TD3's in-tile recomputation of dout by the first input gradient)
  void mlp_actor_backward(Prog& pg, StepBuild& sb, const MlpActor& ac, const View& dout, const PreUse& pdout) {
    const bool sac = algo == RLE_SAC;
    const int D = (int)HS.size();
    Net& pi = net("policy");
    const Layer& Lout = pi.layers[D];
    const View& s = sb.s;
    const bool pz = act_zsaved(actP);
    int ngsq = 0;
    if (!sac) {
      // per-tile grad-square partials for norm/policy (rl/nn/utils.py:13-19)
      for (auto& L : pi.layers) ngsq += dw_gsq_w(L) + dw_gsq_b(L);
      sb.gsq = mem.make<float>(ngsq);
    }
    std::vector<int> tens;
    float* gp = sb.gsq;
    auto gsq_for = [&](const Layer& L, int t_w, int t_b) -> std::pair<float*, float*> {
      if (!sb.gsq) return {nullptr, nullptr};
      int nw = dw_gsq_w(L), nb = dw_gsq_b(L);
      float* w = gp;
      float* b = gp + nw;
      gp += nw + nb;
      for (int i = 0; i < nw; ++i) tens.push_back(t_w);
      for (int i = 0; i < nb; ++i) tens.push_back(t_b);
      return {w, b};
    };
    // actor backward: tensors in parameters() order mlp.0.w, mlp.0.b, mlp.2.w, ...
    std::vector<std::pair<float*, float*>> gl;
    for (int i = 0; i <= D; ++i) gl.push_back(gsq_for(pi.layers[i], 2 * i, 2 * i + 1));
    std::vector<View> hsub(D), hzsub(D);
    for (int i = 0; i < D; ++i) hsub[i] = ac.h[i].sub(0, B);
    if (pz)
      for (int i = 0; i < D; ++i) hzsub[i] = ac.hz[i].sub(0, B);
    // Gradient clipping: the policy optimizer's clip group.  TD3: over norm/policy's partial slots, which the norm
    // passes then fill (the gradient before clipping; offline with lmbda) and OP_CLIP adds as well
    ClipGroup cgs;
    if (clip_on()) {
      cgs = clip_group(1, layer_ptrs(pi), sb.gsq);
      if (offline3()) cgs.gin = sb.bc_s + 1, cgs.gin_id = sb.bc_s_id;
    }
    // What every weight gradient of the actor shares.  TD3: the aliased target policy's Polyak (td3.py:200-204)
    // in the Adam epilogues: one level fewer between the actor update and the next step's target action.
    // Offline TD3: the gradient scaled by lmbda (sb.bc_s[1])
    const DwOpt ao = DwOpt().polyak(!sac && pi_polyak_fused() ? cfg.tau : 0.f)
                         .grad_scale(offline3() ? sb.bc_s + 1 : nullptr, sb.bc_s_id)
                         .clip_in(clip_on() ? &cgs : nullptr);
    // SAC: d1 (the gradient through the raw head, K = 2A <= 48) recomputed in-tile by d0's DX
    const bool pld = sac && sac_bwd_fused() && prelayer_ok_dx(Lout, pi.layers[D - 1]);
    View d = dx(pg, {{dout, &Lout, 0}}, HS[D - 1], B, actP, dsrc_of(actP, hsub[D - 1], hzsub[D - 1]),
                DxOpt().pre_gemm(ac.prea ? &pdout : nullptr).pl_source(pld));
    // (d0 reads the raw head's pre-update weights when it recomputes d1: emitted before that Adam)
    const PreUse pd1 = pld ? pre_layer_dx(Lout, dout, hsub[D - 1]) : PreUse{};
    View dp;
    if (pld) dp = dx(pg, {{d, &pi.layers[D - 1], 0}}, HS[D - 2], B, actP, &hsub[D - 2], DxOpt().pre_gemm(&pd1));
    dw(pg, Lout, dout, {hsub[D - 1]}, B, CNT_ADAM_PI, cfg.policy_lr, DwOpt(ao).gsq_parts(gl[D]));
    if (!pld) dp = dx(pg, {{d, &pi.layers[D - 1], 0}}, HS[D - 2], B, actP, dsrc_of(actP, hsub[D - 2], hzsub[D - 2]));
    dw(pg, pi.layers[D - 1], d, {hsub[D - 2]}, B, CNT_ADAM_PI, cfg.policy_lr, DwOpt(ao).gsq_parts(gl[D - 1]));
    d = dp;
    for (int i = D - 2; i >= 1; --i) {  // (deeper actors)
      dp = dx(pg, {{d, &pi.layers[i], 0}}, HS[i - 1], B, actP, dsrc_of(actP, hsub[i - 1], hzsub[i - 1]));
      dw(pg, pi.layers[i], d, {hsub[i - 1]}, B, CNT_ADAM_PI, cfg.policy_lr, DwOpt(ao).gsq_parts(gl[i]));
      d = dp;
    }
    dw(pg, pi.layers[0], d, {s}, B, CNT_ADAM_PI, cfg.policy_lr, DwOpt(ao).gsq_parts(gl[0]));
    if (clip_on()) clip_close(pg, cgs);
    if (sb.gsq) {
      // tensor t owns tiles [gsq_offs[t], gsq_offs[t+1]) (params() order: w0, b0, w1, b1, ...)
      sb.gsq_offs.assign(1, 0);
      for (size_t i = 0; i < tens.size(); ++i)
        if (i + 1 == tens.size() || tens[i + 1] != tens[i]) sb.gsq_offs.push_back((int)i + 1);
    }
  }
  // Polyak (td3.py:194-204 on policy steps incl. the aliased policy, Q2; sac.py:243-249 every step)
  void mlp_polyak(Prog& pg, const StepBuild& sb) {
    const bool sac = algo == RLE_SAC;
    if (!sac && !sb.policy) return;
    flat(pg, OP_POLYAK, net("target_q1"), &net("q1"), cfg.tau, false);
    flat(pg, OP_POLYAK, net("target_q2"), &net("q2"), cfg.tau, false);
    if (!sac && !pi_polyak_fused()) flat(pg, OP_POLYAK, net("policy"), nullptr, cfg.tau, true);
  }
  // Step end: the info row of the algorithm (and the SAC temperature update)
  void mlp_step_end(Prog& pg, const StepBuild& sb) {
    const bool sac = algo == RLE_SAC, policy = sb.policy;
    float* const ploss_part = sb.ploss.p;
    const int hw = cdiv(B, 4);
    Op op = step_end_op();
    StepEndArgs& a = op.end;
    std::vector<int> rd{sb.qloss.id};
    if (policy) rd.push_back(sb.ploss.id);
    if (!sac) {  // [train/q_fn, train/policy, norm/policy]
      info_sum(a, 0, sb.qloss.p, sb.qloss.n, 1, (cfg.use_lap ? 1.f : 0.5f) / (float)Bv);
      if (policy) {
        info_sum(a, 1, ploss_part, hw, 4, -1.f / (float)Bv);
        a.kind[2] = INFO_GNORM;
        a.gsq = sb.gsq;
        a.ngsq_t = (int)sb.gsq_offs.size() - 1;
        for (size_t q = 0; q < sb.gsq_offs.size(); ++q) a.gsq_off[q] = sb.gsq_offs[q];
        for (auto& L : net("policy").layers) rd.push_back(L.res);
      } else {
        a.kind[1] = INFO_NAN;
        a.kind[2] = INFO_NAN;
      }
      a.ninfo = 3;
      if (offline3()) info_offline(a, rd, sb);
    } else if (cfg.tmp < 0.f) {  // [train/q_fn, tmp, norm/tmp, train/policy, train/tmp, entropy]
      info_sum(a, 0, sb.qloss.p, sb.qloss.n, 1, 0.5f / (float)Bv);
      a.kind[1] = INFO_SAC_TMP;
      a.kind[2] = INFO_SAC_NTMP;
      info_sum(a, 3, ploss_part, hw, 4, 1.f / (float)Bv);
      a.kind[3] = INFO_SAC_POL;
      a.kind[4] = INFO_SAC_TMPL;
      a.kind[5] = INFO_SAC_ENT;
      a.ninfo = 6;
      a.log_alpha = P + (nP - 4);
      a.la_m = P + nP + (nP - 4);
      a.la_v = P + 2 * nP + (nP - 4);
      a.la_t = &ctrl->la_t;
      a.la_lr = cfg.policy_lr;
      a.adam_step = adam_step_of(asc_set);  // (slot 3: the temperature's bias corrections, this step's ctrl)
      a.adam_bc2s = adam_bc2s_of(asc_set);
      rd.push_back(asc_set ? R_ADAMSC1 : R_ADAMSC);
      a.target_entropy = -(float)A;
      a.logpi_part = ploss_part;
      a.nlogpi = hw;
    } else if (offline_sac()) {  // [train/q_fn, train/policy, entropy, train/adv, train/weight]
      // (OP_AWAC's {w logp, lp, adv, w} sums per 4 rows: the policy objective is -mean(w logp))
      const int nw = sb.ploss.n;
      info_sum(a, 0, sb.qloss.p, sb.qloss.n, 1, 0.5f / (float)Bv);
      info_sum(a, 1, ploss_part, nw, 4, -1.f / (float)Bv);
      a.kind[2] = INFO_SAC_ENT;
      info_sum(a, 3, ploss_part + 2, nw, 4, 1.f / (float)Bv);
      info_sum(a, 4, ploss_part + 3, nw, 4, 1.f / (float)Bv);
      a.ninfo = 5;
      a.logpi_part = ploss_part;
      a.nlogpi = nw;
    } else {  // fixed temperature: [train/q_fn, train/policy, entropy]
      info_sum(a, 0, sb.qloss.p, sb.qloss.n, 1, 0.5f / (float)Bv);
      info_sum(a, 1, ploss_part, hw, 4, 1.f / (float)Bv);
      a.kind[2] = INFO_SAC_ENT;
      a.ninfo = 3;
      a.logpi_part = ploss_part;
      a.nlogpi = hw;
    }
    if (n_step > 1) {  // one more column after the agent's own: replay/hops, the mean hops of this step's batch
      REQUIRE(a.ninfo < kInfoMax, "n-step returns: the info row is full");
      info_sum(a, a.ninfo, hops.p, Bv, 1, 1.f / (float)Bv);
      ++a.ninfo;
      rd.push_back(hops.id);
    }
    std::vector<int> cn{CNT_ADAM_Q, 3, CNT_RNG, CNT_TAPE};
    if (policy) cn.push_back(CNT_ADAM_PI);
    add_step_end(pg, op, rd, cn);
  }
  void build_mlp(Prog& pg, bool policy, int set) {
    StepBuild sb = begin_step(pg, policy, set);
    const MlpActor ac = mlp_actor(pg);
    const MlpCritics cr = mlp_critics(pg, sb, ac);
    mlp_critic_backward(pg, sb, cr);
    if (policy && offline_sac()) mlp_policy_awac(pg, sb, ac);
    else if (policy) mlp_policy(pg, sb, ac);
    mlp_polyak(pg, sb);
    mlp_step_end(pg, sb);
  }


  // ---------------------------------------------------------------- graphs
  // Workgroup cap of the scheduler's levels: off by default.  Measured on MI355X: neutral at
  // B = 256 (6494 vs 6481 steps/s) and -12% at B = 1024 (2706 vs 3067), where most levels
  // exceed the resident capacity and deferral only adds levels.  RLE_SCHED_CAP=1 enables it.
  int sched_cap() const {
    if (!plan.sched_cap) return 1 << 30;
    return plan.level_cap > 0 ? plan.level_cap : std::max(256, level_capacity());
  }
  Graph capture(Prog& pg) {
    auto levels = pg.schedule(sched_cap());
    Graph G;
    size_t total = 0;
    for (auto& lv : levels) {
      G.off.push_back((int)total);
      G.nops.push_back((int)lv.size());
      int wg = 0;
      for (auto& op : lv) wg += op.wg_count;
      G.nwg.push_back(wg);
      total += lv.size();
    }
    static const char* kname[] = {"?", "gemm", "normbwd", "sreduce", "sgather", "head", "prio",
                                  "sacfwd", "sacbwd", "end", "polyak", "copy", "maxred", "ctrl", "noise",
                                  "foldbias", "bc"};
    for (size_t l = 0; l < levels.size(); ++l) {
      G.desc += "L" + std::to_string(l) + " wg=" + std::to_string(G.nwg[l]) + ":";
      if (pg.opt.traffic) {
        const LevelTraffic t = level_traffic(levels[l], P, nP, *pg.opt.allocs);
        char buf[220];
        snprintf(buf, sizeof buf, " [KB act_r %.0f act_w %.0f w_r %.0f adam %.0f other %.0f xcd_r %.0f adam_w %.0f]",
                 t.act_r / 1024, t.act_w / 1024, t.w_r / 1024, t.adam / 1024, t.other / 1024, t.xcd_r / 1024,
                 t.adam_w / 1024);
        G.desc += buf;
      }
      for (size_t k = 0; k < levels[l].size(); ++k) {
        const Op& op = levels[l][k];
        G.desc += std::string(" ") + (pg.crit_lv[l][k] ? "*" : "") +
                  (op.kind == OP_AWAC   ? "awac"
                   : op.kind == OP_CLIP ? "clip"
                   : op.kind == OP_LN   ? (op.ln.p > 0.f ? "ln+drop" : "ln")
                   : op.kind == OP_LN_BWD ? (op.ln.p > 0.f ? "ln-bwd+drop" : "ln-bwd")
                                          : kname[op.kind]);
        if (op.kind == OP_GEMM) {
          static const char* kepi[] = {"st", "adam", "mse", "qhead", "nbdot", "act", "qdot", "sacbwd", "sacfwd", "gsq"};
          static_assert(sizeof(kepi) / sizeof(kepi[0]) == EPI_GSQ + 1, "every epilogue has a name");
          // (adam+nbr: the dot partials row-major, RLE_FUSE_NBROWS)
          const char* ep = op.gemm.mode == GEMM_DW && op.gemm.act == kDwNb ? (op.gemm.nbdot_ld < 0 ? "adam+nbr" : "adam+nb")
                           : op.gemm.epi == EPI_GSQ ? (op.gemm.act == kDwGs ? "gsq+gs" : "gsq")  // (the norm pass)
                           : op.gemm.mode == GEMM_DW && op.gemm.act == kDwGs ? "adam+gs"
                           : op.gemm.has_pre == 2                         ? "head+dx"
                           : op.gemm.has_pre == 3                         ? (op.gemm.epi == EPI_QDOT ? "qdot+pl" : "st+pl")
                           : op.gemm.has_pre == 4                         ? "qdot+pl2"
                           : op.gemm.has_pre == 5                         ? "st+sacpre"
                                                                           : kepi[op.gemm.epi];
          G.desc += "[" + std::to_string(op.gemm.M) + "x" + std::to_string(op.gemm.N) + "x" +
                    std::to_string(op.gemm.R) + " " + ep + (op.gemm.hot.wide ? ".w" : "");
          // (an activation past ACT_TANH runs the kActRt instantiation under its ELU id: named, the others are not)
          const int art = op.gemm.mode == GEMM_FWD ? op.gemm.act : op.gemm.mode == GEMM_DX ? op.gemm.dact : ACT_NONE;
          if (art > ACT_TANH) G.desc += art == ACT_LEAKY ? " leaky" : art == ACT_SILU ? " silu" : " gelu";
          G.desc += "]";
        }
        if (std::getenv("RLE_DESC_WG")) G.desc += "/" + std::to_string(op.wg_count);  // trace tools
      }
      G.desc += "\n";
    }
    std::vector<Op> flat_ops;
    flat_ops.reserve(total);
    for (auto& lv : levels)
      for (auto& op : lv) {
        REQUIRE(op.kind != OP_GEMM || gemm_variant_compiled(op.gemm.vid, kernel_set()),
                "capture: a GEMM variant outside the engine's rle_level instance (ops.h RLE_GEMM_VARIANTS sets)");
        // (LeakyReLU / SiLU / GELU: the second dispatch under the ELU ids is the KS_ACT instance's alone)
        REQUIRE(ks_act_rt(kernel_set()) ||
                    ((op.kind != OP_GEMM || op.gemm.mode == GEMM_DW ||
                      (op.gemm.mode == GEMM_FWD ? op.gemm.act : op.gemm.dact) <= ACT_TANH) &&
                     (op.kind != OP_HEAD || op.head.dact <= ACT_TANH)),
                "capture: an activation of the KS_ACT rle_level instance in another instance's program");
        flat_ops.push_back(op);
      }
    G.d_ops = mem.make<Op>(total);
    HIPCHK(hipMemcpy(G.d_ops, flat_ops.data(), total * sizeof(Op), hipMemcpyHostToDevice));
    const char* tr_env = std::getenv("RLE_TRACE");
    if (tr_env && tr_env[0] == '1') {
      for (int w : G.nwg) G.trace_n += w;
      G.trace = mem.make<unsigned long long>((size_t)G.trace_n * trace_stride());
    }
    long long tr_off = 0;
    const bool dpf = plan.dpf != 0;  // (rle_plan dpf: the next level's descriptor prefetch workgroups)
    for (size_t l = 0; l < levels.size(); ++l) {
      // (after the last level: this graph's first, as the next replay is usually of the same graph)
      const size_t ln = l + 1 < levels.size() ? l + 1 : 0;
      level_launches(G.d_ops + G.off[l], levels[l].data(), G.nops[l], G.nwg[l],
                     G.trace ? G.trace + tr_off * trace_stride() : nullptr, G.d_ops + G.off[ln], dpf ? G.nops[ln] : 0,
                     kernel_set(), G.launches);
      tr_off += G.nwg[l];
    }
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    for (const LevelLaunch& L : G.launches) {
      const hipError_t e = launch_packet(L, stream);
      if (e != hipSuccess) {
        hipGraph_t tmp;
        (void)hipStreamEndCapture(stream, &tmp);
        throw Error{RLE_EHIP, std::string("launch during capture: ") + hipGetErrorString(e)};
      }
    }
    HIPCHK(hipStreamEndCapture(stream, &G.g));
    if (plan.dispatch == 1 && !G.trace) {  // the AQL packets' kernel arguments
      std::vector<unsigned char> ka(G.launches.size() * kAqlKaStride, 0);
      for (size_t i = 0; i < G.launches.size(); ++i)
        std::memcpy(ka.data() + i * kAqlKaStride, &G.launches[i].ka, sizeof(LevelArgs));
      G.aql_ka = mem.make<unsigned char>(ka.size());
      HIPCHK(hipMemcpy(G.aql_ka, ka.data(), ka.size(), hipMemcpyHostToDevice));
    }
    HIPCHK(hipGraphInstantiate(&G.x, G.g, nullptr, nullptr, 0));
    return G;
  }

  void alloc_step_buffers() {
    for (BatchSet& b : bsets) {
      b.ss = buf(2 * B, S);
      b.act_in = buf(B, A);
      b.rw = vec(B);
      b.nd = vec(B);
      b.eps = buf(B, A, false, true);
      b.eps2 = buf(B, A, false, true);
      b.ind = mem.make<long long>(B);
      b.u_buf = mem.make<float>(B);
      b.ind_id = next_id++;
    }
    use_set(0);
    bsum_id = next_id++;
  }

  void ensure_tapes(long long n) {
    if (n <= tape_cap) return;
    // tapes are referenced by captured graphs: allocate once at a generous size
    REQUIRE(!built || n <= tape_cap, "tape larger than the capacity fixed at first use");
    tape_cap = std::max<long long>(n, 1024);
    // + 1 row: the last taped step prefetches (and the host discards) one row past the end
    t_u = mem.make<float>((size_t)(tape_cap + 1) * B);
    t_eps = mem.make<float>((size_t)(tape_cap + 1) * B * A);
    t_eps2 = mem.make<float>((size_t)(tape_cap + 1) * B * A);
    t_ind = mem.make<long long>((size_t)(tape_cap + 1) * B);
  }

  // Builds a step program twice: the first pass fixes the level schedule, then
  // GEMM tiles of any level with more workgroups than fit on the device at once
  // are widened (16 -> 32 -> 64 columns, fewer workgroups, longer reductions per
  // wave) and the program is rebuilt with that tile plan (indexed by the GEMM sequence
  // numbers choose_tn hands out).
  template <class F>
  Prog plan_build(F&& f) {
    tn_plan.clear();
    tn_seq = 0;
    const PlanOptions po = prog_options();
    Prog p0(po.asap());  // (the tile widths are planned on the dependency levels, before the rebalance pass)
    f(p0);
    std::vector<int> tplan(tn_seq, 16);
    auto at = [&](int seq) -> int& { return tplan[seq]; };
    auto levels = p0.schedule();
    for (auto& lv : levels)
      for (auto& op : lv)
        if (op.kind == OP_GEMM) at(op.seq) = std::max(op.gemm.tn, plan.tn_min);
    int cap = std::max(256, level_capacity());  // (plan.level_cap 0)
    // TD3 (its first layers folded into 64-wide pre-layer consumers) plans its levels for 7/8 of the
    // resident workgroups: A/B on HalfCheetah, capacity 1024 / 832 / 768 / 640 -> 23.18k / 23.47k /
    // 23.47k / 23.37k steps/s in round 3; with the two-stage prologue and its own kernel instance
    // (round 4, 2 pairs) 1024 / 896 / 768 / 640 -> 25.22k / 25.33k / 25.23k / 24.94k.  TD7 at
    // B >= 1024 plans for 3/2 of them (its levels are over capacity anyway; 2 pairs at B = 1024:
    // 1024 / 1536 / 2048 -> 3564 / 3598 / 3529).  (TD7 B = 256: 1024 best, 896 -1.2%; SAC: 1024 best,
    // 768 -0.8%.)  Round 6, with each level's ops longest first (plan lpt): TD3 at the full capacity again, 4 pairs
    // 896 (7/8) / 960 / 1024 -> 26.53k / 26.55k / 26.62k (profiles/r06_ab_plan_mlp.txt).
    if (algo == RLE_TD3 && !plan.lpt) cap = cap * 7 / 8;
    // (round 6, longest first: TD7 B = 1024 at 5/4, 4 pairs 1,536 / 1,152 / 1,280 / 1,408 -> 3.79k / 3.81k / 3.83k / 3.79k,
    // profiles/r06_ab_b1024_cap.txt)
    if (algo == RLE_TD7 && B >= 1024) cap = plan.lpt ? cap * 5 / 4 : cap * 3 / 2;
    // (plan.level_cap: tuning experiments, and seeds per GPU on streams -- bench.py)
    if (plan.level_cap > 0) cap = plan.level_cap;
    // elementwise ops (Polyak, copies) are short: they free their slots long before the level's
    // GEMMs do, so they count at 1 / flat_div of their workgroups (RLE_FLAT_DIV, A/B; 1 = full)
    const int flat_div = plan.flat_div;  // (A/B 1 / 4 / 1000: SAC 12675 / 13135 / 13122)
    auto wg_of = [&](const Op& op) {
      if (op.kind == OP_POLYAK || op.kind == OP_COPY) return op.wg_count / flat_div;
      if (op.kind != OP_GEMM) return op.wg_count;
      const GemmArgs& g = op.gemm;
      if (g.hot.wide) return op.wg_count;  // (64-row tiles: never widened)
      return g.tiles_m * (cdiv(g.N, at(op.seq)) + (g.epi == EPI_ADAM || g.epi == EPI_GSQ ? 1 : 0));
    };
    for (auto& lv : levels) {
      while (true) {
        long long total = 0;
        for (auto& op : lv) total += wg_of(op);
        if (total <= cap) break;
        int best = -1, best_wg = 0;
        for (auto& op : lv)
          if (op.kind == OP_GEMM && !op.gemm.hot.wide && at(op.seq) < 64 && wg_of(op) > best_wg) {
            best = op.seq;
            best_wg = wg_of(op);
          }
        if (best < 0) break;
        at(best) *= 2;
      }
    }
    tn_plan = tplan;
    tn_seq = 0;
    Prog p(po);
    f(p);
    tn_plan.clear();
    return p;
  }

  // steps per multi-step graph: plan.steps_per_graph (even; 0 = single-step graphs only)
  int pair_k() const {
    // measured on MI355X (tools/abk.sh): TD7 Humanoid K=2/4/6/8 -> 6370/6513/6440/6290
    // steps/s (round 1), K=4/6/8 -> 7744/7785/7789 after the guarded operand rings (with the
    // rebalance pass: K=6/8 -> 7822/7825); TD3 HalfCheetah K=2/4/8/12/16 -> 14072/14885/16066/
    // 16203/16348 and SAC Humanoid K=2/4/8 -> 7874/7977/8052 (with the rebalance pass)
    int k = plan.steps_per_graph;
    if (algo != RLE_SAC && cfg.policy_freq != 2) k = 0;  // the pattern assumes policy_freq 2
    return k >= 2 ? k & ~1 : 0;
  }

  void build() {
    REQUIRE(replay, "no replay bound");
    ensure_tapes(1024);
    const bool sac = algo == RLE_SAC;
    alloc_folds();
    if (clip_on() && !clip_buf) {  // ({total, coef} read NaN until an optimizer's first clipped update)
      clip_buf = mem.make<float>(12);
      std::vector<float> nan(12, std::numeric_limits<float>::quiet_NaN());
      HIPCHK(hipMemcpy(clip_buf, nan.data(), sizeof(float) * 12, hipMemcpyHostToDevice));
      for (int& id : clip_id) id = next_id++;
    }
    multi_k = pair_k();
    // K steps from batch set `set` on, as one program.  TD7 / TD3: policy, plain, ...; SAC: every step is a policy step
    auto steps = [&](int set, int K, bool first_policy) {
      Prog p = plan_build([&](Prog& pg) {
        for (int j = 0; j < K; ++j) {
          const bool policy = sac || (j % 2 == 0) == first_policy;
          if (algo == RLE_TD7) build_td7(pg, policy, (set + j) % 2);
          else build_mlp(pg, policy, (set + j) % 2);
        }
      });
      return capture(p);
    };
    for (int set = 0; set < 2; ++set) {
      Prog pp = aux_prog();
      build_prime(pp, sac, set);
      g_prime[set] = capture(pp);
      g_pol[set] = steps(set, 1, true);
      if (!sac) g_pln[set] = steps(set, 1, false);
      if (!multi_k) continue;
      g_pair[set] = steps(set, multi_k, true);
      for (int r = 0; r < 2; ++r)
        if (kRemK[r] < multi_k) g_rem[r][set] = steps(set, kRemK[r], true);
    }
    if (algo == RLE_TD7) {
      Prog ph = aux_prog();
      build_td7_hard(ph);
      g_hard = capture(ph);
      if (td7_fold()) {
        Prog pf = aux_prog();
        add_target_fold(pf);
        g_fold = capture(pf);
      }
    }
    {
      Prog pz = aux_prog();
      Op z{};
      z.kind = OP_COPY;
      z.flat.dst = reinterpret_cast<float*>(&ctrl->info_slot);  // (int 0 = the bits of float 0)
      z.flat.src = mem.make<float>(4);                          // (zero-filled)
      z.flat.n = 1;
      z.wg_count = 1;
      pz.add(z, {}, {next_id++});
      g_slot0 = capture(pz);
    }
    use_set(0);
    built = true;
  }

  // Adam bias-correction scalars of this step from the completed-step counters; the
  // op has no producers, so it runs in level 0 beside the LAP block sums.
  // (SAC autotune: also the temperature optimizer's bias corrections, from la_t, which the previous
  // step end wrote: R_LA)
  bool sac_tmp_auto() const { return algo == RLE_SAC && cfg.tmp < 0.f; }
  void add_adam_scalars(Prog& pg) {
    std::vector<int> rd{R_CNT};
    if (sac_tmp_auto()) rd.push_back(R_LA);
    pg.add(adam_scalars_op(asc_set), rd, {asc_set ? R_ADAMSC1 : R_ADAMSC});
  }
  Op adam_scalars_op(int set) {
    Op op{};
    op.kind = OP_CTRL;
    op.wg_count = 1;
    CtrlArgs& c = op.ctrl;
    c.mode = 1;
    c.counters = ctrl->counters;
    c.adam_step = adam_step_of(set);
    c.adam_bc2s = adam_bc2s_of(set);
    c.adam_lr[CNT_ADAM_Q] = cfg.critic_lr;
    c.adam_lr[CNT_ADAM_PI] = cfg.policy_lr;
    c.adam_lr[CNT_ADAM_ENC] = cfg.policy_lr;
    if (sac_tmp_auto()) {
      c.la_t = &ctrl->la_t;
      c.la_lr = cfg.policy_lr;
    }
    return op;
  }

  // The same computed eagerly (creation / counters set), for readers outside a step.
  void refresh_adam_scalars() {
    if (!adamsc1) adamsc1 = mem.make<float>(8);
    if (!ctrl_op) ctrl_op = mem.make<Op>(2);
    Op ops[2] = {adam_scalars_op(0), adam_scalars_op(1)};
    ops[1].wg_begin = 1;
    HIPCHK(hipMemcpyAsync(ctrl_op, ops, sizeof(ops), hipMemcpyHostToDevice, stream));
    HIPCHK(launch_level(ctrl_op, ops, 2, 2, stream));
    HIPCHK(hipStreamSynchronize(stream));
  }
  Op* ctrl_op = nullptr;

  // ---------------------------------------------------------------- run
  long long launches = 0;  // rle_level dispatches enqueued by step graphs (rle_launch_count)
  bool aql_active = false;        // inside step(): graphs go to the AQL queue
  // Direct AQL dispatch of the step graphs (rle_step / rle_step_timed wait for their bursts; rle_step_async
  // leaves its burst in flight on the engine's own queue -- each seed on a queue of its own, where hipGraph
  // replays on HIP streams share GPU_MAX_HW_QUEUES hardware queues -- and every other entry point, and
  // every replay operation on a replay the engine is bound to, drains it first: aql_drain).  rle_plan
  // dispatch 0 / 2: hipGraph replays / launches on the stream (A/B; the launch path changes no result).
  bool aql_mode() const { return plan.dispatch == 1; }
  void aql_drain(double* ms = nullptr) {
    if (aql) aql_complete(*aql, ms);
  }
  // (the AQL queue keeps &G.launches until the burst is submitted, AqlQueue::Pending: a program must not move
  // after its first launch.  None does: programs are members or nodes of a std::map, moved in before they run)
  void launch_graph(const Graph& G) {
    if (aql_active && G.aql_ka) {
      aql->pending.push_back({&G.launches, G.aql_ka});
    } else if (plan.dispatch == 2 && !G.trace) {  // (A/B: the launches on the stream, no graph)
      for (const LevelLaunch& L : G.launches) HIPCHK(launch_packet(L, stream));
    } else {
      HIPCHK(hipGraphLaunch(G.x, stream));
    }
    launches += G.nlaunch();
  }
  // The next K steps (multi_k, or a remainder program's) may run as one multi-step program: TD7 (counter
  // bumped first, td7.py:295) / TD3 (td3.py:231) when its first step is a policy step (and, TD7, no step
  // of it needs a hard update); SAC any K steps.
  bool pair_window_ok(int K) const {
    if (!K) return false;
    const long long k1 = algo == RLE_TD7 ? n_runs + 1 : n_runs;
    if (algo != RLE_SAC && k1 % 2) return false;
    if (algo == RLE_TD7) {
      const int tur = std::max(1, cfg.target_update_rate);
      for (long long k = k1; k < k1 + K; ++k)
        if (k % tur == 0) return false;
    }
    return true;
  }
  // host state after a K-step program starting on batch set cur_set was enqueued
  void pair_commit(int K) {
    const int p = cur_set;
    n_runs += K;
    pol_set = p;
    if (algo != RLE_SAC) pln_set = 1 - p;
    last_set = 1 - p;
    cur_set = p;
    if (cfg.use_lap && algo != RLE_SAC) replay->version += K;
    primed = true;
    primed_ver = replay->version;
  }

  void step(int n, float* info_out, float* gpu_ms = nullptr, bool async = false) {
    REQUIRE(replay, "no replay bound");
    REQUIRE(replay->size > 0, "replay is empty");
    if (!built) build();
    const int pf = std::max(1, cfg.policy_freq);
    if (fold_dirty && g_fold.x) launch_graph(g_fold);
    fold_dirty = false;
    int done = 0;
    // direct dispatch (rle_plan dispatch 1): the graphs' levels go to the engine's own queue; the HIP
    // stream is drained first and the queue after each chunk (host-side ordering between them; async:
    // the last chunk stays in flight, aql_drain)
    const bool use_aql = aql_mode() && g_pol[0].aql_ka;
    if (use_aql && !aql) aql = aql_open(cfg.device);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (gpu_ms && !use_aql) {  // (AQL: the levels run outside the stream; host wall time instead)
      HIPCHK(hipEventCreate(&ev0));
      HIPCHK(hipEventCreate(&ev1));
      HIPCHK(hipEventRecord(ev0, stream));
    }
    double aql_ms = 0.0;
    while (done < n) {
      const int chunk = std::min(n - done, info_cap);
      if (use_aql) {
        // the info slot reset is the burst's first packet (g_slot0), in order with the bursts still in flight:
        // no host round trip (a 4-byte H2D copy and a stream sync cost ~20 us per burst, 1% of a 20-step burst)
        HIPCHK(hipStreamSynchronize(stream));
        aql_active = true;
        launch_graph(g_slot0);
        launches -= g_slot0.nlaunch();  // (not a step level)
      } else {
        int zero = 0;
        HIPCHK(hipMemcpyAsync(&ctrl->info_slot, &zero, sizeof(int), hipMemcpyHostToDevice, stream));
      }
      for (int i = 0; i < chunk; ++i) {
        if (ctrl_tape_mode_host) {
          REQUIRE(tape_left > 0, "tape exhausted");
          --tape_left;
        }
        // the batch of this step: prefetched by the previous step, unless anything it was
        // drawn from has changed since (appends, other writers of the priorities, tapes)
        if (!primed || primed_ver != replay->version) launch_graph(g_prime[cur_set]);
        const int p = cur_set;
        // multi-step graph (pair_window_ok)
        // (the longest multi-step program that fits the rest of the chunk: multi_k, then the remainder ones)
        const Graph* mg = nullptr;
        int K = 0;
        for (int r = -1; r < 2 && !mg; ++r) {
          const int k = r < 0 ? multi_k : kRemK[r];
          const Graph& g = r < 0 ? g_pair[p] : g_rem[r][p];
          if (k && g.x && i + k - 1 < chunk && (!ctrl_tape_mode_host || tape_left >= k - 1) && pair_window_ok(k)) {
            mg = &g;
            K = k;
          }
        }
        if (mg) {
          if (ctrl_tape_mode_host) tape_left -= K - 1;
          launch_graph(*mg);
          pair_commit(K);
          i += K - 1;
          continue;
        }
        if (algo == RLE_TD7) {
          ++n_runs;  // td7.py:295 (increment first)
          (n_runs % pf == 0 ? pol_set : pln_set) = p;
          launch_graph((n_runs % pf == 0) ? g_pol[p] : g_pln[p]);
          if (n_runs % std::max(1, cfg.target_update_rate) == 0) launch_graph(g_hard);
        } else if (algo == RLE_TD3) {
          (n_runs % pf == 0 ? pol_set : pln_set) = p;
          launch_graph((n_runs % pf == 0) ? g_pol[p] : g_pln[p]);  // td3.py:231
          ++n_runs;
        } else {
          pol_set = p;
          launch_graph(g_pol[p]);
          ++n_runs;
        }
        last_set = p;
        cur_set = 1 - p;
        if (cfg.use_lap && algo != RLE_SAC) ++replay->version;  // this step wrote priorities
        primed = true;
        primed_ver = replay->version;
      }
      if (use_aql) {
        aql_active = false;
        aql_submit(*aql);
        if (!async) aql_complete(*aql, &aql_ms);
      }
      if (info_out) {
        HIPCHK(hipMemcpyAsync(info_out + (size_t)done * kInfoMax, info, (size_t)chunk * kInfoMax * sizeof(float),
                              hipMemcpyDeviceToHost, stream));
      }
      if (!gpu_ms && !async) HIPCHK(hipStreamSynchronize(stream));
      done += chunk;
    }
    HIPCHK(hipEventRecord(done_ev, stream));  // replay operations wait for this (Replay::wait_users)
    if (gpu_ms && use_aql) {
      *gpu_ms = (float)aql_ms;  // (the levels ran outside the stream: host wall time)
    } else if (gpu_ms) {
      HIPCHK(hipEventRecord(ev1, stream));
      HIPCHK(hipEventSynchronize(ev1));
      HIPCHK(hipEventElapsedTime(gpu_ms, ev0, ev1));
      (void)hipEventDestroy(ev0);
      (void)hipEventDestroy(ev1);
    }
  }
  int ctrl_tape_mode_host = 0;
};

// What the replay asks of its users (replay.h)
void engine_drain(Engine& e) { e.aql_drain(); }
void engine_unbind(Engine& e) { e.replay = nullptr; }

// The engine behind a handle, its rle_step_async burst retired first (Engine::aql_mode)
Engine& drained(rle_engine* h) {
  h->e->aql_drain();
  return *h->e;
}

}  // namespace rle

// ====================================================================== C ABI: the engine entries
// (the replay's: replay.cpp; handles, guard and the last-error string: abi.h)

using rle::drained;
using rle::Engine;
using rle::Error;
using rle::guard;

extern "C" {

const char* rle_last_error(void) { return rle::g_err.c_str(); }

int rle_create(const rle_config* cfg, rle_engine** out) { return rle_create_ext(cfg, nullptr, out); }

int rle_create_ext(const rle_config* cfg, const rle_config_ext* ext, rle_engine** out) {
  return guard([&] {
    REQUIRE(cfg && out, "create: null");
    // the extension as the caller compiled it: fields past ext->size read as 0
    rle_config_ext x{};
    if (ext) {
      // (a size that ends inside a field would pass half of it: only the struct's field boundaries are sizes)
      const int ends[] = {(int)(offsetof(rle_config_ext, bc_alpha) + sizeof(float)),
                          (int)(offsetof(rle_config_ext, awac_lambda) + sizeof(float))};
      REQUIRE(ext->size == ends[0] || ext->size == ends[1],
              "create: rle_config_ext size " + std::to_string(ext->size) + " is not one the struct ever had; the valid "
              "sizes, with the last field each reaches: " + std::to_string(ends[0]) + " (bc_alpha), " +
              std::to_string(ends[1]) + " (awac_lambda)");
      std::memcpy(&x, ext, std::min<size_t>((size_t)ext->size, sizeof x));
    }
    REQUIRE(cfg->algo >= 0 && cfg->algo <= 2, "create: bad algo");
    REQUIRE(cfg->batch > 0 && cfg->batch <= 1024, "create: batch must be in 1..1024");
    REQUIRE(cfg->state_dim <= 1024 && cfg->action_dim <= 128 && cfg->hidden <= 512,
            "create: state_dim <= 1024, action_dim <= 128, hidden <= 512");
    REQUIRE(cfg->state_dim > 0 && cfg->action_dim > 0 && cfg->hidden > 0 && cfg->hidden % 4 == 0,
            "create: bad dims (hidden must be a multiple of 4)");
    REQUIRE(cfg->zs_dim == 0 || (cfg->algo == RLE_TD7 && cfg->zs_dim > 0 && cfg->zs_dim <= 512 && cfg->zs_dim % 4 == 0),
            "create: zs_dim (TD7 only) must be a multiple of 4, <= 512");
    REQUIRE(cfg->n_hidden == 0 || (cfg->algo != RLE_TD7 && cfg->n_hidden >= 2 && cfg->n_hidden <= RLE_MAX_HIDDEN),
            "create: n_hidden (TD3 / SAC only) must be 2..6");
    for (int i = 0; i < cfg->n_hidden; ++i)
      REQUIRE(cfg->hidden_sizes[i] > 0 && cfg->hidden_sizes[i] <= 512 && cfg->hidden_sizes[i] % 4 == 0,
              "create: hidden_sizes must be multiples of 4, <= 512");
    for (int a : {cfg->act_actor, cfg->act_critic, cfg->act_encoder})
      REQUIRE(a >= RLE_ACT_DEFAULT && a <= RLE_ACT_GELU, "create: activation must be an RLE_ACT_* code");
    REQUIRE(cfg->algo == RLE_TD7 || cfg->act_encoder == RLE_ACT_DEFAULT, "create: act_encoder is TD7's (SALEEncoder)");
    REQUIRE(cfg->bc_lambda >= 0.f && std::isfinite(cfg->bc_lambda), "create: bc_lambda must be a finite value >= 0");
    REQUIRE(cfg->bc_lambda == 0.f || cfg->algo == RLE_TD7, "create: bc_lambda (offline mode) is TD7's");
    REQUIRE(x.bc_alpha >= 0.f && std::isfinite(x.bc_alpha), "create: bc_alpha must be a finite value >= 0");
    REQUIRE(x.bc_alpha == 0.f || cfg->algo == RLE_TD3, "create: bc_alpha (offline mode, TD3+BC) is TD3's");
    REQUIRE(x.awac_lambda >= 0.f && std::isfinite(x.awac_lambda), "create: awac_lambda must be a finite value >= 0");
    REQUIRE(x.awac_lambda == 0.f || cfg->algo == RLE_SAC, "create: awac_lambda (offline mode, AWAC) is SAC's");
    REQUIRE(x.awac_lambda == 0.f || (cfg->tmp == 0.f && cfg->use_lap == 0),
            "create: awac_lambda > 0 needs tmp == 0 (no temperature in the offline mode) and use_lap == 0");
    HIPCHK(hipSetDevice(cfg->device));
    auto h = std::make_unique<rle_engine>();
    h->e = std::make_unique<Engine>();
    Engine& e = *h->e;
    e.cfg = *cfg;
    e.bc_alpha = x.bc_alpha;
    e.awac_lambda = x.awac_lambda;
    e.algo = cfg->algo;
    e.S = cfg->state_dim;
    e.Sp = rle::r16(e.S);
    e.A = cfg->action_dim;
    e.Ap = rle::r16(e.A);
    // (TD3 / SAC: H is the LAST hidden width -- what the heads and the output layer read; each
    // layer's own width is in HS)
    e.HS.assign(2, cfg->hidden);
    if (cfg->n_hidden) e.HS.assign(cfg->hidden_sizes, cfg->hidden_sizes + cfg->n_hidden);
    e.H = e.algo == RLE_TD7 ? cfg->hidden : e.HS.back();
    e.Hp = rle::r16(e.H);
    e.Z = cfg->zs_dim ? cfg->zs_dim : cfg->hidden;
    e.Zp = rle::r16(e.Z);
    e.Bv = cfg->batch;
    e.B = (cfg->batch + 15) / 16 * 16;  // (padded rows: zero, masked out of every mean, loss and priority)
    // hidden activations (sale.py:25,67,97; mlp.py:13): the reference defaults unless the config names one
    auto act_of = [](int code, int dflt) {
      return code == RLE_ACT_RELU ? rle::ACT_RELU
             : code == RLE_ACT_ELU ? rle::ACT_ELU
             : code == RLE_ACT_IDENTITY ? rle::ACT_NONE
             : code == RLE_ACT_LEAKY_RELU ? rle::ACT_LEAKY
             : code == RLE_ACT_SILU ? rle::ACT_SILU
             : code == RLE_ACT_GELU ? rle::ACT_GELU
                                    : dflt;
    };
    const bool td7 = e.algo == RLE_TD7;
    e.actP = act_of(cfg->act_actor, rle::ACT_RELU);
    e.actC = act_of(cfg->act_critic, td7 ? rle::ACT_ELU : rle::ACT_RELU);
    e.actE = act_of(cfg->act_encoder, rle::ACT_ELU);
    e.acts_default = e.actP == rle::ACT_RELU && e.actC == (td7 ? rle::ACT_ELU : rle::ACT_RELU) && e.actE == rle::ACT_ELU;
    e.resolve_plan();
    HIPCHK(hipStreamCreateWithFlags(&e.stream.s, hipStreamNonBlocking));
    if (e.algo == RLE_TD7) {
      for (const char* n : {"encoder", "fixed_encoder", "fixed_encoder_target"}) e.nets.push_back(e.make_net(n, "sale_enc"));
      e.nets.push_back(e.make_net("policy", "sale_actor"));
      for (const char* n : {"q1", "q2", "target_q1", "target_q2"}) e.nets.push_back(e.make_net(n, "sale_critic"));
    } else {
      e.nets.push_back(e.make_net("policy", "mlp_actor"));
      for (const char* n : {"q1", "q2", "target_q1", "target_q2"}) e.nets.push_back(e.make_net(n, "mlp_critic"));
    }
    e.layout_params();
    e.ctrl = e.mem.make<rle::Ctrl>(1);
    rle::Ctrl c{};
    c.vmax_key = rle::host_fkey(-1e8f);  // td7.py:84-87
    c.vmin_key = rle::host_fkey(1e8f);
    c.vt[0] = c.vt[1] = 0.f;
    c.max_priority = 1.f;
    HIPCHK(hipMemcpy(e.ctrl, &c, sizeof(c), hipMemcpyHostToDevice));
    if (e.algo == RLE_SAC) {
      const float la = cfg->tmp < 0.f ? 0.f : std::log(cfg->tmp);  // sac.py:56-60
      HIPCHK(hipMemcpy(e.P + (e.nP - 4), &la, 4, hipMemcpyHostToDevice));
    }
    e.info = e.mem.make<float>((size_t)e.info_cap * rle::kInfoMax);
    e.alloc_step_buffers();
    e.refresh_adam_scalars();
    *out = h.release();
  });
}

int rle_plan_default(rle_plan* out) {
  return guard([&] {
    REQUIRE(out, "plan_default: null");
    *out = rle::plan_defaults();
  });
}

int rle_set_plan(rle_engine* h, const rle_plan* plan) {
  return guard([&] {
    REQUIRE(h && plan, "set_plan: null");
    Engine& e = drained(h);
    REQUIRE(!e.built, "set_plan: the engine has already built its step programs (set the plan before the first step)");
    e.plan = *plan;
    e.resolve_plan();
  });
}

int rle_set_grad_clip(rle_engine* h, float max_norm) {
  return guard([&] {
    REQUIRE(h, "set_grad_clip: null");
    REQUIRE(max_norm >= 0.f, "set_grad_clip: max_norm must be >= 0 (0 or +inf: off)");  // (NaN fails too)
    Engine& e = drained(h);
    if (e.built)
      throw Error{RLE_ESTATE, "set_grad_clip: the engine has already built its step programs (set it before the "
                              "first step)"};
    e.clip_max = std::isinf(max_norm) ? 0.f : max_norm;
  });
}

int rle_set_layer_norm(rle_engine* h, int critic) {
  return guard([&] {
    REQUIRE(h, "set_layer_norm: null");
    REQUIRE(critic == 0 || critic == 1, "set_layer_norm: critic is 0 (off) or 1 (on)");
    Engine& e = drained(h);
    REQUIRE(e.algo != RLE_TD7 || !critic,
            "set_layer_norm: TD3 / SAC only (TD7's SALE critics already carry AvgL1Norm)");
    REQUIRE(critic || !(e.drop_p > 0.f),
            "set_layer_norm: critic dropout is on and lives in the row-norm ops (dropout without LayerNorm is not "
            "run; rle_set_critic_dropout(e, 0) first)");
    if (e.built)
      throw Error{RLE_ESTATE, "set_layer_norm: the engine has already built its step programs (set it before the "
                              "first step)"};
    if (e.ln_critic == (critic != 0)) return;
    e.ln_critic = critic != 0;
    // (forward programs captured under the other setting: dropped, rle_eval rebuilds them)
    HIPCHK(hipSetDevice(e.cfg.device));
    for (auto it = e.eval_graphs.begin(); it != e.eval_graphs.end();) {
      if (it->first.rfind("rsample|", 0) == 0) ++it;  // (rle_sac_rsample's: no critic in it)
      else it = e.eval_graphs.erase(it);
    }
  });
}

int rle_get_layer_norm(rle_engine* h, int* critic) {
  return guard([&] {
    REQUIRE(h && critic, "get_layer_norm: null");
    *critic = h->e->ln_critic ? 1 : 0;
  });
}

int rle_set_critic_dropout(rle_engine* h, float p) {
  return guard([&] {
    REQUIRE(h, "set_critic_dropout: null");
    REQUIRE(p >= 0.f && p < 1.f, "set_critic_dropout: p must be in [0, 1) (0: off)");  // (NaN fails too)
    Engine& e = drained(h);
    REQUIRE(e.algo != RLE_TD7 || !(p > 0.f), "set_critic_dropout: TD3 / SAC only (as rle_set_layer_norm)");
    if (e.built)
      throw Error{RLE_ESTATE, "set_critic_dropout: the engine has already built its step programs (set it before "
                              "the first step)"};
    REQUIRE(e.ln_on() || !(p > 0.f),
            "set_critic_dropout: the critics' LayerNorm is off (rle_set_layer_norm(e, 1) first): the dropout lives in "
            "the row-norm ops, dropout without LayerNorm is not run");
    e.drop_p = p;  // (rle_eval's forward programs run without dropout: none to rebuild)
  });
}

int rle_get_critic_dropout(rle_engine* h, float* p) {
  return guard([&] {
    REQUIRE(h && p, "get_critic_dropout: null");
    *p = h->e->drop_p;
  });
}

int rle_dropout_mask(rle_engine* h, long long step, int site, int rows, int width, float* out) {
  return guard([&] {
    REQUIRE(h && out, "dropout_mask: null");
    REQUIRE(site >= 0 && site < 64, "dropout_mask: site is (pass * 2 + twin) * 8 + layer, 0 .. 63");
    REQUIRE(rows >= 1 && rows <= (1 << 20) && width >= 4 && width <= 512 && width % 4 == 0,
            "dropout_mask: rows 1 .. 2^20, width 4 .. 512 in steps of 4");
    Engine& e = drained(h);
    HIPCHK(hipSetDevice(e.cfg.device));
    const size_t bytes = (size_t)rows * width * sizeof(float);
    float* d = nullptr;
    HIPCHK(hipMalloc(&d, bytes));
    const float p = e.drop_p, s = 1.0f / (1.0f - p);
    hipError_t rc = rle::launch_dropout_mask(d, rows, width, (unsigned long long)e.cfg.seed, (unsigned long long)step,
                                             site, p, s, e.stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(e.stream);
    if (rc == hipSuccess) rc = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(rc);
  });
}

int rle_set_n_step(rle_engine* h, int n) {
  return guard([&] {
    REQUIRE(h, "set_n_step: null");
    REQUIRE(n >= 1 && n <= RLE_MAX_N_STEP, "set_n_step: n must be in 1 .. RLE_MAX_N_STEP (1: off)");
    Engine& e = drained(h);
    REQUIRE(e.algo != RLE_TD7 || n == 1,
            "set_n_step: TD3 / SAC only (TD7's encoder learns the one-step model zsa(s, a) -> zs(s') from the same "
            "next-state rows)");
    if (e.built)
      throw Error{RLE_ESTATE, "set_n_step: the engine has already built its step programs (set it before the first "
                              "step)"};
    if (n > 1) {
      HIPCHK(hipSetDevice(e.cfg.device));
      e.ensure_hops();
    }
    e.n_step = n;
  });
}

int rle_get_n_step(rle_engine* h, int* n) {
  return guard([&] {
    REQUIRE(h && n, "get_n_step: null");
    *n = h->e->n_step;
  });
}

int rle_get_grad_clip(rle_engine* h, float* max_norm) {
  return guard([&] {
    REQUIRE(h && max_norm, "get_grad_clip: null");
    *max_norm = h->e->clip_max;
  });
}

int rle_grad_clip_stats(rle_engine* h, float* out6) {
  return guard([&] {
    REQUIRE(h && out6, "grad_clip_stats: null");
    Engine& e = drained(h);
    for (int i = 0; i < 6; ++i) out6[i] = std::numeric_limits<float>::quiet_NaN();
    if (!e.clip_buf) return;
    HIPCHK(hipSetDevice(e.cfg.device));
    HIPCHK(hipStreamSynchronize(e.stream));
    float b[12];
    HIPCHK(hipMemcpy(b, e.clip_buf, sizeof b, hipMemcpyDeviceToHost));
    for (int o = 0; o < 3; ++o) out6[2 * o] = b[4 * o], out6[2 * o + 1] = b[4 * o + 1];
  });
}

int rle_get_plan(rle_engine* h, rle_plan* out) {
  return guard([&] {
    REQUIRE(h && out, "get_plan: null");
    *out = h->e->plan;
  });
}

int rle_destroy(rle_engine* h) {
  return guard([&] { delete h; });
}

int rle_bind_replay(rle_engine* h, rle_replay* r) {
  return guard([&] {
    Engine& e = drained(h);
    REQUIRE(r, "bind: null replay");
    REQUIRE(r->r.S == e.S && r->r.A == e.A, "bind: replay dims differ from agent dims");
    if (e.replay == &r->r) return;
    REQUIRE(!e.built, "bind: engine already bound to another replay");
    if (e.replay) e.replay->remove_user(&e);  // not built yet: move to the new replay
    e.replay = &r->r;
    e.primed = false;
    if (!e.done_ev) HIPCHK(hipEventCreateWithFlags(&e.done_ev, hipEventDisableTiming));
    r->r.users.push_back({&e, e.done_ev});
  });
}

int rle_param_numel(rle_engine* h, const char* net, const char* name, long long* numel) {
  return guard([&] { *numel = h->e->numel(net, name); });
}
int rle_get_param(rle_engine* h, const char* net, const char* name, float* out, long long n) {
  return guard([&] { drained(h).xfer_param(net, name, out, n, false, 0); });
}
int rle_set_param(rle_engine* h, const char* net, const char* name, const float* in, long long n) {
  return guard([&] { drained(h).xfer_param(net, name, const_cast<float*>(in), n, true, 0); });
}
int rle_get_adam(rle_engine* h, const char* net, const char* name, int which, float* out, long long n) {
  return guard([&] {
    REQUIRE(which == 0 || which == 1, "adam: which in {0,1}");
    drained(h).xfer_param(net, name, out, n, false, 1 + which);
  });
}
int rle_set_adam(rle_engine* h, const char* net, const char* name, int which, const float* in, long long n) {
  return guard([&] {
    REQUIRE(which == 0 || which == 1, "adam: which in {0,1}");
    drained(h).xfer_param(net, name, const_cast<float*>(in), n, true, 1 + which);
  });
}

int rle_get_counters(rle_engine* h, long long* out6) {
  return guard([&] {
    Engine& e = drained(h);
    HIPCHK(hipStreamSynchronize(e.stream));
    rle::Ctrl c;
    HIPCHK(hipMemcpy(&c, e.ctrl, sizeof(c), hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) out6[i] = c.counters[i];
    out6[3] = e.n_runs;
    out6[5] = c.la_t;
  });
}

int rle_get_act_counter(rle_engine* h, unsigned long long* out) {
  return guard([&] { *out = h->e->act_counter; });
}

int rle_set_act_counter(rle_engine* h, unsigned long long v) {
  return guard([&] { h->e->act_counter = v; });
}

int rle_set_counters(rle_engine* h, const long long* in6) {
  return guard([&] {
    Engine& e = drained(h);
    HIPCHK(hipStreamSynchronize(e.stream));
    rle::Ctrl c;
    HIPCHK(hipMemcpy(&c, e.ctrl, sizeof(c), hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) c.counters[i] = in6[i];
    c.la_t = in6[5];
    e.n_runs = in6[3];
    e.primed = false;  // the RNG position changed
    HIPCHK(hipMemcpy(e.ctrl, &c, sizeof(c), hipMemcpyHostToDevice));
    e.refresh_adam_scalars();
  });
}

int rle_get_value_bounds(rle_engine* h, float* out4) {
  return guard([&] {
    Engine& e = drained(h);
    HIPCHK(hipStreamSynchronize(e.stream));
    rle::Ctrl c;
    HIPCHK(hipMemcpy(&c, e.ctrl, sizeof(c), hipMemcpyDeviceToHost));
    out4[0] = rle::host_unkey(c.vmax_key);
    out4[1] = rle::host_unkey(c.vmin_key);
    out4[2] = c.vt[0];
    out4[3] = c.vt[1];
  });
}

int rle_set_value_bounds(rle_engine* h, const float* in4) {
  return guard([&] {
    Engine& e = drained(h);
    HIPCHK(hipStreamSynchronize(e.stream));
    rle::Ctrl c;
    HIPCHK(hipMemcpy(&c, e.ctrl, sizeof(c), hipMemcpyDeviceToHost));
    c.vmax_key = rle::host_fkey(in4[0]);
    c.vmin_key = rle::host_fkey(in4[1]);
    c.vt[0] = in4[2];
    c.vt[1] = in4[3];
    HIPCHK(hipMemcpy(e.ctrl, &c, sizeof(c), hipMemcpyHostToDevice));
  });
}

int rle_step(rle_engine* h, int n_steps, float* info_out) {
  return guard([&] {
    REQUIRE(n_steps >= 0, "step: n < 0");
    Engine& e = drained(h);
    HIPCHK(hipSetDevice(e.cfg.device));
    if (e.replay) HIPCHK(hipStreamSynchronize(e.replay->stream));
    e.step(n_steps, info_out);
  });
}

int rle_step_timed(rle_engine* h, int n_steps, float* gpu_ms) {
  return guard([&] {
    REQUIRE(n_steps >= 0 && gpu_ms, "step_timed: bad args");
    Engine& e = drained(h);
    HIPCHK(hipSetDevice(e.cfg.device));
    if (e.replay) HIPCHK(hipStreamSynchronize(e.replay->stream));
    e.step(n_steps, nullptr, gpu_ms);
  });
}

int rle_step_async(rle_engine* h, int n_steps) {
  return guard([&] {
    REQUIRE(n_steps >= 0, "step_async: n < 0");
    Engine& e = *h->e;  // (its earlier bursts stay in flight: the new one queues behind them)
    HIPCHK(hipSetDevice(e.cfg.device));
    if (e.replay) HIPCHK(hipStreamSynchronize(e.replay->stream));
    e.step(n_steps, nullptr, nullptr, true);
  });
}

int rle_set_tapes(rle_engine* h, int n, const float* u, const float* eps, const float* eps_pi, const long long* ind) {
  return guard([&] {
    Engine& e = drained(h);
    HIPCHK(hipStreamSynchronize(e.stream));
    int mode = 0;
    if (n > 0) {
      REQUIRE(n <= 1024, "set_tapes: at most 1024 steps per tape");
      e.ensure_tapes(n);
      const size_t nb = (size_t)n * e.Bv, na = nb * e.A;  // (host tapes: [n][batch rows])
      if (u) HIPCHK(hipMemcpy(e.t_u, u, nb * 4, hipMemcpyHostToDevice));
      if (eps) HIPCHK(hipMemcpy(e.t_eps, eps, na * 4, hipMemcpyHostToDevice));
      if (eps_pi) HIPCHK(hipMemcpy(e.t_eps2, eps_pi, na * 4, hipMemcpyHostToDevice));
      if (ind) {
        const long long size = e.replay ? e.replay->size : 0;
        for (size_t i = 0; i < nb; ++i)
          REQUIRE(ind[i] >= 0 && ind[i] < size, "set_tapes: index outside the bound replay's size");
        HIPCHK(hipMemcpy(e.t_ind, ind, nb * 8, hipMemcpyHostToDevice));
      }
      REQUIRE(u || ind, "set_tapes: need u or ind");
      REQUIRE(e.algo != RLE_SAC || !eps == !eps_pi, "set_tapes: SAC takes eps and eps_pi together");
      mode = (u ? rle::kTapeU : 0) | (ind ? rle::kTapeInd : 0) | (eps ? rle::kTapeEps : 0);
    }
    rle::Ctrl c;
    HIPCHK(hipMemcpy(&c, e.ctrl, sizeof(c), hipMemcpyDeviceToHost));
    c.tape_mode = mode;
    c.counters[5] = 0;
    HIPCHK(hipMemcpy(e.ctrl, &c, sizeof(c), hipMemcpyHostToDevice));
    e.ctrl_tape_mode_host = mode;
    e.tape_left = n;
    e.primed = false;  // a prefetched batch was drawn from the previous draws
  });
}

int rle_last_indices(rle_engine* h, long long* out) {
  return guard([&] {
    Engine& e = drained(h);
    HIPCHK(hipStreamSynchronize(e.stream));
    HIPCHK(hipMemcpy(out, e.bsets[e.last_set].ind, e.Bv * sizeof(long long), hipMemcpyDeviceToHost));
  });
}

int rle_act(rle_engine* h, const float* obs, int n, float* out) {
  return guard([&] {
    Engine& e = drained(h);
    REQUIRE(n > 0 && n <= 1024, "act: 0 < n <= 1024");
    HIPCHK(hipSetDevice(e.cfg.device));
    auto it = e.act_graphs.find(n);
    if (it == e.act_graphs.end()) {
      rle::Prog pg = e.aux_prog();
      const int M = rle::r16(n);  // image rows; rows n..M-1 are padding
      rle::View in = e.buf(M, e.S, true, false);
      rle::View o = e.policy_fwd(pg, in, M, rle::ACT_NONE);
      rle::Graph G = e.capture(pg);
      it = e.act_graphs.emplace(n, std::make_pair(std::move(G), o)).first;
      e.act_inputs[n] = in;
    }
    rle::View in = e.act_inputs[n];
    rle::View o = it->second.second;
    const int W = e.algo == RLE_SAC ? 2 * e.A : e.A;
    const int M = rle::r16(n);
    std::vector<float> img((size_t)M * in.cols, 0.f);
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < e.S; ++c) img[Engine::h_nidx(in.m.cbn, i, c)] = obs[(size_t)i * e.S + c];
    HIPCHK(hipMemcpyAsync(in.m.n, img.data(), img.size() * 4, hipMemcpyHostToDevice, e.stream));
    HIPCHK(hipGraphLaunch(it->second.first.x, e.stream));
    std::vector<float> res((size_t)M * o.cols);
    HIPCHK(hipMemcpyAsync(res.data(), o.m.t, res.size() * 4, hipMemcpyDeviceToHost, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < W; ++c) out[(size_t)i * W + c] = res[Engine::h_tidx(o.m.rbs, i, c)];
  });
}

int rle_set_action_map(rle_engine* h, const float* scale, const float* bias, float exploration_noise) {
  return guard([&] {
    Engine& e = drained(h);
    REQUIRE(scale && bias, "set_action_map: null scale / bias");
    HIPCHK(hipSetDevice(e.cfg.device));
    e.ensure_action_map();
    std::vector<float> m((size_t)2 * e.A + 1);
    std::copy(scale, scale + e.A, m.begin());
    std::copy(bias, bias + e.A, m.begin() + e.A);
    m[2 * e.A] = exploration_noise;
    HIPCHK(hipStreamSynchronize(e.stream));
    HIPCHK(hipMemcpy(e.act_map, m.data(), m.size() * 4, hipMemcpyHostToDevice));
  });
}

int rle_act_sample(rle_engine* h, const float* obs, int n, int mode, const float* eps, float* out) {
  return guard([&] {
    Engine& e = drained(h);
    REQUIRE(n > 0 && n <= 1024 && obs && out, "act_sample: 0 < n <= 1024, obs and out");
    REQUIRE(mode >= 0 && mode <= 2 && (mode != 2 || eps), "act_sample: mode 0 / 1 / 2 (2 needs eps)");
    HIPCHK(hipSetDevice(e.cfg.device));
    e.ensure_action_map();
    auto it = e.act_samplers.find(n);
    if (it == e.act_samplers.end()) {
      Engine::ActSample as;
      const int M = rle::r16(n);
      as.in = e.buf(M, e.S, true, false);
      as.img = (float*)e.pin.alloc((size_t)M * as.in.cols * 4);
      as.ctl = (int*)e.pin.alloc(64);
      as.eps = (float*)e.pin.alloc((size_t)n * e.A * 4);
      as.out = (float*)e.pin.alloc((size_t)n * e.A * 4);
      const rle::ActArgs ao = e.act_args(as, n);
      rle::Prog pg = e.aux_prog();
      const bool sac = e.algo == RLE_SAC;
      const rle::View head = e.policy_fwd(pg, as.in, M, sac ? rle::ACT_NONE : rle::ACT_TANH);
      if (!sac) {  // td7.py:141-162, td3.py:114-135: the tanh head's GEMM becomes the act epilogue (EPI_ACT)
        rle::Op& op = pg.items.back().ops[0];
        op.gemm.epi = rle::EPI_ACT;
        op.gemm.ao = ao;
        pg.refinalize(op.gemm);
      } else {  // sac.py:132-159
        rle::Op op = e.sac_actor_op(rle::OP_SAC_ACTOR, head.m, n);
        op.sac.ao = ao;
        pg.add(op, {head.id}, {});
      }
      as.G = e.capture(pg);
      it = e.act_samplers.emplace(n, std::move(as)).first;
    }
    Engine::ActSample& as = it->second;
    if (n == 1 && !e.chain_tried) {
      e.chain_tried = true;
      static const bool no_chain = std::getenv("RLE_NO_ACT_CHAIN") != nullptr;  // A/B
      e.chain_ok = !no_chain && e.build_chain(e.act_args(as, 1));
    }
    if (n == 1 && e.chain_ok) {  // one launch, in-kernel hand-offs (kernels.hip rle_act_chain)
      rle::ActChainArgs& c = e.chain;
      std::memset(c.obs, 0, sizeof c.obs);
      std::memcpy(c.obs, obs, (size_t)e.S * 4);
      if (++e.chain_tag >= 0x80000000u) e.chain_tag = 1;  // (bit 31 marks poisoned granules)
      c.tag = e.chain_tag;
      as.ctl[8] = 0;  // the error flag of this call (set by a head workgroup whose hand-off failed)
      c.mode = mode;
      c.ctr_lo = (unsigned)e.act_counter;
      c.ctr_hi = (unsigned)(e.act_counter >> 32);
      if (mode == 1) ++e.act_counter;
      if (mode == 2) std::memcpy(c.eps, eps, (size_t)e.A * 4);
      static const bool cprof = std::getenv("RLE_ACT_PROF") != nullptr;
      static double cp[3] = {0, 0, 0};
      static long long ccalls = 0;
      static hipEvent_t ce0 = nullptr, ce1 = nullptr;
      static std::vector<double> sacc;
      if (cprof && !ce0) {
        HIPCHK(hipEventCreate(&ce0));
        HIPCHK(hipEventCreate(&ce1));
        c.stamps = e.mem.make<unsigned long long>((size_t)c.nwg * 16);
        sacc.assign(16, 0.0);
      }
      const auto t0 = std::chrono::steady_clock::now();
      if (cprof) HIPCHK(hipEventRecord(ce0, e.stream));
      HIPCHK(rle::launch_act_chain(c, e.stream));
      c.fail_wg = -1;
      if (cprof) HIPCHK(hipEventRecord(ce1, e.stream));
      const auto t1 = std::chrono::steady_clock::now();
      // the head workgroups' completion tags (system-scope release after their action stores):
      // poll pinned memory instead of waiting for the stream; a failed launch ends the poll
      for (int hw = 0; hw < c.heads; ++hw) {
        for (long long k = 1; e.done_host[hw] != c.tag; ++k) {
          if ((k & 4095) == 0 && hipStreamQuery(e.stream) != hipErrorNotReady) {
            HIPCHK(hipStreamSynchronize(e.stream));
            REQUIRE(e.done_host[hw] == c.tag, "act chain: the kernel ended without its completion tag");
            break;
          }
        }
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      const auto t2 = std::chrono::steady_clock::now();
      if (cprof) HIPCHK(hipStreamSynchronize(e.stream));
      REQUIRE(((volatile int*)as.ctl)[8] == 0, "act chain: a workgroup hand-off failed");
      std::memcpy(out, as.out, (size_t)e.A * 4);
      if (cprof) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ce0, ce1));
        cp[0] += std::chrono::duration<double, std::micro>(t1 - t0).count();
        cp[1] += std::chrono::duration<double, std::micro>(t2 - t1).count();
        cp[2] += ms * 1e3;
        std::vector<unsigned long long> sv((size_t)c.nwg * 16);
        HIPCHK(hipMemcpy(sv.data(), c.stamps, sv.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long t0s = ~0ull;
        for (int q = 0; q < c.nwg; ++q) t0s = std::min(t0s, sv[(size_t)q * 16]);
        for (int k = 1; k < 16; ++k) {  // latest workgroup to reach stamp k, after the first start
          unsigned long long mx = 0;
          for (int q = 0; q < c.nwg; ++q) mx = std::max(mx, sv[(size_t)q * 16 + k]);
          sacc[k] += mx > t0s ? (double)(mx - t0s) * 0.01 : 0.0;  // 100 MHz ticks -> us
        }
        HIPCHK(hipMemset(c.stamps, 0, sv.size() * 8));
        if (++ccalls % 2000 == 0) {
          fprintf(stderr, "act chain (us/call): launch %.2f  sync %.2f  kernel (events) %.2f\n", cp[0] / 2000,
                  cp[1] / 2000, cp[2] / 2000);
          fprintf(stderr, "  stamps (us after first start, latest wg): load %.2f", sacc[1] / 2000);
          for (int k = 2; k < 15; ++k)
            if (sacc[k] > 0) fprintf(stderr, " | hand-off %d %.2f", k - 1, sacc[k] / 2000);
          fprintf(stderr, " | head %.2f\n", sacc[15] / 2000);
          cp[0] = cp[1] = cp[2] = 0;
          std::fill(sacc.begin(), sacc.end(), 0.0);
        }
      }
      return;
    }
    const int M = rle::r16(n);
    static const bool prof = std::getenv("RLE_ACT_PROF") != nullptr;  // phase times, tools/act_bench.py
    static double tp[4] = {0, 0, 0, 0};
    static long long calls = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    const auto t0 = now();
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < e.S; ++c) as.img[Engine::h_nidx(as.in.m.cbn, i, c)] = obs[(size_t)i * e.S + c];
    as.ctl[0] = mode;
    as.ctl[1] = (int)(unsigned)e.act_counter;
    as.ctl[2] = (int)(unsigned)(e.act_counter >> 32);
    if (mode == 1) ++e.act_counter;
    if (mode == 2) std::memcpy(as.eps, eps, (size_t)n * e.A * 4);
    HIPCHK(hipMemcpyAsync(as.in.m.n, as.img, (size_t)M * as.in.cols * 4, hipMemcpyHostToDevice, e.stream));
    const auto t1 = now();
    e.launch_graph(as.G);
    const auto t2 = now();
    HIPCHK(hipStreamSynchronize(e.stream));
    const auto t3 = now();
    std::memcpy(out, as.out, (size_t)n * e.A * 4);
    if (prof) {
      tp[0] += std::chrono::duration<double, std::micro>(t1 - t0).count();
      tp[1] += std::chrono::duration<double, std::micro>(t2 - t1).count();
      tp[2] += std::chrono::duration<double, std::micro>(t3 - t2).count();
      if (++calls % 2000 == 0) {
        fprintf(stderr, "act_sample phases (us/call): stage+H2D %.2f  graph launch %.2f  sync %.2f\n", tp[0] / 2000,
                tp[1] / 2000, tp[2] / 2000);
        tp[0] = tp[1] = tp[2] = 0;
      }
    }
  });
}

int rle_launch_count(rle_engine* h, long long* n) {
  return guard([&] {
    REQUIRE(n, "launch_count: null out");
    *n = h->e->launches;
  });
}

int rle_graph_stats(rle_engine* h, int* lp, int* lplain) {
  return guard([&] {
    Engine& e = drained(h);
    if (!e.built) e.build();
    if (lp) *lp = e.policy_graph().levels();
    if (lplain) *lplain = e.plain_graph().levels();
  });
}

int rle_graph_describe(rle_engine* h, int which, char* buf, int len) {
  return guard([&] {
    Engine& e = drained(h);
    if (!e.built) e.build();
    const rle::Graph& G = e.graph_by(which);
    REQUIRE(buf && len > 0, "describe: bad buffer");
    std::snprintf(buf, (size_t)len, "%s", G.desc.c_str());
  });
}

int rle_graph_trace(rle_engine* h, int which, unsigned long long* out, long long cap, long long* n_out) {
  return guard([&] {
    Engine& e = drained(h);
    REQUIRE(n_out, "trace: null n_out");
    if (!e.built) e.build();
    const rle::Graph& G = e.graph_by(which);
    *n_out = G.trace ? G.trace_n : 0;
    if (!G.trace || !out) return;
    const int st = rle::trace_stride();
    REQUIRE(cap >= G.trace_n * st, "trace: buffer too small");
    HIPCHK(hipStreamSynchronize(e.stream));
    HIPCHK(hipMemcpy(out, G.trace, (size_t)G.trace_n * st * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *n_out = G.trace_n;
  });
}

int rle_trace_stride(void) { return rle::trace_stride(); }

// The failed-queue state machine of the AQL path without a device (no HSA call is reached): a closed
// queue refuses new bursts and completes at once, for the engine that timed out and for every engine
// sharing its hardware queue; doorbell groups never straddle the ring's end.
int rle_aql_selftest(void) {
  return guard([&] { rle::aql_selftest(); });
}

// The launch planner on a level made up from the three fields it reads of each op (no device: the table
// addresses are only copied into the packets).
int rle_level_plan(const int* kind, const int* vid, const int* wg_begin, int nops, int nwg, unsigned long long d_ops,
                   unsigned long long next_ops, int next_nops, int ks, unsigned* out, int cap, int* n, int* op_bytes) {
  return guard([&] {
    REQUIRE(kind && vid && wg_begin && nops > 0 && n && cap >= 0 && (out || cap == 0), "level_plan: bad args");
    *n = 0;
    if (op_bytes) *op_bytes = (int)sizeof(rle::Op);
    std::vector<rle::Op> ops((size_t)nops);
    for (int q = 0; q < nops; ++q) {
      ops[q].kind = kind[q];
      ops[q].wg_begin = wg_begin[q];
      if (kind[q] == rle::OP_GEMM) ops[q].gemm.vid = vid[q];
    }
    std::vector<rle::LevelLaunch> L;
    rle::level_launches(reinterpret_cast<const rle::Op*>(d_ops), ops.data(), nops, nwg, nullptr,
                        reinterpret_cast<const rle::Op*>(next_ops), next_nops, ks, L);
    *n = (int)L.size();
    for (int i = 0; i < *n && i < cap; ++i) {
      std::memcpy(out + 22 * i, &L[i].ka, sizeof(rle::LevelArgs));
      out[22 * i + 20] = L[i].grid;
      out[22 * i + 21] = (unsigned)L[i].ks;
    }
  });
}

// The scheduler on a program made up from the fields it reads of each op (no device: the items are filled
// directly, so the operand-less GEMMs never meet gemm_finalize / check_gemm; diagnostic switches off).
int rle_schedule_plan(const int* item, const int* kind, const int* wg_count, const int* attr, int nops, const int* rd_off,
                      const int* rd, const int* wr_off, const int* wr, int nitems, const rle_plan* plan, int wg_cap,
                      int* level, int* pos, int* wg_begin) {
  return guard([&] {
    REQUIRE(item && kind && wg_count && attr && nops > 0 && rd_off && wr_off && nitems > 0 && plan && wg_cap > 0 &&
                level && pos && wg_begin,
            "schedule_plan: bad args");
    REQUIRE(rd_off[0] == 0 && wr_off[0] == 0 && (rd || rd_off[nitems] == 0) && (wr || wr_off[nitems] == 0),
            "schedule_plan: resource offsets start at 0");
    const rle::PlanOptions o = rle::plan_knobs(*plan);  // (rb and xcd go unread: no GEMM is finalised here)
    REQUIRE(o.balance >= 0 && o.balance <= 3 && o.tiny_w >= 0 && o.uni_w >= 0 && o.tiny_wg >= 0 && o.pl_w >= 0 &&
                o.lap_w >= 0 && o.head_w >= 0 && o.adam_w >= 0 && (o.lpt == 0 || o.lpt == 1),
            "schedule_plan: the plan's scheduling fields must be resolved (no -1)");
    rle::Prog pg(o);
    pg.items.resize((size_t)nitems);
    for (int i = 0; i < nitems; ++i) {
      REQUIRE(rd_off[i + 1] >= rd_off[i] && wr_off[i + 1] >= wr_off[i], "schedule_plan: resource offsets must not decrease");
      pg.items[i].rd.assign(rd + rd_off[i], rd + rd_off[i + 1]);
      pg.items[i].wr.assign(wr + wr_off[i], wr + wr_off[i + 1]);
    }
    for (int q = 0; q < nops; ++q) {
      REQUIRE(item[q] >= 0 && item[q] < nitems && (q == 0 ? item[q] == 0 : item[q] == item[q - 1] || item[q] == item[q - 1] + 1),
              "schedule_plan: ops of one item are consecutive, items in order");
      REQUIRE(wg_count[q] >= 0, "schedule_plan: workgroup count");
      rle::Op op{};
      op.kind = kind[q];
      op.wg_count = wg_count[q];
      op.seq = q;  // (the op's index, to find it again in the levels)
      const int* a = attr + 4 * (size_t)q;
      if (op.kind == rle::OP_GEMM) op.gemm.R = a[0], op.gemm.tn = a[1], op.gemm.epi = a[2], op.gemm.has_pre = a[3];
      else if (op.kind == rle::OP_SAMPLE_GATHER) op.sample.lap = a[0];
      else if (op.kind == rle::OP_STEP_END) op.end.mode = a[0];
      pg.items[item[q]].ops.push_back(op);
    }
    REQUIRE(item[nops - 1] == nitems - 1, "schedule_plan: every item has an op");
    const auto levels = pg.schedule(wg_cap);
    for (size_t l = 0; l < levels.size(); ++l)
      for (size_t k = 0; k < levels[l].size(); ++k) {
        const rle::Op& op = levels[l][k];
        level[op.seq] = (int)l;
        pos[op.seq] = (int)k;
        wg_begin[op.seq] = op.wg_begin;
      }
  });
}

// The hazard check's conflict sweep on given byte ranges (no device).
int rle_hazard_scan(const unsigned long long* lo, const unsigned long long* hi, const int* write, const int* op, int n,
                    const int* item, int nops, int* op_a, int* op_b) {
  int hit = 0;
  const int rc = guard([&] {
    REQUIRE(n >= 0 && nops >= 0 && op_a && op_b && (n == 0 || (lo && hi && write && op)) && (nops == 0 || item),
            "hazard_scan: bad args");
    std::vector<rle::HazardRec> recs((size_t)n);
    for (int k = 0; k < n; ++k) {
      REQUIRE(lo[k] < hi[k] && op[k] >= 0 && op[k] < nops, "hazard_scan: a range needs lo < hi and an op below nops");
      recs[k] = {(uintptr_t)lo[k], (uintptr_t)hi[k], write[k] != 0, op[k]};
    }
    const auto [a, b] = rle::hazard_scan(recs, std::vector<int>(item, item + nops));
    *op_a = a < 0 ? -1 : recs[a].op;
    *op_b = b < 0 ? -1 : recs[b].op;
    hit = a >= 0;
  });
  return rc ? rc : hit;
}

int rle_aql_wait_plan(double expected_us, double elapsed_us, double timeout_s, double* sleep_us) {
  double sl = 0.0;
  const int act = rle::aql_wait_step(expected_us, elapsed_us, timeout_s, &sl);
  if (sleep_us) *sleep_us = sl;
  return act;
}

int rle_state_toc(rle_engine* h, int what, rle_state_entry* entries, int cap, int* n) {
  return guard([&] {
    REQUIRE(h && n && cap >= 0 && (entries || cap == 0), "state_toc: bad args");
    const Engine::StateToc& t = h->e->state_toc(what);
    *n = (int)t.entries.size();
    for (int i = 0; i < cap && i < *n; ++i) entries[i] = t.entries[i];
  });
}

int rle_state_export(rle_engine* h, int what, float* out, long long n_floats) {
  return guard([&] {
    REQUIRE(h && out, "state_export: null");
    Engine& e = drained(h);
    Engine::StateToc& t = e.state_toc(what);
    REQUIRE(n_floats == t.total, "state_export: n_floats " + std::to_string(n_floats) + ", the packed state has " +
                                     std::to_string(t.total) + " floats");
    HIPCHK(hipSetDevice(e.cfg.device));
    e.state_io_init(t);
    const size_t bytes = (size_t)t.total * sizeof(float);
    HIPCHK(rle::launch_state_pack(e.state_args(t), e.stream));
    HIPCHK(hipMemcpyAsync(e.state_host, e.state_dev, bytes, hipMemcpyDeviceToHost, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    std::memcpy(out, e.state_host, bytes);
  });
}

int rle_state_import(rle_engine* h, int what, const float* in, long long n_floats) {
  return guard([&] {
    REQUIRE(h && in, "state_import: null");
    Engine& e = drained(h);
    Engine::StateToc& t = e.state_toc(what);
    REQUIRE(n_floats == t.total, "state_import: n_floats " + std::to_string(n_floats) + ", the packed state has " +
                                     std::to_string(t.total) + " floats");
    HIPCHK(hipSetDevice(e.cfg.device));
    e.state_io_init(t);
    const size_t bytes = (size_t)t.total * sizeof(float);
    HIPCHK(hipStreamSynchronize(e.stream));  // (the pinned image: no earlier copy still reads it)
    std::memcpy(e.state_host, in, bytes);
    HIPCHK(hipMemcpyAsync(e.state_dev, e.state_host, bytes, hipMemcpyHostToDevice, e.stream));
    HIPCHK(rle::launch_state_unpack(e.state_args(t), e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    e.fold_dirty = true;  // (as rle_set_param: the folded target-critic weights follow the parameters)
  });
}

int rle_copy_nets(rle_engine* dst, rle_engine* src) {
  return guard([&] {
    REQUIRE(dst && src, "copy_nets: null engine");
    Engine& d = drained(dst);
    Engine& s = drained(src);
    REQUIRE(d.same_shapes(s), "copy_nets: the engines differ in algorithm or layer shapes");
    if (dst == src) return;
    HIPCHK(hipSetDevice(s.cfg.device));
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipSetDevice(d.cfg.device));
    // every net's N image | T image | bias is one run of the parameter arena; the log_alpha slot behind it stays
    const size_t bytes = (size_t)(d.nP - 4) * sizeof(float);
    if (d.cfg.device == s.cfg.device) HIPCHK(hipMemcpyAsync(d.P, s.P, bytes, hipMemcpyDeviceToDevice, d.stream));
    else HIPCHK(hipMemcpyPeerAsync(d.P, d.cfg.device, s.P, s.cfg.device, bytes, d.stream));
    HIPCHK(hipStreamSynchronize(d.stream));
    d.fold_dirty = true;
  });
}

int rle_copy_state(rle_engine* dst, rle_engine* src) {
  return guard([&] {
    Engine& d = drained(dst);
    Engine& s = drained(src);
    // (nP and the algorithm alone would also pass two MLPs whose widths are a permutation of each other)
    REQUIRE(d.same_shapes(s), "copy_state: config mismatch");
    d.act_counter = s.act_counter;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(d.P, s.P, 3 * d.nP * sizeof(float), hipMemcpyDeviceToDevice));
    rle::Ctrl c;
    HIPCHK(hipMemcpy(&c, s.ctrl, sizeof(c), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(d.ctrl, &c, sizeof(c), hipMemcpyHostToDevice));
    d.n_runs = s.n_runs;
    d.primed = false;
    d.fold_dirty = true;
    d.refresh_adam_scalars();  // (as rle_set_counters: both batch sets' copies, for readers outside a step)
  });
}

int rle_eval(rle_engine* h, int what, const char* net, const char* enc, const float* s, const float* a, int n,
             float* out) {
  return guard([&] {
    REQUIRE(h && net && s && out && n > 0 && n <= 1024, "eval: bad args (0 < n <= 1024)");
    REQUIRE(what == RLE_EVAL_Q || what == RLE_EVAL_ZS || what == RLE_EVAL_ZSA, "eval: bad `what`");
    REQUIRE(what == RLE_EVAL_ZS || a, "eval: needs actions");
    Engine& e = drained(h);
    const bool td7 = e.algo == RLE_TD7;
    REQUIRE(what == RLE_EVAL_Q || td7, "eval: encoder outputs exist for TD7 only");
    REQUIRE(!(td7 && what == RLE_EVAL_Q) || enc, "eval: TD7 critics need the encoder of their embeddings");
    HIPCHK(hipSetDevice(e.cfg.device));
    const std::string key = std::to_string(what) + "|" + net + "|" + (enc ? enc : "") + "|" + std::to_string(n);
    auto it = e.eval_graphs.find(key);
    if (it == e.eval_graphs.end()) {
      rle::Net& N = e.net(net);
      rle::Prog pg = e.aux_prog();
      const int M = rle::r16(n);
      Engine::EvalGraph eg;
      eg.in0 = e.buf(M, e.S, true, false);
      eg.in1 = e.buf(M, e.A, true, false);
      if (what == RLE_EVAL_Q) {
        if (td7) {  // SALECritic.estimate_q_value (sale.py:106-121) on (s, a, zsa, zs) of `enc`
          rle::Net& E = e.net(enc);
          REQUIRE(N.kind == "sale_critic" && E.kind == "sale_enc", "eval: Q needs a critic net and an encoder");
          rle::View zs = e.enc_zs(pg, E, eg.in0, M);
          rle::View zsa = e.enc_zsa(pg, E, zs, eg.in1, M);
          rle::View c01 = e.fwd(pg, N.layers[0], {{eg.in0}, {eg.in1}}, M, rle::ACT_NONE, Engine::FwdOpt().norm());
          rle::View c1 = e.fwd(pg, N.layers[1], {{c01}, {zsa}, {zs}}, M, e.actC);
          rle::View c2 = e.fwd(pg, N.layers[2], {{c1}}, M, e.actC);
          eg.out = e.fwd(pg, N.layers[3], {{c2}}, M, rle::ACT_NONE);
        } else {  // MLPCritic.estimate_q_value (mlp.py:98-101)
          REQUIRE(N.kind == "mlp_critic", "eval: Q needs a critic net");
          eg.out = e.ln_on() ? e.mlp_critic_eval_ln(pg, N, eg.in0, eg.in1, M, n)
                             : e.mlp_fwd(pg, N, {{eg.in0}, {eg.in1}}, M, rle::ACT_NONE, e.actC);
        }
        eg.width = 1;
      } else {
        REQUIRE(N.kind == "sale_enc", "eval: ZS / ZSA need an encoder net");
        rle::View zs = e.enc_zs(pg, N, eg.in0, M);
        eg.out = what == RLE_EVAL_ZS ? e.normfwd(pg, zs) : e.enc_zsa(pg, N, zs, eg.in1, M);
        eg.width = e.Z;
      }
      eg.G = e.capture(pg);
      it = e.eval_graphs.emplace(key, std::move(eg)).first;
    }
    Engine::EvalGraph& eg = it->second;
    e.upload(eg.in0, s, n, e.S);
    if (a) e.upload(eg.in1, a, n, e.A);
    HIPCHK(hipGraphLaunch(eg.G.x, e.stream));
    e.download(eg.out, out, n, eg.width);
  });
}

int rle_sac_rsample(rle_engine* h, const float* mean, const float* log_std, const float* eps, int n, float* action,
                    float* log_pi) {
  return guard([&] {
    REQUIRE(h && mean && log_std && eps && action && log_pi && n > 0 && n <= 1024, "sac_rsample: bad args");
    Engine& e = drained(h);
    REQUIRE(e.algo == RLE_SAC, "sac_rsample: SAC engines only");
    HIPCHK(hipSetDevice(e.cfg.device));
    const int A = e.A;
    const std::string key = "rsample|" + std::to_string(n);
    auto it = e.eval_graphs.find(key);
    if (it == e.eval_graphs.end()) {
      rle::Prog pg = e.aux_prog();
      const int M = rle::r16(n);
      Engine::EvalGraph eg;
      eg.in0 = e.buf(M, 2 * A);              // raw head output: mean | log_std (as mlp.4's output)
      eg.in1 = e.buf(M, A, false, true);     // eps
      eg.out = e.buf(M, A);                  // tanh action
      rle::View lp = e.vec(M);
      eg.out_vec = lp.p;
      rle::Op op = e.sac_actor_op(rle::OP_SAC_ACTOR, eg.in0.m, n);
      rle::SacActorArgs& sa = op.sac;
      sa.eps = eg.in1.m;
      sa.eps2 = eg.in1.m;
      sa.eps_row_split = 0;  // every row draws from eps
      sa.act = eg.out.m;
      sa.logpi = lp.p;
      pg.add(op, {eg.in0.id, eg.in1.id}, {eg.out.id, lp.id});
      eg.width = A;
      eg.G = e.capture(pg);
      it = e.eval_graphs.emplace(key, std::move(eg)).first;
    }
    Engine::EvalGraph& eg = it->second;
    std::vector<float> raw((size_t)n * 2 * A);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < A; ++j) {
        raw[(size_t)i * 2 * A + j] = mean[(size_t)i * A + j];
        raw[(size_t)i * 2 * A + A + j] = log_std[(size_t)i * A + j];
      }
    e.upload(eg.in0, raw.data(), n, 2 * A);
    e.upload(eg.in1, eps, n, A);
    HIPCHK(hipGraphLaunch(eg.G.x, e.stream));
    e.download(eg.out, action, n, A);
    HIPCHK(hipMemcpy(log_pi, eg.out_vec, (size_t)n * 4, hipMemcpyDeviceToHost));
  });
}

int rle_get_info(rle_engine* h, int n, float* out) {
  return guard([&] {
    Engine& e = drained(h);
    REQUIRE(out && n >= 0 && n <= e.info_cap, "get_info: 0 <= n <= info capacity (4096)");
    HIPCHK(hipStreamSynchronize(e.stream));
    HIPCHK(hipMemcpy(out, e.info, (size_t)n * rle::kInfoMax * sizeof(float), hipMemcpyDeviceToHost));
  });
}

int rle_synchronize(rle_engine* h) {
  return guard([&] { HIPCHK(hipStreamSynchronize(drained(h).stream)); });
}

}  // extern "C"
