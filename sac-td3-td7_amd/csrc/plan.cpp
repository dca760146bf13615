// The program planner (plan.h): GEMM layout checks and finalisation, the host replay of the GEMM's address
// arithmetic, per-op byte ranges and the level conflict sweep, the traffic model, and Prog's scheduler.
// Pure host logic: no HIP or HSA call, nothing global or thread-local, no environment variable.
#include "plan.h"

#include <algorithm>
#include <cstdio>
#include <string>

namespace rle {

// Layout invariants the GEMM main loop relies on (kernels.hip, "GEMM"): reduction
// segments 16-aligned, sorted and disjoint; every segment of a FWD/DX operand
// and of a DW A operand spans the whole operand row range (x0 == 0); DW B
// segments split the columns at 16-aligned bounds and share one reduction range.
void check_gemm(const GemmArgs& g) {
  auto chk = [&](const Operand& o, bool xsplit, int xn) {
    REQUIRE(o.nseg >= 1 && o.nseg <= kMaxSeg, "gemm: bad segment count");
    for (int q = 0; q < o.nseg; ++q) {
      const Seg& s = o.seg[q];
      REQUIRE(s.p != nullptr && s.r0 % 16 == 0 && s.r1 > s.r0, "gemm: bad reduction segment");
      if (!xsplit) {
        REQUIRE(s.x0 == 0 && s.x1 >= xn, "gemm: segment must span the operand rows");
        if (q) REQUIRE(s.r0 == r16(o.seg[q - 1].r1), "gemm: reduction segments must be back to back");
      } else {
        REQUIRE(s.x0 % 16 == 0 && s.x1 % 16 == 0 && s.r0 == o.seg[0].r0 && s.r1 == o.seg[0].r1,
                "gemm: bad column split");
      }
    }
  };
  chk(g.A, false, g.M);
  chk(g.B, g.mode == GEMM_DW, g.N);
  if (g.mode == GEMM_DX || (g.mode == GEMM_FWD && g.B.nseg > 1)) {  // W segment q pairs with A segment q
    REQUIRE(g.B.nseg == g.A.nseg, "gemm: one W segment per A segment");
    for (int q = 0; q < g.A.nseg; ++q)
      REQUIRE(g.B.seg[q].r0 == g.A.seg[q].r0 && g.B.seg[q].r1 == g.A.seg[q].r1, "gemm: W / A segment mismatch");
  }
  REQUIRE(g.R <= 16 * 1024, "gemm: reduction too long");
}

static void xcd_plan(GemmArgs& g, bool xcd);

bool gemm_variant_compiled(int vid, int ks) {
#define RLE_VID(mode, epi, act, norm, pre, pk, sets) \
  (vid == gemm_vid(mode, epi, act, norm, pre) && (ks < 0 || variant_in_set(sets, ks))) ||
  return RLE_GEMM_VARIANTS(RLE_VID) false;
#undef RLE_VID
}

void gemm_finalize(GemmArgs& g, bool xcd) {
  int norm = 0;
  for (int q = 0; q < g.A.nseg; ++q) norm |= g.A.seg[q].norm.part != nullptr;
  for (int q = 0; q < g.B.nseg; ++q) norm |= g.B.seg[q].norm.part != nullptr;
  // (act: the id's activation field; an activation past ACT_TANH, act_rt, takes ELU's -- ops.h act_vslot)
  const int act_rt = g.mode == GEMM_FWD ? g.act : (g.mode == GEMM_DX ? g.dact : ACT_NONE);
  const int act = g.mode == GEMM_DW ? g.act : act_vslot(act_rt);
  REQUIRE(act_rt >= ACT_NONE && act_rt <= ACT_GELU, "gemm: activation");
  REQUIRE(act_rt <= ACT_TANH || ((g.has_pre == 0 || g.has_pre == 2) &&
                                 (g.epi == EPI_STORE || g.epi == EPI_QDOT || g.epi == EPI_QHEAD)),
          "gemm: LeakyReLU / SiLU / GELU run the plain and fused-loss-head paths only (kernels.hip kActRt)");
  REQUIRE(g.mode != GEMM_DX || !norm, "gemm: no DX variant with normed operands");
  REQUIRE(g.mode != GEMM_DW || g.epi == EPI_ADAM || g.epi == EPI_GSQ,
          "gemm: DW is always fused with Adam (or is its norm pass, EPI_GSQ)");
  REQUIRE(g.epi != EPI_GSQ || (g.mode == GEMM_DW && g.adam.gsq && g.adam.gsq_b),
          "gemm: the norm pass is a weight gradient with partial slots for the weights and the bias");
  // (kDwGs with normed operands: the clipped TD7 programs' scaled Adam pass; kDwNb | kDwGs has no compiled form --
  // clipped programs run without RLE_FUSE_NBDEFER)
  REQUIRE(g.mode != GEMM_DW || act == ACT_NONE || (act == kDwGs && g.gscale) ||
              (act == kDwNb && !norm && g.nbx.t && g.nbm.part && g.nbdot && g.R <= 1024),
          "gemm: deferred AvgL1Norm backward / gradient scale operands");
  REQUIRE(g.mode != GEMM_DW || (act == kDwGs) == (g.gscale != nullptr), "gemm: gscale is the kDwGs variant's");
  REQUIRE(g.epi != EPI_NBDOT || (g.mode == GEMM_DX && act == ACT_NONE && g.nbx.t && g.norm_out),
          "gemm: EPI_NBDOT is a plain DX with x and partials");
  // row-major dot partials (RLE_FUSE_NBROWS): 16-row tiles write them; one thread per row reads rs / 4 float4s
  REQUIRE(g.norm_ld >= 0 || (g.epi == EPI_NBDOT && !g.hot.wide && -g.norm_ld % 4 == 0 && g.tiles_n <= -g.norm_ld),
          "gemm: row-major partials are the EPI_NBDOT producer's");
  REQUIRE(!(g.mode == GEMM_DW && act == kDwNb && g.nbdot_ld < 0) ||
              (g.nbm.nparts == 1 && g.R <= kThreads && -g.nbdot_ld % 4 == 0 && -g.nbdot_ld <= 16 &&
               g.nbdot_n <= -g.nbdot_ld),
          "gemm: row-major dot partials need the finalized mean and one row per thread");
  REQUIRE(g.epi != EPI_MSE || act == ACT_NONE, "gemm: MSE epilogue takes no activation");
  REQUIRE((g.dact == ACT_NONE) == (g.dsrc.t == nullptr) || g.mode != GEMM_DX, "gemm: DX derivative source");
  REQUIRE(g.has_pre != 1 || ((g.mode == GEMM_FWD || g.mode == GEMM_DX) && g.prea.N <= 32 && g.prea.seg < g.A.nseg &&
                               g.A.seg[g.prea.seg].r1 - g.A.seg[g.prea.seg].r0 <= 32 && g.prea.mode == g.mode &&
                               g.prea.R % 16 == 0),
          "gemm: pre-GEMM layout");
  {  // the fused head (kernels.hip headdx_reduce): q of every twin from EPI_QDOT partials
    const HeadArgs& h = g.hd;
    const bool pol = h.mode == HEAD_MLP_POLICY;
    const bool modes = (h.mode == HEAD_TD7_LOSS && h.tgt_mode == HEAD_TD7_TARGET && h.vt && h.vmax_key && h.vmin_key) ||
                       (h.mode == HEAD_MLP_LOSS && h.tgt_mode == HEAD_MLP_TARGET && !h.vt) ||
                       (pol && h.tgt_mode < 0 && !h.lap && h.tp_n[0] == 0 && h.tp_n[1] == 0);
    const bool parts = h.qp[0] && h.qp[1] && h.qp_n[0] <= 64 && h.qp_n[1] <= 64 &&
                       (pol || (h.tp[0] && h.tp[1] && h.tp_n[0] <= 64 && h.tp_n[1] <= 64));
    REQUIRE(g.has_pre != 2 || (g.mode == GEMM_DX && g.epi == EPI_STORE && (act == ACT_ELU || act == ACT_RELU) &&
                               !norm && g.A.nseg == 1 && modes && parts && h.dact == act_rt && (!h.sac || h.logpi) &&
                               (!h.lap || h.prio) && h.H <= 256 && h.H % 4 == 0 && g.R == r16(h.H) &&
                               g.M % 16 == 0 && h.rows == h.nvalid && h.rows <= g.M && g.M - h.rows < 16 &&
                               (g.head_n == 0 || g.head_n == 1)),
            "gemm: fused loss head layout");
  }
  REQUIRE(g.epi != EPI_SACFWD || (g.mode == GEMM_FWD && act == ACT_NONE && !norm && g.has_pre == 0 && g.tn == 64 &&
                                   g.tiles_n == 1 && g.sf.A <= 32 && g.sf.ls_off + g.sf.A <= g.N && g.sf.eps.t &&
                                   g.sf.eps2.t && (g.sf.act.n || g.sf.act.t) && g.sf.logpi),
          "gemm: SAC actor forward epilogue operands");
  REQUIRE(g.epi != EPI_SACBWD || (g.mode == GEMM_DX && act == ACT_NONE && !norm && g.has_pre == 0 && g.sb.raw.t &&
                                   g.sb.eps2.t && (g.sb.dout.n || g.sb.dout.t) && g.sb.log_alpha &&
                                   g.sb.ls_off >= g.sb.mean_off + g.N),
          "gemm: SAC actor backward epilogue operands");
  REQUIRE((g.has_pre != 3 && g.has_pre != 4) || (((g.mode == GEMM_FWD && (g.epi == EPI_STORE || g.epi == EPI_QDOT) && g.prea.bias) ||
                                (g.mode == GEMM_DX && g.epi == EPI_STORE && g.prea.dsrc.t)) &&
                               act == ACT_RELU && !norm && g.A.nseg == 1 && g.prea.seg == 0 && g.prea.mode == g.mode &&
                               g.prea.act == ACT_RELU && g.prea.N == g.A.seg[0].r1 - g.A.seg[0].r0 && g.prea.N <= 256 &&
                               g.prea.N % 16 == 0 && g.prea.R % 16 == 0 && g.prea.R <= 48 && g.prea.B.nseg == 1 &&
                               g.R == g.prea.N &&  // (<= 16 chunks per wave: kernels.hip PK 3 holds them all)
                               !g.pre.t && g.B.nseg == 1),
          "gemm: pre-layer layout");
  {  // has_pre 4: the pre-layer's input segment prea2.seg from the pre-GEMM prea2 (kernels.hip PK 4: its
     // output, at most 2 column blocks, in LDS; FWD with target smoothing, as pre_actor_fwd builds it)
    const PreArgs& q = g.prea2;
    REQUIRE(g.has_pre != 4 || (g.mode == GEMM_FWD && g.epi == EPI_QDOT && q.mode == GEMM_FWD && q.N <= 32 &&
                               q.R % 16 == 0 && q.R <= 16 * 1024 && q.A.nseg == 1 && q.B.nseg == 1 &&
                               q.seg == 1 && g.prea.A.nseg == 2 && g.prea.A.seg[0].r0 == 0 &&
                               g.prea.A.seg[q.seg].r1 - g.prea.A.seg[q.seg].r0 <= 16 &&
                               g.prea.A.seg[q.seg].r0 % 16 == 0),
            "gemm: two-stage pre-layer layout");
  }
  {  // has_pre 5: SAC's raw head + rsample (kernels.hip sacraw_*, PK 5) as segment prea.seg of a ReLU forward
    const PreArgs& q = g.prea;
    REQUIRE(g.has_pre != 5 || (g.mode == GEMM_FWD && g.epi == EPI_STORE && act == ACT_RELU && !norm &&
                               q.mode == GEMM_FWD && q.A.nseg == 1 && q.B.nseg == 1 && q.sac_a >= 1 &&
                               q.N == 2 * q.sac_a && q.N <= 48 && q.R % 16 == 0 && q.R <= 256 && q.bias &&
                               q.noise.t && q.seg < g.A.nseg && g.A.seg[q.seg].r1 - g.A.seg[q.seg].r0 <= 32 &&
                               g.A.seg[q.seg].r1 - g.A.seg[q.seg].r0 >= q.sac_a),
            "gemm: SAC pre-GEMM layout");
  }
  REQUIRE(g.epi != EPI_SACFWD || (g.R <= 256 && g.N <= 48 && g.A.nseg == 1 && g.B.nseg == 1),
          "gemm: SAC raw head (kernels.hip sacraw_*: three column blocks, R <= 256)");
  REQUIRE(g.has_pre >= 0 && g.has_pre <= 5, "gemm: pre kind");
  // (has_pre 4 takes the pre-layer's id with the norm bit, which no pre-layer variant uses; has_pre 5 a
  // pre-GEMM id with the norm bit on a ReLU forward, which no pre-GEMM consumer has)
  g.vid = g.has_pre == 4   ? gemm_vid(g.mode, g.epi, act, 1, 3)
          : g.has_pre == 5 ? gemm_vid(g.mode, g.epi, act, 1, 1)
                           : gemm_vid(g.mode, g.epi, act, norm, g.has_pre);
  REQUIRE(gemm_variant_compiled(g.vid), "gemm: no compiled variant for this mode / epilogue / activation / norm / pre "
                                        "(ops.h RLE_GEMM_VARIANTS)");
  REQUIRE(g.tn == 16 || g.tn == 32 || g.tn == 64, "gemm: tile width");
  g.ks_log = g.tn == 16 ? 2 : (g.tn == 32 ? 1 : 0);
  REQUIRE(g.R % 16 == 0, "gemm: reduction length must be a multiple of 16");
  REQUIRE((long long)g.tiles_m * g.tiles_n < 65536, "gemm: too many tiles");
  // 64-row LDS-staged tiles (kernels.hip gemm_wide): one of its variants, 64-wide tiles over whole 64-row blocks,
  // no in-tile prologue, no target smoothing; tiles_m stays the 16-row block count (loss partial slots)
  REQUIRE(!g.hot.wide || (wide_variant(g.mode, g.epi, g.has_pre) && (g.tn == 64 || g.tn == 32) &&
                          g.hot.wide == g.tn && g.M % 64 == 0 && g.tiles_m * 16 == g.M && !g.noise.t &&
                          g.N % g.tn == 0),
          "gemm: wide tile layout");
  g.inv_tiles_n = 1.f / (float)g.tiles_n;
  GemmHot& h = g.hot;
  h.ks_log = g.ks_log;
  h.tiles_n = g.tiles_n;
  h.tn = g.tn;
  h.N = g.N;
  h.R = g.R;
  h.inv_tiles_n = g.inv_tiles_n;
  h.bias_col = g.epi == EPI_ADAM || g.epi == EPI_GSQ ? g.adam.bias_col : 0;
  h.nseg_a = g.A.nseg;
  h.nseg_b = g.B.nseg;
  h.a0xs = g.A.seg[0].xs;
  h.a0r0 = g.A.seg[0].r0;
  h.a0r1 = g.A.seg[0].r1;
  h.b0xs = g.B.seg[0].xs;
  h.a0p = g.A.seg[0].p;
  h.b0p = g.B.seg[0].p;
  h.bias = g.epi == EPI_ADAM || g.epi == EPI_GSQ ? nullptr : g.bias;
  h.tiles = (g.hot.wide ? g.tiles_m / 4 : g.tiles_m) * g.tiles_n;
  xcd_plan(g, xcd);
}

// XCD-aware tile order of a GEMM (GemmHot::xb): each of the 8 XCDs takes ~tiles/8 tiles as
// a band-ordered run.  Band width b (in tiles) minimises the operand blocks one XCD reads:
// ceil(share / b) A row-blocks of 16 rows plus b B column-blocks of tn columns (both x R).
// rle_plan.xcd 0 keeps the plain row-major tile order.
static void xcd_plan(GemmArgs& g, bool xcd) {
  GemmHot& h = g.hot;
  h.xb = 0;
  if (!xcd) return;
  const int tm = g.hot.wide ? g.tiles_m / 4 : g.tiles_m, rh = g.hot.wide ? 64 : 16;  // tile rows, rows per tile
  const int T = tm * g.tiles_n;
  if (T < 16 || g.tiles_n < 2) return;
  const int share = (T + 7) / 8;
  int best = g.tiles_n;
  long long bc = -1;
  for (int b = 1; b <= g.tiles_n; ++b) {
    const long long rows = std::min<long long>(tm, (share + b - 1) / b + 1);  // a run may straddle a row
    const long long cost = rows * rh + (long long)std::min(b, share) * g.tn;
    if (bc < 0 || cost < bc) {
      bc = cost;
      best = b;
    }
  }
  h.xb = best;
  h.tmb = tm * best;
  h.nfull = g.tiles_n / best;
  h.inv_tmb = 1.f / (float)h.tmb;
  h.inv_xb = 1.f / (float)best;
  const int blast = g.tiles_n - h.nfull * best;
  h.inv_blast = blast ? 1.f / (float)blast : 0.f;
  std::vector<char> seen((size_t)T, 0);  // the order must be a permutation of the tiles
  for (int t = 0; t < T; ++t) {
    int it, jt;
    xcd_tile(t, T, g.tiles_n, h.xb, h.tmb, h.nfull, h.inv_tmb, h.inv_xb, h.inv_blast, it, jt);
    const bool ok = it >= 0 && it < tm && jt >= 0 && jt < g.tiles_n && !seen[(size_t)it * g.tiles_n + jt];
    if (!ok) {
      h.xb = 0;
      return;
    }
    seen[(size_t)it * g.tiles_n + jt] = 1;
  }
}


// ---- RLE_AUDIT=1: every byte range a GEMM op's workgroups can touch (the address arithmetic of
// kernels.hip gemm_v / pre_issue / pre_finish, replayed on the host) must lie inside one live
// device allocation.  A debugging aid for new tile layouts; off in production.
// RLE_HAZARD=1 reuses the same address replay to collect each op's byte ranges (Access) instead
// of checking them against the allocations: see level_hazards().
namespace {
// One replay of a GEMM's address arithmetic into its sink.
struct GemmAudit {
  const AuditSink sink;
  int tile = -1;  // the workgroup whose ranges the sink receives
  void audit_range(const void* base, long long lo, long long bytes, const char* what, const GemmArgs& g, int w = 0);
  void audit_mat(const Mat& m, int r, int c, const char* what, const GemmArgs& g, bool need_n = false,
                 bool need_t = false, int w = 0);
  void audit_norm(const NormRef& nr, int row, int nrows, const GemmArgs& g);
  void audit_gemm(const GemmArgs& g0);
};
}  // namespace

void audit_gemm(const GemmArgs& g, const AuditSink& sink) { GemmAudit{sink}.audit_gemm(g); }

// RLE_AUDIT=1 for a LayerNorm row op (kernels.hip op_ln): every 16 x 16 block its workgroups load or store -- rows
// [0, rows), columns [0, 16-padded width) of each image it names -- and its rstd vector lie inside an allocation.
static void audit_ln(const Op& op, const AllocRegistry& allocs) {
  const LnArgs& a = op.ln;
  const bool bwd = op.kind == OP_LN_BWD;
  auto fail = [&](const char* what) {
    char msg[200];
    snprintf(msg, sizeof msg, "audit: %s outside its allocation (%s rows %d nvalid %d width %d)", what,
             bwd ? "ln-bwd" : "ln", a.rows, a.nvalid, a.width);
    throw Error{RLE_EINVAL, msg};
  };
  auto range = [&](const void* base, long long lo, long long bytes, const char* what) {
    uintptr_t alo, ahi;
    const uintptr_t p = (uintptr_t)base + (uintptr_t)lo;
    if (!base || lo < 0 || !allocs.containing(p, &alo, &ahi) || p + (uintptr_t)bytes > ahi) fail(what);
  };
  if (a.rows <= 0 || a.rows % 16 || a.nvalid < 0 || a.nvalid > a.rows || a.width < 4 || a.width > 512 || a.width % 4 ||
      op.wg_count * 4 < a.rows)
    fail("shape");
  auto mat = [&](const Mat& m, bool need_n, const char* what) {
    if (need_n && !m.n) fail(what);
    if (m.cbn < (a.width + 15) / 16 && m.n) fail(what);
    for (int r = 0; r < a.rows; r += 16)
      for (int c = 0; c < a.width; c += 16) {
        if (m.n) range(m.n, h_nblk(m.cbn, r, c), 1024, what);
        if (m.t) range(m.t, h_tblk(m.rbs, r, c), 1024, what);
      }
  };
  mat(a.x, true, bwd ? "ln-bwd dh" : "ln z");
  mat(a.y, true, bwd ? "ln-bwd dz" : "ln h");
  if (bwd || a.u.n) mat(a.u, true, "ln u");
  if (bwd || a.rstd) range(a.rstd, 0, (long long)a.rows * 4, "ln rstd");
  if (!bwd && !a.u.n != !a.rstd) fail("ln u / rstd (kept together)");
  // (critic dropout: the probability, the site -- counter word .y = 2 + site stays clear of the step streams' 0 and
  // 1 -- the row count b * 128 + j4 fits a word with, and the step counter it reads)
  if (!(a.p >= 0.f && a.p < 1.f)) fail("ln dropout p");
  if (a.p > 0.f) {
    if (a.site < 0 || a.site >= 64 || a.rows > (1 << 25) || a.s != 1.0f / (1.0f - a.p)) fail("ln dropout site / scale");
    range(a.step, 0, 8, "ln dropout step counter");
  }
}

void GemmAudit::audit_range(const void* base, long long lo, long long bytes, const char* what, const GemmArgs& g,
                            int w) {
  if (bytes <= 0) return;
  const uintptr_t a = (uintptr_t)base + (uintptr_t)lo, b = a + (uintptr_t)bytes;
  if (sink.out) {
    sink.out->push_back({a, b, w, what, tile});
    return;
  }
  uintptr_t alo, ahi;
  const bool ok = base != nullptr && lo >= 0 && sink.allocs && sink.allocs->containing(a, &alo, &ahi) && b <= ahi;
  if (!ok) {
    char msg[256];
    snprintf(msg, sizeof msg, "audit: %s [%lld, +%lld) outside its allocation (gemm mode %d epi %d M %d N %d R %d tn %d)",
             what, lo, bytes, g.mode, g.epi, g.M, g.N, g.R, g.tn);
    throw Error{RLE_EINVAL, msg};
  }
}

void GemmAudit::audit_mat(const Mat& m, int r, int c, const char* what, const GemmArgs& g, bool need_n, bool need_t,
                          int w) {
  if (m.n) audit_range(m.n, h_nblk(m.cbn, r, c), 1024, what, g, w);
  if (m.t) audit_range(m.t, h_tblk(m.rbs, r, c), 1024, what, g, w);
  if (need_n && !m.n) throw Error{RLE_EINVAL, std::string("audit: no N image for ") + what};
  if (need_t && !m.t) throw Error{RLE_EINVAL, std::string("audit: no T image for ") + what};
}

void GemmAudit::audit_norm(const NormRef& nr, int row, int nrows, const GemmArgs& g) {
  if (!nr.part) return;
  for (int p = 0; p < nr.nparts; ++p)
    audit_range(nr.part, ((long long)p * nr.ld + nr.row0 + row) * 4, (long long)nrows * 4, "norm partials", g);
}

void GemmAudit::audit_gemm(const GemmArgs& g0) {
  // (a 64-row tile, kernels.hip gemm_wide: the byte ranges of the four 16-row tn-64 tiles it covers, in row-major
  // order -- its loss partial slots are theirs)
  GemmArgs gw;
  if (g0.hot.wide) {
    gw = g0;
    gw.hot.wide = 0;
    gw.hot.xb = 0;
    gw.hot.tiles = gw.tiles_m * gw.tiles_n;
    gw.ks_log = 0;
  }
  const GemmArgs& g = g0.hot.wide ? gw : g0;
  const GemmHot& h = g.hot;
  // wave w of a 16 x tn tile: column group w >> ks_log, reduction split w & (2^ks_log - 1)
  const int NB = g.tn / 16, T = g.tiles_m * g.tiles_n, ks = 1 << g.ks_log;
  const int nch = g.R / 16, per = (nch + ks - 1) / ks;
  for (int t = 0; t < T; ++t) {
    tile = g0.hot.wide ? -1 : t;
    int it, jt;
    if (h.xb) xcd_tile(t, h.tiles, h.tiles_n, h.xb, h.tmb, h.nfull, h.inv_tmb, h.inv_xb, h.inv_blast, it, jt);
    else {
      it = (int)(((float)t + 0.5f) * g.inv_tiles_n);
      jt = t - it * g.tiles_n;
    }
    const int i0 = it * 16, jt0 = jt * g.tn;
    const bool dw_epi = g.epi == EPI_ADAM || g.epi == EPI_GSQ;  // (the norm pass tiles as its Adam pass does)
    const int bias_col = dw_epi ? g.adam.bias_col : 0;
    const bool bias_tile = dw_epi && jt0 >= bias_col;
    bool on[4];
    for (int cb = 0; cb < NB; ++cb) on[cb] = bias_tile ? cb == 0 : jt0 + cb * 16 < g.N;
    for (int w = 0; w < 4; ++w) {
      const int cgw = w >> g.ks_log;
      const int c0 = (w & (ks - 1)) * per, c1 = std::min(nch, c0 + per);
      bool mine[4] = {false, false, false, false};  // the wave's column block
      if (cgw < NB) mine[cgw] = on[cgw];
      if (g.mode != GEMM_DW) {
        const bool wabs = g.mode == GEMM_FWD && g.B.nseg == 1;
        for (int q = 0; q < g.A.nseg; ++q) {
          const Seg& sa = g.A.seg[q];
          const Seg& sb = g.B.seg[wabs ? 0 : q];
          const int s0 = sa.r0 / 16, k0 = std::max(c0, s0), k1 = std::min(c1, (sa.r1 + 15) / 16);
          if (k0 >= k1) continue;
          const int kb = wabs ? k0 : k0 - s0;
          if (!mine[0] && !mine[1] && !mine[2] && !mine[3]) continue;  // inactive wave: no loads
          if (!((g.has_pre == 1 || g.has_pre >= 3) && q == g.prea.seg)) {
            audit_range(sa.p, ((long long)(i0 / 16) * sa.xs + (k0 - s0)) * 1024, (long long)(k1 - k0) * 1024, "A", g);
            if (sa.norm.part) audit_norm(sa.norm, i0, 16, g);
          }
          for (int cb = 0; cb < NB; ++cb)
            if (mine[cb])
              audit_range(sb.p, ((long long)(jt0 / 16 + cb) * sb.xs + kb) * 1024, (long long)(k1 - k0) * 1024, "B", g);
        }
        // pre-GEMM operands (pre_issue / pre_finish): 16 rows at i0, both column blocks (has_pre 2,
        // the fused loss head, keeps HeadArgs in the same union: its reads are not audited here)
        if (g.has_pre == 3 || g.has_pre == 4) {  // pre-layer (prelayer_*): every A chunk, the wave's 4 W column
                                                 // blocks, bias (has_pre 4: segment prea2.seg from LDS)
          const PreArgs& p = g.prea;
          for (int k = 0; k < p.R / 16; ++k) {
            int q = 0;
            for (int u = 1; u < p.A.nseg; ++u)
              if (k >= p.A.seg[u].r0 / 16) q = u;
            const Seg& sa = p.A.seg[q];
            if (!(g.has_pre == 4 && q == g.prea2.seg))
              audit_range(sa.p, ((long long)(i0 / 16) * sa.xs + (k - sa.r0 / 16)) * 1024, 1024, "prelayer A", g);
            for (int c = 0; c < 4; ++c)
              if ((w * 4 + c) * 16 < p.N)
                audit_range(p.B.seg[0].p, ((long long)(w * 4 + c) * p.B.seg[0].xs + k) * 1024, 1024, "prelayer W", g);
          }
          for (int c = 0; c < 4; ++c)
            if ((w * 4 + c) * 16 < p.N) {
              if (p.mode == GEMM_FWD)
                audit_range(p.bias, (long long)(w * 4 + c) * 64, (long long)std::min(16, p.N - (w * 4 + c) * 16) * 4,
                            "prelayer bias", g);
              else
                audit_range(p.dsrc.t, h_tblk(p.dsrc.rbs, i0, (w * 4 + c) * 16), 1024, "prelayer dsrc", g);
            }
        }
        if (g.has_pre == 5) {  // sacraw_issue: the wave's 4 chunks of A and of the 3 W column blocks; bias, noise
          const PreArgs& p = g.prea;
          const int nchp = p.R / 16, k0 = std::min(nchp, w * 4), k1 = std::min(nchp, w * 4 + 4);
          if (k1 > k0) {
            const Seg& sa = p.A.seg[0];
            audit_range(sa.p, ((long long)(i0 / 16) * sa.xs + k0) * 1024, (long long)(k1 - k0) * 1024, "sacpre A", g);
            for (int c = 0; c < 3; ++c)
              audit_range(p.B.seg[0].p, ((long long)c * p.B.seg[0].xs + k0) * 1024, (long long)(k1 - k0) * 1024,
                          "sacpre W", g);
          }
          audit_range(p.bias, 0, (long long)p.N * 4, "sacpre bias", g);
          for (int c = 0; c < p.sac_a; c += 16) audit_range(p.noise.t, h_tblk(p.noise.rbs, i0, c), 1024, "sacpre eps", g);
        }
        if (g.has_pre == 1 || g.has_pre == 4) {
          const PreArgs& p = g.has_pre == 4 ? g.prea2 : g.prea;
          const int nchp = p.R / 16, perp = (nchp + 3) / 4;
          const int c0p = w * perp, c1p = std::min(nchp, c0p + perp);
          const bool wp = p.mode == GEMM_FWD && p.B.nseg == 1;
          for (int q = 0; q < p.A.nseg; ++q) {
            const Seg& sa = p.A.seg[q];
            const Seg& sb = p.B.seg[wp ? 0 : q];
            const int s0 = sa.r0 / 16, k0 = std::max(c0p, s0), k1 = std::min(c1p, (sa.r1 + 15) / 16);
            if (k0 >= k1) continue;
            const int kb = wp ? k0 : k0 - s0;
            audit_range(sa.p, ((long long)(i0 / 16) * sa.xs + (k0 - s0)) * 1024, (long long)(k1 - k0) * 1024, "pre A", g);
            audit_range(sb.p, (long long)kb * 1024, (long long)(k1 - k0) * 1024, "pre B", g);
            if (p.N > 16) audit_range(sb.p, ((long long)sb.xs + kb) * 1024, (long long)(k1 - k0) * 1024, "pre B1", g);
          }
          if (w == 0) {
            for (int cb = 0; cb < 2 && cb * 16 < p.N; ++cb) {
              if (p.mode == GEMM_FWD) {
                if (p.bias) audit_range(p.bias, cb * 64, (long long)std::min(16, p.N - cb * 16) * 4, "pre bias", g);
                if (p.noise.t) audit_range(p.noise.t, h_tblk(p.noise.rbs, i0, cb * 16), 1024, "pre noise", g);
              } else {
                audit_range(p.dsrc.t, h_tblk(p.dsrc.rbs, i0, cb * 16), 1024, "pre dsrc", g);
              }
            }
          }
        }
      } else {
        const int nrun = c1 > c0 ? c1 - c0 : 0;
        if (!nrun || !(mine[0] || mine[1] || mine[2] || mine[3])) continue;
        audit_range(h.a0p, ((long long)(i0 / 16) * h.a0xs + c0) * 1024, (long long)nrun * 1024, "DW A", g);
        if (g.act == kDwNb || (g.nbx.t && g.nbm.part))
          audit_range(g.nbx.t, ((long long)(i0 / 16) * g.nbx_xs + c0) * 1024, (long long)nrun * 1024, "DW x", g);
        if (bias_tile) continue;
        for (int cb = 0; cb < NB; ++cb) {
          if (!mine[cb]) continue;
          const int xq = jt0 + cb * 16;
          int qb = 0;
          for (int q = 1; q < g.B.nseg; ++q)
            if (xq >= g.B.seg[q].x0) qb = q;
          const Seg& sb = g.B.seg[qb];
          audit_range(sb.p, ((long long)((xq - sb.x0) / 16) * sb.xs + c0) * 1024, (long long)nrun * 1024, "DW B", g);
        }
      }
    }
    if (g.mode == GEMM_DW)
      for (int q = 0; q < g.B.nseg; ++q)
        if (g.B.seg[q].norm.part) audit_norm(g.B.seg[q].norm, 0, g.B.seg[q].r1 - g.B.seg[q].r0, g);
    // epilogue: column block w of the tile, rows i0..i0+15
    for (int w = 0; w < NB; ++w) {
      const int j0 = jt0 + w * 16;
      const bool active = bias_tile ? w == 0 : j0 < g.N;
      if (!active) continue;
      const int ncol = bias_tile ? 1 : std::min(16, g.N - j0);
      switch (g.epi) {
        case EPI_ADAM: {
          const AdamArgs& ad = g.adam;
          if (bias_tile) {
            for (long long o : {0LL, ad.mo, ad.vo}) audit_range(ad.b, (o + i0) * 4, 64, "adam bias", g, 1);
          } else {
            for (long long o : {0LL, ad.mo, ad.vo})
              audit_range(ad.w.t, o * 4 + h_tblk(ad.w.rbs, i0, j0), 1024, "adam w.t", g, 1);
            audit_range(ad.w.n, h_nblk(ad.w.cbn, i0, j0), 1024, "adam w.n", g, 1);
          }
          if (ad.gsq) {
            if (bias_tile) audit_range(ad.gsq_b, (long long)it * 4, 4, "gsq_b", g, 1);
            else audit_range(ad.gsq, ((long long)it * (g.tiles_n - 1) + jt) * 4, 4, "gsq", g, 1);
          }
          break;
        }
        case EPI_GSQ: {  // (the norm pass: the tile's partial and nothing else)
          const AdamArgs& ad = g.adam;
          if (bias_tile) audit_range(ad.gsq_b, (long long)it * 4, 4, "gsq_b", g, 1);
          else audit_range(ad.gsq, ((long long)it * (g.tiles_n - 1) + jt) * 4, 4, "gsq", g, 1);
          break;
        }
        default: {
          audit_mat(g.out, i0, j0, "out", g, false, false, 1);
          if (g.bias) audit_range(g.bias, (long long)j0 * 4, (long long)ncol * 4, "bias", g);
          if (g.mode == GEMM_FWD && g.pre.t) audit_mat(g.pre, i0, j0, "pre-act", g, false, false, 1);
          if (g.mode == GEMM_DX && g.dact != ACT_NONE) audit_mat(g.dsrc, i0, j0, "dsrc", g, false, true);
          if (g.noise.t && i0 + 15 >= g.noise_row0) {
            const int r0 = std::max(i0, g.noise_row0) - g.noise_row0;
            audit_range(g.noise.t, h_tblk(g.noise.rbs, r0, j0), 1024, "noise", g);
            audit_range(g.noise.t, h_tblk(g.noise.rbs, i0 + 15 - g.noise_row0, j0), 1024, "noise", g);
          }
          if (g.epi == EPI_NBDOT) audit_mat(g.nbx, i0, j0, "nbx", g, false, true);
          if (g.epi == EPI_SACFWD && w == 0) {  // the tile's rows: noise, action, log pi
            const SacFwdArgs& sf = g.sf;
            for (int c : {0, sf.A - 1}) {
              if (i0 < sf.eps_row_split) audit_mat(sf.eps2, i0, c, "sac eps2", g, false, true);
              else audit_mat(sf.eps, i0 - sf.eps_row_split, c, "sac eps", g, false, true);
              audit_mat(sf.act, i0, c, "sac act", g, false, false, 1);
            }
            audit_range(sf.logpi, (long long)i0 * 4, 64, "sac logpi", g, 1);
          }
          if (g.epi == EPI_SACBWD) {  // columns j0 .. j0 + ncol - 1 of the mean and log_std blocks
            const SacBwdArgs& sb = g.sb;
            audit_mat(sb.eps2, i0, j0, "sac eps2", g, false, true);
            for (int off : {sb.mean_off, sb.ls_off})
              for (int c : {off + j0, off + j0 + ncol - 1}) {
                audit_mat(sb.raw, i0, c, "sac raw", g, false, true);
                audit_mat(sb.dout, i0, c, "sac dout", g, false, false, 1);
              }
            audit_range(sb.log_alpha, 0, 4, "sac alpha", g);
          }
          if (g.epi == EPI_MSE) {
            audit_mat(g.tgt, i0, j0, "tgt", g, false, true);
            audit_norm(g.tgt_norm, i0, 16, g);
          }
          if (g.epi == EPI_QHEAD || g.epi == EPI_QDOT) audit_range(g.qw, h_nblk(g.qw_cbn, 0, j0), 1024, "qw", g);
          if (g.epi == EPI_QHEAD && t == 0) audit_range(g.qb, 0, 4, "qb", g);
          if (g.norm_out && g.norm_ld < 0) {  // (row-major partials: one float per row)
            for (int r = 0; r < 16; ++r)
              audit_range(g.norm_out, ((long long)(i0 + r) * -g.norm_ld + jt) * 4, 4, "norm_out", g, 1);
          } else if (g.norm_out) {
            audit_range(g.norm_out, ((long long)jt * g.norm_ld + i0) * 4, 64, "norm_out", g, 1);
          }
          if (g.epi == EPI_MSE || g.epi == EPI_QHEAD) audit_range(g.loss_part, (long long)t * 4, 4, "loss_part", g, 1);
        }
      }
    }
  }
  if (g.epi == EPI_ADAM) {  // this step's bias corrections (Ctrl / adamsc1)
    audit_range(g.adam.step, 0, 4, "adam step", g);
    audit_range(g.adam.bc2s, 0, 4, "adam bc2s", g);
    if (g.gscale) audit_range(g.gscale, 0, 4, "adam gscale", g);
  }
  if (g.epi == EPI_GSQ && g.gscale) audit_range(g.gscale, 0, 4, "gsq gscale", g);
  if (g.has_pre == 2) {  // the fused loss head (kernels.hip headdx_reduce), tile rows i0 .. i0 + 15
    const HeadArgs& h = g.hd;
    const int hn = g.head_n;
    audit_range(h.w[hn], 0, (long long)h.w_cbn * 1024, "head w3", g);
    for (int n = 0; n < 2; ++n) {
      audit_range(h.b[n], 0, 4, "head b3", g);
      if (h.tb[n]) audit_range(h.tb[n], 0, 4, "head tb3", g);
    }
    if (h.vt) audit_range(h.vt, 0, 8, "head vt", g);
    if (h.sac) audit_range(h.log_alpha, 0, 4, "head alpha", g);
    for (int it = 0; it < g.tiles_m; ++it) {
      const int i0 = it * 16;
      for (int n = 0; n < 2; ++n) {
        for (int p = 0; p < h.qp_n[n]; ++p) audit_range(h.qp[n], ((long long)p * h.qp_ld + i0) * 4, 64, "head qp", g);
        for (int p = 0; p < h.tp_n[n]; ++p) audit_range(h.tp[n], ((long long)p * h.tp_ld + i0) * 4, 64, "head tp", g);
      }
      if (h.reward) audit_range(h.reward, (long long)i0 * 4, 64, "head reward", g);
      if (h.notdone) audit_range(h.notdone, (long long)i0 * 4, 64, "head notdone", g);
      if (h.sac) audit_range(h.logpi, (long long)i0 * 4, 64, "head logpi", g);
      // tile column 0 stores the head's outputs of its rows
      if (hn == 0 && h.lap) audit_range(h.prio, (long long)i0 * 4, 64, "head prio", g, 1);
      if (h.dq[hn].t) audit_range(h.dq[hn].t, h_tblk(h.dq[hn].rbs, i0, 0), 1024, "head dq", g, 1);
      if (h.dz[hn].n || h.dz[hn].t)
        for (int c = 0; c < g.R; c += 16) audit_mat(h.dz[hn], i0, c, "head dz", g, false, false, 1);
      if (hn == 0) {
        if (h.loss_part) audit_range(h.loss_part, (long long)(i0 / 4) * 16, 64, "head loss", g, 1);
        if (h.vmax_key) audit_range(h.vmax_key, 0, 4, "head vmax", g, 1);
        if (h.vmin_key) audit_range(h.vmin_key, 0, 4, "head vmin", g, 1);
      }
    }
  }
  if (g.mode == GEMM_DW && g.act == kDwNb) {
    audit_norm(g.nbm, 0, g.R, g);
    if (g.nbdot_ld < 0)  // (row-major: every row's whole stride is loaded, kernels.hip nb_rows_issue)
      audit_range(g.nbdot, 0, (long long)g.R * -g.nbdot_ld * 4, "nbdot", g);
    else
      for (int p = 0; p < g.nbdot_n; ++p) audit_range(g.nbdot, (long long)p * g.nbdot_ld * 4, (long long)g.R * 4, "nbdot", g);
  }
}

// ---- RLE_HAZARD=1: byte-level check of every level's ops against each other.  The scheduler
// orders ops by declared resources; this replays what each op's workgroups actually touch
// (GEMMs: audit_gemm's per-tile address replay; other ops: their descriptor's buffers, a tensor
// image from its pointer to the end of its allocation) and fails the build if a byte one op of a
// level stores is read or stored by another op of the same level -- a race whose outcome would
// depend on workgroup timing.  Ops of one program item (row pieces of one GEMM) are exempt from
// each other: they write disjoint rows by construction.
namespace {
// The byte ranges of one op, appended to v (allocs: where a buffer declared whole ends).
struct OpAccesses {
  const AllocRegistry& allocs;
  uintptr_t alloc_end(const void* p) const { return allocs.end_of(p); }
  void acc_whole(std::vector<Access>& v, const void* p, int w, const char* what) const;
  void acc_mat(std::vector<Access>& v, const Mat& m, int w, const char* what) const;
  void op_accesses(const Op& op, std::vector<Access>& v) const;
};
}  // namespace
void OpAccesses::acc_whole(std::vector<Access>& v, const void* p, int w, const char* what) const {
  if (p) v.push_back({(uintptr_t)p, alloc_end(p), w, what});
}
static void acc_bytes(std::vector<Access>& v, const void* p, long long bytes, int w, const char* what) {
  if (p && bytes > 0) v.push_back({(uintptr_t)p, (uintptr_t)p + (uintptr_t)bytes, w, what});
}
void OpAccesses::acc_mat(std::vector<Access>& v, const Mat& m, int w, const char* what) const {
  acc_whole(v, m.n, w, what);
  acc_whole(v, m.t, w, what);
}
void OpAccesses::op_accesses(const Op& op, std::vector<Access>& v) const {
  switch (op.kind) {
    case OP_GEMM: {
      audit_gemm(op.gemm, AuditSink{nullptr, &v});
      break;
    }
    case OP_NORMBWD: {
      const NormBwdArgs& a = op.nb;
      if (a.fwd == 2) {  // finalize: partials in, one mean per row out
        acc_whole(v, a.norm.part, 0, "nb norm");
        acc_bytes(v, a.mout, (long long)a.rows * 4, 1, "nb mean");
        break;
      }
      acc_mat(v, a.g, 0, "nb g");
      acc_mat(v, a.x, 0, "nb x");
      acc_whole(v, a.norm.part, 0, "nb norm");
      acc_mat(v, a.dx, 1, "nb dx");
      break;
    }
    case OP_SAMPLE_REDUCE:
    case OP_SAMPLE_GATHER:
    case OP_NOISE: {
      const SampleArgs& s = op.sample;
      acc_bytes(v, s.size, 8, 0, "sample size");
      acc_bytes(v, s.tape_mode, 4, 0, "tape mode");
      acc_bytes(v, s.tape_pos, 8, 0, "tape pos");
      acc_bytes(v, s.ctrl_rng, 8, 0, "rng step");
      if (op.kind == OP_NOISE) {
        acc_whole(v, s.tape_eps, 0, "tape eps");
        acc_whole(v, s.tape_eps2, 0, "tape eps2");
        acc_mat(v, s.eps, 1, "eps");
        acc_mat(v, s.eps2, 1, "eps2");
        break;
      }
      acc_whole(v, s.priority, 0, "priority");
      acc_whole(v, s.bsum, op.kind == OP_SAMPLE_REDUCE, "bsum");
      acc_whole(v, s.ssum, op.kind == OP_SAMPLE_REDUCE, "ssum");
      if (op.kind == OP_SAMPLE_REDUCE) break;
      for (const void* r : {(const void*)s.state, (const void*)s.next_state, (const void*)s.action,
                            (const void*)s.reward, (const void*)s.notdone})
        acc_whole(v, r, 0, "replay");
      acc_whole(v, s.tape_u, 0, "tape u");
      acc_whole(v, s.tape_ind, 0, "tape ind");
      if (s.pend_n) {
        acc_bytes(v, s.pend_ind, 8LL * s.pend_n, 0, "pending ind");
        acc_bytes(v, s.pend_p, 4LL * s.pend_n, 0, "pending p");
      }
      acc_mat(v, s.ss, 1, "batch ss");
      acc_mat(v, s.a, 1, "batch a");
      acc_whole(v, s.r, 1, "batch r");
      acc_whole(v, s.nd, 1, "batch nd");
      acc_whole(v, s.ind, 1, "batch ind");
      acc_whole(v, s.u_out, 1, "batch u");
      if (s.n_step > 1) {  // (n-step returns: the write pointer beside the size, and the rows' hop counts)
        acc_bytes(v, s.ptr, 8, 0, "replay ptr");
        acc_whole(v, s.hops_out, 1, "batch hops");
      }
      break;
    }
    case OP_HEAD: {
      const HeadArgs& h = op.head;
      for (int n = 0; n < 2; ++n) {
        acc_mat(v, h.h[n], 0, "head h");
        acc_mat(v, h.dsrc[n], 0, "head dsrc");
        acc_bytes(v, h.w[n], (long long)h.w_cbn * 1024, 0, "head w");
        acc_bytes(v, h.b[n], 4, 0, "head b");
        if (h.tgt_mode >= 0) {
          acc_mat(v, h.th[n], 0, "head th");
          acc_bytes(v, h.tw[n], (long long)h.w_cbn * 1024, 0, "head tw");
          acc_bytes(v, h.tb[n], 4, 0, "head tb");
        }
        acc_whole(v, h.qp[n], 0, "head qp");
        acc_whole(v, h.tp[n], 0, "head tp");
        acc_mat(v, h.dz[n], 1, "head dz");
        acc_mat(v, h.dq[n], 1, "head dq");
      }
      acc_whole(v, h.reward, 0, "head reward");
      acc_whole(v, h.notdone, 0, "head notdone");
      const bool tgt = h.mode == HEAD_TD7_TARGET || h.mode == HEAD_MLP_TARGET;
      acc_whole(v, h.y, tgt || h.tgt_mode >= 0, "head y");
      acc_whole(v, h.logpi, 0, "head logpi");
      acc_bytes(v, h.log_alpha, 4, 0, "head log_alpha");
      acc_bytes(v, h.vt, 8, 0, "head vt");
      acc_whole(v, h.loss_part, 1, "head loss");
      acc_whole(v, h.prio, 1, "head prio");
      if (h.mode == HEAD_TD7_TARGET || h.tgt_mode == HEAD_TD7_TARGET) {
        acc_bytes(v, h.vmax_key, 4, 1, "head vmax");
        acc_bytes(v, h.vmin_key, 4, 1, "head vmin");
      }
      break;
    }
    case OP_PRIORITY: {
      const PriorityArgs& a = op.prio;
      acc_whole(v, a.p, 0, "prio p");
      acc_whole(v, a.ind, 0, "prio ind");
      acc_whole(v, a.priority, 1, "priority");
      acc_whole(v, a.bsum, 1, "bsum");
      acc_whole(v, a.ssum, 1, "ssum");
      acc_bytes(v, a.max_priority, 4, 1, "max priority");
      break;
    }
    case OP_SAC_ACTOR:
    case OP_SAC_ACTOR_BWD: {
      const SacActorArgs& a = op.sac;
      acc_mat(v, a.out, 0, "sac out");
      acc_mat(v, a.eps2, 0, "sac eps2");
      if (op.kind == OP_SAC_ACTOR) {
        acc_mat(v, a.eps, 0, "sac eps");
        acc_mat(v, a.act, 1, "sac act");
        acc_whole(v, a.logpi, 1, "sac logpi");
      } else {
        acc_mat(v, a.da, 0, "sac da");
        acc_bytes(v, a.log_alpha, 4, 0, "sac log_alpha");
        acc_mat(v, a.dout, 1, "sac dout");
      }
      break;
    }
    case OP_STEP_END: {  // (mode 1: counters + temperature; mode 2: the info row; 0: both)
      const StepEndArgs& a = op.end;
      const bool info = a.mode != 1, ctr = a.mode != 2, scr = a.mode == 2 && a.sac_scratch;
      if (info)
        for (int k = 0; k < a.ninfo; ++k)
          if (a.part[k]) acc_bytes(v, a.part[k], (long long)a.npart[k] * a.stride[k] * 4, 0, "info part");
      if (a.logpi_part && !scr) acc_bytes(v, a.logpi_part, (long long)a.nlogpi * 16, 0, "logpi part");
      if (info && a.gsq && a.ngsq_t > 0) acc_bytes(v, a.gsq, (long long)a.gsq_off[a.ngsq_t] * 4, 0, "gsq");
      if (ctr) acc_bytes(v, a.counters, 16 * 8, 1, "counters");
      if (info) acc_bytes(v, a.info_slot, 4, 1, "info slot");
      if (info) acc_whole(v, a.info, 1, "info ring");
      if (a.log_alpha && !scr) acc_bytes(v, a.log_alpha, 4, ctr && a.la_lr > 0.f, "log_alpha");
      if (ctr && a.la_lr > 0.f) {
        acc_bytes(v, a.la_m, 4, 1, "la_m");
        acc_bytes(v, a.la_v, 4, 1, "la_v");
        acc_bytes(v, a.la_t, 8, 1, "la_t");
      }
      if (a.sac_scratch) acc_bytes(v, a.sac_scratch, 8, a.mode == 1, "sac scratch");
      // (offline TD3 reads lmbda too, INFO_SUM_BC3 / INFO_BCS1: bytes [4, 8) of OP_BC's out)
      if (info && a.bcs) acc_bytes(v, a.bcs, a.kind[1] == INFO_SUM_BC3 ? 8 : 4, 0, "bc q_abs");
      break;
    }
    case OP_POLYAK:
    case OP_COPY: {
      const FlatArgs& f = op.flat;
      acc_bytes(v, f.dst, f.n * 4, 1, "flat dst");
      if (!f.self_alias) acc_bytes(v, f.src, f.n * 4, 0, "flat src");
      break;
    }
    case OP_MAXRED: {
      const FlatArgs& f = op.flat;
      if (f.stage == 0) {
        acc_bytes(v, f.size, 8, 0, "maxred size");
        acc_whole(v, f.src, 0, "maxred src");
        acc_bytes(v, f.partial, (long long)f.nwg * 4, 1, "maxred partial");
      } else {
        acc_bytes(v, f.partial, (long long)f.nwg * 4, 0, "maxred partial");
        acc_bytes(v, f.out, 4, 1, "maxred out");
      }
      break;
    }
    case OP_CTRL: {
      const CtrlArgs& c = op.ctrl;
      if (c.mode == 0) {
        acc_bytes(v, c.vmax_key, 4, 0, "vmax key");
        acc_bytes(v, c.vmin_key, 4, 0, "vmin key");
        acc_bytes(v, c.vt, 8, 1, "vt");
      } else {
        acc_bytes(v, c.counters, 3 * 8, 0, "counters");
        acc_bytes(v, c.adam_step, (c.la_t ? 4 : 3) * 4, 1, "adam step");
        acc_bytes(v, c.adam_bc2s, (c.la_t ? 4 : 3) * 4, 1, "adam bc2s");
        if (c.la_t) acc_bytes(v, c.la_t, 8, 0, "la_t");
      }
      break;
    }
    case OP_BC: {
      const BcArgs& b = op.bc;
      if (b.mode == 0) {
        acc_whole(v, b.pi.n, 0, "bc pi");
        acc_whole(v, b.a.n, 0, "bc a");
        acc_whole(v, b.e.n, 1, "bc e");
        acc_bytes(v, b.part, (long long)((b.nvalid + 15) / 16) * 4, 1, "bc part");
        break;
      }
      if (b.mode == 3) {  // (offline TD3 beside the fused head: mode 1's reads, mode 2's writes)
        for (int n = 0; n < 2; ++n) {
          acc_bytes(v, b.qp[n], (long long)b.qp_n[n] * b.qp_ld * 4, 0, "bc qp");
          acc_bytes(v, b.qb[n], 4, 0, "bc b3");
        }
        acc_whole(v, b.eye.t, 1, "bc eye");
        acc_bytes(v, b.out, 8, 1, "bc q_abs lmbda");
        break;
      }
      if (b.mode == 2) {  // (offline TD3: the policy head's loss partials, slot 1 of every group of qp_ld)
        acc_bytes(v, b.qp[0], ((long long)(b.qp_n[0] - 1) * b.qp_ld + 1) * 4, 0, "bc |min| partials");
        acc_whole(v, b.eye.t, 1, "bc eye");
        acc_bytes(v, b.out, 8, 1, "bc q_abs lmbda");
        break;
      }
      for (int n = 0; n < 2; ++n) {
        acc_bytes(v, b.qp[n], (long long)b.qp_n[n] * b.qp_ld * 4, 0, "bc qp");
        acc_bytes(v, b.qb[n], 4, 0, "bc b3");
      }
      acc_whole(v, b.eye.t, 1, "bc eye");
      acc_bytes(v, b.out, 4, 1, "bc q_abs");
      break;
    }
    case OP_AWAC: {  // (rows < nvalid of every operand; whole images where a row's floats are scattered)
      const AwacArgs& a = op.awac;
      acc_mat(v, a.raw, 0, "awac raw");
      acc_mat(v, a.a, 0, "awac a");
      for (int n = 0; n < 2; ++n) {
        acc_mat(v, a.qd[n], 0, "awac q(s, a)");
        acc_mat(v, a.qv[n], 0, "awac q(s, a_pi)");
      }
      acc_bytes(v, a.logpi, (long long)a.nvalid * 4, 0, "awac logpi");
      acc_mat(v, a.dout, 1, "awac dout");
      acc_bytes(v, a.adv, (long long)a.nvalid * 4, 1, "awac adv");
      acc_bytes(v, a.w, (long long)a.nvalid * 4, 1, "awac w");
      acc_bytes(v, a.part, (long long)((a.nvalid + 3) / 4) * 16, 1, "awac partials");
      break;
    }
    case OP_CLIP: {
      const ClipArgs& c = op.clip;
      acc_bytes(v, c.part, (long long)c.n * 4, 0, "clip partials");
      if (c.gin) acc_bytes(v, c.gin, 4, 0, "clip gin");
      acc_bytes(v, c.out, 8, 1, "clip total coef");
      acc_bytes(v, c.scale, 4, 1, "clip scale");
      break;
    }
    case OP_LN:
    case OP_LN_BWD: {  // (rows [0, rows) of every image, each row's floats scattered over its row block: whole images)
      const LnArgs& a = op.ln;
      const bool bwd = op.kind == OP_LN_BWD;
      acc_mat(v, a.x, 0, bwd ? "ln-bwd dh" : "ln z");
      acc_mat(v, a.y, 1, bwd ? "ln-bwd dz" : "ln h");
      acc_mat(v, a.u, bwd ? 0 : 1, "ln u");
      acc_bytes(v, a.rstd, (long long)a.rows * 4, bwd ? 0 : 1, "ln rstd");
      if (a.p > 0.f) acc_bytes(v, a.step, 8, 0, "rng step");  // (critic dropout: the mask stream's step word)
      break;
    }
    case OP_FOLDBIAS: {
      const FoldBiasArgs& f = op.fb;
      acc_bytes(v, f.wn, (long long)((f.H + 15) / 16) * f.cbn * 1024, 0, "fold w");
      acc_bytes(v, f.bin, (long long)f.H * 4, 0, "fold bin");
      acc_bytes(v, f.bbase, (long long)f.H * 4, 0, "fold bbase");
      acc_bytes(v, f.bout, (long long)f.H * 4, 1, "fold bout");
      break;
    }
    default:
      throw Error{RLE_EINVAL, "hazard check: unknown op kind " + std::to_string(op.kind)};
  }
}

std::pair<int, int> hazard_scan(const std::vector<HazardRec>& recs, const std::vector<int>& item) {
  std::vector<int> all(recs.size());  // the records in order of their start
  for (size_t k = 0; k < all.size(); ++k) all[k] = (int)k;
  std::sort(all.begin(), all.end(), [&](int x, int y) { return recs[x].lo < recs[y].lo; });
  // sweep: active intervals (those whose hi > current lo); report a pair from different items
  // where one side writes
  std::vector<int> act;
  for (int k : all) {
    const HazardRec& c = recs[k];
    size_t keep = 0;
    for (int j : act)
      if (recs[j].hi > c.lo) act[keep++] = j;
    act.resize(keep);
    for (int j : act) {
      const HazardRec& o = recs[j];
      if (o.op == c.op || item[o.op] == item[c.op] || !(o.w || c.w)) continue;
      return {j, k};
    }
    act.push_back(k);
  }
  return {-1, -1};
}

void level_hazards(const std::vector<Op>& ops, const std::vector<int>& item, int level, const AllocRegistry& allocs) {
  std::vector<HazardRec> all;
  std::vector<const char*> what;
  std::vector<Access> v;
  const OpAccesses acc{allocs};
  for (size_t i = 0; i < ops.size(); ++i) {
    v.clear();
    acc.op_accesses(ops[i], v);
    for (const Access& a : v) {
      all.push_back({a.lo, a.hi, a.w, (int)i});
      what.push_back(a.what);
    }
  }
  const auto [jo, jc] = hazard_scan(all, item);
  if (jo < 0) return;
  const HazardRec &o = all[jo], &c = all[jc];
  char msg[320];
  snprintf(msg, sizeof msg, "hazard: level %d op %d (%s, kind %d, %s) and op %d (%s, kind %d, %s) overlap at %#lx", level,
           o.op, what[jo], ops[o.op].kind, o.w ? "write" : "read", c.op, what[jc], ops[c.op].kind, c.w ? "write" : "read",
           (unsigned long)c.lo);
  throw Error{RLE_EINVAL, msg};
}

static double union_bytes(std::vector<std::pair<uintptr_t, uintptr_t>>& v) {
  std::sort(v.begin(), v.end());
  double tot = 0;
  uintptr_t lo = 0, hi = 0;
  bool open = false;
  for (auto& r : v) {
    if (!open || r.first > hi) {
      if (open) tot += (double)(hi - lo);
      lo = r.first;
      hi = r.second;
      open = true;
    } else {
      hi = std::max(hi, r.second);
    }
  }
  if (open) tot += (double)(hi - lo);
  return tot;
}
LevelTraffic level_traffic(const std::vector<Op>& ops, const float* P, size_t nP, const AllocRegistry& allocs) {
  LevelTraffic t;
  const OpAccesses acc{allocs};
  std::vector<std::pair<uintptr_t, uintptr_t>> ar, aw, wr, ad;
  std::vector<std::pair<uintptr_t, uintptr_t>> xr[8], once;  // (per-XCD model: GEMM reads by XCD, other reads)
  const uintptr_t p0 = (uintptr_t)P, p1 = p0 + 3 * nP * 4;
  std::vector<Access> v;
  for (const Op& op : ops) {
    v.clear();
    if (op.kind == OP_SAMPLE_GATHER) {  // rows of the batch + one path down the LAP sum tree per query
      const SampleArgs& s = op.sample;
      t.other += (double)s.nq * (2.0 * s.Sp + s.Ap + 2) * 4 + (s.lap ? s.nq * (64.0 * 8 + 64 * 4) + s.nblk * 8.0 : 0);
      t.act_w += (double)s.B * ((s.ss.n != nullptr) + (s.ss.t != nullptr)) * 2 * s.Sp * 4 +
                 (double)s.B * ((s.a.n != nullptr) + (s.a.t != nullptr)) * s.Ap * 4 + s.B * 20.0;
      if (s.n_step > 1) {  // n-step returns: a state and a next_state row, reward and notdone per further hop (the
                           // walk's upper bound: every hop's loads are issued), and the hop count per row
        t.other += (double)s.nq * (s.n_step - 1) * (2.0 * s.Sp + 2) * 4;
        t.act_w += s.B * 4.0;
      }
      continue;
    }
    if (op.kind == OP_PRIORITY) {  // the scattered rows (a 64-B line each) and their two sums
      t.other += (double)op.prio.B * (8 + 4) + op.prio.B * 64.0 * 3;
      continue;
    }
    if (op.kind == OP_MAXRED && op.flat.stage == 0) {
      t.other += 4.0 * 1e6;  // (the replay size is a device value: the 1M benchmark ring)
      continue;
    }
    acc.op_accesses(op, v);
    for (const Access& a : v) {
      const std::string what = a.what ? a.what : "";
      if (what.rfind("tape", 0) == 0) continue;  // (declared whole; read only in tape mode, one row)
      const bool in_p = a.lo >= p0 && a.hi <= p1;
      // (reads: every range not stored, and Adam's T-image / bias ranges, which hold p, m, v read and then written)
      if (!a.w || what == "adam w.t" || what == "adam bias") {
        if (op.kind == OP_GEMM && a.t >= 0) xr[(op.wg_begin + a.t) & 7].push_back({a.lo, a.hi});
        else once.push_back({a.lo, a.hi});
      }
      if (what.rfind("adam", 0) == 0) {
        if (a.w) t.adam_w += (double)(a.hi - a.lo);
        ad.push_back({a.lo, a.hi});
        if (what == "adam w.t" || what == "adam bias") ad.push_back({a.lo, a.hi});  // (read and written)
      } else if (a.w) {
        aw.push_back({a.lo, a.hi});
      } else if (in_p) {
        wr.push_back({a.lo, a.hi});
      } else {
        ar.push_back({a.lo, a.hi});
      }
    }
  }
  t.act_r += union_bytes(ar);
  t.act_w += union_bytes(aw);
  t.w_r += union_bytes(wr);
  // Adam ranges: each listed range once per direction (reads p, m, v; writes p T, m, v, p N)
  double adam = 0;
  for (auto& r : ad) adam += (double)(r.second - r.first);
  t.adam = adam;
  double xb = union_bytes(once);
  for (auto& r : xr) xb += union_bytes(r);
  t.xcd_r = xb;
  return t;
}

// ---- struct Prog: dependency levelling, rebalance, longest-first order, wg_begin (rules: plan.h)
bool Prog::rb_eligible(const GemmArgs& g) {
  bool seg_ok = true;  // (the tile's column blocks lie in one X segment, kernels.hip rb path)
  for (int q = 0; q < g.B.nseg; ++q) seg_ok = seg_ok && g.B.seg[q].x0 % g.tn == 0;
  return g.mode == GEMM_DW && (g.tn == 32 || g.tn == 64) && g.has_pre == 0 && seg_ok;
}

void Prog::add_group(std::vector<Op> ops, std::vector<int> rd, std::vector<int> wr) {
  for (Op& op : ops)
    if (op.kind == OP_GEMM) {
      op.gemm.hot.rb = opt.rb && rb_eligible(op.gemm) ? 1 : 0;
      gemm_finalize(op.gemm, opt.xcd != 0);
      check_gemm(op.gemm);
      if (opt.audit) audit_gemm(op.gemm, AuditSink{opt.allocs, nullptr});
    } else if ((op.kind == OP_LN || op.kind == OP_LN_BWD) && opt.audit) {
      audit_ln(op, *opt.allocs);
    }
  Item it;
  it.ops = std::move(ops);
  it.rd = std::move(rd);
  it.wr = std::move(wr);
  items.push_back(std::move(it));
}

int Prog::op_weight(const Op& op) const {
  int x = 8;
  if (op.kind == OP_GEMM)
    x = op.gemm.R * op.gemm.tn / 1024 + (op.gemm.epi == EPI_ADAM ? opt.adam_w : 0) + (op.gemm.has_pre >= 3 ? opt.pl_w : 0);
  else if (op.kind == OP_HEAD) x = opt.head_w;
  // (a LayerNorm row op: 4 rows per workgroup, two or three float4s per lane and two wave sums -- one load round
  // trip and two dependent reductions whatever the width, so about a narrow GEMM tile; set by that reasoning, not
  // tuned: the ops sit alone on their levels of the critic chain, where the weight moves nothing)
  else if (op.kind == OP_LN || op.kind == OP_LN_BWD) x = 4 + op.ln.width / 128;
  else if (op.kind == OP_SAMPLE_GATHER) x = op.sample.lap ? opt.lap_w : uniform_weight();  // (uniform: a
                                                                                     // ~6 us gather)
  else if (op.kind == OP_STEP_END && op.end.mode != 1) x = tiny_weight();  // (one workgroup, ~4 KB of straight-line
                                                       // code fetched at L2 latency: 7-8 us)
  return x;
}

int Prog::item_weight(const Item& it) const {
  int w = 0;
  for (const Op& op : it.ops) w = std::max(w, op_weight(op));
  return w;
}

std::vector<std::vector<int>> Prog::successors() const {
  const int n = (int)items.size();
  std::vector<std::vector<int>> succ(n);
  std::map<int, int> lastw;
  std::map<int, std::vector<int>> readers;
  for (int i = 0; i < n; ++i) {
    const Item& it = items[i];
    auto edge = [&](int from) {
      if (from >= 0) succ[from].push_back(i);
    };
    for (int r : it.rd)
      if (r >= 0 && lastw.count(r)) edge(lastw[r]);
    for (int w : it.wr) {
      if (w < 0) continue;
      if (lastw.count(w)) edge(lastw[w]);
      for (int j : readers[w]) edge(j);
    }
    for (int w : it.wr)
      if (w >= 0) {
        lastw[w] = i;
        readers[w].clear();
      }
    for (int r : it.rd)
      if (r >= 0) readers[r].push_back(i);
  }
  return succ;
}

void Prog::mark_critical(int maxl) {
  const int n = (int)items.size();
  const auto succ = successors();
  std::vector<int> tail(n, 0);
  for (int i = n - 1; i >= 0; --i)
    for (int s : succ[i]) tail[i] = std::max(tail[i], tail[s] + 1);
  crit.assign(n, 0);
  for (int i = 0; i < n; ++i) crit[i] = items[i].level + tail[i] == maxl;
}

void Prog::rebalance(int maxl, std::vector<int>& nops, std::vector<int>& nwg, int wg_cap) {
  const int n = (int)items.size();
  const auto succ = successors();
  std::vector<int> wmax(maxl + 1, 0);
  for (auto& it : items) wmax[it.level] = std::max(wmax[it.level], item_weight(it));
  const int cap = std::min(wg_cap, 1024);
  for (int i = n - 1; i >= 0; --i) {
    Item& it = items[i];
    int hi = maxl;
    for (int s : succ[i]) hi = std::min(hi, items[s].level - 1);
    const int cur = it.level;
    if (hi <= cur) continue;
    int wg = 0;
    for (auto& op : it.ops) wg += op.wg_count;
    const int wt = item_weight(it);
    bool adam = false;
    for (auto& op : it.ops) adam = adam || (op.kind == OP_GEMM && op.gemm.epi == EPI_ADAM);
    if (opt.balance >= 2 && adam) continue;
    const int wfac = opt.balance >= 3 ? 2 : 1;
    int best = -1;
    for (int l = cur + 1; l <= hi; ++l) {
      if (nops[l] + (int)it.ops.size() > max_ops || wt * wfac > wmax[l] || nwg[l] + wg > cap) continue;
      if (nwg[l] + wg >= nwg[cur]) continue;
      if (best < 0 || nwg[l] < nwg[best]) best = l;
    }
    // a one-workgroup op (the step end) that is the longest of its level: into the first level
    // of its window that has a longer op, so its time hides there
    if (best < 0 && tiny_moves() && wg <= opt.tiny_wg && wt >= wmax[cur]) {
      for (int l = cur + 1; l <= hi && best < 0; ++l)
        if (wmax[l] > wt && nops[l] + (int)it.ops.size() <= max_ops && nwg[l] + wg <= cap) best = l;
    }
    if (best < 0) continue;
    nops[cur] -= (int)it.ops.size();
    nwg[cur] -= wg;
    nops[best] += (int)it.ops.size();
    nwg[best] += wg;
    it.level = best;
  }
}

std::vector<std::vector<Op>> Prog::schedule(int wg_cap) {
  std::map<int, int> lw, lr;
  int maxl = -1;
  std::vector<int> nops, nwg;
  for (auto& it : items) {
    int l = 0;
    for (int r : it.rd)
      if (r >= 0 && lw.count(r)) l = std::max(l, lw[r] + 1);
    for (int w : it.wr) {
      if (w < 0) continue;
      if (lw.count(w)) l = std::max(l, lw[w] + 1);
      if (lr.count(w)) l = std::max(l, lr[w] + 1);
    }
    // a level of more than max_ops ops would take two launches: defer to the next level
    // with room (every dependence is still met at a later level)
    int wg = 0;
    for (auto& op : it.ops) wg += op.wg_count;
    while (l < (int)nops.size() &&
           (nops[l] + (int)it.ops.size() > max_ops || (nwg[l] > 0 && nwg[l] + wg > wg_cap)))
      ++l;
    if (l >= (int)nops.size()) {
      nops.resize(l + 1, 0);
      nwg.resize(l + 1, 0);
    }
    nops[l] += (int)it.ops.size();
    nwg[l] += wg;
    it.level = l;
    for (int w : it.wr)
      if (w >= 0) lw[w] = l;
    for (int r : it.rd)
      if (r >= 0) lr[r] = std::max(lr.count(r) ? lr[r] : -1, l);
    maxl = std::max(maxl, l);
  }
  if (opt.crit) mark_critical(maxl);
  if (opt.balance) rebalance(maxl, nops, nwg, wg_cap);
  std::vector<std::vector<Op>> levels(maxl + 1);
  std::vector<std::vector<int>> owner(maxl + 1);
  crit_lv.assign(maxl + 1, {});
  for (size_t i = 0; i < items.size(); ++i)
    for (auto& op : items[i].ops) {
      levels[items[i].level].push_back(op);
      owner[items[i].level].push_back((int)i);
      crit_lv[items[i].level].push_back(crit.empty() ? 0 : crit[i]);
    }
  if (opt.lpt)  // longest first (rle_plan lpt): a stable sort of each level by the estimated workgroup time
    for (size_t l = 0; l < levels.size(); ++l) {
      std::vector<int> ix(levels[l].size());
      for (size_t k = 0; k < ix.size(); ++k) ix[k] = (int)k;
      std::stable_sort(ix.begin(), ix.end(),
                       [&](int a, int b) { return op_weight(levels[l][a]) > op_weight(levels[l][b]); });
      std::vector<Op> lv;
      std::vector<int> ow;
      std::vector<char> cr;
      for (int k : ix) {
        lv.push_back(levels[l][k]);
        ow.push_back(owner[l][k]);
        cr.push_back(crit_lv[l][k]);
      }
      levels[l].swap(lv);
      owner[l].swap(ow);
      crit_lv[l].swap(cr);
    }
  if (opt.hazard)
    for (size_t l = 0; l < levels.size(); ++l) level_hazards(levels[l], owner[l], (int)l, *opt.allocs);
  for (auto& lv : levels) {
    int wg = 0;
    for (auto& op : lv) {
      op.wg_begin = wg;
      wg += op.wg_count;
    }
  }
  return levels;
}

}  // namespace rle
