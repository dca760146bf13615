/*
 * rle.h — C ABI of the MI355X off-policy update engine (librle.so).
 *
 * The reference (seungju-k1m/sac-td3-td7) has no FFI: its hot path is the
 * Python method Agent.train_ops(batch, replay_buffer) (rl/agent/abc.py:23-28)
 * driven by run_train_ops (rl/runner/run.py:87-96).  This ABI sits UNDER the
 * Python classes that mirror that interface (sac-td3-td7_amd/rl); each entry
 * point below names the reference interface it replaces.
 *
 * Conventions: every function returns 0 on success or a negative error code;
 * rle_last_error() returns a thread-local message for the last failure.  All
 * pointers are host pointers borrowed for the duration of the call; the
 * engine owns all device memory.  A handle is bound to one device and one
 * HIP stream and is not thread-safe.  Plain C types only (no torch types).
 */
#ifndef RLE_H
#define RLE_H

#ifdef __cplusplus
extern "C" {
#endif

#define RLE_TD7 0
#define RLE_TD3 1
#define RLE_SAC 2

#define RLE_INFO_MAX 8
#define RLE_MAX_N_STEP 8 /* rle_set_n_step / rle_replay_gather_nstep: the longest n-step return */

#define RLE_OK 0
#define RLE_EINVAL (-1)
#define RLE_EHIP (-2)
#define RLE_ESTATE (-3)

typedef struct rle_replay rle_replay;
typedef struct rle_engine rle_engine;

typedef struct rle_config {
  int algo;                 /* RLE_TD7 / RLE_TD3 / RLE_SAC */
  int state_dim, action_dim;  /* 1..1024, 1..128 */
  int hidden;               /* hidden width, a multiple of 4, <= 512 (TD7: hdim; TD3/SAC: every hidden layer unless
                               n_hidden is set) */
  int batch;                /* B, 1..1024 (padded to 16 rows inside; the padded rows count in nothing) */
  int use_lap;              /* TD7/TD3: LAP Huber + priority update */
  float discount;           /* td7.py:37 / td3.py:36 / sac.py:30 */
  float policy_lr, critic_lr;
  float tau;                /* TD3/SAC Polyak */
  float target_policy_noise, noise_clip;
  int policy_freq;          /* TD7/TD3 */
  int target_update_rate;   /* TD7 hard update period */
  float min_log_std, max_log_std;  /* SAC */
  float tmp;                /* SAC: < 0 => auto temperature (sac.py:36,55) */
  unsigned long long seed;  /* Philox stream for sampling / noise */
  int device;
  /* Net shapes beyond the defaults (make_nn, td7.py:46-61 / td3.py:44-58 / sac.py:40-52): */
  int zs_dim;               /* TD7: SALE embedding width (sale.py:23 zs_dim); 0 = hidden; a multiple of 4, <= 512.  `hidden` is hdim */
  int n_hidden;             /* TD3/SAC: hidden layers of make_mlp (mlp.py:10-35), 2..RLE_MAX_HIDDEN; 0 = two
                               layers of `hidden` (mlp.py:45-47) */
  int hidden_sizes[8];      /* TD3/SAC: their widths, input side first (each a multiple of 4, <= 512) */
  /* Hidden-layer activations (RLE_ACT_*: ReLU, ELU, Identity, LeakyReLU, SiLU, GELU; 0 = the reference default of
     that net), forward and backward as torch computes them in fp32.  TD7: SALEActor / SALECritic /
     SALEEncoder `activ` (sale.py:25,67,97: ReLU / ELU / ELU); TD3/SAC: make_mlp's action_fn of the policy and of the
     critics (mlp.py:13, default ReLU; act_encoder must be 0).  A non-default activation runs its programs on the
     extended kernel instance (LeakyReLU / SiLU / GELU: on a copy of it that also holds their variants) without
     RLE_FUSE_PRELAYER, PRE, TWOSTAGE and SACPRE (and, for identity critics, without QDOT and HEADDX). */
  int act_actor, act_critic, act_encoder;
  /* TD7 offline mode (the paper's behaviour-cloning term; the reference names it, rl/cli.py:110-123, and does
     not implement it): on policy steps the actor objective is
       -mean(cat Q) + bc_lambda * mean|cat Q|.detach() * mse(pi(s), a)      (a: the batch's stored action).
     0 = online: the programs are the online ones, op for op.  > 0 (the paper: 0.1): every program with a policy
     step gains two forward GEMMs that store the per-row q of the policy pass (EPI_QDOT partials, beside the
     q-head GEMMs), two small ops off the chain (OP_BC: the mse and lmbda 2 (pi - a) / (B A) once the actor
     output exists; q_abs and q_abs I a level after the partials) and one reduction segment of r16(A) rows in
     the action-gradient GEMM, which adds dL_bc / d pi ahead of tanh'.  The in-tile recomputation of that
     gradient (RLE_FUSE_PRE) takes the same extra segment, so no fusion is dropped and the policy step keeps
     its level count.  The info row gains train/bc (the mse) and train/q_abs after
     train/policy (NaN on other steps).  The parameter layout does not change: rle_copy_state, rle_copy_nets
     and rle_state_* work between engines whose bc_lambda differ.  Negative, NaN, or > 0 with another
     algorithm: RLE_EINVAL. */
  float bc_lambda;
} rle_config;
/* Extension of rle_config.  rle_config itself is frozen (bc_lambda stays its last field); later settings are
   added here, at the end, and a caller compiled against an older header keeps working: `size` tells the
   library how much of the struct the caller knows, and every field past it reads as 0. */
typedef struct rle_config_ext {
  int size;        /* sizeof(rle_config_ext) as the caller compiled it; fields past it read as 0 */
  /* TD3 offline mode (TD3+BC, Fujimoto & Gu 2021; the reference does not implement it): on policy steps the
     actor objective is
       -lmbda * mean(min(Q1, Q2)) + mse(pi(s), a),   lmbda = bc_alpha / mean|min(Q1, Q2)|.detach()
     (a: the batch's stored action; every mean over the B valid rows; min(Q1, Q2) is this code base's TD3
     objective, td3.py:191; no guard for mean|Q| = 0, as in the paper's code: lmbda is then inf).  0 = online: the
     programs are the online ones, op for op.  > 0 (the paper: 2.5): the backward chain stays the online one
     (dL/dq = -1/B, so it carries the gradient of L / lmbda); two small ops off the chain (OP_BC: the mse and
     2 (pi - a) / (B A) once the actor output exists; q_abs, lmbda and (q_abs / bc_alpha) I beside the fused
     policy head from the policy pass's q row partials, or a level after the standalone head from its |min|
     partials) feed one more reduction segment of r16(A) rows into the
     action-gradient GEMM (and its in-tile recomputation, RLE_FUSE_PRE), and the actor's Adam epilogues and
     the norm/policy partials multiply the accumulated gradient by the device scalar lmbda.  No fusion is
     dropped; a plain step keeps its level count, a policy step too under the default plan (at most one more
     with the standalone loss head).  The info row gains train/bc (the mse)
     and train/lmbda after norm/policy (NaN on other steps).  The parameter layout does not change:
     rle_copy_state, rle_copy_nets and rle_state_* work between engines whose bc_alpha differ.  Negative, NaN,
     infinite, > 0 with another algorithm, or a `size` that does not reach the field (see awac_lambda for the
     valid sizes): RLE_EINVAL. */
  float bc_alpha;
  /* SAC offline mode (AWAC, Nair et al. 2020; the reference does not implement it): the critic step is SAC's own
     at a fixed temperature of 0, and the policy step minimises
       L = -mean(w log pi(a | s)),   w = min(exp((Q(s, a) - Q(s, a_pi)) / awac_lambda), 100).detach()
     (a: the batch's stored action, clamped to +-(1 - 1e-6) before atanh; a_pi: the policy's own rsample;
     Q = min(Q1, Q2) of the updated critics; log pi: the squashed Gaussian's, with annotation.py:12 EPS; every mean
     over the B valid rows; no guard for a tiny sigma).  0 = online: the programs are the online ones, op for op.
     > 0 (the paper: 1): requires algo == RLE_SAC, tmp == 0 and use_lap == 0.  No gradient passes through the
     critics: the policy phase forwards them on (s, a) and (s, a_pi), one row-wise op (OP_AWAC) forms adv, w and
     dL / d(mean | log_std), and the actor's backward and Adam run from there as online; the critics' input
     gradients, the squashed-Gaussian backward, the policy loss head and the temperature update are absent.  A step
     has no more levels than online.  The info row is train/q_fn, train/policy (= L), entropy, train/adv (mean
     advantage) and train/weight (mean w).  The parameter layout is that of a fixed-temperature SAC engine:
     rle_copy_state, rle_copy_nets and rle_state_* work between engines whose awac_lambda differ.  Negative, NaN,
     infinite, > 0 with another algorithm, with tmp != 0 or with use_lap: RLE_EINVAL.
     `size`: one of the sizes this struct ever had, 8 (through bc_alpha) or 12 (through awac_lambda); any other
     value, one that ends inside a field included, is RLE_EINVAL. */
  float awac_lambda;
} rle_config_ext;
#define RLE_MAX_HIDDEN 6
#define RLE_ACT_DEFAULT 0
#define RLE_ACT_RELU 1
#define RLE_ACT_ELU 2       /* alpha = 1 (F.elu / nn.ELU defaults) */
#define RLE_ACT_IDENTITY 3  /* action_fn "Identity" / nn.Identity(): no activation between the Linear layers */
#define RLE_ACT_LEAKY_RELU 4 /* negative_slope = 0.01 (F.leaky_relu / nn.LeakyReLU defaults) */
#define RLE_ACT_SILU 5
#define RLE_ACT_GELU 6      /* the exact erf form (F.gelu / nn.GELU defaults, approximate "none") */
/* Any other code is RLE_EINVAL.  Not run: Tanh as a hidden activation, other slopes / alphas, GELU's tanh
   approximation, and every other activation. */

/* Step-program plan: the schedule and tile-plan choices that decide how the step's reductions are
 * split (so its fp32 summation order) and how its ops are fused.  Every engine starts from the
 * defaults (rle_plan_default); rle_set_plan changes them before the engine's first step, and
 * rle_get_plan reports the values in effect.  No environment variable changes a plan. */
#define RLE_FUSE_PRELAYER (1u << 0)  /* small-K first layers recomputed in-tile by the next layer   */
#define RLE_FUSE_PRE      (1u << 1)  /* actor output layer recomputed in-tile by its consumers      */
#define RLE_FUSE_QDOT     (1u << 2)  /* TD7 q from per-tile row partials of the last hidden layers  */
#define RLE_FUSE_HEADDX   (1u << 3)  /* critic loss heads fused into the DX of the last hidden layer */
#define RLE_FUSE_NBDEFER  (1u << 4)  /* TD7 AvgL1Norm backward deferred into the weight gradient    */
#define RLE_FUSE_SACFWD   (1u << 5)  /* SAC rsample in the actor raw head's epilogue                */
#define RLE_FUSE_SACBWD   (1u << 6)  /* SAC squashed-Gaussian backward in the da DX's epilogue      */
#define RLE_FUSE_FOLD     (1u << 7)  /* TD7 fixed target encoder's zsa3 folded into target critics  */
#define RLE_FUSE_PIPOLYAK (1u << 8)  /* TD3 aliased target-policy Polyak in the actor's Adam         */
#define RLE_FUSE_ENDSPLIT (1u << 9)  /* step end split into counters and info row                  */
#define RLE_FUSE_PRIOSAMPLE (1u << 10) /* LAP priority update applied by the next batch's sampler (opt-in,
                                        fuse_on): one level fewer per step pair, but the heavy critic
                                        weight-gradient ops then share a level with the next batch's
                                        first layers (TD7 Humanoid A/B: -4.5%)                        */
#define RLE_FUSE_TWOSTAGE (1u << 11) /* TD3 target critics' first layer (behind the pre-GEMM target
                                        action) recomputed in-tile by their second layer             */
#define RLE_FUSE_SACPRE   (1u << 12) /* SAC raw head + target rsample recomputed in-tile by the target
                                        critics' first layer                                         */
#define RLE_FUSE_NORMFIN  (1u << 13) /* TD7: the AvgL1Norm row means finalized once (a small op the level after
                                        their producer) for the weight gradients' per-row tables      */
#define RLE_FUSE_NBROWS   (1u << 14) /* TD7: the deferred AvgL1Norm backward's dot partials stored row-major, so a
                                        weight-gradient workgroup builds a row's two scalars from 1-5 loads, not 32
                                        (B <= 256 on the TD7 instance; the same floats either way)   */
#define RLE_FUSE_OPT_IN RLE_FUSE_PRIOSAMPLE  /* fusions off unless set in fuse_on                      */
typedef struct rle_plan {
  int level_cap;        /* workgroups per level the tile planner targets (0: resident capacity; TD7 at B >= 1024 5/4
                           (3/2 when lpt is 0); TD3 7/8 when lpt is 0) */
  int steps_per_graph;  /* steps per multi-step graph (-1: TD7 6, SAC 8, TD3 16; 0: single-step only)  */
  int pre_tn;           /* tile width of pre-GEMM consumers (0: TD3 64, else 32)                         */
  int pl_tn;            /* tile width of pre-layer consumers (0: SAC 32, else 64)                        */
  int tn_min;           /* narrowest GEMM tile (0: 16)                                                   */
  int flat_div;         /* Polyak / copy workgroups count 1 / flat_div in the planner (0: 4)            */
  int balance;          /* rebalance pass: 0 off, 1 any item, 2 no Adam items, 3 no Adam items and only under a
                           twice-longer op (-1: TD7 3, SAC 2, TD3 1)                                        */
  int tiny_w, uni_w, tiny_wg;  /* rebalance weights: step end, uniform sampler, tiny-op bound (-1: 30,
                                  SAC 30 / TD3 8 / TD7 60, 2) */
  int sched_cap;        /* 1: the scheduler defers ops past level_cap workgroups to a later level       */
  unsigned fuse_off;    /* RLE_FUSE_* bits switched off (A/B, tests); 0 = every default fusion on       */
  unsigned fuse_on;     /* RLE_FUSE_OPT_IN bits switched on                                             */
  int rb;               /* 1: 32 / 64-wide weight-gradient tiles register-blocked (the 4 waves split the batch
                           rows, each accumulates every column block; -1: default)                       */
  int pl_w;             /* rebalance weight added to GEMMs with an in-tile prologue (pre-layer, two-stage,
                           SAC raw head; -1: default, SAC 24, else 0)                                     */
  int lap_w, head_w, adam_w; /* rebalance weights: LAP sampler, loss head, added to Adam-epilogue GEMMs
                                (-1: 60, 60, SAC 16 / else 8)                                             */
  int wide;             /* 64 / 32: forward / input-gradient GEMMs over >= 64 rows as 64 x 64 / 64 x 32 tiles with
                           every W chunk staged once in LDS for the tile's four 16-row blocks (kernels.hip
                           gemm_wide; 1 = 64; 0 off; -1: default = off, slower than the 16-row tiles as
                           measured)                                                     */
  int lpt;              /* 1: each level's ops in its launch ordered longest first (estimated workgroup time),
                           so a level with more workgroups than the device holds dispatches its long tiles in
                           the first round and its long workgroups start first; 0: program order; -1: default = 1) */
  /* Launch choices (they change no result: the same ops, tiles and summation order either way) */
  int dispatch;         /* how the step programs' level launches reach the device: 1 direct AQL kernel-dispatch
                           packets in the engine's own HSA queue; 0 hipGraph replays on the engine's HIP stream;
                           2 level launches on the stream without a graph (A/B); -1: default = 1            */
  int dpf;              /* 1: each launch leads with one workgroup per XCD that loads the next launch's op
                           descriptors into that XCD's L2; 0 off (A/B); -1: default = 1                     */
  int xcd;              /* 1: XCD-aware tile order (each XCD a compact band of a GEMM's tiles); 0 row-major
                           (A/B); -1: default = 1                                                          */
} rle_plan;

/* ---- replay memory: rl/replay_memory/{lap,simple}.py ---------------------- */

/* LAPReplayMemory.__init__ (lap.py:15-29) / SimpleReplayMemory.__init__ (simple.py:15-27). */
int rle_replay_create(int device, long long capacity, int state_dim, int action_dim, int lap,
                      rle_replay** out);
int rle_replay_destroy(rle_replay* r);
/* append (lap.py:31-43): rows of fp32 state[S], action[A] (already a/scale - bias), reward,
 * next_state[S], notdone (1 - terminated).  count rows, host pointers. */
int rle_replay_append(rle_replay* r, const float* state, const float* action, const float* reward,
                      const float* next_state, const float* notdone, long long count);
/* ptr / size / max_priority (lap.py:18-29, len = ptr Q6). */
int rle_replay_state(rle_replay* r, long long* ptr, long long* size, float* max_priority);
/* Test / bench hooks. */
int rle_replay_fill_random(rle_replay* r, long long count, unsigned long long seed);
int rle_replay_get_priority(rle_replay* r, float* out, long long n);
int rle_replay_set_priority(rle_replay* r, const float* p, long long n, float max_priority);
/* Device LAP/uniform index search with given uniforms (lap.py:47-54, simple.py:45-54). */
int rle_replay_sample_indices(rle_replay* r, int n, const float* u, long long* ind_out);
/* LAPReplayMemory.update_priority (lap.py:66-69) with explicit indices (any values; with a
 * priority below 1 the block sums are recomputed instead of updated in place).  Every replay
 * operation waits for the steps already enqueued by engines bound to the replay. */
int rle_replay_update_priority(rle_replay* r, int n, const long long* ind, const float* p);
/* LAPReplayMemory.reset_max_priority (lap.py:71-73). */
int rle_replay_reset_max_priority(rle_replay* r);
/* Gather rows (state, action, reward, next_state, notdone) for indices (lap.py:55-60). */
int rle_replay_gather(rle_replay* r, int n, const long long* ind, float* state, float* action,
                      float* reward, float* next_state, float* notdone);
/* The n-step law.  For a sampled slot i of a ring with capacity cap, `size` rows, write pointer ptr, n = n_step and
 * gamma = discount, everything in fp32 with one rounding per product and per sum (no contraction):
 *   cur = i; R = reward[cur]; g = 1.0f; hops = 1
 *   while hops < n:
 *       if notdone[cur] == 0: break                                  (terminated)
 *       nxt = cur + 1; if nxt == cap: nxt = 0
 *       if nxt >= size or nxt == ptr: break                          (cur is the newest row)
 *       if bits(next_state[cur, :S]) != bits(state[nxt, :S]): break  (episode cut)
 *       g = g * gamma; R = R + g * reward[nxt]; cur = nxt; hops += 1
 *   out: state[i], action[i], R, next_state[cur], g * notdone[cur], hops
 * Continuity comes from the data: row nxt continues row cur iff the S stored next_state words of cur equal the S
 * state words of nxt as 32-bit patterns (so -0.0 != 0.0, and a NaN equals itself only with the same payload).  That
 * catches time-limit truncation, resets, rle_replay_import seams and the write head, needs no column of its own (the
 * ring, the packed row, snapshots and rle_replay_copy are unchanged), and survives rle_replay_normalize_states, which
 * applies one fp32 expression to equal bits.  The one false positive: an episode whose reset state equals the previous
 * row's next_state bit for bit is taken as its continuation.
 * rle_replay_gather_nstep is the law's observable, as rle_replay_gather is the ring's: it runs the device function
 * the step's sampler runs (on that sampler's kernel instance) for the given indices, each in 0 .. size-1, and returns
 * the n-step host batch: state [n][S], action [n][A], reward [n] (R), next_state [n][S] (of the last hop), notdone [n]
 * (gamma^(hops-1) * notdone of the last hop) and hops [n]; any output pointer may be NULL.  n_step 1 .. RLE_MAX_N_STEP
 * (else RLE_EINVAL); n_step = 1 returns bit for bit what rle_replay_gather returns, and hops 1.  Syncs. */
int rle_replay_gather_nstep(rle_replay* r, int n, const long long* ind, int n_step, float discount, float* state,
                            float* action, float* reward, float* next_state, float* notdone, int* hops);
/* Whole-replay state.  The reference's replays are NumPy arrays and Python scalars (lap.py:18-29,
 * simple.py:15-27), so pickle.dumps(replay) and copy.deepcopy(replay) work on them as they are, as
 * deepcopy(agent) does on the agent (run_w_checkpoint.py:72).  These entries give the HBM ring the same. */
/* Rows per internal staging chunk of export / import / gather (no GPU call). */
int rle_replay_io_rows(void);
/* The arrays of lap.py:18-28 / simple.py:15-26 for slots first .. first+count-1 -> host, unpadded fp32
 * (state [count][S], action [count][A], reward, next_state, notdone, priority [count]); any pointer may be
 * NULL; priority: LAP replays only.  A host read: waits for the bound engines' enqueued steps. */
int rle_replay_export(rle_replay* r, long long first, long long count, float* state, float* action,
                      float* reward, float* next_state, float* notdone, float* priority);
/* The reverse (unpickling those arrays): host -> slots first .. first+count-1.  Moves neither ptr nor size;
 * a NULL priority leaves the priorities alone; the LAP sums follow in rle_replay_set_state. */
int rle_replay_import(rle_replay* r, long long first, long long count, const float* state,
                      const float* action, const float* reward, const float* next_state,
                      const float* notdone, const float* priority);
/* ptr, size, max_priority (lap.py:18-19,29) after an import: recomputes the LAP block and sub-block sums
 * (rows at or past size count as 0) and makes bound engines redraw their prefetched batch. */
int rle_replay_set_state(rle_replay* r, long long ptr, long long size, float max_priority);
/* copy.deepcopy(replay) on the device(s): the whole ring, priorities, LAP sums, ptr / size / max_priority of
 * src into dst (same capacity, dims and lap; the two may live on different GPUs).  No host round trip. */
int rle_replay_copy(rle_replay* dst, rle_replay* src);
/* Dataset state normalisation on the device (the TD3+BC recipe's; a 1M-row Humanoid ring would otherwise make
 * a 3 GB host round trip).  Like every replay operation they first wait for the bound engines' enqueued steps. */
/* Per-feature mean and population std (ddof 0) of `state` over rows [0, size): fp64 accumulation,
 * two passes (mean, then centred squares), fixed reduction order (per-workgroup partials whose count depends
 * on size and state_dim alone, added in ascending order); results rounded to fp32.  mean [S], std [S].
 * NULL pointer: RLE_EINVAL; size == 0: RLE_ESTATE. */
int rle_replay_state_stats(rle_replay* r, float* mean, float* std);
/* state and next_state of rows [0, size) <- (x - shift[j]) / scale[j] in fp32, in that order of operations.
 * The ring's pad columns stay zero, rows at or past size, priorities and LAP sums are untouched, and bound
 * engines redraw their prefetched batch.  shift [S], scale [S]; a NULL pointer, a non-finite shift, a zero
 * or non-finite scale: RLE_EINVAL; size == 0: RLE_ESTATE. */
int rle_replay_normalize_states(rle_replay* r, const float* shift, const float* scale);

/* ---- agent: rl/agent/{td7,td3,sac}.py ------------------------------------- */

/* TD7.__init__ (td7.py:34-87) / TD3.__init__ (td3.py:33-74) / SAC.__init__ (sac.py:27-77). */
int rle_create(const rle_config* cfg, rle_engine** out);
/* The same with an extension (NULL: every extension field 0; rle_create is exactly this with NULL). */
int rle_create_ext(const rle_config* cfg, const rle_config_ext* ext, rle_engine** out);
int rle_destroy(rle_engine* e);
/* The default plan (every field "default"); the engine's plan before its first step; the plan in
 * effect (defaults resolved for this engine's algorithm and device). */
int rle_plan_default(rle_plan* out);
int rle_set_plan(rle_engine* e, const rle_plan* plan);
int rle_get_plan(rle_engine* e, rle_plan* out);
/* Gradient-norm clipping in the device step (torch.nn.utils.clip_grad_norm_ per optimizer, error_if_nonfinite
 * False: a NaN or inf norm propagates).  One max_norm for every optimizer of a gradient step: TD7's encoder, the
 * critics (q1 + q2, one optimizer) and SAC's policy every step, the TD7 / TD3 policy on policy steps; SAC's
 * temperature is never clipped.  total = sqrt(sum over the optimizer's tensors of sum g^2),
 * coef = min(1, max_norm / (total + 1e-6)), g <- g * coef.  TD3's norm/policy info stays the norm before clipping.
 * 0 or +inf: off (the default): the unclipped step programs op for op, on the kernel instance they run on today.
 * > 0: clip every optimizer of the step to this global L2 norm (the programs then run on a kernel instance of
 * their own, without RLE_FUSE_NBDEFER).  Before the engine's first step only (RLE_ESTATE after it); negative or
 * NaN: RLE_EINVAL.  rle_copy_state, rle_copy_nets and rle_state_* work between engines whose setting differs. */
int rle_set_grad_clip(rle_engine* e, float max_norm);
int rle_get_grad_clip(rle_engine* e, float* max_norm);  /* (0: off) */
/* {total, coef} of the last update of each optimizer: [0] critics, [1] policy, [2] TD7 encoder (NaN for an
 * optimizer that has not stepped or when clipping is off).  Syncs. */
int rle_grad_clip_stats(rle_engine* e, float* out6);
/* Parameter-free LayerNorm (torch.nn.LayerNorm(width, elementwise_affine=False), eps 1e-5) after every hidden
 * Linear of q1, q2 and their targets, before the activation; the H -> 1 output layer and the actor are unchanged.
 * It runs in every pass of the critics: the target, online and policy passes of the step, AWAC's forward-only
 * passes and rle_eval(RLE_EVAL_Q).  Per row, in fp32, over the layer's `width` columns: mu = sum z / width,
 * var = sum (z - mu)^2 / width (biased, two passes), u = (z - mu) / sqrt(var + 1e-5), h = act(u).  No parameter:
 * the parameter arena, the packed state, the state_dict names and rle_copy_state / rle_copy_nets / rle_state_*
 * are unchanged and work between engines whose setting differs.
 * critic: 0 off (default: the programs and the kernel instance of today, op for op), 1 on (the programs then run
 * on a kernel instance of their own, the critic heads stand-alone; composes with every activation, both offline
 * modes and rle_set_grad_clip).  TD3 / SAC only (TD7: RLE_EINVAL).  Before the engine's first step (RLE_ESTATE
 * after it); forward programs captured earlier (rle_eval) are dropped and rebuilt.
 * Not run: an affine LayerNorm, another eps, LayerNorm in the actor, RMSNorm / BatchNorm. */
int rle_set_layer_norm(rle_engine* e, int critic);
int rle_get_layer_norm(rle_engine* e, int* critic);
/* Critic dropout (the DroQ critic: Linear -> Dropout(p) -> LayerNorm -> activation): inverted dropout as
 * torch.nn.Dropout(p) in train mode on the output z of every hidden Linear of q1, q2 and their targets, ahead of the
 * LayerNorm, inside the row-norm ops: keep_j = u01(word_j) >= p, zd_j = keep_j ? z_j * s : 0 with s = 1 / (1 - p) in
 * float32, then the LayerNorm of rle_set_layer_norm on zd; backward dz_j = keep_j ? dzd_j * s : 0.  An all-dropped
 * row is legal (zd 0, var 0, u 0).  Active in every critic pass of a gradient step -- target, online and policy
 * pass, AWAC's two forward-only passes -- and off in rle_eval(RLE_EVAL_Q), which is inference.  The H -> 1 output
 * layer and the actor are unchanged.
 * The mask: Philox4x32-10 keyed by cfg.seed at counter (b * 128 + j4, 2 + site, step_lo, step_hi); the four output
 * words are columns 4 j4 .. 4 j4 + 3 of batch row b; step is the RNG step counter (rle_get_counters()[4]) of the
 * step that consumes the batch, read on the device; site = (pass * 2 + twin) * 8 + layer with pass 0 target,
 * 1 online, 2 policy (AWAC: Q(s, a_pi)), 3 AWAC's Q(s, a), twin 0 / 1, layer 0 .. RLE_MAX_HIDDEN-1.  The backward
 * op draws the mask again: nothing is stored, and masks are never taped (rle_set_tapes).
 * p: 0 <= p < 1 (NaN, negative or >= 1: RLE_EINVAL); 0 is off (default: the LayerNorm programs and their kernel
 * instance, op for op; p > 0 runs on a kernel instance of its own with the same level counts).  p > 0
 * needs the critics' LayerNorm on at the call (RLE_EINVAL otherwise: dropout without LayerNorm is not run), and
 * rle_set_layer_norm(e, 0) while p > 0 is RLE_EINVAL.  TD3 / SAC only (TD7: RLE_EINVAL).  Before the engine's
 * first step (RLE_ESTATE after it).  Not part of the state: rle_copy_state / rle_copy_nets / rle_state_* work
 * between engines whose p differ.
 * Not run: dropout without LayerNorm, dropout in the actor, taped masks. */
int rle_set_critic_dropout(rle_engine* e, float p);
int rle_get_critic_dropout(rle_engine* e, float* p);
/* The mask stream's observable, as rle_replay_fill_random is for its streams: runs the device's mask function (the
 * one the row ops call) for `rows` batch rows and `width` columns (4 .. 512, a multiple of 4; rows <= 2^20) of
 * `site` (0 .. 63) at RNG step `step`, with the engine's p, and writes rows x width floats, row-major, each 0
 * (dropped) or s = 1 / (1 - p) (kept).  With p = 0 (dropout off) every element is kept and the output is all ones.
 * Syncs. */
int rle_dropout_mask(rle_engine* e, long long step, int site, int rows, int width, float* out);
/* n-step returns (TD3 / SAC): the step's sampler gathers, for every sampled slot, the n-step batch row of the law at
 * rle_replay_gather_nstep with gamma = cfg.discount -- the n-step reward in the reward column, the last hop's
 * next_state in the next-state rows, gamma^(hops-1) * notdone in the not-done column -- so the critic target
 * y = r + gamma * notdone * Q'(s') becomes R + gamma^hops * notdone_last * Q'(s'_last), and every head, loss, LAP
 * priority, offline mode, clip, LayerNorm and dropout path downstream runs unchanged, op for op.  Indices (sampled,
 * LAP or taped) stay those of the first row; rle_last_indices and the priority update refer to it.
 * n: 1 .. RLE_MAX_N_STEP (else RLE_EINVAL); 1 is off (default: today's programs on today's kernel instance; n > 1
 * runs on a kernel instance of its own with the same level counts).  n > 1 on TD7 is RLE_EINVAL: its encoder learns
 * the one-step model zsa(s, a) -> zs(s') from the same next-state rows.  Before the engine's first step (RLE_ESTATE
 * after it).  Not part of the state: rle_copy_state / rle_copy_nets / rle_state_* work between engines whose n differ.
 * With n > 1 the info row gains one column after the agent's own: replay/hops, the mean hops of the step's batch.
 * Not run: n-step for TD7, an explicit episode-end column, per-row n, lambda-returns, n-step on a host batch. */
int rle_set_n_step(rle_engine* e, int n);
int rle_get_n_step(rle_engine* e, int* n);
/* Bind the replay the step samples from (the replay_buffer arg of train_ops). */
int rle_bind_replay(rle_engine* e, rle_replay* r);
/* Parameter import/export in the reference's state_dict layout (Agent.load_state_dict,
 * td7.py:114-125; deepcopy / pickle, abc.py:38-55).  net: "policy", "q1", "q2", "target_q1",
 * "target_q2", "encoder", "fixed_encoder", "fixed_encoder_target"; name: e.g. "q01.weight",
 * "mlp.2.bias"; SAC temperature: net "tmp", name "log_alpha". */
int rle_param_numel(rle_engine* e, const char* net, const char* name, long long* numel);
int rle_get_param(rle_engine* e, const char* net, const char* name, float* out, long long n);
int rle_set_param(rle_engine* e, const char* net, const char* name, const float* in, long long n);
/* Optimizer state: which = 0 (m) / 1 (v) of the param's Adam; step counter per optimizer. */
int rle_get_adam(rle_engine* e, const char* net, const char* name, int which, float* out, long long n);
int rle_set_adam(rle_engine* e, const char* net, const char* name, int which, const float* in,
                 long long n);
/* The same state in ONE device pass.  The per-tensor entries above make a host round trip per tensor (a TD7
 * agent has 84 parameter and 72 moment tensors); these move every selected tensor with one launch of a pack
 * kernel and one copy through a pinned image.  `what`: a mask of RLE_STATE_*.  The packed state is the
 * concatenation of the logical row-major tensors (the arrays rle_get_param / rle_get_adam return), in the
 * order of rle_state_toc: arenas in mask-bit order (params, m, v); within one, nets in the engine's order,
 * layers in order, weight before bias, and for SAC "tmp" / "log_alpha" last.  The Adam arenas list only the
 * nets that have an optimiser (policy, q1, q2, TD7's encoder; SAC's tmp). */
#define RLE_STATE_PARAMS 1
#define RLE_STATE_ADAM_M 2
#define RLE_STATE_ADAM_V 4
#define RLE_STATE_ALL 7
typedef struct rle_state_entry {
  char net[32];         /* "policy", "target_q1", ..., "tmp" */
  char name[32];        /* "q01.weight", "mlp.2.bias", "log_alpha" */
  int arena;            /* 0 params, 1 Adam m, 2 Adam v */
  int reserved;
  long long offset;     /* floats from the start of the packed state */
  long long numel;
} rle_state_entry;
/* Table of contents of the packed state of `what`: up to cap records into entries (may be NULL with cap 0),
 * *n = the number of tensors.  Entry i + 1 starts where entry i ends; the last one ends at the state's size
 * in floats.  No GPU call. */
int rle_state_toc(rle_engine* e, int what, rle_state_entry* entries, int cap, int* n);
/* Packed state -> out [n_floats] / in [n_floats] -> the engine.  n_floats must be the size rle_state_toc
 * reports (RLE_EINVAL otherwise, as for an empty or unknown mask).  Export: waits for enqueued steps, one pack
 * launch, one copy, one sync.  Import: the reverse; parameters are written as both GEMM images, every padded
 * row and column as zero, and the engine's derived state is invalidated as rle_set_param does. */
int rle_state_export(rle_engine* e, int what, float* out, long long n_floats);
int rle_state_import(rle_engine* e, int what, const float* in, long long n_floats);
/* Agent.load_state_dict(agent) (td7.py:114-125, td3.py:94-100, sac.py:101-107) on the device(s): every
 * network's parameters of src into dst -- not the Adam moments, counters, value bounds, RNG position or SAC
 * log_alpha.  Same algorithm and identical layer shapes required (RLE_EINVAL); batch size and plan may differ,
 * and the two may live on different GPUs (a peer copy).  No host round trip. */
int rle_copy_nets(rle_engine* dst, rle_engine* src);
/* Device counters: [0] critic Adam t, [1] policy Adam t, [2] encoder Adam t, [3] n_runs,
 * [4] rng step, [5] SAC temperature Adam t. */
int rle_get_counters(rle_engine* e, long long* out6);
int rle_set_counters(rle_engine* e, const long long* in6);
// Philox counter of the act path's exploration draws (rle_act_sample mode 1): carried across
// engine rebuilds and pickling so a rebuilt agent does not repeat earlier draws (the reference's
// torch.randn stream, td7.py:153, never restarts either).
int rle_get_act_counter(rle_engine* e, unsigned long long* out);
int rle_set_act_counter(rle_engine* e, unsigned long long v);
/* TD7 value clipping state [value_max, value_min, value_target_max, value_target_min]. */
int rle_get_value_bounds(rle_engine* e, float* out4);
int rle_set_value_bounds(rle_engine* e, const float* in4);

/* n_steps x Agent.train_ops(replay.sample(B), replay) (run_train_ops, run.py:87-96), fully on
 * device incl. sampling and LAP priority update.  info_out: [n_steps][RLE_INFO_MAX] (per-agent
 * key order; NaN = None).  One host sync per call. */
int rle_step(rle_engine* e, int n_steps, float* info_out);
/* Benchmark form of rle_step: n_steps without info readback; *gpu_ms = the engine's elapsed time.
 * Under the default direct AQL dispatch (rle_plan.dispatch 1; the levels go to the engine's own HSA
 * queue, opened at its first step) that is HOST WALL time from the first doorbell to the last
 * packet's completion signal; with dispatch 0 / 2 (hipGraph replays / launches on the stream) it is
 * HIP event time on the engine's stream.  The host thread sleeps while the expected remainder of the burst exceeds 150 us
 * and spins only for the tail (rle_aql_wait_plan); a burst that does not complete within 60 s closes
 * the engine's queue (every later step fails).  Syncs once at the end. */
int rle_step_timed(rle_engine* e, int n_steps, float* gpu_ms);
/* Enqueue n_steps as rle_step does, without any host sync or info readback (the device info
 * ring keeps the last rows); rle_synchronize waits.  Lets one host thread drive several
 * independent seeds (engines, each on its own stream) on one GPU concurrently -- SURVEY
 * §8(f) rank 4, beyond the reference's one agent per process (scripts/td7_exp.sh:1-4). */
int rle_step_async(rle_engine* e, int n_steps);
/* Parity / explicit-batch mode: replace draws of the next n_steps with tapes; each tape
 * is optional and a NULL one keeps its Philox stream.  u [n][B] (torch.rand in sample),
 * eps [n][B][A] (randn_like target noise, or SAC next-state rsample noise), eps_pi [n][B][A]
 * (SAC policy rsample noise; SAC takes eps and eps_pi together), ind [n][B] (explicit
 * indices, e.g. the batch a replay's sample() drew; overrides u).  At least one of u / ind.
 * Pass n_steps = 0 to return to Philox; stepping past the tape's end is an error.
 * Critic dropout's masks (rle_set_critic_dropout) are never taped: they come from their own Philox stream whatever
 * the tapes hold, and rle_dropout_mask reads that stream out for a host reference. */
int rle_set_tapes(rle_engine* e, int n_steps, const float* u, const float* eps, const float* eps_pi,
                  const long long* ind);
/* Last sampled indices (LAPReplayMemory.ind) [B]. */
int rle_last_indices(rle_engine* e, long long* ind_out);
/* Agent.sample / _inference_action forward (td7.py:158-162, td3.py:131-135, sac.py:154-159):
 * obs [n][S] (n <= 1024) -> out [n][W]: TD7 tanh actor output (W = A); TD3 actor MLP output
 * before tanh (W = A); SAC raw (mean | log_std) head (W = 2A).  Raw network outputs (evaluation and
 * diagnostics); rle_act_sample returns the environment action. */
int rle_act(rle_engine* e, const float* obs, int n, float* out);
/* Agent.sample (td7.py:141-156, td3.py:114-129, sac.py:132-152) as ONE device program: the B = n
 * actor (TD7: + fixed encoder) forward, exploration noise, clip and the action map, written by the
 * last kernel straight into pinned host memory.  obs [n][S] -> out [n][A] environment actions:
 *   TD7 / TD3: clip(tanh(pi(s)) + exploration_noise * eps, -1, 1) * scale + bias
 *   SAC:       tanh(mean + exp(clamp(log_std)) * eps) * scale + bias
 * mode 0: deterministic (eps = 0); 1: eps from the engine's own Philox stream (counter advanced
 * per call; the reference draws torch.randn_like from torch's global generator instead);
 * 2: eps given as eps [n][A] (parity tape).  Syncs. */
int rle_act_sample(rle_engine* e, const float* obs, int n, int mode, const float* eps, float* out);
/* The environment action map of rle_act_sample: scale [A], bias [A] (get_action_bias_scale,
 * rl/utils/miscellaneous.py:59-66) and TD7 / TD3 exploration_noise (td7.py:41, td3.py:40).
 * Default: identity, 0.1. */
int rle_set_action_map(rle_engine* e, const float* scale, const float* bias, float exploration_noise);
/* Forward diagnostics on a given batch (host rows s [n][S], a [n][A], n <= 1024), for parity
 * checks of the nets the step trains:
 *   RLE_EVAL_Q:   critic `net`'s estimate_q_value -> out [n].  TD7 (SALECritic, sale.py:106-121)
 *                 on zs = encode_state(s), zsa = encode_state_action(zs, a) of encoder `enc`
 *                 (online critics use "fixed_encoder", target critics "fixed_encoder_target",
 *                 td7.py:175-230); TD3/SAC (MLPCritic, mlp.py:98-101) ignore `enc`.
 *   RLE_EVAL_ZS:  encoder `net`'s encode_state(s) (sale.py:41-46) -> out [n][zs_dim] (a unused).
 *   RLE_EVAL_ZSA: encoder `net`'s encode_state_action(encode_state(s), a) (sale.py:48-55)
 *                 -> out [n][zs_dim].
 * Runs on the engine's stream after any enqueued step; syncs. */
#define RLE_EVAL_Q 0
#define RLE_EVAL_ZS 1
#define RLE_EVAL_ZSA 2
int rle_eval(rle_engine* e, int what, const char* net, const char* enc, const float* s, const float* a, int n,
             float* out);
/* SAC._rsample (sac.py:164-172) on given distribution parameters through the step's own
 * squashed-Gaussian op: log_std clamped to [min_log_std, max_log_std] (sac.py:154-159),
 * u = mean + eps * exp(log_std), action = tanh(u), log_pi [n] (annotation.py:12 EPS). */
int rle_sac_rsample(rle_engine* e, const float* mean, const float* log_std, const float* eps, int n, float* action,
                    float* log_pi);
/* Info rows [n][RLE_INFO_MAX] of the last rle_step / rle_step_async call (its first n steps;
 * n <= 4096).  Syncs the engine stream. */
int rle_get_info(rle_engine* e, int n, float* out);
/* rle_level dispatches enqueued so far by rle_step* (every step graph replay: single-step,
 * multi-step, batch prime, hard update, fold refresh); differences over a timed burst give
 * the exact launches per gradient step (roofline accounting).  Engine-side, no sync. */
int rle_launch_count(rle_engine* e, long long* n);
/* Launches per gradient step of each captured graph kind (for roofline accounting). */
int rle_graph_stats(rle_engine* e, int* levels_policy_step, int* levels_plain_step);
/* Human-readable description of a captured graph (which: 0 policy step, 1 plain step,
 * 2 hard update): one line per level with workgroups and ops.  Writes at most len bytes. */
int rle_graph_describe(rle_engine* e, int which, char* buf, int len);
/* Diagnostics: phase timestamps of the last replay of a captured graph (graphs are
 * traced only when RLE_TRACE=1 is set in the environment before the first step).
 * out[4*w .. 4*w+3] = s_memrealtime (100 MHz) at entry, main-loop start, main-loop
 * end (GEMM ops) and exit of workgroup w, levels concatenated in order; *n_out = number
 * of workgroups written (0 when tracing is off). */
int rle_graph_trace(rle_engine* e, int which, unsigned long long* out, long long cap, long long* n_out);
/* Timestamps per workgroup in rle_graph_trace rows: 4, or 16 in diagnostics builds
 * (-DRLE_TRACE_FINE: slots 4.. are finer in-op stamps). */
int rle_trace_stride(void);
/* The AQL wait policy of rle_step / rle_step_timed (no GPU): given the expected duration of what is
 * outstanding and the time waited so far, returns 0 spin on the completion signal, 1 sleep *sleep_us
 * then check again, 2 time out (the engine's queue is then closed). */
int rle_aql_wait_plan(double expected_us, double elapsed_us, double timeout_s, double* sleep_us);
/* Self-test of the AQL queue's failure handling (no GPU, no HSA call): a queue closed by a timed-out
 * burst refuses new bursts and completes at once, also for other engines sharing its hardware queue,
 * and no doorbell publishes a run of packets that straddles the ring's end.  0 when every check holds. */
int rle_aql_selftest(void);
/* The launch planner alone (no GPU, no HIP or HSA call): the rle_level dispatches of one level of nops ops
 * -- op q of kind[q], GEMM variant vid[q] (read for GEMM ops only), first workgroup wg_begin[q]; nwg workgroups
 * in all -- whose op table lies at device address d_ops, followed by a level of next_nops ops at next_ops
 * (the addresses are copied, never read).  *n: the dispatches, of which at most cap are written to out, 22
 * dwords each: rle_level's 20-dword argument segment (12 op-table entries; the ops, trace and next-ops
 * addresses, 2 dwords each; the lines to prefetch; 1 pad), the workgroup count and the kernel instance ks.
 * *op_bytes: the size of one op descriptor.  A dispatch over the workgroup bound: RLE_EHIP and *n = 0. */
int rle_level_plan(const int* kind, const int* vid, const int* wg_begin, int nops, int nwg, unsigned long long d_ops,
                   unsigned long long next_ops, int next_nops, int ks, unsigned* out, int cap, int* n, int* op_bytes);
/* The level scheduler alone (no GPU, no HIP or HSA call, diagnostic switches off) on a made-up program of nitems
 * items holding nops ops, in program order.  Op q belongs to item item[q] (item[0] = 0; item[q] is item[q-1] or
 * item[q-1] + 1, so the ops of an item are consecutive and every item has at least one), is of kind kind[q]
 * (ops.h OpKind: GEMM 1, sampler gather 4, loss head 5, step end 9, ...), takes wg_count[q] workgroups, and
 * carries attr[4q .. 4q+3], the only other fields the scheduler's weights read: for a GEMM {R, tn, epi,
 * has_pre} (weight R * tn / 1024, + adam_w when epi is 1, the Adam epilogue, + pl_w when has_pre >= 3); for
 * the sampler gather {lap, 0, 0, 0} (lap_w, or uni_w when 0); for the step end {mode, 0, 0, 0} (tiny_w, or 8
 * when tiny_w is 0, unless mode is 1); ignored for every other kind (the loss head weighs head_w, the rest 8).
 * Item i reads resources rd[rd_off[i] .. rd_off[i+1] - 1] and writes wr[wr_off[i] .. wr_off[i+1] - 1]
 * (rd_off, wr_off: nitems + 1 non-decreasing offsets from 0; a negative resource id orders nothing).
 * Of *plan only balance, tiny_w, uni_w, tiny_wg, pl_w, lap_w, head_w, adam_w and lpt are read, as resolved
 * values (-1 is an error here, not "default").  wg_cap > 0: workgroups a level may hold before a further
 * item is deferred (1 << 30: none).  Out, per op q: level[q], its dependency level; pos[q], its place in that
 * level's launch order; wg_begin[q], the level's workgroups before it. */
int rle_schedule_plan(const int* item, const int* kind, const int* wg_count, const int* attr, int nops, const int* rd_off,
                      const int* rd, const int* wr_off, const int* wr, int nitems, const rle_plan* plan, int wg_cap,
                      int* level, int* pos, int* wg_begin);
/* The conflict sweep of the RLE_HAZARD=1 level check alone (no GPU): n byte ranges [lo[k], hi[k]) (lo < hi), in
 * any order, that op op[k] (0 <= op[k] < nops) reads or, write[k] != 0, stores; item[j]: the program item of op
 * j.  Two ranges conflict when they share a byte, at least one of them is stored, and they belong to different
 * ops of different items.  Returns 0 and *op_a = *op_b = -1 when none do; else 1 with the first conflict met
 * when the ranges are swept by ascending lo: *op_b the op of the range the sweep stands at, *op_a that of the
 * range begun before it that still covers its first byte.  Negative: an RLE_* error. */
int rle_hazard_scan(const unsigned long long* lo, const unsigned long long* hi, const int* write, const int* op, int n,
                    const int* item, int nops, int* op_a, int* op_b);
/* Copy all weights/optimizer state/counters of src into dst (checkpoint agent,
 * ckpt_agent.load_state_dict(agent), run_w_checkpoint.py:140), and the act path's exploration counter
 * (rle_get_act_counter).  Same algorithm and identical layer shapes required; the batch size may differ. */
int rle_copy_state(rle_engine* dst, rle_engine* src);
int rle_synchronize(rle_engine* e);

const char* rle_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RLE_H */
