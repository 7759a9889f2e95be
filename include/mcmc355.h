/*
 * mcmc355.h — C-ABI of libmcmc355.so, the MI355X (gfx950) HMC / NUTS engine.
 *
 * This is the drop-in boundary for the reference's sampling hot path
 * (korentomas/mlx-mcmc):
 *
 *   reference symbol                                   replaced by
 *   -------------------------------------------------  ------------------------------
 *   mlx_mcmc/kernels/hmc.py:7-206   hmc()              mc_hmc_run (+ mc_state_init)
 *   mlx_mcmc/kernels/hmc.py:53-67   grad_log_prob      mc_logp_grad (tape evaluator)
 *   mlx_mcmc/kernels/hmc.py:69-100  leapfrog_step      (fused inside mc_hmc_run)
 *   mlx_mcmc/kernels/hmc.py:102-111 hamiltonian        (fused inside mc_hmc_run)
 *   mlx_mcmc/kernels/hmc.py:113-153 hmc_step           (fused inside mc_hmc_run)
 *   mlx_mcmc/kernels/nuts.py:16-358 nuts()             mc_nuts_run (+ mc_state_init)
 *   mlx_mcmc/kernels/metropolis.py:6-101               mc_mh_run (+ mc_state_init)
 *     metropolis_hastings()
 *   mlx_mcmc/kernels/nuts.py:137-218 build_tree        (iterative, inside mc_nuts_run)
 *   mlx_mcmc/kernels/nuts.py:119-135 no_u_turn         (inside mc_nuts_run)
 *   mlx_mcmc/distributions/normal.py:33-56 log_prob    MC_DIST_NORMAL term / mc_dist_log_prob
 *   mlx_mcmc/distributions/halfnormal.py:34-63         MC_DIST_HALFNORMAL term / mc_dist_log_prob
 *   mlx_mcmc/distributions/exponential.py:48-71        MC_DIST_EXPONENTIAL term / mc_dist_log_prob
 *   mlx_mcmc/distributions/gamma.py:40-88              MC_DIST_GAMMA term / mc_dist_log_prob
 *   mlx_mcmc/distributions/beta.py:37-91               MC_DIST_BETA term / mc_dist_log_prob
 *   mlx.core.random (key/split/normal/uniform)         Philox4x32-10 counter RNG, mc_rng_fill
 *   examples/06_nuts_comparison.py:22-41 compute_ess   mc_series_stats (MC_ST_ESS)
 *   README.md:214 roadmap "R-hat" (no reference code)  mc_stats_reduce + mc_rhat; rank-normalised:
 *                                                      mc_rank_diag, mc_geyer_ess_host
 *   mlx_mcmc/inference/mcmc.py:191-227 summary         mc_pool_moments, mc_select
 *   README.md roadmap "Model comparison (WAIC, LOO)"   mc_pointwise_stats (no reference code)
 *   README.md:216 roadmap "Posterior predictive checks" mc_predictive, mc_predictive_draw
 *   README.md roadmap "Model comparison (WAIC, LOO)"   mc_psis_loo, mc_psis_fit_host (no reference code)
 *     (no reference code; Distribution.sample stays the host sampler)
 *
 * The reference is pure Python on MLX and has no FFI of its own; the
 * Python host layer of this repository (mlx_mcmc_amd/_lib.py) binds these
 * symbols with ctypes — see INTEGRATION.md for the binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - All array arguments named *_dev are device pointers (HIP, current
 *     device); the caller owns them.  The library owns only mc_program.
 *   - Every entry point returns 0 on success or a negative MC_ERR_* code;
 *     nothing throws or aborts across the ABI.  mc_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - Launch functions are asynchronous on the given stream and never
 *     allocate, free or synchronise (they are graph-capturable).
 *   - Parameters are one flat float32 vector of length n_params (the
 *     concatenation of the user's parameter dict in insertion order).
 */
#ifndef MCMC355_H
#define MCMC355_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 2: mc_operand.transform (formerly `reserved`) and mc_term.affine are
 * read and validated (an unknown transform, or a transform on a non-parameter
 * operand, is MC_ERR_INVALID): callers written against ABI 1 must zero them. */
#define MC_ABI_VERSION 2

/* ---- error codes -------------------------------------------------------- */
#define MC_OK              0
#define MC_ERR_INVALID    -1   /* bad argument / malformed program           */
#define MC_ERR_UNSUPPORTED -2  /* well-formed but outside what the kernels do */
#define MC_ERR_HIP        -3   /* HIP runtime error                          */
#define MC_ERR_NOMEM      -4   /* device allocation failed                   */
#define MC_ERR_TIMEOUT    -5   /* a sliced launch's cross-workgroup exchange  */
                               /* did not complete (see mc_workspace_status)  */

/* ---- the tape: a log density as a sum of fused distribution terms ------- */
/* A term is  weight * sum_i dist(loc_i, scale_i).log_prob(value_i)  over n
 * broadcast elements.  This is exactly the shape every reference model takes
 * (e.g. tests/test_hmc.py:187-198, examples/02_hmc_comparison.py:40-52).   */
/* Operand slots of a term: value, then (loc | alpha), then (scale | rate |
 * beta).  The gammaln normalisers of Gamma and Beta are evaluated at the
 * current shape values but carry no gradient, exactly as the reference's
 * host-side scipy gammaln (gamma.py:48-59, beta.py:45-57).                   */
typedef enum {
    MC_DIST_NORMAL      = 0,  /* normal.py:33-56       (value, loc, scale)   */
    MC_DIST_HALFNORMAL  = 1,  /* halfnormal.py:34-63   (value, -, scale)     */
    MC_DIST_EXPONENTIAL = 2,  /* exponential.py:48-71  (value, -, rate)      */
    MC_DIST_GAMMA       = 3,  /* gamma.py:40-88        (value, alpha, beta)  */
    MC_DIST_BETA        = 4,  /* beta.py:37-91         (value, alpha, beta)  */
    MC_DIST_IDENTITY    = 5,  /* weight * sum_i value_i   (value, -, -):  a   */
                              /* parameter expression added to the log      */
                              /* density (the Jacobian of a reparameterised */
                              /* parameter, `lp + log_sigma`)               */
    MC_DIST_EXPR        = 6   /* weight * sum_i root_i of an elementwise     */
                              /* expression (mc_expr, mc_program_create_expr) */
} mc_dist_kind;

typedef enum {
    MC_OP_NONE    = 0,  /* operand unused (HalfNormal loc)                   */
    MC_OP_CONST   = 1,  /* broadcast float constant `value`                  */
    MC_OP_PSCALAR = 2,  /* broadcast parameter q[param_offset]               */
    MC_OP_DATA    = 3,  /* data[pool_offset + i]        (float32 data pool)  */
    MC_OP_PVEC    = 4,  /* q[param_offset + i]                               */
    MC_OP_GATHER  = 5   /* q[param_offset + index[pool_offset + i]] (int32)  */
} mc_operand_kind;

/* An elementwise transform of a parameter operand (PSCALAR / PVEC / GATHER),
 * applied in f32 before the term reads it, its derivative applied to the
 * operand's cotangent as mx.grad's VJPs do (exp: c * exp(x); log: c / x):
 * `Normal(mu, mx.exp(log_sigma))`, `Normal(0, 1).log_prob(mx.log(x))`.      */
typedef enum {
    MC_XF_NONE = 0,
    MC_XF_EXP  = 1,
    MC_XF_LOG  = 2
} mc_transform_kind;

typedef struct mc_operand {
    int32_t kind;          /* mc_operand_kind                               */
    int32_t param_offset;  /* PSCALAR / PVEC / GATHER                       */
    int64_t pool_offset;   /* DATA: float pool; GATHER: index pool          */
    float   value;         /* CONST                                         */
    int32_t transform;     /* mc_transform_kind (parameter operands only;   */
                           /* was `reserved`: zero-initialised callers get  */
                           /* MC_XF_NONE)                                   */
} mc_operand;

typedef struct mc_term {
    int32_t    dist;       /* mc_dist_kind                                  */
    int32_t    affine;     /* 0, or k + 1: the loc is affine, affines[k]    */
    int64_t    n;          /* broadcast length (>= 1)                       */
    float      weight;     /* multiplies the term (1.0 for `lp += term`)    */
    float      reserved1;
    mc_operand value, loc, scale;
} mc_term;

/* An affine loc (the reference differentiates any MLX expression of the
 * parameters, hmc.py:53-67; these are the linear-predictor forms):
 *     loc_i = loc_i + slope_i * x_i      (f32: one product, then one sum)
 * for a Normal term whose `affine` field is k + 1 (affines[k]).  slope is
 * CONST or PSCALAR; x is DATA, PVEC or a GATHER; the term's own loc operand is
 * CONST, PSCALAR, DATA, PVEC or a GATHER.  A non-injective gather may only
 * be the loc itself with a DATA x (alpha[group] + beta * x: the segmented
 * tape); x's parameter range must not overlap another accumulating operand
 * of the term (MC_ERR_UNSUPPORTED otherwise).  Examples: a + b * x (linear
 * regression), mu + tau * z (non-centred hierarchy), alpha[g] + beta * x
 * (varying intercepts).  Affine programs run on the chain-per-workgroup
 * kernels (k_hmc, k_nuts, k_mh).                                            */
typedef struct mc_affine {
    mc_operand slope, x;
} mc_affine;

/* Expression terms (MC_DIST_EXPR).  The reference differentiates ANY MLX
 * expression of the parameters (hmc.py:53-67 mx.grad over the user's
 * log_prob, nuts.py:76-87); the fused terms above cover the distribution
 * shapes, and an expression term covers everything else that is elementwise:
 *     weight * sum_i root_i
 * where the term's nodes form a DAG evaluated per broadcast element i in f32
 * (MLX's elementwise ops, each rounded once) and differentiated in reverse
 * mode with the VJPs mx.grad uses.  Node k's arguments are nodes of the same
 * term with smaller indices (a, b, c; -1 = unused); the last node is the
 * root.  Leaves are mc_operands: CONST, PSCALAR, DATA, PVEC or GATHER
 * (transform MC_XF_NONE — mx.exp / mx.log are nodes here).  Vector leaves
 * have the term's length n.  Every non-injective GATHER leaf of a term must
 * use the same index values (e.g. alpha[g] + beta[g] * x): the term is then
 * evaluated per group run (segmented, deterministic); anything else is
 * strided.  A term holds at most MC_EXPR_MAX_NODES nodes.                 */
#define MC_EXPR_MAX_NODES 32
typedef enum {
    MC_EX_LEAF    = 0,   /* the node's operand                               */
    MC_EX_ADD     = 1,   /* a + b                                            */
    MC_EX_SUB     = 2,   /* a - b                                            */
    MC_EX_MUL     = 3,   /* a * b                                            */
    MC_EX_DIV     = 4,   /* a / b                                            */
    MC_EX_NEG     = 5,   /* -a                                               */
    MC_EX_EXP     = 6,   /* exp a                                            */
    MC_EX_LOG     = 7,   /* log a                                            */
    MC_EX_SQRT    = 8,   /* sqrt a                                           */
    MC_EX_SQUARE  = 9,   /* a * a                                            */
    MC_EX_POW     = 10,  /* a ** b                                           */
    MC_EX_ABS     = 11,  /* |a|                                              */
    MC_EX_LOG1P   = 12,  /* log(1 + a)                                       */
    MC_EX_TANH    = 13,  /* tanh a                                           */
    MC_EX_SIGMOID = 14,  /* 1 / (1 + exp(-a))                                */
    MC_EX_NORMAL_LP      = 15,  /* Normal(b, c).log_prob(a)  normal.py:49-56 */
    MC_EX_HALFNORMAL_LP  = 16,  /* HalfNormal(c).log_prob(a) halfnormal.py:43-63 */
    MC_EX_EXPONENTIAL_LP = 17,  /* Exponential(c).log_prob(a) exponential.py:48-71 */
    MC_EX_WHERE   = 18,  /* a != 0 ? b : c, a a CONST / DATA leaf or a       */
                         /* comparison node (mx.where over a data mask or a  */
                         /* traced condition; no cotangent through a)        */
    MC_EX_GAMMA_LP = 19, /* Gamma(b, c).log_prob(a)  gamma.py:48-88: gammaln */
                         /* (b) at the current value, no cotangent through it */
    MC_EX_BETA_LP  = 20, /* Beta(b, c).log_prob(a)   beta.py:45-91: log B(b, */
                         /* c) at the current values, no cotangent through it */
    MC_EX_GT       = 21, /* a > b  as 1 / 0 (mx.greater: a mask, no cotangent) */
    MC_EX_GE       = 22, /* a >= b                                           */
    MC_EX_LT       = 23, /* a < b                                            */
    MC_EX_LE       = 24, /* a <= b                                           */
    /* Log masses of count data (no reference code: its distributions are
     * continuous).  y (and n) are CONST or DATA leaves — MC_ERR_UNSUPPORTED
     * otherwise — and take no cotangent; the normalisers log C(n, y) and
     * -lgamma(y + 1) are constants of the data and are NOT part of the node
     * (the caller adds them as a leaf).  With
     *   softplus(x) = max(x, 0) + log1p(exp(-|x|)),  sigma(x) = 1 / (1 + exp(-x))
     * in f32, one rounding per operation:                                    */
    MC_EX_BERNOULLI_LOGIT_LP = 25, /* a = y in {0, 1}, b = eta:               */
                         /* -softplus(y != 0 ? -eta : eta); d eta = y - sigma */
    MC_EX_BINOMIAL_LOGIT_LP = 26,  /* a = y, b = n, c = eta; n >= 0,          */
                         /* 0 <= y <= n, both integer-valued:                 */
                         /* y eta - n softplus(eta); d eta = y - n sigma(eta) */
    MC_EX_POISSON_LOG_LP = 27,     /* a = y >= 0 integer-valued, b = theta:   */
                         /* e = exp(theta); y == 0 ? -e : y theta - e;        */
                         /* d theta = y - e                                   */
    /* Outside the support: -inf, no cotangent.  A NaN eta / theta gives NaN;
     * infinite ones follow the formulas (IEEE).  Bernoulli: the certain
     * outcome -0, the impossible one -inf.  Binomial: eta = +inf NaN;
     * eta = -inf gives -inf for y > 0 and NaN for y = 0.  Poisson:
     * theta = -inf gives -0 for y = 0 and -inf for y > 0; theta = +inf gives
     * -inf for y = 0 and NaN for y > 0.                                      */
    /* The two nodes of a K-class (Categorical) log mass: a log-sum-exp that
     * chains over the K class logits, and a selection by the observed label
     * that chains over the K classes (mlx_mcmc/distributions/categorical.py:
     * log(p / sum p)[y], -inf for an invalid index).  Code 28 is not
     * assigned: it stays an unknown op (MC_ERR_INVALID), as callers written
     * against the count nodes were promised.                                 */
    MC_EX_LOGADDEXP = 29, /* log(exp a + exp b) (mx.logaddexp), f32, one       */
                         /* rounding per operation, with d = (a == b ? 0 :    */
                         /* a - b):  max(a, b) + log1p(exp(-|d|));            */
                         /* da = c sigma(d), sigma(d) = 1 / (1 + exp(-d)), and */
                         /* db = c - da: the class cotangents of a chained    */
                         /* softmax sum to c.  a == b (equal infinities       */
                         /* included): a + log 2, c / 2 to each argument.  One */
                         /* argument -inf: the other argument, which takes    */
                         /* all of c; +inf beside anything smaller: +inf,     */
                         /* likewise.  A NaN argument gives NaN (value and    */
                         /* both cotangents).                                 */
    MC_EX_PICK     = 30, /* a == k ? b : c.  a = y is the label, a CONST or   */
                         /* DATA leaf (MC_ERR_UNSUPPORTED otherwise); the     */
                         /* class k is the node's own constant, leaf.value    */
                         /* (PICK and the Student-t nodes are the non-leaf    */
                         /* nodes that read their leaf field).  Nothing flows */
                         /* to a; the cotangent goes to the branch taken.  A  */
                         /* NaN y takes c.                                    */
    /* Student-t log densities (no reference code), WITHOUT the normaliser
     * lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2 (+ log 2 for the
     * half form), which the caller adds as a CONST leaf.  The degrees of
     * freedom nu are the node's own constant, leaf.value, finite and positive
     * (MC_ERR_INVALID otherwise); a, b, c may be any nodes.  Code 31 is not
     * assigned and stays an unknown op.  In f32, one rounding per operation:
     *   d = v - m (half: d = v); z = d / s; q = z z; w = q / nu
     *   lp = (-log s) - (nu + 1) / 2 * log1p(w)
     *   r = z / (nu + q); g = (nu + 1) r; t = g / s
     *   dv = -c t, dm = c t, ds = c (g z - 1) / s                            */
    MC_EX_STUDENT_T_LP = 32,       /* a = value v, b = loc m, c = scale s     */
    MC_EX_HALF_STUDENT_T_LP = 33   /* a = v, c = s (b unused, -1): -inf and   */
                         /* no cotangent unless v >= 0 (a NaN v: -inf)        */
    /* Edge classes.  q = inf (|z| beyond ~1.8e19, an infinite v or m, s = 0
     * beside d != 0): lp = -inf (NaN for s = 0) and every cotangent 0.  A NaN
     * v, m or s: NaN in the value and the cotangents.  s < 0: NaN; s = inf:
     * -inf; s = 0 with d = 0: NaN — as MC_EX_NORMAL_LP.  Half form: v = -0 is
     * inside the support.  Cauchy and half-Cauchy are nu = 1.                */
    /* The log mass of label y under class logits eta_0 .. eta_{K-1} is
     *   SUB( PICK_{K-1}(y, eta_{K-1}, ... PICK_0(y, eta_0, -inf)),
     *        LOGADDEXP(... LOGADDEXP(eta_0, eta_1) ..., eta_{K-1}) )
     * with one label leaf.  A label outside 0 .. K-1, or not an integer,
     * falls through every PICK to the -inf constant: the log mass is -inf, as
     * the reference's for an invalid index, while the log-sum side still
     * carries its finite cotangent (-softmax) to the logits.                 */
} mc_expr_op;

/* The count distributions of mc_discrete_log_prob / mc_predictive_draw_discrete. */
typedef enum {
    MC_DISCRETE_BERNOULLI = 0,   /* Bernoulli(logit eta)                      */
    MC_DISCRETE_BINOMIAL  = 1,   /* Binomial(total, logit eta)                */
    MC_DISCRETE_POISSON   = 2    /* Poisson(log rate eta)                     */
} mc_discrete_kind;

typedef struct mc_expr_node {
    int32_t    op;         /* mc_expr_op                                    */
    int32_t    a, b, c;    /* argument nodes (index within the term), or -1 */
    mc_operand leaf;       /* MC_EX_LEAF                                    */
} mc_expr_node;

/* The nodes of one expression term: nodes[first .. first + count). */
typedef struct mc_expr {
    int32_t first, count;
} mc_expr;

typedef struct mc_program mc_program;

/* Build a program.  data / index are HOST arrays; the library copies them to
 * the device (and, for terms that gather through an unsorted index, stores a
 * permuted copy so that every term is processed in index order — this is what
 * makes the gather gradient a deterministic segmented sum).  Validates every
 * operand range.  lp_const is added to the total log density.              */
int mc_program_create(const mc_term* terms, int32_t n_terms, int32_t n_params,
                      float lp_const,
                      const float* data, int64_t n_data,
                      const int32_t* index, int64_t n_index,
                      mc_program** out);
/* mc_program_create ignores mc_term.affine (formerly reserved0); only
 * mc_program_create_affine reads it, so zero-initialise it there.          */
/* mc_program_create with affine loc operands (affines[0 .. n_affines)).    */
int mc_program_create_affine(const mc_term* terms, int32_t n_terms,
                             const mc_affine* affines, int32_t n_affines,
                             int32_t n_params, float lp_const,
                             const float* data, int64_t n_data,
                             const int32_t* index, int64_t n_index,
                             mc_program** out);
/* mc_program_create_affine with expression terms: a term whose dist is
 * MC_DIST_EXPR names exprs[k] through its `affine` field (k + 1) and leaves
 * value / loc / scale MC_OP_NONE.  Expression programs run on the
 * chain-per-workgroup kernels (k_hmc, k_nuts, k_mh, mc_logp_grad); the
 * sliced planners decline them.                                           */
int mc_program_create_expr(const mc_term* terms, int32_t n_terms,
                           const mc_affine* affines, int32_t n_affines,
                           const mc_expr* exprs, int32_t n_exprs,
                           const mc_expr_node* nodes, int32_t n_nodes,
                           int32_t n_params, float lp_const,
                           const float* data, int64_t n_data,
                           const int32_t* index, int64_t n_index,
                           mc_program** out);
int mc_program_destroy(mc_program* prog);
int32_t mc_program_num_params(const mc_program* prog);
/* The launch geometry the engine picked: waves per chain (1, 4 or 16).     */
int32_t mc_program_waves_per_chain(const mc_program* prog);

/* Sliced layout (HMC only; hmc.py:7-206 with a different work split).  A
 * program whose terms each have at most one per-element parameter operand
 * can be split into S data slices: parameters touched by one slice only
 * become private to it, broadcast parameters are replicated, and one
 * workgroup evaluates one slice for a block of 8 or 16 chains; the slices of
 * a block exchange their log p / broadcast-cotangent / kinetic partials once
 * per leapfrog step.  Results equal the chain-per-workgroup kernel's up to
 * fp32 summation order and do not depend on how chains are split over
 * launches or GPUs.  num_slices: 0 = automatic (the default chosen by
 * mc_program_create: 16 for >= 65536 elements, 8 for >= 16384, 4 for >= 2048
 * when the lane-resident kernel takes the layout, else unsliced — and then
 * planned as ONE slice of the lane-resident kernel when it qualifies),
 * 1 = off (the chain-per-workgroup kernel k_hmc), 2..64 = that many
 * (MC_ERR_UNSUPPORTED if the program does not qualify).  NUTS, MH,
 * mc_logp_grad and mc_state_init always use the chain-per-workgroup kernels. */
int mc_program_set_slices(mc_program* prog, int32_t num_slices);
int32_t mc_program_num_slices(const mc_program* prog);
/* Which kernel runs a sliced HMC program.  kernel: 0 = automatic (the
 * lane-resident kernel when the layout qualifies: <= 16 slices, <= 4
 * broadcast parameters, <= 256 private parameters per slice, every
 * per-element parameter operand private; else the term interpreter),
 * 1 = term interpreter, 2 = lane-resident (MC_ERR_UNSUPPORTED if the layout
 * does not qualify; mc_last_error says why).  mc_program_slice_kernel returns
 * the kernel a launch with L > 0 will use: 0 unsliced, 1 interpreter, 2
 * lane-resident.  Both compute the same sampler; they differ in fp32
 * summation order only.  On an unsliced program, 2 plans it as one slice of
 * the lane-resident kernel (no exchange; an error if it does not qualify), 0
 * does so when it qualifies and 1 keeps k_hmc.  mc_program_set_slices resets
 * the choice's layout.                                                      */
int mc_program_set_slice_kernel(mc_program* prog, int32_t kernel);
int32_t mc_program_slice_kernel(const mc_program* prog);
/* 1 when a lane-resident launch of this program runs the fast-form kernel
 * k_hmc_lf (every slice term a swept N(theta[g], scale) term over data or a
 * direct theta ~ N(loc, scale) term, every scalar term the own prior of a
 * broadcast parameter; MC_LANES_FAST=0 in the environment turns it off),
 * 0 when it runs k_hmc_lr or no lane-resident kernel, -1 on a null program. */
int32_t mc_program_lanes_fast(const mc_program* prog);
/* The lane-resident plan's geometry, for tests and diagnostics: register
 * slots per lane (1, 2 or 4: private parameters per slice / 64, rounded up)
 * and lanes per private parameter (1, or a power of two up to 16 when a
 * slice holds at most 32 of them; MC_LANES_REP caps it), and the widest
 * bundle of private parameters one element of a gathered expression term
 * reads (alpha[g] + beta[g] * x: 2; 0 without such a term).  0 when the
 * program has no lane-resident plan, -1 on a null program.                  */
int32_t mc_program_lane_slots(const mc_program* prog);
int32_t mc_program_lane_rep(const mc_program* prog);
int32_t mc_program_lane_bundle(const mc_program* prog);
/* 1 when HMC launches of the program take the dense route: a fast-form
 * hierarchical program under automatic slicing runs a chain pair per
 * workgroup (k_hmc_lf reads no observation per step, so the pair's slices are
 * the waves of one workgroup exchanging through LDS, or one wave without an
 * exchange), on a plan of its own beside the program's; *slices its slices
 * (waves per chain pair: 1, 4 or 8) and *slots its register slots per lane
 * (either may be NULL).  0 (and zeros) when HMC runs the program-level plan:
 * an explicit slice count, another form, MC_LANES_FAST=0 / MC_LANES_FORM=0.
 * NUTS, MH and the pointwise kernels always run the program-level plan.
 * -1 on a null program.                                                     */
int32_t mc_program_hmc_dense(const mc_program* prog, int32_t* slices, int32_t* slots);
/* Test hook: how the dense HMC route draws its momenta and accept uniforms.
 * 0: HMC launches run the program-level plan; 1: the dense plan has a lane RNG
 * plan (a Philox block per lane); 2: it has none and the workgroup draws every
 * block once, handing the normals out through LDS; 3: none, and every lane
 * draws its own (MC_HMC_DENSE_RNG=0 when the plan was made).  The draws are the
 * same bits in every mode.  -1 on a null program.                              */
int32_t mc_debug_hmc_dense_rng(const mc_program* prog);
/* Chains per workgroup (1 | 2) of a dense HMC launch of `num_chains` chains of
 * the program on the current device.  The 4- and 8-wave dense kernels run one
 * chain per workgroup while the launch has at most as many chains as the
 * device has CUs (a CU per chain; pairs would leave half of them without a
 * wave) and a chain pair above; both give the same bytes.
 * MC_HMC_DENSE_CHAINS=1|2 in the environment when the plan was made fixes it.
 * 0 when HMC launches do not take the dense route or take its one-wave kernel
 * (always a pair per wave); -1 on a null program or without a device.        */
int32_t mc_program_hmc_dense_chains(const mc_program* prog, int64_t num_chains);
/* Test hook: that rule as a pure function of the launch's chains, the device's
 * CU count and the override (`forced`: 1 | 2, or 0 for none).                */
int32_t mc_debug_hmc_dense_chains(int64_t num_chains, int32_t cus, int32_t forced);
/* Why the program's HMC launches do not run the lane-resident kernel (e.g.
 * "lane-resident kernel: more than 4 broadcast parameters"), or "" when they
 * do or no plan was attempted; valid until the next set_slices /
 * set_slice_kernel / destroy.  The chain-per-workgroup and interpreter
 * kernels are 2-4x slower on programs the automatic plan would slice: the
 * Python driver turns a non-empty note on such a program into a warning. */
const char* mc_program_kernel_note(const mc_program* prog);
/* 1 when mc_nuts_run with this max_tree_depth runs the lane-resident NUTS
 * kernel k_nuts_lr (a program planned as one lane-resident slice; its arena
 * fits LDS; MC_NUTS_LANES=0 in the environment turns it off), 2 when it runs
 * its register-only variant (no broadcast parameter, no scalar term, one
 * Normal term with at most one element per parameter and a data or constant
 * scale: the gradient from per-parameter registers), 0 when it runs k_nuts,
 * 3 when it runs the sliced NUTS kernel k_nuts_sl (a program sliced onto the
 * fast-form lane layout of k_hmc_lf: one chain per wave per slice, one record
 * exchange per leaf; max_tree_depth <= 12 and the LDS arenas fit), -1 on a
 * null program.  All take the reference's decisions; they differ in fp32
 * summation order only.                                                     */
int32_t mc_program_nuts_lanes(const mc_program* prog, int32_t max_tree_depth);

/* Batched tape evaluation: for every point p, logp[p] = log density at
 * q[p, :] and grad[p, :] = its gradient (replaces hmc.py:53-67 mx.grad).   */
int mc_logp_grad(const mc_program* prog, int64_t n_points,
                 const float* q_dev, float* logp_dev, float* grad_dev,
                 void* hip_stream);

/* Elementwise Distribution.log_prob (normal.py:33-56, halfnormal.py:34-63,
 * exponential.py:48-71, gamma.py:61-88, beta.py:59-91):
 * out[i] = log_prob(value[i]; loc|alpha[i|0], scale|rate|beta[i|0]).  The
 * middle operand may be NULL for HalfNormal and Exponential.  *_bcast = 1
 * means the operand is a single element.                                    */
int mc_dist_log_prob(int32_t dist, int64_t n,
                     const float* value_dev, int32_t value_bcast,
                     const float* loc_dev, int32_t loc_bcast,
                     const float* scale_dev, int32_t scale_bcast,
                     float* out_dev, void* hip_stream);

/* The count nodes' values elementwise (the device functions of
 * MC_EX_BERNOULLI_LOGIT_LP / MC_EX_BINOMIAL_LOGIT_LP / MC_EX_POISSON_LOG_LP,
 * without the normaliser): out[i] = node(value[i|0], total[i|0], eta[i|0]);
 * kind is an mc_discrete_kind, eta the logit or the log rate; total may be
 * NULL unless kind is MC_DISCRETE_BINOMIAL.  *_bcast = 1: a single element. */
int mc_discrete_log_prob(int32_t kind, int64_t n,
                         const float* value_dev, int32_t value_bcast,
                         const float* total_dev, int32_t total_bcast,
                         const float* eta_dev, int32_t eta_bcast,
                         float* out_dev, void* hip_stream);

/* The Student-t nodes' values elementwise (the device function of
 * MC_EX_STUDENT_T_LP / MC_EX_HALF_STUDENT_T_LP, without the normaliser):
 * out[i] = node(value[i|0], loc[i|0], scale[i|0]) at df, finite and positive;
 * half != 0 is the half form, which reads no loc (loc_dev may be NULL).
 * *_bcast = 1: a single element.                                            */
int mc_student_t_log_prob(float df, int32_t half, int64_t n,
                          const float* value_dev, int32_t value_bcast,
                          const float* loc_dev, int32_t loc_bcast,
                          const float* scale_dev, int32_t scale_bcast,
                          float* out_dev, void* hip_stream);

/* ---- per-chain state ---------------------------------------------------- */
/* State blob layout (device memory, mc_state_bytes(prog, C) bytes):
 *   [mc_chain_scalars x C][pad to 256 B][q: C x D f32][pad][g: C x D f32]
 * mc_state_offsets() returns the byte offsets of q and g.                  */
typedef struct mc_chain_scalars {
    double  step_size;      /* epsilon (Python float in the reference)      */
    double  step_size_bar;  /* NUTS dual averaging epsilon_bar (nuts.py:64) */
    double  h_bar;          /* NUTS dual averaging H_bar (nuts.py:65)       */
    double  alpha_sum;      /* NUTS: sum of per-iteration accept stats      */
    float   mu;             /* NUTS: f32 log(10*eps0) (nuts.py:63)          */
    float   logp;           /* log density at the current position          */
    int32_t n_accept;       /* accepted (HMC) / alpha>0.5 (NUTS) this phase */
    int32_t n_total;        /* iterations in this phase                     */
    int32_t warmup_accept;  /* counters frozen at the warmup->sampling edge */
    int32_t warmup_total;
    int64_t depth_sum;      /* NUTS: sum of tree depths this phase          */
    int64_t warmup_depth_sum;
    int64_t n_grad;         /* gradient evaluations so far                  */
    int32_t n_divergent;    /* NUTS: leaves that failed the DELTA_MAX test  */
    int32_t reserved;
} mc_chain_scalars;

int64_t mc_state_bytes(const mc_program* prog, int64_t num_chains);
int mc_state_offsets(const mc_program* prog, int64_t num_chains,
                     int64_t* q_offset, int64_t* g_offset);
/* Set q = q0, evaluate logp/grad there, step_size = eps0, counters = 0,
 * NUTS dual-averaging state = (mu = f32 log(10 eps0), eps_bar = 1, H_bar = 0)
 * (nuts.py:62-68, hmc.py:157).                                              */
int mc_state_init(const mc_program* prog, int64_t num_chains,
                  const float* q0_dev, double step_size,
                  void* state_dev, void* hip_stream);

/* ---- sampling runs ------------------------------------------------------ */
/* Iterations are numbered globally: [0, num_warmup) is warmup, then
 * [num_warmup, num_warmup + num_samples) is sampling.  A launch runs
 * iterations [iter_begin, iter_begin + iter_count) for every chain, so a run
 * may be split over several launches (progress printing, bench steps).
 * Draws are a pure function of (seed, chain_offset + chain, iteration, ...),
 * so results do not depend on how chains are split over launches or GPUs. */
typedef struct mc_run_config {
    int64_t  num_chains;       /* chains in this launch                      */
    int64_t  chain_offset;     /* global index of chain 0 (RNG stream id)    */
    int64_t  num_warmup;
    int64_t  num_samples;
    int64_t  iter_begin;
    int64_t  iter_count;
    int64_t  sample_begin;     /* samples buffer holds sample indices        */
    int64_t  sample_capacity;  /*   [sample_begin, sample_begin + capacity)  */
    uint64_t seed;
    double   step_size;        /* initial epsilon (NUTS mu uses it)          */
    double   target_accept;
    int32_t  num_leapfrog_steps; /* HMC L                                    */
    int32_t  max_tree_depth;     /* NUTS                                     */
    int32_t  adapt_step_size;
    int32_t  slice_mode;         /* NUTS: 0 = reference f32 exp/log (Q7),    */
                                 /*       1 = exact double log u             */
} mc_run_config;

/* Optional per-(chain, iteration) trace; any pointer may be NULL.
 * Arrays are [num_chains, capacity] for iterations [iter_begin, +capacity). */
typedef struct mc_trace {
    int64_t  iter_begin;
    int64_t  capacity;
    uint8_t* accepted;      /* HMC accept bit; NUTS alpha > 0.5             */
    float*   accept_stat;   /* HMC log-accept ratio; NUTS alpha (nuts.py:287) */
    double*  step_size;     /* epsilon used in the iteration                */
    float*   energy;        /* HMC H_init; NUTS H0                          */
    int32_t* tree_depth;    /* NUTS j; HMC L                                */
    int32_t* n_leapfrog;    /* leapfrog steps (= new gradient evaluations)  */
} mc_trace;

/* HMC (hmc.py:7-206).  samples_dev: [num_chains, sample_capacity, D] f32 or
 * NULL.  workspace: mc_hmc_workspace_bytes() bytes of device memory (may be
 * 0 bytes when the per-chain arena fits in LDS).                            */
int64_t mc_hmc_workspace_bytes(const mc_program* prog, int64_t num_chains);
/* The lane-resident kernel continues its exchange tags across launches on a
 * workspace and clears the workspace only the first time it sees its address
 * (and after another kernel used it or a timeout was reported).  A caller
 * that frees or repurposes a workspace between sliced HMC launches calls
 * mc_workspace_release(ws) first.                                           */
int mc_workspace_release(const void* workspace_dev);

/* Test hook for the exchange kernels' timeout path (no reference counterpart):
 * while on != 0, the last workgroup of every sliced HMC launch exits without
 * publishing, so the other slices of its chain block time out;
 * mc_workspace_status then reports MC_ERR_TIMEOUT and the next launch on the
 * workspace starts clean.  The state of a timed-out chain block is undefined
 * in general and the caller re-initialises those chains: the HMC and MH
 * kernels write a chain's state only at launch exit (a stranded block keeps
 * the state the launch found), but sliced NUTS writes an accepted draw's
 * private parameters when its tree level completes, and its shared
 * parameters, log density and scalars at exit (csrc/nuts_sliced.h).  The
 * hook faults before the first leaf, where every kernel keeps the state.  */
int mc_debug_exchange_fault(int on);
/* Test hook: 0 runs the fast-form kernel k_hmc_lf with the term form read at
 * run time (FORM = -1) instead of its compile-time instantiations; 1 restores
 * the default.  Results agree up to fp32 summation order.                  */
int mc_debug_lanes_forms(int on);
/* Test hook: 0 runs every lane-resident HMC launch on the general kernel
 * k_hmc_lr instead of the fast-form k_hmc_lf (as MC_LANES_FAST=0 in the
 * environment); 1 restores the default.  Results agree up to fp32
 * summation order.                                                        */
int mc_debug_lanes_fast(int on);
/* Test hook for k_nuts_lr's variants: -1 (default) picks the fastest variant
 * the program qualifies for; 0 forces the generic lane evaluator (SPEC 0);
 * 1 forces the specialised variant (SPEC 1) where the program qualifies,
 * skipping the register-only one.  Trees agree up to fp32 summation order. */
int mc_debug_nuts_variant(int variant);
/* Test hook for the sliced NUTS kernel k_nuts_sl (csrc/nuts_sliced.h): 0
 * runs sliced fast-form programs on k_nuts (the tape) instead, 1 on k_nuts_sl,
 * -1 restores the default (MC_NUTS_SLICED from the environment, else on).
 * Trees agree up to fp32 summation order.                                  */
int mc_debug_nuts_sliced(int on);
/* Diagnostic of the same-XCD exchange (csrc/sliced.h xcd_announce /
 * xcd_agree): the exchange groups (chain blocks, counted by their slice 0)
 * launched on `ws` since it was last cleared whose slices all sat on one XCD
 * (their records then stay in that XCD's L2), and those whose did not.      */
int mc_debug_workspace_xcd(const void* ws, int32_t* local, int32_t* remote);
/* The same-XCD exchange (L2-resident records, csrc/host.h xcd_round_robin):
 * 0 off, 1 on where the device's workgroup placement allows it, -1 the
 * default (MC_XCD_LOCAL from the environment, else on).  Results are the same
 * bits either way.                                                          */
int mc_debug_xcd_local(int on);
/* The sliced Metropolis-Hastings kernel k_mh_sl (csrc/mh_sliced.h):
 * mc_program_mh_sliced is 1 when mc_mh_run runs it (a program sliced onto
 * the fast-form lane layout: one wave per chain and slice, one log-p record
 * exchange per iteration), 0 when it runs k_mh on the tape, -1 on a null
 * program; mc_debug_mh_sliced: 0 forces k_mh, 1 allows k_mh_sl, -1 the
 * default (MC_MH_SLICED from the environment, else on).                    */
int32_t mc_program_mh_sliced(const mc_program* prog);
int mc_debug_mh_sliced(int on);
/* Expression terms (MC_DIST_EXPR) compiled per program (csrc/jit.hip):
 * hiprtc compiles the tape kernels' expression instantiations with each
 * term's node DAG as straight-line code (the interpreter's operations in its
 * order: bit-identical results), at the first launch that needs them; code
 * objects are cached per structure in the process and on disk ($MC_JIT_CACHE,
 * else ~/.cache/mcmc355).  mc_debug_expr_jit: 0 keeps the interpreter, 1 the
 * JIT, -1 the default (MC_EXPR_JIT from the environment, else on).
 * mc_program_expr_jit: 1 when the program's expression terms run compiled,
 * 0 when it has none or the JIT is off, -2 when their compilation failed (the
 * interpreter runs; mc_program_kernel_note says why), -1 on a null program. */
int mc_debug_expr_jit(int on);
int32_t mc_program_expr_jit(const mc_program* prog);
/* Test hooks without a device: mc_debug_program_host_only(1) makes the next
 * programs built on this thread host tables only (never launch them);
 * mc_debug_expr_jit_source copies the generated source of a program's
 * expression terms (returns its length); mc_debug_expr_jit_compile compiles
 * it into `kernel` (e.g. "mc::k_hmc<8, true, true>"), MC_OK or the
 * compiler's log as the error.                                              */
int mc_debug_program_host_only(int on);
int64_t mc_debug_expr_jit_source(const mc_program* prog, char* buf, int64_t cap);
int mc_debug_expr_jit_compile(const mc_program* prog, const char* kernel);
/* Test hook without a device: plan a host-only program's S slices onto the
 * lane-resident layout (host tables only); with expression terms on it,
 * mc_debug_expr_jit_source / _compile take a "mc::k_hmc_lr<...>" kernel name
 * and give / compile the lane-resident source (jit.hip gen_lane_source).  */
int mc_debug_lane_plan_host(mc_program* prog, int32_t num_slices);
/* host-only program (mc_debug_program_host_only): plan it with S slices and
 * write one 64-bit FNV-1a digest per host table: 13 of the slice plan (its
 * scalars S, Lp, Pmax, Dsh, nitems, sdata_floats, combine, then terms, sterms,
 * data, index, blocks, gidx), then 24 of the lane plan (ok, rs, rep, S, Dsh,
 * nitems, sdata_floats, shl, shxf, shid, n_generic, fast, form, has_xf,
 * has_expr, nuts_expr, bundle, then terms, data, blocks, gidx, sterms, rng,
 * gx_off); n_out >= 37.  Returns the planner's status: all digests 0 when the
 * slice planner refuses; the lane digests 0 and MC_ERR_UNSUPPORTED (the reason
 * in mc_last_error) when only the lane planner declines.                    */
int mc_debug_plan_digest(mc_program* prog, int32_t num_slices, uint64_t* out, int32_t n_out);
/* Test hook (host table, also of a host-only program after
 * mc_debug_lane_plan_host): the lane plan's moment constants, four floats
 * (c, R, Q, n) per [slice][4 slots][64 lanes]: of the run of the first swept
 * term that (slot, lane) holds, its centre c = (float) mean, R = sum (x - c),
 * Q = sum (x - c)^2 (float64 sums in element order, rounded once) and element
 * count; zeros for an empty run.  Not among the digests above (derived from
 * `data`).  Returns the number of floats (out may be NULL), negative on error. */
int64_t mc_debug_lane_moments(const mc_program* prog, float* out, int64_t n_out);
int64_t mc_debug_expr_jit_lane_source(const mc_program* prog, char* buf, int64_t cap);
/* Test hook (host tables, also of a host-only program): the tape plan of term
 * `term` in evaluation order (wave tasks last, csrc/program.hip), ten values,
 * n_out >= 10: dist, n (clamped to INT32_MAX), primary (-1 strided, else the
 * operand slot of the non-injective gather), npass, pass_masks (4 bits per
 * pass: 1 value, 2 loc, 4 scale, 8 log p), wave_task (-1 or the wave), ncomb
 * (> 0: split runs, the groups combined), ntiles, nvirt, sync_before.
 * MC_ERR_INVALID for a null program or buffer, n_out < 10 or a term out of
 * range.  Changes nothing.                                                  */
int mc_debug_term_plan(const mc_program* prog, int32_t term, int32_t* out, int32_t n_out);
/* Test hooks (host code, no device): the samplers' Box-Muller pair from two
 * Philox words per pair (words [n][2] -> out [n][2] f32) and their f32 log
 * of a uniform in (0, 1] (philox.h mc_box_muller / mc_logf_unit).         */
int mc_box_muller_host(const uint32_t* words, int64_t n, float* out);
int mc_logf_unit_host(const float* x, int64_t n, float* out);
/* After a sliced mc_hmc_run: MC_OK, or MC_ERR_TIMEOUT if an exchange timed
 * out (the launch then left its chains' state unchanged or partial).
 * Synchronises the stream.  Always MC_OK for an unsliced program.         */
int mc_workspace_status(const mc_program* prog, const void* workspace_dev,
                        int64_t workspace_bytes, void* hip_stream);
int mc_hmc_run(const mc_program* prog, const mc_run_config* cfg,
               void* state_dev, float* samples_dev, const mc_trace* trace,
               void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* NUTS (nuts.py:16-358), iterative tree building, max_tree_depth <= 16.    */
int64_t mc_nuts_workspace_bytes(const mc_program* prog, int64_t num_chains,
                                int32_t max_tree_depth);
int mc_nuts_run(const mc_program* prog, const mc_run_config* cfg,
                void* state_dev, float* samples_dev, const mc_trace* trace,
                void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* ---- diagonal mass matrix (no reference counterpart: its README roadmap
 * lists "Mass matrix adaptation") -------------------------------------------
 * A per-chain metric M = diag(1 / minv) for HMC and NUTS on the
 * chain-per-workgroup kernels k_hmc / k_nuts.  With msqrt_j = 1 / sqrt(minv_j),
 * computed when minv_j is set (all f32, no FMA contraction):
 *   momentum r_j = z_j * msqrt_j  (z_j the normal element j draws without a
 *   metric), velocity v_j = minv_j * r_j, kinetic energy 0.5 sum r_j v_j, drift
 *   q_j += e * v_j; kicks, accept rule, slice and the U-turn test (on the
 *   momentum r) as without a metric.  minv = 1 reproduces mc_hmc_run /
 *   mc_nuts_run on those kernels bit for bit.
 * Adaptation (adapt != 0, warmup iterations only; Stan's windows, per chain,
 * never pooled): with W = num_warmup, init = 75, term = 50, base = 25, or
 * init = floor(0.15 W), term = floor(0.1 W), base = W - init - term when
 * init + term + base > W; nothing is adapted when W < 20.  Windows tile
 * [init, W - term): the first has base iterations, each next twice the one
 * before, and a window is stretched to W - term when the one after it would
 * not fit.  After every iteration of a window the chain's position enters a
 * Welford accumulator (f32); at the window's last iteration, with n draws,
 *   minv_j = (n / (n + 5)) * M2_j / (n - 1) + 1e-3 * (5 / (n + 5))
 * (a value that is not finite or not positive keeps the old one), msqrt is
 * recomputed and the accumulator reset.  NUTS then restarts dual averaging
 * (mu = f32 log(10 * eps), H_bar = 0, eps_bar = 1, its iteration counter m
 * counts from the restart); HMC keeps its x0.95 / x1.05 rule.
 *
 * The metric lives in its own device buffer of mc_metric_bytes() bytes, the
 * state blob is unchanged:
 *   [mc_metric_scalars x C][pad to 256 B][minv C x D f32][pad][msqrt][pad]
 *   [mean][pad][M2]
 * (mc_metric_offsets gives the byte offsets of the four sections).  The
 * adaptation state persists in it, so a run may be cut into launches anywhere
 * and chains may be split over launches and devices without changing a bit. */
typedef struct mc_metric_scalars {
    int32_t n_window;   /* draws in the window's accumulator                 */
    int32_t n_updates;  /* metric updates so far                            */
    int64_t da_origin;  /* NUTS: iteration of the last dual-averaging restart */
} mc_metric_scalars;

/* The window ends (exclusive; the metric is updated after iteration end - 1)
 * for num_warmup warmup iterations: writes the first min(count, cap) into
 * ends (may be NULL) and returns the count.  Host only.                     */
int32_t mc_metric_schedule(int64_t num_warmup, int64_t* ends, int32_t cap);
int64_t mc_metric_bytes(const mc_program* prog, int64_t num_chains);
int mc_metric_offsets(const mc_program* prog, int64_t num_chains, int64_t* minv_offset,
                      int64_t* msqrt_offset, int64_t* mean_offset, int64_t* m2_offset);
/* Fill the metric buffer: minv from inv_mass_dev ([C, D] f32, or one [D]
 * vector for every chain when bcast = 1, or ones when NULL), msqrt from it,
 * accumulator and scalars zero.  An entry that is not finite or not positive
 * is MC_ERR_INVALID.  Not a launch function: the values are validated on the
 * host, so it synchronises the stream.  (For a program built under
 * mc_debug_program_host_only both pointers are host memory: the validation
 * and the layout can be checked without a device.)                         */
int mc_metric_init(const mc_program* prog, int64_t num_chains, const float* inv_mass_dev,
                   int32_t bcast, void* metric_dev, void* hip_stream);
/* mc_hmc_run / mc_nuts_run with the metric of metric_dev (same workspace
 * sizes); adapt != 0 adapts it during the warmup iterations of the launch.
 * MC_ERR_UNSUPPORTED for a program whose launches would not go to k_hmc /
 * k_nuts (a sliced or lane-resident plan: build the program with
 * mc_program_set_slices(prog, 1)).  Asynchronous, no allocation.           */
int mc_hmc_run_metric(const mc_program* prog, const mc_run_config* cfg,
                      void* state_dev, float* samples_dev, const mc_trace* trace,
                      void* workspace_dev, int64_t workspace_bytes, void* metric_dev,
                      int32_t adapt, void* hip_stream);
int mc_nuts_run_metric(const mc_program* prog, const mc_run_config* cfg,
                       void* state_dev, float* samples_dev, const mc_trace* trace,
                       void* workspace_dev, int64_t workspace_bytes, void* metric_dev,
                       int32_t adapt, void* hip_stream);

/* The metric on the lane-resident NUTS kernel (opt-in; mc_nuts_run_metric and
 * the default routing are unchanged).  mc_program_nuts_metric_lanes: 1 when
 * mc_nuts_run with this max_tree_depth runs k_nuts_lr's register-only variant
 * (mc_program_nuts_lanes == 2), else 0; -1 on a null program.
 * mc_nuts_run_metric_lanes: mc_nuts_run_metric's arguments and validations,
 * on k_nuts_lr<..., MET> (csrc/nuts_lanes.h): the same draws and decision
 * rules as k_nuts with a metric (summation order differs as between the two
 * kernels without one), a metric of ones gives mc_nuts_run's bits.
 * MC_ERR_UNSUPPORTED, with the reason in mc_last_error, when the query above is
 * not 1: the program is not planned as one lane-resident slice, it has
 * broadcast parameters or scalar terms, or a parameter has more than one
 * element.  No workspace is needed (one that is passed is forgotten as
 * mc_nuts_run does); mc_debug_nuts_variant does not apply.  Asynchronous, no
 * allocation.                                                               */
int32_t mc_program_nuts_metric_lanes(const mc_program* prog, int32_t max_tree_depth);
int mc_nuts_run_metric_lanes(const mc_program* prog, const mc_run_config* cfg,
                             void* state_dev, float* samples_dev, const mc_trace* trace,
                             void* workspace_dev, int64_t workspace_bytes, void* metric_dev,
                             int32_t adapt, void* hip_stream);

/* Random-walk Metropolis-Hastings (metropolis.py:6-101): per iteration
 * q' = q + f32(z * f32(proposal_scale)), z ~ N(0, I) (Philox, tag
 * MC_RNG_TAG_PROPOSAL), accept iff f32 log U < f32(lp(q') - lp(q)) (NaN
 * rejects), the current point is stored after every iteration.  The forward
 * tape only: one log density evaluation per iteration.  Every iteration of
 * the launch is a sampling iteration (set num_warmup = 0; MCMC.run's warmup
 * is a separate sampler run with its own seed, mcmc.py:145-178).  Uses
 * num_chains, chain_offset, iter_begin/iter_count, sample_begin/capacity and
 * seed of cfg; the state's logp (mc_state_init) is the current log density.
 * The gradient section of the state is not updated.  Trace: accepted,
 * accept_stat = log ratio, step_size = proposal scale, energy = log p.      */
int64_t mc_mh_workspace_bytes(const mc_program* prog, int64_t num_chains);
int mc_mh_run(const mc_program* prog, const mc_run_config* cfg, double proposal_scale,
              void* state_dev, float* samples_dev, const mc_trace* trace,
              void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* ---- RNG (replaces mx.random for the sampler draws) --------------------- */
/* Philox4x32-10 (Salmon et al., SC'11).  key = (seed lo, seed hi); counter =
 * (chain, iteration, tag << 24 | sub, index).  mode 0: raw u32 words
 * (out is uint32[n*4]); 1: f32 uniforms in (0,1) ((w >> 9) + 0.5) 2^-23;
 * 2: f32 standard normals, double-precision Box-Muller on word pairs.
 * Element e uses counter (chain, iteration, tag<<24 | sub, index0 + e).     */
#define MC_RNG_TAG_MOMENTUM 1
#define MC_RNG_TAG_ACCEPT   2
#define MC_RNG_TAG_SLICE    3
#define MC_RNG_TAG_DEPTH    4
#define MC_RNG_TAG_MERGE    5
#define MC_RNG_TAG_PROPOSAL 6   /* Metropolis-Hastings random-walk noise      */
#define MC_RNG_TAG_PREDICT  7   /* posterior predictive replicates (mc_predictive) */
#define MC_RNG_TAG_USER     16
int mc_rng_fill(uint64_t seed, uint32_t chain, uint32_t iteration,
                uint32_t tag, uint32_t sub, uint32_t index0, int64_t n,
                int32_t mode, void* out_dev, void* hip_stream);

/* ---- diagnostics over a sample buffer [C, S, D] (device, f32) ---------- */
/* A series is samples[c, :, d].  mc_series_stats writes stats[f * C*D + c*D + d]
 * (f64, device) for each field f:                                            */
#define MC_ST_ESS     0   /* compute_ess (examples/06_nuts_comparison.py:22-41):
                             n / (1 + 2 sum rho_k), lags 1 .. min(S/2, max_lag)-1,
                             stopping at (and including) the first rho < 0.05;
                             S when the variance is 0.  max_lag = 100 there.  */
#define MC_ST_MEAN    1   /* series mean                                      */
#define MC_ST_M2      2   /* sum of squared deviations from the mean          */
#define MC_ST_HMEAN0  3   /* mean of draws [0, S/2)                           */
#define MC_ST_HMEAN1  4   /* mean of draws [S - S/2, S)                       */
#define MC_ST_HM2_0   5   /* sum of squared deviations, first half            */
#define MC_ST_HM2_1   6   /* sum of squared deviations, second half           */
#define MC_ST_COUNT   7
int mc_series_stats(int64_t C, int64_t S, int64_t D, const float* samples_dev,
                    int32_t max_lag, double* stats_dev, void* hip_stream);
/* Chain-order reduction to out_dev[2, D] (f64).  center_dev == NULL:
 *   out[0][d] = sum of the 2C half-chain means, out[1][d] = sum_c ESS.
 * center_dev = that out[0] summed over every rank (m_total = all half chains):
 *   out[0][d] = sum (half mean - center[d]/m_total)^2,
 *   out[1][d] = sum of half-chain variances (ddof 1).
 * Multi-GPU: all-reduce (sum) out between the two calls and after the second. */
int mc_stats_reduce(int64_t C, int64_t S, int64_t D, const double* stats_dev,
                    const double* center_dev, int64_t m_total, double* out_dev,
                    void* hip_stream);
/* Split R-hat (Gelman et al., BDA3 eq. 11.4) over m_total half chains of
 * S/2 draws from the second reduction: rhat_dev[D] (f64).  S >= 4.          */
int mc_rhat(int64_t D, int64_t m_total, int64_t S, const double* spread_dev,
            double* rhat_dev, void* hip_stream);
/* Pooled mean and std (ddof 0) of every value of elements [off, off+len)
 * over all chains and draws (mcmc.py:205-206): out_dev[2] f64.             */
int mc_pool_moments(int64_t C, int64_t S, int64_t D, const double* stats_dev,
                    int64_t off, int64_t len, double* out_dev, void* hip_stream);
/* Exact order statistics (0-based ranks k[0..nk), host array, nk <= 8) of the
 * pooled values of elements [off, off+len): out_dev[nk] f32; NaN if any
 * pooled value is NaN (np.percentile / np.median, mcmc.py:207-209).          */
int64_t mc_select_workspace_bytes(int32_t nk);
int mc_select(int64_t C, int64_t S, int64_t D, const float* samples_dev,
              int64_t off, int64_t len, int32_t nk, const int64_t* k,
              float* out_dev, void* workspace_dev, int64_t workspace_bytes,
              void* hip_stream);

/* ---- pointwise log-likelihood over kept draws (no reference code: its README
 * roadmap lists "Model comparison (WAIC, LOO)") ------------------------------
 * The likelihood is a program of its own, traced like log_prob.  Every element
 * of every term is one observation: M = sum_t n_t, term by term in the order
 * the caller passed them and inside a term in the caller's element order.  The
 * pointwise value of element i of term t under a draw q is
 *     x = weight_t * lp_{t,i}(q)                (one f32 product)
 * with lp the tape's per-element f32 arithmetic (csrc/eval.h elem_eval and, for
 * expression terms, ex_fwd): the value the samplers' generic element path
 * forms.  The program's lp_const belongs to no observation and is left out.
 *
 * mc_program_num_elements returns M (host tables: also of a host-only
 * program).  mc_program_enable_pointwise builds and uploads, once, a view of
 * the terms and pools in the caller's order (the samplers' layouts are
 * permuted: segment tiles, slice plans, index-sorted copies); programs that
 * never call it pay nothing; MC_ERR_UNSUPPORTED, naming the term, for a term
 * the pointwise kernel cannot evaluate.  Not a launch function (it allocates).
 *
 * mc_pointwise_stats: samples_dev is the samplers' [C, S, D] buffer (D the
 * program's parameter count); stats_dev[f * M + o] (f64) receives, per
 * observation o over the C * S draws, the fields below; matrix_dev is NULL or
 * [C, S, M] f32 and then receives every pointwise value (small problems and
 * tests).  A launch function: asynchronous, no allocation, no synchronisation;
 * workspace_dev holds mc_pointwise_workspace_bytes(prog, C, S) bytes (0 is
 * possible: workspace_dev may then be NULL).  The draws are split into blocks
 * whose number depends on (C, S, the program) only and whose partials are
 * merged in block order: two calls give the same bits, with or without
 * matrix_dev.
 *
 * The six fields are a mergeable partial: two shards of draws combine exactly
 * into the whole (max / rescale for the first two, Chan's update for mean and
 * M2; with a non-finite draw on either side MEAN is the sum of the sides'
 * non-finite MEANs and M2 is NaN).  Accumulation is f64.  Non-finite values
 * follow NumPy float64 semantics: a -inf draw adds 0 to SUMEXP and makes MEAN
 * -inf and M2 NaN; all draws -inf gives MAX = -inf and SUMEXP = 0 (no NaN in
 * those two); a NaN draw makes MAX, SUMEXP and MEAN NaN.                     */
#define MC_PW_MAX       0   /* max over draws of x                            */
#define MC_PW_SUMEXP    1   /* sum over draws of exp(x - MAX)                 */
#define MC_PW_N         2   /* draws counted                                  */
#define MC_PW_MEAN      3   /* mean of x                                      */
#define MC_PW_M2        4   /* sum of squared deviations from the mean        */
#define MC_PW_NONFINITE 5   /* draws whose x is +-inf or NaN                  */
#define MC_PW_COUNT     6
int64_t mc_program_num_elements(const mc_program* prog);
int mc_program_enable_pointwise(mc_program* prog);
int64_t mc_pointwise_workspace_bytes(const mc_program* prog, int64_t C, int64_t S);
int mc_pointwise_stats(const mc_program* prog, int64_t C, int64_t S,
                       const float* samples_dev, double* stats_dev, float* matrix_dev,
                       void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* ---- posterior predictive replicates over kept draws (no reference code: its
 * README roadmap lists posterior predictive checks) --------------------------
 * On the pointwise view of a likelihood program (mc_program_enable_pointwise,
 * reused as built): every element of every term is one observation o, in the
 * caller's order.  A replicate y_rep[c, s, o] is a pure function of (seed,
 * global chain c + chain_offset, iteration s + iter_offset, o) and the term's
 * f32 operand values at that draw (what the pointwise kernel forms; the affine
 * loc as m + b * x) — not of the block split, of how chains are split over
 * calls or ranks, of thin, or of whether replicates are stored.  The term's
 * weight is ignored: a replicate comes from the untempered observation model.
 *
 * Counter: Philox (chain, iteration, MC_RNG_TAG_PREDICT << 24 | sub, o), words
 * w.x .. w.w; sub is the attempt of a rejection sampler, 0 elsewhere; Beta's
 * second Gamma uses sub = 0x100 + attempt.  With z0 the first normal of
 * Box-Muller on (w.x, w.y), u01(w) = (f32(w) + 0.5) 2^-32 and log the
 * samplers' f32 log (csrc/philox.h mc_box_muller, mc_u01_boxf, mc_logf_unit;
 * IEEE operations only: host and device give the same bits):
 *   Normal       loc + scale * z0
 *   HalfNormal   |scale * z0|
 *   Exponential  -log(u01(w.x)) / rate
 *   Gamma(a, b)  Marsaglia and Tsang (2000): d = a' - 1/3, c = 1 / sqrt(9 d),
 *                per attempt x = z0, v = (1 + c x)^3, accepted when v > 0 and
 *                log u01(w.z) < x^2 / 2 + d (1 - v + log v); the variate is
 *                d v / b.  a < 1: a' = a + 1 and the variate is multiplied by
 *                U^(1/a) = f32(exp(f64(log U / a))), U = u01 of attempt 0's
 *                w.w (the one value where host and device may differ, in the
 *                last bit, with probability ~1e-8); else a' = a.  At most 32
 *                attempts (each rejects with probability < 0.05), then NaN.
 *   Beta(a, b)   X / (X + Y), X ~ Gamma(a, 1), Y ~ Gamma(b, 1)
 * A scale, rate or shape that is <= 0 or NaN gives NaN (as a NaN loc does),
 * never a hang.  Identity terms and expression terms have no sampling
 * distribution — MC_ERR_UNSUPPORTED, naming the term, before any launch —
 * except the count terms: an expression term whose root is
 * MC_EX_BERNOULLI_LOGIT_LP / MC_EX_BINOMIAL_LOGIT_LP / MC_EX_POISSON_LOG_LP, or
 * ADD of such a node and a CONST / DATA leaf (the normaliser) in either order.
 * Their replicates come from the node's eta / theta (and n) at the draw — the
 * term's nodes below the count node, evaluated as the pointwise kernel does —
 * and the observation is the node's y.  Exact samplers (csrc/predictive.h
 * states them in full), double arithmetic from IEEE operations only, uniforms
 * u(w) = (w + 1/2) 2^-32:
 *   Bernoulli    [log u01(w.x) - log(1 - u01(w.x)) < eta] (the samplers' f32 log)
 *   Poisson      lambda = exp(theta) < 10: sequential-search inversion of
 *                u(w.x); else Hormann's PTRS (1993), one block per attempt
 *                (U = u(w.x) - 1/2, V = u(w.y)).  NaN for a NaN theta and for
 *                lambda >= 2^23.
 *   Binomial     p' = min(p, 1 - p), p = sigmoid(eta): inversion of u(w.x)
 *                when n p' < 10, else Hormann's BTRS (1993); reflected when
 *                p > 1/2.  NaN for a NaN eta and for n negative, non-integer
 *                or >= 2^23.
 * At most 32 attempts, then NaN.  An inversion's uniform resolves 2^-32:
 * outcomes beyond the 1 - 2^-33 quantile do not occur.
 * The Student-t terms have a sampling distribution by the same rule: the root
 * is MC_EX_STUDENT_T_LP / MC_EX_HALF_STUDENT_T_LP, or ADD of such a node and a
 * CONST / DATA leaf.  Value, loc and scale are the node's arguments at the
 * draw; one rule for every nu (Cauchy included), f32 IEEE operations:
 *   z0 the first normal of mc_box_muller(w.x, w.y), attempt 0's block
 *   g ~ Gamma(nu / 2, 1) by the Gamma sampler above on Beta's second sub range
 *   t = z0 / sqrt(g / (nu / 2));  Student-t: loc + scale t;  half: |scale t|
 * NaN for a scale that is <= 0 or NaN, a NaN loc, and an exhausted Gamma.
 * For nu < 2 the Gamma shape is below 1 and its last-bit caveat applies.
 *
 * mc_predictive_draw: the scalar definition on the host (no device, no
 * allocation): *out = the replicate of observation obs under (dist, loc or
 * alpha, scale / rate / beta).  MC_ERR_UNSUPPORTED for any other dist.
 *
 * mc_predictive_draw_discrete: its counterpart for the count terms (kind an
 * mc_discrete_kind, total the Binomial's n, eta the logit / log rate).
 *
 * mc_predictive_draw_student_t: the same for the Student-t terms (half != 0:
 * the half form, loc unread).  df that is <= 0 or NaN gives NaN.
 *
 * mc_predictive_eq: mc_predictive plus equal_dev, NULL or [M] f64: the finite
 * replicates EQUAL to the observation (the ties a discrete PIT needs; the five
 * fields are unchanged).  mc_predictive is mc_predictive_eq with NULL.  The
 * ties are counted for programs with a count term only
 * (mc_program_num_count_terms > 0: every term of such a program is counted,
 * the fused ones too); equal_dev on any other program is MC_ERR_UNSUPPORTED,
 * and those programs' kernels and workspace size are what they were.  With a
 * count term the workspace holds one more f64 per block and observation.
 *
 * mc_program_num_count_terms: how many terms of the pointwise view have a
 * count sampler (known from program creation: no device, no view needed).
 * Student-t terms are not count terms: a program whose expression samplers are
 * all Student-t has no ties, and its workspace is five fields per block.
 *
 * mc_predictive: samples_dev is the [C, S, D] buffer; thin >= 1 processes
 * iterations s = 0, thin, 2 thin, ... of every chain (S' = ceil(S / thin); the
 * counter carries the true s + iter_offset).  stats_dev[f * M + o] (f64)
 * receives the fields below over the C * S' processed draws; yrep_dev is NULL
 * or [C, S', M] f32 and then receives every replicate.  A launch function:
 * asynchronous, no allocation, no synchronisation; workspace_dev holds
 * mc_predictive_workspace_bytes(prog, C, S, thin) bytes (0 is possible).  The
 * block split depends on (C, S, thin, the program) only and the partials are
 * merged in block order: two calls give the same bits, with or without
 * yrep_dev.  The five fields are a mergeable partial (Chan's update over the
 * finite counts N - NONFINITE, counts added).                               */
#define MC_PP_N         0   /* draws processed                                */
#define MC_PP_MEAN      1   /* mean of the finite replicates (NaN: none)      */
#define MC_PP_M2        2   /* their sum of squared deviations from the mean  */
#define MC_PP_BELOW     3   /* finite replicates < the observation (the term's
                               value operand at that draw)                    */
#define MC_PP_NONFINITE 4   /* replicates that are +-inf or NaN               */
#define MC_PP_COUNT     5
int mc_predictive_draw(int dist, float loc_or_alpha, float scale_or_rate_or_beta,
                       uint64_t seed, uint32_t chain, uint32_t iter, uint32_t obs, float* out);
int32_t mc_program_num_count_terms(const mc_program* prog);
int mc_predictive_draw_discrete(int kind, float total, float eta, uint64_t seed,
                                uint32_t chain, uint32_t iter, uint32_t obs, float* out);
int mc_predictive_draw_student_t(float df, float loc, float scale, int half, uint64_t seed,
                                 uint32_t chain, uint32_t iter, uint32_t obs, float* out);
int64_t mc_predictive_workspace_bytes(const mc_program* prog, int64_t C, int64_t S,
                                      int64_t thin);
int mc_predictive(const mc_program* prog, int64_t C, int64_t S, int64_t thin, uint64_t seed,
                  int64_t chain_offset, int64_t iter_offset, const float* samples_dev,
                  double* stats_dev, float* yrep_dev, void* workspace_dev,
                  int64_t workspace_bytes, void* hip_stream);
int mc_predictive_eq(const mc_program* prog, int64_t C, int64_t S, int64_t thin, uint64_t seed,
                     int64_t chain_offset, int64_t iter_offset, const float* samples_dev,
                     double* stats_dev, double* equal_dev, float* yrep_dev,
                     void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* ---- PSIS-LOO over kept draws (no reference code: its README roadmap lists
 * "Model comparison (WAIC, LOO)") ---------------------------------------------
 * Pareto-smoothed importance sampling leave-one-out (Vehtari, Gelman and Gabry
 * 2017) on the pointwise view of a likelihood program
 * (mc_program_enable_pointwise, reused as built).  For observation o over the
 * N = C * S draws, l_s is the f32 pointwise value mc_pointwise_stats forms (the
 * same bits; -0 taken as +0); everything after the selection is f64:
 *   1 tail length  Mt = min(ceil(min(N / 5, 3 sqrt(N / r_eff))), N - 1), r_eff a
 *                  positive scalar (mc_psis_tail_len)
 *   2 cutoff       L, the (Mt + 1)-th smallest l counted with multiplicity
 *   3 tail         { s : l_s < L } (strict: ties at the cutoff drop out, so
 *                  n = |tail| <= Mt); lmin the smallest l
 *   4 exceedances  the tail in decreasing l, t_1 >= ... >= t_n;
 *                  e_c = exp(lmin - L), y_j = exp(lmin - t_j) - e_c (ascending)
 *   5 fit          Zhang and Stephens (2009) with the PSIS paper's prior.
 *                  n <= 4: khat = +inf, sigma = NaN, nothing is smoothed.  Else
 *                  m = 30 + floor(sqrt(n)); y_q the floor(n / 4 + 1/2)-th
 *                  smallest y; b_i = (1 - sqrt(m / (i - 1/2))) / (3 y_q) + 1 / y_n
 *                  (i = 1 .. m); kappa_i = mean_j log1p(-b_i y_j);
 *                  L_i = n (log(-b_i / kappa_i) - kappa_i - 1);
 *                  w_i = 1 / sum_j exp(L_j - L_i), normalised to sum 1 (no
 *                  small-weight filter); bbar = sum w_i b_i;
 *                  kbar = mean_j log1p(-bbar y_j); sigma = -kbar / bbar;
 *                  khat = (n kbar + 5) / (n + 10).  IEEE arithmetic throughout:
 *                  a degenerate tail gives NaN khat and sigma, never an error.
 *   6 smoothing    when khat is finite and sigma > 0: p_j = (j - 1/2) / n,
 *                  q_j = sigma expm1(-khat log1p(-p_j)) / khat (|khat| <
 *                  DBL_EPSILON: -sigma log1p(-p_j)); the tail's log weights
 *                  become lw_j = min(log(q_j + e_c), 0) in rank order.  Every
 *                  other draw, and the tail when nothing is smoothed, keeps
 *                  lw_s = lmin - l_s.
 *   7 elpd         log((N - n) + sum_tail exp(t_j + lw_j - lmin))
 *                  - log(sum_tail exp(lw_j) + sum_rest exp(lmin - l_s)) + lmin
 *                  (the difference of the logs first); the rest sum is an f64
 *                  sum per block of draws, the blocks merged in order.
 *   8 non-finite   an observation with any non-finite draw gets NaN ELPD, KHAT
 *                  and SIGMA: counted by the caller (MC_PW_NONFINITE), never
 *                  raised.
 *
 * mc_psis_fit_host: steps 5 and 6 on the host (no device), the code the fit
 * kernel runs: tail_desc[n] is the tail in decreasing l; *khat and *sigma are
 * written; lw_out is NULL or [n] and receives the log weights in rank order.
 *
 * mc_psis_loo: a launch function (asynchronous, no allocation, no
 * synchronisation).  out_dev[f * M + o] (f64) receives the fields below;
 * tail_dev is NULL or [M, Mt] f32 and receives each observation's tail in
 * ascending l, NaN after its n-th entry.  workspace_dev holds
 * mc_psis_workspace_bytes(prog, C, S, r_eff) bytes: O(M * Mt) f32 for the tails
 * plus the per-block partials; the C * S * M matrix is never stored (the draws
 * are re-evaluated: eight passes of an exact radix select of L, one gather).
 * Mt above 2048 (kPsisMaxTail: the fit kernel sorts a tail in LDS) is
 * MC_ERR_UNSUPPORTED from mc_psis_workspace_bytes, before any launch.  The
 * split into blocks depends on (C, S, r_eff, the program) only; counts are
 * integers and every f64 sum has a fixed order: two calls give the same bits,
 * with or without tail_dev.  No atomics, nothing waits on another workgroup. */
#define MC_PSIS_ELPD    0   /* elpd_loo of the observation                     */
#define MC_PSIS_KHAT    1   /* Pareto shape estimate (+inf: n <= 4)            */
#define MC_PSIS_SIGMA   2   /* Pareto scale estimate (NaN: n <= 4)             */
#define MC_PSIS_CUTOFF  3   /* L                                               */
#define MC_PSIS_MIN     4   /* lmin                                            */
#define MC_PSIS_TAILN   5   /* n                                               */
#define MC_PSIS_COUNT   6
int64_t mc_psis_tail_len(int64_t N, double r_eff);
int mc_psis_fit_host(const float* tail_desc, int64_t n, float cutoff, float lmin,
                     double* khat, double* sigma, double* lw_out);
int64_t mc_psis_workspace_bytes(const mc_program* prog, int64_t C, int64_t S, double r_eff);
int mc_psis_loo(const mc_program* prog, int64_t C, int64_t S, double r_eff,
                const float* samples_dev, double* out_dev, float* tail_dev,
                void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* ---- Rank-normalised split R-hat, bulk-ESS and tail-ESS (Vehtari, Gelman,
 * Simpson, Carpenter and Buerkner 2021, Bayesian Analysis 16(2); no reference
 * code) ---------------------------------------------------------------------
 * For one element d of a [C, S, D] f32 buffer:
 *   split chains   h = floor(S / 2); the halves are draws [0, h) and [S - h, S)
 *                  of every chain (the middle draw of an odd S is dropped, as
 *                  mc_series_stats drops it): m = 2C split chains of n = h
 *                  draws, N = m n, position p = j n + i.  n < 4: every output
 *                  is NaN.
 *   pool           over the N split draws: the median as np.median of f32, q05
 *                  and q95 as np.percentile of f32 with the 'linear' rule (the
 *                  ranks and the weight formed in f32 on the host, the two-
 *                  branch interpolation in f32 on the device).
 *   ranks          r = the average rank of every value among the N (ties share
 *                  the mean of their positions; -0 and +0 are equal; +-inf
 *                  have ranks); z = ndtri((r - 3/8) / (N + 1/4)) in f64.
 *   R(y), y [m, n] W = mean_j var_j (ddof 1), B/n = var_j(mean_j, ddof 1),
 *                  var+ = (n - 1)/n W + B/n, R = sqrt(var+ / W).
 *   ESS(y)         acov_j(t) = (1/n) sum_{i < n - t} (y_ji - mean_j)(y_j,i+t -
 *                  mean_j), a_t = mean_j acov_j(t), W = a_0 n / (n - 1),
 *                  rho_t = 1 - (W - a_t) / var+, rho_0 = 1; then the sequence
 *                  rule of Stan's compute_effective_sample_size (Geyer's
 *                  initial positive and monotone sequences over pairs):
 *                    r[0] = even = 1; r[1] = odd = rho_1; t = 1
 *                    while t < n - 3 and even + odd > 0:
 *                        even = rho_{t+1}; odd = rho_{t+2}
 *                        if even + odd >= 0: r[t+1] = even; r[t+2] = odd
 *                        t += 2
 *                    max_t = t - 2
 *                    if even > 0: r[max_t + 1] = even
 *                    for t = 1, 3, ... <= max_t - 2:
 *                        if r[t+1] + r[t+2] > r[t-1] + r[t]:
 *                            r[t+1] = r[t+2] = (r[t-1] + r[t]) / 2
 *                    tau = -1 + 2 sum(r[0 .. max_t]) + r[max_t + 1]
 *                    tau = max(tau, 1 / log10(N)); ESS = N / tau
 *                  (entries of r never written are 0).
 *   outputs        RHAT_BULK = R(z(y)); RHAT_FOLDED = R(z(|y - median|)), the
 *                  difference and its absolute value in f32; RHAT_RANK the
 *                  larger; ESS_BULK = ESS(z(y)); ESS_TAIL = min(ESS(1[y <=
 *                  q05]), ESS(1[y <= q95])); CONSTANT = 1 where all N draws are
 *                  equal, else 0.
 *   edges          an element with a NaN draw: NaN in the five, CONSTANT 0.  W
 *                  = 0 (a constant element, a constant indicator): NaN.
 *
 * mc_rank_diag: a launch function (asynchronous, no allocation, no
 * synchronisation).  out_dev is [MC_RD_COUNT, D] f64.  z_dev is NULL or
 * [D, 2C, n] f64 and receives the bulk z-scores (small problems and tests).
 * Elements are processed in batches that share workspace_dev
 * (mc_rank_diag_workspace_bytes(C, S, D) bytes: 28 N bytes per element of a
 * batch plus the sort's histograms and the split-chain means); the batch size depends on (C, S, D) and
 * a fixed cap only, never on the device.  Pairs (key, position) are sorted by a
 * stable LSD radix sort, in one workgroup's LDS for N <= 8192, else across
 * workgroups; counts are integers and every f64 sum has a fixed order: two
 * calls give the same bits, on either path, with any batch size, with or
 * without z_dev.  N >= 2^31 is MC_ERR_UNSUPPORTED.
 *
 * mc_geyer_ess_host: the sequence rule on the host (no device), the code the
 * kernel runs: rho[n - 1] holds rho_1 .. rho_{n-1}, n >= 4.
 *
 * mc_debug_rank_path: 0 automatic; 1 the multi-workgroup sort for every N; 2
 * batches of at most 3 elements.  Returns the previous value. */
#define MC_RD_RHAT_BULK    0
#define MC_RD_RHAT_FOLDED  1
#define MC_RD_RHAT_RANK    2
#define MC_RD_ESS_BULK     3
#define MC_RD_ESS_TAIL     4
#define MC_RD_CONSTANT     5
#define MC_RD_COUNT        6
int64_t mc_rank_diag_workspace_bytes(int64_t C, int64_t S, int64_t D);
int mc_rank_diag(int64_t C, int64_t S, int64_t D, const float* samples_dev, double* out_dev,
                 double* z_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream);
int mc_geyer_ess_host(const double* rho, int64_t n, int64_t N, double* ess);
int mc_debug_rank_path(int path);

const char* mc_last_error(void);
int32_t mc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MCMC355_H */
