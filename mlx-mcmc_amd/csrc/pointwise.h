// pointwise.h — per-observation log-likelihood statistics over kept draws
// (mc_pointwise_stats; no reference counterpart: its README roadmap lists
// "Model comparison (WAIC, LOO)").
//
// A likelihood program's every element is one observation: M = sum_t n_t, in
// the caller's term and element order (the pointwise view of the program,
// run_pointwise.hip — not the samplers' permuted layouts).  For a [C, S, D]
// sample buffer the value of observation o under draw r = c * S + s is
//     x[r, o] = weight_t * lp_{t,i}(q_r)            (one f32 product)
// with lp the tape's own per-element arithmetic (eval.h elem_eval, xf_apply,
// the affine loc's two roundings, lg_norm_dev; ex_fwd for expression terms),
// so a value is what the sampler's generic element path computes.  The
// C * S * M values are never stored (unless the caller passes a matrix):
//
//   k_pointwise   grid (tiles, B).  A tile is up to 256 consecutive elements
//                 of ONE term (the term descriptor is workgroup-uniform: scalar
//                 loads), one observation per thread; block b walks draws
//                 [b * per, (b + 1) * per).  A thread keeps its element's data
//                 values and parameter offsets in registers — at most five
//                 operands — and reads the parameters of a draw straight from
//                 the draw's row of the sample buffer: every workgroup of one
//                 b reads the same rows at about the same time, so the rows
//                 are served by L1 / L2 and nothing is staged in LDS (a row is
//                 D floats; D is unbounded, and a thread needs <= 5 of them).
//                 The maximum and the sum of exponentials are kept online
//                 per draw; the values of kPwBatch draws stay in registers
//                 for the two passes of the moments (mean, then squared
//                 deviations: one f64 division per batch, not per draw).
//                 Writes one partial per (b, observation).
//   k_pw_merge    one thread per observation merges the B partials in block
//                 order.
// B and the tiling depend on (C, S, the program) only — never on the device —
// so two calls give the same bits, with or without the matrix.
//
// Accumulation over draws is f64 throughout (the exponentials too: the
// statistics are compared with a float64 reduction of the same f32 values at
// 1e-10).  A partial is the six fields of mcmc355.h (MC_PW_*):
//   MAX, SUMEXP   running maximum m and sum exp(x - m), rescaled when m moves
//   N             draws counted
//   MEAN, M2      Chan's pairwise update of per-batch two-pass moments
//   NONFINITE     draws whose x is +-inf or NaN
// Non-finite draws follow NumPy float64 semantics: a -inf draw adds 0 to the
// sum of exponentials (all draws -inf: MAX = -inf, SUMEXP = 0, no NaN in those
// two), a NaN draw makes MAX and SUMEXP NaN; with any non-finite draw MEAN is
// the sum of the non-finite values (-inf, +inf or NaN, as np.mean gives) and M2
// is NaN (as np.var gives).  pw_merge applies the same rules to two partials.
#pragma once
#include "eval.h"

namespace mc {

enum { PW_MAX = 0, PW_SUMEXP, PW_N, PW_MEAN, PW_M2, PW_NONFINITE, PW_COUNT };

constexpr int kPwBlock = 256;  // observations per tile (threads per workgroup)
constexpr int kPwBatch = 8;    // draws whose values share one moment update

// A tile: elements [e0, e0 + 256) and [0, n) of term `term`, observations o0 ...
struct PwTile {
    int64_t e0;
    int64_t o0;
    int32_t term;
    int32_t pad;
};

// The pointwise view: terms, nodes and pools as the caller passed them.
struct PwCtx {
    const DevTerm* terms;
    const DevExprNode* nodes;
    const float* data;
    const int32_t* index;
    const PwTile* tiles;
    int64_t M;
    int32_t D;
    int32_t ntiles;
};

struct PwAcc {
    double m, s, n, mean, m2, nf;
};

// max as np.max takes it: a NaN wins and stays
MC_DEV float pw_maxf(float a, float x) { return (x > a || x != x) ? x : a; }
__host__ __device__ inline double pw_maxd(double a, double x) {
    return (x > a || x != x) ? x : a;
}
__host__ __device__ inline bool pw_finite(double x) { return x - x == 0.0; }

// A <- A u B (both non-empty): max / rescale, Chan's update.
__host__ __device__ inline void pw_merge(PwAcc& A, const PwAcc& B) {
    const double m = pw_maxd(A.m, B.m);
    const double sa = A.m == m ? A.s : A.s * exp(A.m - m);
    const double sb = B.m == m ? B.s : B.s * exp(B.m - m);
    A.m = m;
    A.s = sa + sb;
    const double n = A.n + B.n;
    if (A.nf > 0.0 || B.nf > 0.0) {
        // (a partial with non-finite draws carries their class in MEAN; one
        // without, a finite mean that does not change the class)
        A.mean = A.nf > 0.0 ? (B.nf > 0.0 ? A.mean + B.mean : A.mean) : B.mean;
        A.m2 = __builtin_nan("");
    } else {
        const double d = B.mean - A.mean;
        const double r = 1.0 / n;
        A.mean += d * (B.n * r);
        A.m2 += B.m2 + d * d * (A.n * B.n * r);
    }
    A.n = n;
    A.nf += B.nf;
}

// One value into the running maximum and the sum of exponentials about it
// (rescaled when the maximum moves; a -inf value adds 0, also to an all -inf
// sum; a NaN maximum lands in the rescale every time: the sum stays NaN).
MC_DEV void pw_lse(PwAcc& A, float x) {
    const double xd = (double)x;
    const double mn = pw_maxd(A.m, xd);
    if (mn != A.m) {
        A.s *= exp(A.m - mn);
        A.m = mn;
    }
    A.s += (x == -__builtin_inff()) ? 0.0 : exp(xd - A.m);
}

// The moments of the last kb <= kPwBatch values of the window x (two passes
// in registers), merged into the accumulator by Chan's update; non-finite
// values are counted and summed apart (their class: -inf, +inf or NaN).
MC_DEV void pw_moments(PwAcc& A, double& nfsum, const float (&x)[kPwBatch], int kb) {
    double sum = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < kPwBatch; ++k) {
        if (k >= kPwBatch - kb) {
            const double xd = (double)x[k];
            if (pw_finite(xd)) {
                sum += xd;
                cnt += 1.0;
            } else {
                nfsum += xd;
                A.nf += 1.0;
            }
        }
    }
    if (cnt > 0.0) {
        const double bmean = sum / cnt;
        double bm2 = 0.0;
#pragma unroll
        for (int k = 0; k < kPwBatch; ++k) {
            if (k >= kPwBatch - kb) {
                const double xd = (double)x[k];
                if (pw_finite(xd)) {
                    const double e = xd - bmean;
                    bm2 += e * e;
                }
            }
        }
        if (A.n == 0.0) {
            A.mean = bmean;
            A.m2 = bm2;
            A.n = cnt;
        } else {
            const double d = bmean - A.mean;
            const double tot = A.n + cnt;
            const double r = 1.0 / tot;
            A.mean += d * (cnt * r);
            A.m2 += bm2 + d * d * (A.n * cnt * r);
            A.n = tot;
        }
    }
}

// An operand of the thread's element: a parameter offset into the draw's row
// (with its transform), or the element's constant / data value.
struct PwOp {
    int64_t j;
    float c;
    int32_t xf;
    bool par;
};
MC_DEV PwOp pw_operand(const DevOperand& o, int64_t i, const PwCtx& P) {
    PwOp r;
    r.j = 0;
    r.c = 0.0f;
    r.xf = o.xf;
    r.par = false;
    switch (o.kind) {
        case MC_OP_CONST:
            r.c = o.cval;
            break;
        case MC_OP_PSCALAR:
            r.par = true;
            r.j = o.poff;
            break;
        case MC_OP_DATA:
            r.c = P.data[o.pool + i];
            break;
        case MC_OP_PVEC:
            r.par = true;
            r.j = (int64_t)o.poff + i;
            break;
        case MC_OP_GATHER:
            r.par = true;
            r.j = (int64_t)o.poff + P.index[o.pool + i];
            break;
        default:
            break;
    }
    return r;
}
// (eval.h fetch's value: the transform applied to the f32 parameter)
MC_DEV float pw_value(const PwOp& r, const float* __restrict__ q) {
    return r.par ? xf_apply(r.xf, q[r.j]) : r.c;
}

// Forward walk of an expression term's nodes for element i at q (eval.h
// eval_expr_n's forward half on the nodes as validated: original pools, no
// run layout).  NMAX 16 keeps val[] in registers; 32 may spill to scratch.
template <int NMAX>
MC_DEV void pw_expr_walk(const DevTerm& T, const PwCtx& P, const float* __restrict__ q, int64_t i,
                         int stop, float (&val)[NMAX]) {
    const MC_CONST DevExprNode* N = cptr(P.nodes) + T.expr_base;
    for (int k = 0; k < stop && k < NMAX; ++k) {
        const int op = N[k].op;
        float v;
        if (op == MC_EX_LEAF) {
            const int kind = N[k].leaf.kind;
            const int poff = N[k].leaf.poff;
            const int64_t pool = N[k].leaf.pool;
            if (kind == MC_OP_CONST) v = N[k].leaf.cval;
            else if (kind == MC_OP_PSCALAR) v = q[poff];
            else if (kind == MC_OP_DATA) v = P.data[pool + i];
            else if (kind == MC_OP_PVEC) v = q[poff + i];
            else v = q[poff + P.index[pool + i]];
        } else {
            const int a = N[k].a, b = N[k].b, c = N[k].c;
            v = ex_fwd(op, val[a], b >= 0 ? val[b] : 0.0f, c >= 0 ? val[c] : 0.0f,
                       N[k].leaf.cval);
        }
        val[k] = v;
    }
}
// (stop: the nodes [0, stop) are evaluated — the whole term here; predictive.h
// stops before a count node to read its arguments)
template <int NMAX>
MC_DEV float pw_expr(const DevTerm& T, const PwCtx& P, const float* __restrict__ q, int64_t i) {
    const int nn = T.expr_n;
    float val[NMAX];
    pw_expr_walk<NMAX>(T, P, q, i, nn, val);
    return T.weight * val[nn - 1];
}

// The thread's element of term T, decoded once: its operands (at most five)
// and eval_term's ulogs / ulg choices.
struct PwElem {
    PwOp ov, om, os, ob, ox;
    bool expr, aff, clogs, need_logs, need_lg, use_clg;
};
template <int NMAX>
MC_DEV PwElem pw_elem(const DevTerm& T, const PwCtx& P, int64_t i) {
    PwElem E;
    E.expr = false;
    if constexpr (NMAX > 0) E.expr = T.dist == MC_DIST_EXPR;
    E.aff = E.clogs = E.need_logs = E.need_lg = E.use_clg = false;
    E.ov = E.om = E.os = E.ob = E.ox = PwOp{0, 0.0f, 0, false};
    if (!E.expr) {
        E.ov = pw_operand(T.op[0], i, P);
        E.om = pw_operand(T.op[1], i, P);
        E.os = pw_operand(T.op[2], i, P);
        E.aff = T.affine != 0;
        if (E.aff) {
            E.ob = pw_operand(T.ab, i, P);
            E.ox = pw_operand(T.ax, i, P);
        }
        // eval_term's ulogs / ulg: the precomputed f32 log of a constant scale
        // and normaliser of constant shapes, else from the current values
        E.clogs = T.op[2].kind == MC_OP_CONST;
        E.need_logs = T.dist == MC_DIST_NORMAL || T.dist == MC_DIST_HALFNORMAL ||
                      T.dist == MC_DIST_EXPONENTIAL || T.dist == MC_DIST_GAMMA;
        E.need_lg = T.dist == MC_DIST_GAMMA || T.dist == MC_DIST_BETA;
        E.use_clg = !lg_per_element(T.dist, T.op[1].kind, T.op[2].kind) &&
                    !(T.op[1].kind == MC_OP_PSCALAR || T.op[2].kind == MC_OP_PSCALAR);
    }
    return E;
}

// The pointwise value of the element under the draw whose row is q: the one
// definition every unit on the pointwise view evaluates (k_pointwise, psis.h),
// so they form the same bits.
template <int NMAX, bool LG>
MC_DEV float pw_elem_value(const PwElem& E, const DevTerm& T, const PwCtx& P,
                           const float* __restrict__ q, int64_t i) {
    if constexpr (NMAX > 0) {
        if (E.expr) return pw_expr<NMAX>(T, P, q, i);
    }
    const float v = pw_value(E.ov, q);
    float m = pw_value(E.om, q);
    if (E.aff) m = m + pw_value(E.ob, q) * pw_value(E.ox, q);
    const float s = pw_value(E.os, q);
    const float logs = E.need_logs ? (E.clogs ? T.clogs : logf(s)) : 0.0f;
    float lg = T.clg;
    if constexpr (LG) {
        if (E.need_lg && !E.use_clg) lg = lg_norm_dev(T.dist, m, s);
    }
    return T.weight * elem_eval(T.dist, T.c0, v, m, s, logs, lg).lp;
}

// NMAX == 0: fused terms only; 16 / 32: expression terms of up to that many
// nodes as well (separate instantiations, as the tape kernels' EX variants:
// programs without expression terms keep the fused path's registers).
// LG: the program has a Gamma / Beta term whose normaliser follows the draw
// (float64 lgamma: ~100 VGPRs the other programs' kernel does not carry).
template <int NMAX, bool LG>
__global__ __launch_bounds__(kPwBlock) void k_pointwise(PwCtx P, int64_t N, int64_t per,
                                                        const float* __restrict__ samples,
                                                        double* __restrict__ part,
                                                        float* __restrict__ matrix) {
    const PwTile tile = P.tiles[blockIdx.x];
    // (the tile's term is the same in every lane: scalar loads of its descriptor)
    const DevTerm T = load_term(cptr(P.terms) + __builtin_amdgcn_readfirstlane(tile.term));
    const int64_t i = tile.e0 + threadIdx.x;
    if (i >= T.n) return;  // (no barrier and no LDS below)
    const int64_t o = tile.o0 + threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    const int64_t r1 = r0 + per < N ? r0 + per : N;
    const int64_t D = P.D;

    PwAcc A = {-(double)__builtin_inff(), 0.0, 0.0, 0.0, 0.0, 0.0};
    double nfsum = 0.0;
    const PwElem E = pw_elem<NMAX>(T, P, i);

    for (int64_t r = r0; r < r1; r += kPwBatch) {
        const int kb = r1 - r < kPwBatch ? (int)(r1 - r) : kPwBatch;
        // one draw at a time (the element code is emitted once); its value
        // enters a register window of the batch's values, newest last
        float x[kPwBatch];
#pragma unroll
        for (int k = 0; k < kPwBatch; ++k) x[k] = 0.0f;
#pragma unroll 1
        for (int k = 0; k < kb; ++k) {
            const float* __restrict__ q = samples + (r + k) * D;
            const float xk = pw_elem_value<NMAX, LG>(E, T, P, q, i);
            if (matrix) matrix[(r + k) * P.M + o] = xk;
            pw_lse(A, xk);
#pragma unroll
            for (int j = 0; j + 1 < kPwBatch; ++j) x[j] = x[j + 1];
            x[kPwBatch - 1] = xk;
        }
        pw_moments(A, nfsum, x, kb);
    }
    if (A.nf > 0.0) {
        A.mean = nfsum;
        A.m2 = __builtin_nan("");
    }
    double* out = part + (int64_t)blockIdx.y * PW_COUNT * P.M + o;
    out[PW_MAX * P.M] = A.m;
    out[PW_SUMEXP * P.M] = A.s;
    out[PW_N * P.M] = A.n + A.nf;
    out[PW_MEAN * P.M] = A.mean;
    out[PW_M2 * P.M] = A.m2;
    out[PW_NONFINITE * P.M] = A.nf;
}

// stats[f * M + o] from the B partials of observation o, in block order
// (internal linkage: predictive.h brings this header into a second unit)
static __global__ __launch_bounds__(256) void k_pw_merge(const double* __restrict__ part,
                                                         int64_t M, int32_t B,
                                                         double* __restrict__ stats) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M) return;
    auto load = [&](int b) {
        const double* p = part + (int64_t)b * PW_COUNT * M + o;
        PwAcc X;
        X.m = p[PW_MAX * M];
        X.s = p[PW_SUMEXP * M];
        X.n = p[PW_N * M];
        X.mean = p[PW_MEAN * M];
        X.m2 = p[PW_M2 * M];
        X.nf = p[PW_NONFINITE * M];
        return X;
    };
    PwAcc A = load(0);
    for (int b = 1; b < B; ++b) pw_merge(A, load(b));
    stats[PW_MAX * M + o] = A.m;
    stats[PW_SUMEXP * M + o] = A.s;
    stats[PW_N * M + o] = A.n;
    stats[PW_MEAN * M + o] = A.mean;
    stats[PW_M2 * M + o] = A.m2;
    stats[PW_NONFINITE * M + o] = A.nf;
}

}  // namespace mc
