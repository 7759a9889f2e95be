// predictive.h — posterior predictive replicates and per-observation checks
// over kept draws (mc_predictive; no reference counterpart: its README roadmap
// lists posterior predictive checks).
//
// A replicate y_rep[c, s, o] is a pure function of (seed, global chain
// c + chain_offset, iteration s + iter_offset, observation o) and the f32
// operand values of o's term at that draw — of nothing else: not of how the
// draws are split into blocks, how chains are split over calls or ranks, thin,
// or whether the replicates are stored.
//
//   counter   mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, sub, o): sub is
//             the attempt of a rejection sampler (0 elsewhere); Beta's second
//             Gamma uses sub = 0x100 + attempt.
//   operands  what k_pointwise forms (pw_operand / pw_value with xf_apply, the
//             affine loc as m + b * x: two roundings).  The term's weight is
//             ignored: a replicate comes from the untempered observation model.
//   samplers  pp_draw below: MC_HD, IEEE operations only (+, -, *, /, sqrt;
//             the library is built with -ffp-contract=off) and mc_logf_unit
//             for every log, so host and device give the same bits.  The one
//             exception is the power U^(1/alpha) of a Gamma shape below 1
//             (mc_expf_ref: a double exp rounded once; host and device may
//             differ in the last bit with philox.h's ~1e-8 probability).
//     Normal       loc + scale * z0,  z0 of mc_box_muller(w.x, w.y) (z1 is
//                  discarded: using it would tie two observations' draws)
//     HalfNormal   fabsf(scale * z0)
//     Exponential  -mc_logf_unit(mc_u01_boxf(w.x)) / rate
//     Gamma(a, b)  Marsaglia and Tsang (2000), "A simple method for generating
//                  gamma variables": d = a - 1/3, c = 1 / sqrt(9 d); per attempt
//                  one Philox block: x = z0 of (w.x, w.y), u = u01(w.z);
//                  v = (1 + c x)^3; accept when v > 0 and
//                  log u < x^2 / 2 + d (1 - v + log v)  (the exact test alone:
//                  the paper's squeeze only saves logs); the variate is d v.
//                  a < 1: Gamma(a + 1) U^(1/a), U = u01 of attempt 0's w.w.
//                  At most kPpAttempts attempts (each rejects with probability
//                  < 0.05), then NaN.  Divided by b.
//     Beta(a, b)   X / (X + Y), X ~ Gamma(a, 1), Y ~ Gamma(b, 1)
//   invalid    a scale, rate or shape that is <= 0 or NaN gives NaN (and a NaN
//              loc does): never a hang — the attempt loop has a compile-time
//              bound.
//
//   k_predictive<GB>  grid (tiles, B) on the pointwise view (pointwise.h PwCtx,
//                 tiles of <= 256 consecutive elements of one term), one
//                 observation per thread, its operands decoded once into
//                 registers as in k_pointwise.  Block b walks the processed
//                 draws [b * per, (b + 1) * per) of the C * S' processed draws
//                 (S' = ceil(S / thin): iterations 0, thin, 2 thin, ... of
//                 every chain; the counter carries the true iteration) and
//                 reads a draw's parameters from its row of the [C, S, D]
//                 buffer.  Per draw a thread forms its replicate, stores it
//                 when the caller passed a [C, S', M] buffer, and folds it
//                 into its partial: pw_moments' batch-of-8 two-pass moments
//                 and Chan's update over the FINITE replicates (non-finite
//                 ones are counted and kept apart), and the count of finite
//                 replicates below the observation (the term's value operand
//                 at that draw).  No LDS, no atomics, nothing between
//                 workgroups.  GB = true carries the Gamma / Beta rejection
//                 loop; GB = false (programs without such terms) does not.
//   k_pp_merge    one thread per observation merges the B partials in block
//                 order.
// B and the tiling depend on (C, S, thin, the program) only — never on the
// device — so two calls give the same bits, with or without the replicates.
//
// A partial is the five f64 fields of mcmc355.h (MC_PP_*): N draws processed,
// MEAN and M2 of the finite replicates (NaN when there is none), BELOW,
// NONFINITE.
#pragma once
#include "philox.h"
#include "mcmc355.h"

constexpr int kPpAttempts = 32;  // rejection attempts before a Gamma draw gives NaN

MC_HD float pp_nan() { return __builtin_nanf(""); }

// Gamma(a, 1), a > 0 (the caller has checked), attempts at sub0 + t.
MC_HD float pp_gamma_unit(float a, uint64_t seed, uint32_t chain, uint32_t iter, uint32_t sub0,
                          uint32_t obs) {
    const bool small = a < 1.0f;
    const float a1 = small ? a + 1.0f : a;
    const float d = a1 - 0x1.555556p-2f;  // f32(1/3)
    const float c = 1.0f / sqrtf(9.0f * d);
    float out = pp_nan();
    float boost = 1.0f;
#pragma unroll 1
    for (int t = 0; t < kPpAttempts; ++t) {
        const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, sub0 + (uint32_t)t, obs);
        if (t == 0 && small) boost = mc_expf_ref(mc_logf_unit(mc_u01_boxf(w.w)) / a);
        float x, x1;
        mc_box_muller(w.x, w.y, &x, &x1);
        const float t1 = 1.0f + c * x;
        if (!(t1 > 0.0f)) continue;
        const float v = t1 * t1 * t1;
        const float lu = mc_logf_unit(mc_u01_boxf(w.z));
        if (lu < 0.5f * x * x + d * (1.0f - v + mc_logf_unit(v))) {
            out = d * v;
            break;
        }
    }
    return small ? out * boost : out;
}

// The replicate of one observation: m = loc / alpha, s = scale / rate / beta.
// GB = false leaves Gamma and Beta (NaN) to the other instantiation.
template <bool GB>
MC_HD float pp_draw(int dist, float m, float s, uint64_t seed, uint32_t chain, uint32_t iter,
                    uint32_t obs) {
    if (dist == MC_DIST_NORMAL || dist == MC_DIST_HALFNORMAL || dist == MC_DIST_EXPONENTIAL) {
        if (!(s > 0.0f)) return pp_nan();
        const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, 0u, obs);
        if (dist == MC_DIST_EXPONENTIAL) return -mc_logf_unit(mc_u01_boxf(w.x)) / s;
        float z0, z1;
        mc_box_muller(w.x, w.y, &z0, &z1);
        return dist == MC_DIST_NORMAL ? m + s * z0 : fabsf(s * z0);
    }
    if constexpr (GB) {
        if (dist == MC_DIST_GAMMA || dist == MC_DIST_BETA) {
            if (!(m > 0.0f) || !(s > 0.0f)) return pp_nan();
            const float x = pp_gamma_unit(m, seed, chain, iter, 0u, obs);
            if (dist == MC_DIST_GAMMA) return x / s;
            const float y = pp_gamma_unit(s, seed, chain, iter, 0x100u, obs);
            return x / (x + y);
        }
    }
    return pp_nan();
}

#if defined(__HIPCC__)
#include "pointwise.h"

namespace mc {

enum { PP_N = 0, PP_MEAN, PP_M2, PP_BELOW, PP_NONFINITE, PP_COUNT };

// The processed draws of a launch: draw p = (c, k) is row c * S + k * thin of
// the sample buffer, chain c + chain0, iteration k * thin + iter0.
struct PpRun {
    int64_t S, Sp, thin, Np, per;
    uint64_t seed;
    uint32_t chain0, iter0;
};

template <bool GB>
__global__ __launch_bounds__(kPwBlock) void k_predictive(PwCtx P, PpRun R,
                                                         const float* __restrict__ samples,
                                                         double* __restrict__ part,
                                                         float* __restrict__ yrep) {
    const PwTile tile = P.tiles[blockIdx.x];
    const DevTerm T = load_term(cptr(P.terms) + __builtin_amdgcn_readfirstlane(tile.term));
    const int64_t i = tile.e0 + threadIdx.x;
    if (i >= T.n) return;  // (no barrier and no LDS below)
    const int64_t o = tile.o0 + threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.y * R.per;
    const int64_t p1 = p0 + R.per < R.Np ? p0 + R.per : R.Np;
    const int64_t D = P.D;

    const PwOp ov = pw_operand(T.op[0], i, P);
    const PwOp om = pw_operand(T.op[1], i, P);
    const PwOp os = pw_operand(T.op[2], i, P);
    const bool aff = T.affine != 0;
    PwOp ob = ov, ox = ov;
    if (aff) {
        ob = pw_operand(T.ab, i, P);
        ox = pw_operand(T.ax, i, P);
    }

    PwAcc A = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double nfsum = 0.0, below = 0.0;
    // (one division per block; the walk below steps (c, k) without one)
    int64_t c = p0 / R.Sp, k = p0 - c * R.Sp;
    for (int64_t p = p0; p < p1; p += kPwBatch) {
        const int kb = p1 - p < kPwBatch ? (int)(p1 - p) : kPwBatch;
        float x[kPwBatch];
#pragma unroll
        for (int j = 0; j < kPwBatch; ++j) x[j] = 0.0f;
#pragma unroll 1
        for (int b = 0; b < kb; ++b) {
            const int64_t s = k * R.thin;
            const float* __restrict__ q = samples + (c * R.S + s) * D;
            const float v = pw_value(ov, q);
            float m = pw_value(om, q);
            if (aff) m = m + pw_value(ob, q) * pw_value(ox, q);
            const float sc = pw_value(os, q);
            const float y = pp_draw<GB>(T.dist, m, sc, R.seed, R.chain0 + (uint32_t)c,
                                        R.iter0 + (uint32_t)s, (uint32_t)o);
            if (yrep) yrep[(p + b) * P.M + o] = y;
            // (a non-finite y compares false or is dropped here: BELOW counts
            // finite replicates only)
            if (y - y == 0.0f && y < v) below += 1.0;
#pragma unroll
            for (int j = 0; j + 1 < kPwBatch; ++j) x[j] = x[j + 1];
            x[kPwBatch - 1] = y;
            if (++k == R.Sp) {
                k = 0;
                ++c;
            }
        }
        pw_moments(A, nfsum, x, kb);
    }
    if (A.n == 0.0) A.mean = A.m2 = __builtin_nan("");
    double* out = part + (int64_t)blockIdx.y * PP_COUNT * P.M + o;
    out[PP_N * P.M] = A.n + A.nf;
    out[PP_MEAN * P.M] = A.mean;
    out[PP_M2 * P.M] = A.m2;
    out[PP_BELOW * P.M] = below;
    out[PP_NONFINITE * P.M] = A.nf;
}

// stats[f * M + o] from the B partials of observation o, in block order:
// Chan's update over the finite counts (a side without finite replicates
// leaves the other's moments), counts added.
static __global__ __launch_bounds__(256) void k_pp_merge(const double* __restrict__ part,
                                                         int64_t M, int32_t B,
                                                         double* __restrict__ stats) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M) return;
    const double* p = part + o;
    double n = p[PP_N * M], mean = p[PP_MEAN * M], m2 = p[PP_M2 * M], below = p[PP_BELOW * M],
           nf = p[PP_NONFINITE * M];
    for (int b = 1; b < B; ++b) {
        p = part + (int64_t)b * PP_COUNT * M + o;
        const double bn = p[PP_N * M], bnf = p[PP_NONFINITE * M];
        const double na = n - nf, nb = bn - bnf;
        if (nb > 0.0) {
            if (na > 0.0) {
                const double d = p[PP_MEAN * M] - mean;
                const double r = 1.0 / (na + nb);
                mean += d * (nb * r);
                m2 += p[PP_M2 * M] + d * d * (na * nb * r);
            } else {
                mean = p[PP_MEAN * M];
                m2 = p[PP_M2 * M];
            }
        }
        n += bn;
        nf += bnf;
        below += p[PP_BELOW * M];
    }
    stats[PP_N * M + o] = n;
    stats[PP_MEAN * M + o] = mean;
    stats[PP_M2 * M + o] = m2;
    stats[PP_BELOW * M + o] = below;
    stats[PP_NONFINITE * M + o] = nf;
}

}  // namespace mc
#endif  // __HIPCC__
