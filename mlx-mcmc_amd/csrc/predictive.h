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
//   count terms  an expression term whose root is a count node of eval.h
//             (MC_EX_BERNOULLI_LOGIT_LP / MC_EX_BINOMIAL_LOGIT_LP /
//             MC_EX_POISSON_LOG_LP), or ADD(that node, a CONST / DATA leaf),
//             has a sampling distribution (internal.h PwSampler, recorded at
//             program creation): per draw the term's nodes below the count
//             node are evaluated (pw_expr_walk: eta / theta, n and the
//             observed y are node values) and pp_draw_discrete draws the
//             replicate.  Exact samplers, no normal approximation; every loop
//             has a compile-time bound and exhaustion gives NaN.  Their
//             uniforms are u(w) = (w + 1/2) 2^-32 in double (mc_u01_f64):
//             resolution 2^-32, so an inversion cannot return an outcome
//             beyond the 1 - 2^-33 quantile.  exp and log are pp_exp / pp_log
//             below: double, from +, -, *, /, rint, frexp and ldexp alone, so
//             host and device take the same decisions.
//     Bernoulli(eta)    y = [log u - log(1 - u) < eta], u = mc_u01_boxf(w.x)
//                  (24-bit significand: 1 - u has resolution 2^-24; u rounds
//                  to 1 with probability 2^-25 and then y = 0), both logs
//                  mc_logf_unit: no exponential.  NaN eta: NaN.
//     Poisson(theta)    lambda = pp_exp(theta); NaN when lambda is NaN or
//                  >= 2^23 (an f32 count is no longer exact), 0 when lambda
//                  is 0.  lambda < 10: sequential search from 0 on u(w.x) of
//                  attempt 0 through p_0 = exp(-lambda), p_k = p_(k-1)
//                  lambda / k (at most kPpInvMax terms).  Else Hormann's PTRS
//                  ("The transformed rejection method for generating Poisson
//                  random variables", 1993): b = 0.931 + 2.53 sqrt(lambda),
//                  a = -0.059 + 0.02483 b, 1/alpha = 1.1239 + 1.1328 / (b -
//                  3.4), vr = 0.9277 - 3.6224 / (b - 2); per attempt U = u(w.x)
//                  - 1/2, V = u(w.y), us = 1/2 - |U|, k = floor((2 a / us + b)
//                  U + lambda + 0.43); accept when us >= 0.07 and V <= vr;
//                  reject when k < 0 or (us < 0.013 and V > us); else accept
//                  when log(V / alpha / (a / us^2 + b)) <= k log lambda -
//                  lambda - log k!.
//     Binomial(n, eta)  NaN for a NaN eta and for n negative, non-integer or
//                  >= 2^23.  e = pp_exp(-|eta|), q = 1 / (1 + e), p = e q =
//                  min(sigma(eta), 1 - sigma(eta)); the count k of the rarer
//                  outcome is drawn and reflected (n - k) when eta > 0.
//                  n p < 10: sequential search from 0 on u(w.x) through p_0 =
//                  q^n, p_(k+1) = p_k e (n - k) / (k + 1) (k = n ends it).
//                  Else Hormann's BTRS ("The generation of binomial random
//                  variates", 1993): s = sqrt(n p q), b = 1.15 + 2.53 s, a =
//                  -0.0873 + 0.0248 b + 0.01 p, c = n p + 1/2, vr = 0.92 -
//                  4.2 / b, alpha = (2.83 + 5.1 / b) s, m = floor((n + 1) p);
//                  per attempt U, V, us as above, k = floor((2 a / us + b) U
//                  + c); accept when us >= 0.07 and V <= vr; reject when k < 0
//                  or k > n; else accept when log(V alpha / (a / us^2 + b)) <=
//                  log m! + log (n - m)! - log k! - log (n - k)! + (k - m)
//                  log(p / q), log(p / q) = -|eta|.
//     log k!       a table below 10, else Stirling's series of lgamma(k + 1)
//                  to the 1 / x^7 term (error below 1e-12).
//     At most kPpAttempts attempts (PTRS and BTRS accept more than two in
//     three), then NaN.
//
//   Student-t terms  an expression term whose root is MC_EX_STUDENT_T_LP /
//             MC_EX_HALF_STUDENT_T_LP, or ADD(that node, a CONST / DATA leaf),
//             is recorded and walked as the count terms are (PwSampler kinds
//             PW_SAMPLER_STUDENT_T / PW_SAMPLER_HALF_STUDENT_T, nu in the
//             descriptor); value, loc and scale are node values at the draw.
//             pp_student_t, f32 IEEE operations and the samplers above only —
//             the same function on host and device — one rule for every nu,
//             Cauchy (nu = 1) included:
//               NaN when !(s > 0), !(nu > 0) or m is NaN
//               z0 = the first normal of mc_box_muller(w.x, w.y), attempt 0
//               g  = pp_gamma_unit(nu / 2) on sub = 0x100 + attempt (Beta's
//                    second-Gamma range; NaN when its attempts are exhausted)
//               t  = z0 / sqrt(g / (nu / 2))
//               Student-t: m + s t        half form: |s t|
//             (a normal over the root of an independent chi-square over its
//             degrees of freedom).  For nu < 2 the Gamma shape nu / 2 is below
//             1, so the mc_expf_ref caveat above applies: host and device may
//             differ in the last bit with philox.h's ~1e-8 probability, as for
//             Gamma today.  These terms are not count terms: they run the
//             NMAX kernel but add no ties (mc_program_num_count_terms).
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
//                 NMAX = 16 / 32 (programs with count terms of up to that many
//                 nodes, or a caller that asks for the ties) adds the count
//                 terms' path and EQUAL, the finite replicates equal to the
//                 observation (a sixth f64 per observation, kept apart from
//                 the five fields); NMAX = 0 is the kernel without either.
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

// ---- count samplers ------------------------------------------------------
constexpr int kPpInvMax = 128;  // terms of a sequential search (means below 10)

// exp(x) in double from IEEE operations: x = k ln 2 + r, |r| <= ln 2 / 2,
// Taylor's series of exp(r) to r^13 (4e-18), scaled by 2^k.  0 below -700,
// +inf above 700, NaN for NaN.
MC_HD double pp_exp(double x) {
    if (x != x) return x;
    if (x < -700.0) return 0.0;
    if (x > 700.0) return (double)__builtin_inff();
    const double k = rint(x * 1.4426950408889634);
    const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return ldexp(p, (int)k);
}
// log(x) in double, x positive, finite and normal: x = m 2^k, m in [sqrt(2) / 2,
// sqrt(2)), s = (m - 1) / (m + 1), log m = 2 atanh(s) to s^25 (1e-20).
MC_HD double pp_log(double x) {
    int k;
    double m = frexp(x, &k);
    if (m < 0.70710678118654752) {
        m = m * 2.0;
        k -= 1;
    }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = 1.0 / 25.0;
    p = p * z + 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    const double dk = (double)k;
    return dk * 6.93147180369123816490e-01 + (dk * 1.90821492927058770002e-10 + 2.0 * s * p);
}
// log k!, k a non-negative integer value.
MC_HD double pp_logfact(double k) {
    if (k < 10.0) {
        const int j = (int)k;
        return j < 2 ? 0.0
             : j == 2 ? 0.693147180559945309
             : j == 3 ? 1.791759469228055001
             : j == 4 ? 3.178053830347945620
             : j == 5 ? 4.787491742782045994
             : j == 6 ? 6.579251212010100995
             : j == 7 ? 8.525161361065414300
             : j == 8 ? 10.60460290274525023
                      : 12.80182748008146961;
    }
    const double x = k + 1.0;
    const double r = 1.0 / x, r2 = r * r;
    const double c = r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
    return ((x - 0.5) * pp_log(x) - x) + (0.918938533204672742 + c);
}

MC_HD float pp_bernoulli(float eta, uint64_t seed, uint32_t chain, uint32_t iter, uint32_t obs) {
    if (eta != eta) return pp_nan();
    const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, 0u, obs);
    const float u = mc_u01_boxf(w.x);
    const float um = 1.0f - u;
    if (!(um > 0.0f)) return 0.0f;  // (the logit of u = 1 is +inf)
    return (mc_logf_unit(u) - mc_logf_unit(um) < eta) ? 1.0f : 0.0f;
}

MC_HD float pp_poisson(float theta, uint64_t seed, uint32_t chain, uint32_t iter, uint32_t obs) {
    const double lam = pp_exp((double)theta);
    if (!(lam < 8388608.0)) return pp_nan();
    if (lam == 0.0) return 0.0f;
    float out = pp_nan();
    if (lam < 10.0) {
        const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, 0u, obs);
        const double u = mc_u01_f64(w.x);
        double pk = pp_exp(-lam), F = pk;
#pragma unroll 1
        for (int k = 0; k < kPpInvMax; ++k) {
            if (u <= F) {
                out = (float)k;
                break;
            }
            pk = pk * lam / (double)(k + 1);
            F += pk;
        }
        return out;
    }
    const double slam = sqrt(lam), loglam = pp_log(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
#pragma unroll 1
    for (int t = 0; t < kPpAttempts; ++t) {
        const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, (uint32_t)t, obs);
        const double U = mc_u01_f64(w.x) - 0.5, V = mc_u01_f64(w.y);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) {
            out = (float)k;
            break;
        }
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if (pp_log(V * invalpha / (a / (us * us) + b)) <= (k * loglam - lam) - pp_logfact(k)) {
            out = (float)k;
            break;
        }
    }
    return out;
}

MC_HD float pp_binomial(float nf, float eta, uint64_t seed, uint32_t chain, uint32_t iter,
                        uint32_t obs) {
    if (!(nf >= 0.0f) || !(nf < 8388608.0f) || nf != floorf(nf) || eta != eta) return pp_nan();
    const double n = (double)nf;
    const double ae = fabs((double)eta);
    const double e = pp_exp(-ae);  // p / q of the rarer outcome
    const double q = 1.0 / (1.0 + e), p = e * q;
    double kk = -1.0;
    if (n * p < 10.0) {
        const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, 0u, obs);
        const double u = mc_u01_f64(w.x);
        double pk = pp_exp(n * pp_log(q)), F = pk;
#pragma unroll 1
        for (int k = 0; k < kPpInvMax; ++k) {
            const double dk = (double)k;
            if (u <= F || dk >= n) {
                kk = dk;
                break;
            }
            pk = pk * e * ((n - dk) / (dk + 1.0));
            F += pk;
        }
    } else {
        const double spq = sqrt(n * p * q);
        const double b = 1.15 + 2.53 * spq;
        const double a = -0.0873 + 0.0248 * b + 0.01 * p;
        const double c = n * p + 0.5;
        const double vr = 0.92 - 4.2 / b;
        const double alpha = (2.83 + 5.1 / b) * spq;
        const double m = floor((n + 1.0) * p);
        const double hm = pp_logfact(m) + pp_logfact(n - m);
#pragma unroll 1
        for (int t = 0; t < kPpAttempts; ++t) {
            const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, (uint32_t)t, obs);
            const double U = mc_u01_f64(w.x) - 0.5, V = mc_u01_f64(w.y);
            const double us = 0.5 - fabs(U);
            const double k = floor((2.0 * a / us + b) * U + c);
            if (k < 0.0 || k > n) continue;
            if (us >= 0.07 && V <= vr) {
                kk = k;
                break;
            }
            if (pp_log(V * alpha / (a / (us * us) + b)) <=
                ((hm - pp_logfact(k)) - pp_logfact(n - k)) - (k - m) * ae) {
                kk = k;
                break;
            }
        }
    }
    if (kk < 0.0) return pp_nan();
    return (float)(eta > 0.0f ? n - kk : kk);
}

// The replicate of one observation of a count term: kind an mc_discrete_kind,
// eta the logit / log rate, total the Binomial's n.
MC_HD float pp_draw_discrete(int kind, float total, float eta, uint64_t seed, uint32_t chain,
                             uint32_t iter, uint32_t obs) {
    if (kind == MC_DISCRETE_BERNOULLI) return pp_bernoulli(eta, seed, chain, iter, obs);
    if (kind == MC_DISCRETE_BINOMIAL) return pp_binomial(total, eta, seed, chain, iter, obs);
    if (kind == MC_DISCRETE_POISSON) return pp_poisson(eta, seed, chain, iter, obs);
    return pp_nan();
}

// The replicate of one observation of a Student-t term (header comment above):
// m + s t or |s t| with t = z0 / sqrt(g / (nu / 2)), g ~ Gamma(nu / 2, 1).
MC_HD float pp_student_t(float nu, float m, float s, bool half, uint64_t seed, uint32_t chain,
                         uint32_t iter, uint32_t obs) {
    if (!(s > 0.0f) || !(nu > 0.0f) || m != m) return pp_nan();
    const mc_u32x4 w = mc_draw(seed, chain, iter, MC_RNG_TAG_PREDICT, 0u, obs);
    float z0, z1;
    mc_box_muller(w.x, w.y, &z0, &z1);
    const float a = 0.5f * nu;
    const float g = pp_gamma_unit(a, seed, chain, iter, 0x100u, obs);
    const float t = z0 / sqrtf(g / a);
    return half ? fabsf(s * t) : m + s * t;
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

template <bool GB, int NMAX>
__global__ __launch_bounds__(kPwBlock) void k_predictive(PwCtx P, PpRun R,
                                                         const float* __restrict__ samples,
                                                         double* __restrict__ part,
                                                         float* __restrict__ yrep,
                                                         const PwSampler* __restrict__ samp,
                                                         double* __restrict__ eqpart) {
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

    // a count term (wave-uniform, as the tile's term): its sampler
    PwSampler sd = kPwNoSampler;
    if constexpr (NMAX > 0) {
        if (T.dist == MC_DIST_EXPR) {
            const MC_CONST PwSampler* sp = cptr(samp) + __builtin_amdgcn_readfirstlane(tile.term);
            sd.kind = sp->kind;
            sd.node = sp->node;
            sd.y = sp->y;
            sd.tot = sp->tot;
            sd.eta = sp->eta;
            sd.nu = sp->nu;
        }
    }

    PwAcc A = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double nfsum = 0.0, below = 0.0;
    [[maybe_unused]] double equal = 0.0;
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
            float v = 0.0f, y = 0.0f;
            bool count_term = false;
            if constexpr (NMAX > 0) count_term = sd.kind >= 0;
            if (count_term) {
                if constexpr (NMAX > 0) {
                    float val[NMAX];
                    pw_expr_walk<NMAX>(T, P, q, i, sd.node, val);
                    v = val[sd.y];
                    const float tot = sd.tot >= 0 ? val[sd.tot] : 0.0f;
                    if (sd.kind >= PW_SAMPLER_STUDENT_T)
                        y = pp_student_t(sd.nu, tot, val[sd.eta],
                                         sd.kind == PW_SAMPLER_HALF_STUDENT_T, R.seed,
                                         R.chain0 + (uint32_t)c, R.iter0 + (uint32_t)s,
                                         (uint32_t)o);
                    else
                        y = pp_draw_discrete(sd.kind, tot, val[sd.eta], R.seed,
                                             R.chain0 + (uint32_t)c, R.iter0 + (uint32_t)s,
                                             (uint32_t)o);
                }
            } else {
                v = pw_value(ov, q);
                float m = pw_value(om, q);
                if (aff) m = m + pw_value(ob, q) * pw_value(ox, q);
                const float sc = pw_value(os, q);
                y = pp_draw<GB>(T.dist, m, sc, R.seed, R.chain0 + (uint32_t)c,
                                R.iter0 + (uint32_t)s, (uint32_t)o);
            }
            if (yrep) yrep[(p + b) * P.M + o] = y;
            // (a non-finite y compares false or is dropped here: BELOW and
            // EQUAL count finite replicates only)
            if (y - y == 0.0f && y < v) below += 1.0;
            if constexpr (NMAX > 0) {
                if (y - y == 0.0f && y == v) equal += 1.0;
            }
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
    if constexpr (NMAX > 0) {
        if (eqpart) eqpart[(int64_t)blockIdx.y * P.M + o] = equal;
    }
}

// stats[f * M + o] from the B partials of observation o, in block order:
// Chan's update over the finite counts (a side without finite replicates
// leaves the other's moments), counts added.
static __global__ __launch_bounds__(256) void k_pp_merge(const double* __restrict__ part,
                                                         int64_t M, int32_t B,
                                                         double* __restrict__ stats,
                                                         const double* __restrict__ eqpart,
                                                         double* __restrict__ equal) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M) return;
    if (equal) {  // (counts: exact in any order)
        double e = 0.0;
        for (int b = 0; b < B; ++b) e += eqpart[(int64_t)b * M + o];
        equal[o] = e;
    }
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
