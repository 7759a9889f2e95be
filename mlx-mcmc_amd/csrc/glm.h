// glm.h — design-matrix GLMs: eta = X beta [+ intercept] [+ offset] under a
// Normal, Bernoulli-logit or Poisson-log likelihood (include/mcmc355.h mc_glm).
//
// Every other kernel here gives a chain its own workgroup or lanes; on a dense
// X[N, P] that re-reads X once per chain per leapfrog step.  Here 32 chains
// are the N dimension of two FP32 MFMA products (v_mfma_f32_32x32x2_f32):
//     eta[rows, 32 chains] = X[rows, P] . B[P, 32]      (forward)
//     G[P, 32 chains]     += X^T[P, rows] . R[rows, 32] (backward)
// so X is read once per block of 32 chains and the matrix pipe does the
// multiply-adds.
//
// k_glm_grad<FAM, PT>: grid (S row slices, chain blocks), 4 waves; a wave walks
// the 32-row tiles w, w + 4, ... of its slice.
//   operands   A (32 x 2): lane l holds A[l % 32][l / 32]; B (2 x 32): lane l
//              holds B[l / 32][l % 32]; the 32 x 32 accumulator: register v of
//              lane l holds row 8 (v / 4) + 4 (l / 32) + v % 4, column l % 32.
//   forward    A from X^T (stored as well as X: lane l reads row tile + l % 32
//              of column 2k + l / 32, 32 consecutive floats per half wave), B
//              from the block's coefficients in LDS ([Pp][32], staged once).
//   elementwise in the accumulator layout: + intercept, + offset, then the
//              family's device function of eval.h (ex_normal, ex_bernoulli_lp,
//              ex_poisson_lp and the cotangent factors the tape applies), giving
//              l and r = dl / d eta; rows past N give 0.
//   backward   accumulator register v of r IS a B operand (its k = 0 half is
//              row 8 (v / 4) + v % 4, its k = 1 half the row 4 below), so each
//              register feeds one MFMA per 32-wide coefficient tile with A =
//              X[those two rows][tile + l % 32] from the row-major X: no
//              shuffle, no LDS.  G stays in PT x 16 accumulator registers per
//              lane for the whole launch (PT = Pp / 32 <= 8: P <= 256;
//              glm_wide.h splits G's columns over the waves instead and
//              takes P <= 1024 on the same partial block).
//   output     the waves add G through LDS in wave order (the coefficient
//              buffer, free by then) and the workgroup writes one partial
//              block [Pp + 4][32] to its slot (slice, chain block): rows Pp,
//              Pp + 1, Pp + 2 hold sum r (the intercept's cotangent), the
//              scale's cotangent and l.  No atomics, no cross-workgroup waits.
// X, X^T, y and the offset are stored zero-padded to multiples of 32 rows and
// Pp columns, so ragged edges are zero operands and nothing reads past an array.
//
// k_glm_hmc_step: one workgroup per chain block adds the S partials in slice
// order, adds the priors (elem_eval) and performs one phase of k_hmc's
// iteration (hmc.h) on positions and momenta kept chain-minor in the
// workspace: the same Philox block and word per (seed, chain, iteration,
// element), the same f32 products per element, accept rule, step-size rule and
// NaN handling.  A chain is one MFMA column and columns never mix, so its
// draws do not depend on how chains are split over blocks, launches or GPUs.
#pragma once
#include "eval.h"
#include "internal.h"
#include "philox.h"

namespace mc {

constexpr int kGlmChains = 32;  // chains per block: the MFMA tile's N dimension
constexpr int kGlmExtra = 4;    // rows of a partial block after the Pp of G
constexpr int kGlmStripes = 8;  // k_glm_hmc_step: threads per chain

struct GlmPrior {
    int32_t dist, poff, n, xf;
    float weight, c0, m, s, logs, lg;
};

struct GlmDev {
    const float* X;    // [Np][Pp] row-major, zero-padded
    const float* XT;   // [Pp][Np]
    const float* y;    // [Np]
    const float* off;  // [Np] or null
    const GlmPrior* priors;
    int32_t n_priors, family;
    int32_t N, P, Np, Pp, NT;  // NT = Np / 32 row tiles
    int32_t D, boff;
    int32_t ik, ipoff;  // intercept: MC_OP_NONE / CONST / PSCALAR
    float ival;
    int32_t sk, spoff, sxf;  // scale (normal family): CONST / PSCALAR
    float sval;
    float c0;  // normal: -0.5 log(2 pi)
    float lp_const;
    // MC_GLM_CATEGORICAL_LOGIT (glm_softmax.h): K classes padded to Kp (a power of
    // two), CPB = 32 / Kp chains per gradient block; B[p, k] is parameter boff +
    // p K + k, the class intercepts aoff .. aoff + K (aoff < 0: none)
    int32_t K, Kp, CPB, aoff;
};

typedef float glm_acc __attribute__((ext_vector_type(16)));

// Positions are addressed as q[cb * 32 * D + j * sc + d * sp] for chain j of
// block cb, parameter d: (sc, sp) = (D, 1) for a row-major [C][D] array,
// (1, 32) for the chain-minor workspace copy.
template <int FAM, int PT>
__global__ void __launch_bounds__(256)
k_glm_grad(GlmDev G, const float* q, int sc, int sp, int64_t C, int S, float* part) {
    extern __shared__ __attribute__((aligned(16))) float coef[];  // [PT * 32][32]
    __shared__ float ex[3][kGlmChains];
    const int s = blockIdx.x, cb = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const float* qb = q + (int64_t)cb * kGlmChains * G.D;
    for (int e = tid; e < PT * 1024; e += 256) {
        const int p = e >> 5, jj = e & 31;
        const bool ok = p < G.P && (int64_t)cb * kGlmChains + jj < C;
        coef[e] = ok ? qb[(int64_t)jj * sc + (int64_t)(G.boff + p) * sp] : 0.0f;
    }
    const bool live = (int64_t)cb * kGlmChains + j < C;
    float icpt = 0.0f, scale = 1.0f, logs = 0.0f;
    if (G.ik == MC_OP_CONST) icpt = G.ival;
    else if (G.ik == MC_OP_PSCALAR && live) icpt = qb[(int64_t)j * sc + (int64_t)G.ipoff * sp];
    if constexpr (FAM == MC_GLM_NORMAL) {
        if (G.sk == MC_OP_CONST) scale = G.sval;
        else if (live) scale = xf_apply(G.sxf, qb[(int64_t)j * sc + (int64_t)G.spoff * sp]);
        logs = ex_log(scale);
    }
    __syncthreads();

    glm_acc acc[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[pt][v] = 0.0f;
    float sl = 0.0f, sr = 0.0f, sd = 0.0f;
    const int t0 = (int)((int64_t)s * G.NT / S), t1 = (int)((int64_t)(s + 1) * G.NT / S);
    for (int t = t0 + wave; t < t1; t += 4) {
        const int row0 = t * 32;
        // forward: eta[32 rows][32 chains] over the Pp coefficients, two per MFMA
        glm_acc eta;
#pragma unroll
        for (int v = 0; v < 16; ++v) eta[v] = 0.0f;
        const float* xt = G.XT + (int64_t)h * G.Np + row0 + j;
        const float* bc = coef + h * 32 + j;
#pragma unroll 8
        for (int k = 0; k < PT * 16; ++k)
            eta = __builtin_amdgcn_mfma_f32_32x32x2f32(xt[(int64_t)(2 * k) * G.Np], bc[k * 64], eta,
                                                       0, 0, 0);
        // elementwise, in the accumulator layout
        glm_acc r;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int rb = row0 + 8 * g4 + 4 * h;
            const float4 yv = *reinterpret_cast<const float4*>(G.y + rb);
            float4 ov = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (G.off) ov = *reinterpret_cast<const float4*>(G.off + rb);
            const float ys[4] = {yv.x, yv.y, yv.z, yv.w};
            const float os[4] = {ov.x, ov.y, ov.z, ov.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int v = 4 * g4 + u;
                float e = eta[v] + icpt;
                if (G.off) e = e + os[u];
                const float yy = ys[u];
                float lp, rr, ds = 0.0f;
                if constexpr (FAM == MC_GLM_NORMAL) {
                    const ElemOut o = ex_normal(G.c0, yy, e, scale, logs);
                    lp = o.lp;
                    rr = o.dm;
                    ds = o.ds;
                } else if constexpr (FAM == MC_GLM_BERNOULLI_LOGIT) {
                    lp = ex_bernoulli_lp(yy, e);
                    rr = ex_bernoulli_in(yy) ? yy - ex_sigmoid(e) : 0.0f;
                } else {
                    lp = ex_poisson_lp(yy, e);
                    rr = ex_is_count(yy) ? yy - ex_exp(e) : 0.0f;
                }
                const bool in = rb + u < G.N;
                lp = in ? lp : 0.0f;
                rr = in ? rr : 0.0f;
                ds = in ? ds : 0.0f;
                sl += lp;
                sr += rr;
                sd += ds;
                r[v] = rr;
            }
        }
        // backward: G[tile pt] += X[two rows of register v][tile pt]^T . r_v
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float* xr = G.X + (int64_t)(row0 + 8 * (v / 4) + (v % 4) + 4 * h) * G.Pp + j;
#pragma unroll
            for (int pt = 0; pt < PT; ++pt)
                acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(xr[pt * 32], r[v], acc[pt], 0, 0, 0);
        }
    }

    // the waves' sums, added in wave order through LDS (the coefficients are done)
    sl = sl + __shfl_xor(sl, 32);
    sr = sr + __shfl_xor(sr, 32);
    sd = sd + __shfl_xor(sd, 32);
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int pt = 0; pt < PT; ++pt)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int o = (pt * 32 + 8 * (v / 4) + 4 * h + (v % 4)) * 32 + j;
                    coef[o] = (w == 0) ? acc[pt][v] : coef[o] + acc[pt][v];
                }
            if (h == 0) {
                ex[0][j] = (w == 0) ? sr : ex[0][j] + sr;
                ex[1][j] = (w == 0) ? sd : ex[1][j] + sd;
                ex[2][j] = (w == 0) ? sl : ex[2][j] + sl;
            }
        }
        __syncthreads();
    }
    float* out = part + ((int64_t)s * gridDim.y + cb) * (int64_t)((PT * 32 + kGlmExtra) * 32);
    for (int e = tid; e < PT * 1024; e += 256) out[e] = coef[e];
    if (tid < 3 * kGlmChains) out[PT * 1024 + tid] = ex[tid >> 5][tid & 31];
}

// ---- the reduce over slices and the priors, per (chain, parameter) ------------
struct GlmPart {
    const float* part;  // slot (slice 0, this chain block)
    int64_t stride;     // floats between the slices of a chain block
    int S;
    int col;            // softmax: the chain's first column (class 0) in its block
};

MC_DEV float glm_part_sum(const GlmPart& R, int row, int j) {
    float x = 0.0f;
    for (int s = 0; s < R.S; ++s) x += R.part[s * R.stride + row * 32 + j];
    return x;
}

// The partials of chain c = 32 cb + j of a launch: the chain block's slot, or
// for a softmax program (glm_softmax.h: CPB chains per gradient block, class-
// minor columns) the slot of gradient block c / CPB and the chain's first column.
MC_DEV GlmPart glm_part_of(const GlmDev& G, GlmPart R, int cb, int64_t c) {
    const int64_t blk = (int64_t)(G.Pp + kGlmExtra) * 32;
    if (G.family == MC_GLM_CATEGORICAL_LOGIT) {
        R.part += (c / G.CPB) * blk;
        R.col = (int)(c % G.CPB) * G.Kp;
    } else {
        R.part += (int64_t)cb * blk;
    }
    return R;
}

// the chain's log likelihood: row Pp + 2 of its column, or of its K class columns
// in class order
MC_DEV float glm_part_lp(const GlmDev& G, const GlmPart& R, int j) {
    if (G.family != MC_GLM_CATEGORICAL_LOGIT) return glm_part_sum(R, G.Pp + 2, j);
    float l = 0.0f;
    for (int k = 0; k < G.K; ++k) l += glm_part_sum(R, G.Pp + 2, R.col + k);
    return l;
}

// d log likelihood / d q[d] of chain j (qd = q[d])
MC_DEV float glm_like_grad(const GlmDev& G, const GlmPart& R, int j, int d, float qd) {
    if (G.family == MC_GLM_CATEGORICAL_LOGIT) {
        const int e = d - G.boff, a = d - G.aoff;
        if (e >= 0 && e < G.P * G.K) return glm_part_sum(R, e / G.K, R.col + e % G.K);
        if (G.aoff >= 0 && a >= 0 && a < G.K) return glm_part_sum(R, G.Pp, R.col + a);
        return 0.0f;
    }
    float g = 0.0f;
    if (d >= G.boff && d < G.boff + G.P) g += glm_part_sum(R, d - G.boff, j);
    if (G.ik == MC_OP_PSCALAR && d == G.ipoff) g += glm_part_sum(R, G.Pp, j);
    if (G.family == MC_GLM_NORMAL && G.sk == MC_OP_PSCALAR && d == G.spoff)
        g += xf_chain(G.sxf, glm_part_sum(R, G.Pp + 1, j), qd, xf_apply(G.sxf, qd));
    return g;
}

MC_DEV void glm_prior(const GlmDev& G, int d, float qd, float& g, float& lp) {
    for (int t = 0; t < G.n_priors; ++t) {
        const GlmPrior T = G.priors[t];
        if (d < T.poff || d >= T.poff + T.n) continue;
        const float v = xf_apply(T.xf, qd);
        const ElemOut e = elem_eval(T.dist, T.c0, v, T.m, T.s, T.logs, T.lg);
        lp += T.weight * e.lp;
        g += xf_chain(T.xf, T.weight * e.dv, qd, v);
    }
}

// the sum of x over the 8 threads of a chain, in stripe order
MC_DEV float glm_chain_sum(float x, float (*red)[kGlmChains], int pr, int j) {
    red[pr][j] = x;
    __syncthreads();
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < kGlmStripes; ++k) s += red[k][j];
    __syncthreads();
    return s;
}

// The thread layout of the kernels below: 256 threads per chain block, thread
// (j = tid % 32: the chain, pr = tid / 32) owns the parameters of the Philox
// momentum blocks m = pr, pr + 8, ...: elements 4 m .. 4 m + 3.
#define GLM_FOR_OWNED(D)                              \
    for (int m_ = pr; 4 * m_ < (D); m_ += kGlmStripes) \
        for (int k_ = 0, d = 4 * m_; k_ < 4 && d < (D); ++k_, ++d)

// mc_logp_grad / mc_state_init: the gradient kernel's partials to log p and
// its gradient at the row-major points q (INIT: and the chain state).
template <bool INIT>
__global__ void __launch_bounds__(256)
k_glm_finish(GlmDev G, int64_t C, const float* q, GlmPart R0, float* logp, float* grad,
             double eps0, float mu, mc_chain_scalars* scal, float* st_q) {
    __shared__ float red[kGlmStripes][kGlmChains];
    const int cb = blockIdx.x, j = threadIdx.x & 31, pr = threadIdx.x >> 5;
    const int64_t c = (int64_t)cb * kGlmChains + j;
    const bool live = c < C;
    const int D = G.D;
    const GlmPart R = glm_part_of(G, R0, cb, c);
    float lpp = 0.0f;
    if (live) {
        GLM_FOR_OWNED(D) {
            const float qd = q[c * D + d];
            float g = glm_like_grad(G, R, j, d, qd);
            glm_prior(G, d, qd, g, lpp);
            grad[c * D + d] = g;
            if constexpr (INIT) st_q[c * D + d] = qd;
        }
    }
    const float lps = glm_chain_sum(lpp, red, pr, j);
    if (live && pr == 0) {
        const float lp = (G.lp_const + glm_part_lp(G, R, j)) + lps;
        if constexpr (INIT) {
            mc_chain_scalars sc = {};
            sc.step_size = eps0;
            sc.step_size_bar = 1.0;
            sc.h_bar = 0.0;
            sc.mu = mu;
            sc.logp = lp;
            sc.n_grad = 1;
            scal[c] = sc;
        } else {
            logp[c] = lp;
        }
    }
}

// One phase of an HMC iteration (hmc.h k_hmc's operations per element):
//   0  iteration start: momentum draw, H_init, first half kick, drift
//   1  interior: second half kick of the step before, first of the next, drift
//   2  iteration end: last half kick, H, accept / reject, step-size rule,
//      counters, trace and sample
// Phases 1 and 2 read the partials of the gradient launch before them.  qT / pT
// are the proposal and its momentum, chain-minor: [chain block][D][32].
enum { GLM_START = 0, GLM_INTERIOR = 1, GLM_END = 2 };

template <int = 0>  // (a template so that every unit including this header may)
__global__ void __launch_bounds__(256)
k_glm_hmc_step(GlmDev G, RunArgs A, int phase, int64_t it, mc_chain_scalars* scal, float* st_q,
               float* st_g, float* samples, TraceDev tr, float* qT, float* pT, float* H0,
               GlmPart R0) {
    __shared__ float red[kGlmStripes][kGlmChains];
    const mc_run_config& cfg = A.cfg;
    const int cb = blockIdx.x, j = threadIdx.x & 31, pr = threadIdx.x >> 5;
    const int64_t c = (int64_t)cb * kGlmChains + j;
    const bool live = c < cfg.num_chains;
    const int D = G.D;
    const int L = cfg.num_leapfrog_steps;
    float* qt = qT + (int64_t)cb * D * 32 + j;  // element d at qt[d * 32]
    float* pt = pT + (int64_t)cb * D * 32 + j;
    const GlmPart R = glm_part_of(G, R0, cb, c);
    const double eps = live ? scal[c].step_size : 0.0;
    const float lp = live ? scal[c].logp : 0.0f;  // (read before thread 0 of the chain updates it)
    const float h = (float)(0.5 * eps);
    const float e = (float)eps;
    const uint32_t chain_id = (uint32_t)(cfg.chain_offset + c);

    if (phase == GLM_START) {
        float kp = 0.0f;
        if (live) {
            for (int m = pr; 4 * m < D; m += kGlmStripes) {
                const mc_u32x4 r = mc_draw(cfg.seed, chain_id, (uint32_t)it, MC_RNG_TAG_MOMENTUM,
                                           0, (uint32_t)m);
                float z[4];
                mc_box_muller(r.x, r.y, &z[0], &z[1]);
                mc_box_muller(r.z, r.w, &z[2], &z[3]);
                for (int k = 0; k < 4; ++k) {
                    const int d = 4 * m + k;
                    if (d >= D) break;
                    kp += z[k] * z[k];
                    float pj = z[k];
                    float qd = st_q[c * D + d];
                    if (L > 0) {
                        pj = pj + h * st_g[c * D + d];
                        qd = qd + e * pj;
                    }
                    pt[d * 32] = pj;
                    qt[d * 32] = qd;
                }
            }
        }
        const float ks = glm_chain_sum(kp, red, pr, j);
        if (live && pr == 0) H0[c] = -lp + 0.5f * ks;
        return;
    }
    if (phase == GLM_INTERIOR) {
        if (!live) return;
        GLM_FOR_OWNED(D) {
            const float qd = qt[d * 32];
            float g = glm_like_grad(G, R, j, d, qd), lpp = 0.0f;
            glm_prior(G, d, qd, g, lpp);
            float pj = pt[d * 32];
            pj = pj + h * g;  // second half kick of the step before
            pj = pj + h * g;  // first half kick of the next
            pt[d * 32] = pj;
            qt[d * 32] = qd + e * pj;
        }
        return;
    }
    // GLM_END
    float kp1 = 0.0f, lpp = 0.0f;
    if (live) {
        GLM_FOR_OWNED(D) {
            const float qd = qt[d * 32];
            float pj = pt[d * 32];
            if (L > 0) {
                float g = glm_like_grad(G, R, j, d, qd);
                glm_prior(G, d, qd, g, lpp);
                pj = pj + h * g;
                pt[d * 32] = g;  // the momentum is done: keep the gradient for the accept
            }
            kp1 += pj * pj;
        }
    }
    const float ks = glm_chain_sum(kp1, red, pr, j);
    const float lps = glm_chain_sum(lpp, red, pr, j);
    if (!live) return;
    const float lpn = L > 0 ? (G.lp_const + glm_part_lp(G, R, j)) + lps : lp;
    const float H1 = -lpn + 0.5f * ks;
    const float Hi = H0[c];
    const float ratio = -(H1 - Hi);
    const mc_u32x4 ru = mc_draw(cfg.seed, chain_id, (uint32_t)it, MC_RNG_TAG_ACCEPT, 0, 0);
    const float logu = mc_logf_u01(mc_u01_f32(ru.x));
    const bool accepted = logu < ratio;
    const bool warm = it < cfg.num_warmup;
    if (accepted && L > 0) {
        GLM_FOR_OWNED(D) {
            st_q[c * D + d] = qt[d * 32];
            st_g[c * D + d] = pt[d * 32];
        }
    }
    if (!warm && samples != nullptr) {
        const int64_t sidx = it - cfg.num_warmup - cfg.sample_begin;
        if (sidx >= 0 && sidx < cfg.sample_capacity) {
            float* out = samples + (c * cfg.sample_capacity + sidx) * (int64_t)D;
            GLM_FOR_OWNED(D) out[d] = st_q[c * D + d];  // (written above by this thread)
        }
    }
    if (pr != 0) return;
    mc_chain_scalars& sc = scal[c];
    int n_acc = sc.n_accept, n_tot = sc.n_total;
    if (it == cfg.num_warmup) {  // hmc.py:175-180
        sc.warmup_accept = n_acc;
        sc.warmup_total = n_tot;
        n_acc = 0;
        n_tot = 0;
    }
    n_acc += accepted ? 1 : 0;
    n_tot += 1;
    double eps_next = eps;
    if (warm && cfg.adapt_step_size && it > 10) {
        const double rate = (double)n_acc / (double)n_tot;
        eps_next = (rate < cfg.target_accept) ? eps * 0.95 : eps * 1.05;
    }
    const int64_t ti = it - tr.iter_begin;
    if (ti >= 0 && ti < tr.capacity) {
        const int64_t o = c * tr.capacity + ti;
        if (tr.accepted) tr.accepted[o] = accepted ? 1 : 0;
        if (tr.accept_stat) tr.accept_stat[o] = ratio;
        if (tr.step_size) tr.step_size[o] = eps;
        if (tr.energy) tr.energy[o] = Hi;
        if (tr.tree_depth) tr.tree_depth[o] = L;
        if (tr.n_leapfrog) tr.n_leapfrog[o] = L;
    }
    if (accepted && L > 0) sc.logp = lpn;
    sc.step_size = eps_next;
    sc.n_accept = n_acc;
    sc.n_total = n_tot;
    sc.n_grad += L;
}

}  // namespace mc

// ---- host side (plan_glm.hip, run_glm.hip) -------------------------------------
#include <string>
struct GlmPlan {
    mc::GlmDev dev = {};      // device pointers below, owned by the program
    float *d_X = nullptr, *d_XT = nullptr, *d_y = nullptr, *d_off = nullptr;
    mc::GlmPrior* d_priors = nullptr;
    int PT = 1;               // 32-wide coefficient tiles: 1, 2, 4 or 8
    // mc_program_create_glm_wide: the gradient runs on k_glm_grad_wide (glm_wide.h),
    // every wave owning PTW 32-wide coefficient tiles: Pp = 128 PTW, PT = 4 PTW
    bool wide = false;
    int PTW = 0;
    // mc_program_create_glm_softmax: family MC_GLM_CATEGORICAL_LOGIT on
    // k_glm_softmax_grad (glm_softmax.h), dev.CPB chains per gradient block
    bool softmax = false;
    int slices = 0;           // mc_program_set_slices: 0 automatic, else 1 .. 64
    // partials of mc_logp_grad / mc_state_init, which take no workspace: room for
    // kScratchBlocks chain blocks of 64 slices, used in stream order
    float* d_scratch = nullptr;
    // the pointwise view (run_glm_pointwise.hip): the per-observation normaliser
    // [Np]; null until mc_program_enable_pointwise
    float* d_norm = nullptr;
    // mc_nuts_run_glm's count of chains still running, read after every batch of
    // ticks: one pinned host word, allocated with the program
    int32_t* h_left = nullptr;
    std::string note;         // the plan in words (mc_program_kernel_note)
};
constexpr int kGlmScratchBlocks = 8;
constexpr int kGlmMaxSlices = 64;
// floats of one partial block
inline int64_t glm_block_floats(const GlmPlan* g) {
    return (int64_t)(g->dev.Pp + mc::kGlmExtra) * mc::kGlmChains;
}
// gradient blocks of a launch of C chains: 32 chains each, CPB on a softmax plan
inline int64_t glm_grad_blocks(const GlmPlan* g, int64_t C) {
    const int64_t per = g->softmax ? g->dev.CPB : mc::kGlmChains;
    return (C + per - 1) / per;
}
// row slices of a launch of C chains (plan_glm.hip)
int glm_plan_slices(const GlmPlan* g, int64_t C);
// k_glm_grad, k_glm_grad_wide on a wide plan or k_glm_softmax_grad on a softmax
// plan, at the positions q (strides sc, sp: above) of C chains, S slices
// (run_glm.hip)
int glm_launch_grad(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S, float* part,
                    hipStream_t st);
