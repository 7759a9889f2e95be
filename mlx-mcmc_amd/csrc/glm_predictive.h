// glm_predictive.h — posterior predictive replicates of a design-matrix program
// over kept draws (mc_glm_predictive on a program of mc_program_create_glm;
// DESIGN §3.23).
//
// k_predictive (predictive.h) gives a thread one observation and at most five
// operands of a draw's row.  Here the operand is a P-long dot product per
// (observation, draw): over all processed draws the linear predictor is the
// GEMM of glm_pointwise.h,  eta[N obs, R draws] = X[N, P] . B^T[P, R],  and the
// replicate of an entry is predictive.h's sampler applied to the f32 eta —
//     Normal      pp_draw<false>(MC_DIST_NORMAL, eta, scale, ...)
//     Bernoulli   pp_draw_discrete(MC_DISCRETE_BERNOULLI, 0, eta, ...)
//     Poisson     pp_draw_discrete(MC_DISCRETE_POISSON, 0, eta, ...)
// on the counter (seed, chain, iteration, MC_RNG_TAG_PREDICT, sub, observation),
// reduced over the draw axis to predictive.h's partial.  Neither eta nor the
// replicates are stored (unless the caller passes yrep).
//
// k_glm_predictive<FAM, PT>: grid (ceil(NT / 4), B draw blocks), 4 waves.
//   rows       as k_glm_pointwise: wave w of workgroup x owns the 32-row tile
//              4 x + w for the launch, its X^T A operands resident in Pp / 2
//              registers.
//   draws      block b walks the processed draws [b per, (b + 1) per) in tiles
//              of 32.  Processed draw p = (c, k), c = p / S', k = p % S', is row
//              c S + k thin of the sample buffer, chain chain0 + c, iteration
//              iter0 + k thin.  Threads 0 .. 31 resolve (c, k) for one draw of
//              a tile each — one division per thread and launch, then steps of
//              32 with a division only where k wraps past S' — and write row,
//              chain and iteration to a parity-indexed LDS table two tiles
//              ahead, between the loop's two barriers.  The coefficient stage
//              reads its rows from that table: no division per load.
//   stage      glm_pointwise.h's: a tile's coefficients read coalesced into
//              registers before the current tile's MFMAs, written transposed
//              to coef[Pp][33] after its epilogue.  Threads 0 .. 31 stage the
//              draw's intercept and scale (xf_apply once per draw) and its two
//              counter words beside them.
//   forward    k_glm_grad's loop: k ascending, two coefficients per
//              v_mfma_f32_32x32x2_f32; then + intercept, then + offset, in the
//              accumulator layout: the bits of k_glm_pointwise's eta.
//   turn       eta itself goes through the wave's LDS patch [32][33] (not a
//              density: the sampler runs after the turn).  Afterwards lane l is
//              observation l % 32 and holds draws 16 (l / 32) .. + 15 of the tile.
//   epilogue   per draw, in draw order, a lane runs the sampler (emitted once:
//              the loop over a batch is not unrolled), stores the replicate
//              when yrep is given (the 32 observations of a half wave are one
//              128-byte segment of a draw's row), counts the finite replicates
//              below (count families: and equal to) its observation, and folds
//              batches of kPwBatch through pw_moments as k_predictive does.
//              Rows past N and draws past the block run no sampler.  Every
//              sampler loop has predictive.h's compile-time bound.
//   output     lanes 32 .. 63 hand their accumulator to lanes 0 .. 31 (Chan's
//              update over the finite counts, lower half first: k_pp_merge's
//              rules); one partial per (draw block, observation) in
//              k_predictive's layout, merged by k_pp_merge unchanged.
// eta's bits do not depend on the draw-block split, thin or the offsets, so a
// replicate is a function of its counter and the draw's parameters alone.
// Rows past N, coefficients past P and draws past the block are zero operands
// or masked: nothing reads past an array.
#pragma once
#include "glm_pointwise.h"
#include "predictive.h"

namespace mc {

template <int FAM, int PT>
__global__ void __launch_bounds__(256)
k_glm_predictive(GlmDev G, PpRun R, const float* __restrict__ samples, double* __restrict__ part,
                 double* __restrict__ eqpart, float* __restrict__ yrep) {
    constexpr int Pp = 32 * PT;
    constexpr int NPRE = 4 * PT;  // staged coefficients per thread and tile
    __shared__ float coef[Pp * kGpwLd];
    __shared__ int64_t trow[2][kGlmChains];      // by tile parity: a draw's sample row, -1 past the block
    __shared__ uint32_t tctr[2][2][kGlmChains];  // ... its chain and iteration words
    __shared__ float ex[2][kGlmChains];          // the current tile, per draw: intercept, scale
    __shared__ uint32_t ectr[2][kGlmChains];     // ... chain and iteration words
    __shared__ float obs[4][2][32];              // per wave: y, offset of its rows
    __shared__ float patch[4][32 * kGpwLd];      // per wave: the turn
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const int t = blockIdx.x * 4 + wave;
    const bool act = t < G.NT;  // (an idle wave computes its workgroup's last tile, unwritten)
    const int row0 = (act ? t : G.NT - 1) * 32;
    const int64_t r0 = (int64_t)blockIdx.y * R.per;
    const int64_t r1 = r0 + R.per < R.Np ? r0 + R.per : R.Np;
    const int64_t D = G.D;

    // ---- the draw table (threads 0 .. 31: draw tid of the tile after the last tabled)
    int64_t tp = r0 + tid, tc = 0, tk = 0;
    if (tid < kGlmChains) {
        tc = tp / R.Sp;
        tk = tp - tc * R.Sp;
    }
    auto table = [&](int par) {
        trow[par][tid] = tp < r1 ? tc * R.S + tk * R.thin : -1;
        tctr[par][0][tid] = R.chain0 + (uint32_t)tc;
        tctr[par][1][tid] = R.iter0 + (uint32_t)(tk * R.thin);
        tp += 32;
        tk += 32;
        if (tk >= R.Sp) {
            const int64_t w = tk / R.Sp;
            tc += w;
            tk -= w * R.Sp;
        }
    };

    // ---- the stage: a tile's global loads, then their LDS stores ---------------
    float pre[NPRE], pi = 0.0f, ps = 0.0f;
    uint32_t pc = 0u, pit = 0u;
    bool plive = false;
    auto fetch = [&](int par) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = tid + 256 * i, jj = e / Pp, p = e % Pp;
            const int64_t row = trow[par][jj];
            pre[i] = (p < G.P && row >= 0) ? samples[row * D + G.boff + p] : 0.0f;
        }
        if (tid < kGlmChains) {
            const int64_t row = trow[par][tid];
            plive = row >= 0;
            pc = tctr[par][0][tid];
            pit = tctr[par][1][tid];
            if (G.ik == MC_OP_PSCALAR && plive) pi = samples[row * D + G.ipoff];
            if constexpr (FAM == MC_GLM_NORMAL) {
                if (G.sk != MC_OP_CONST && plive) ps = samples[row * D + G.spoff];
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = tid + 256 * i, jj = e / Pp, p = e % Pp;
            coef[p * kGpwLd + jj] = pre[i];
        }
        if (tid < kGlmChains) {
            float icpt = 0.0f, scale = 1.0f;
            if (G.ik == MC_OP_CONST) icpt = G.ival;
            else if (G.ik == MC_OP_PSCALAR && plive) icpt = pi;
            if constexpr (FAM == MC_GLM_NORMAL) {
                if (G.sk == MC_OP_CONST) scale = G.sval;
                else if (plive) scale = xf_apply(G.sxf, ps);
            }
            ex[0][tid] = icpt;
            ex[1][tid] = scale;
            ectr[0][tid] = pc;
            ectr[1][tid] = pit;
        }
    };
    if (tid < kGlmChains) {
        table(0);
        table(1);
    }
    __syncthreads();
    fetch(0);

    // ---- the wave's rows: y, offset; its A operands ----------------------------
    if (lane < 32) {
        obs[wave][0][lane] = G.y[row0 + lane];
        obs[wave][1][lane] = G.off ? G.off[row0 + lane] : 0.0f;
    }
    const float* xt = G.XT + (int64_t)h * G.Np + row0 + j;
    float a[PT * 16];
#pragma unroll
    for (int k = 0; k < PT * 16; ++k) a[k] = xt[(int64_t)(2 * k) * G.Np];
    store();
    __syncthreads();

    PwAcc A = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // (n: the finite replicates; m, s unused)
    double nfsum = 0.0, below = 0.0;
    [[maybe_unused]] double equal = 0.0;
    float* pt = patch[wave];
    const int64_t o = (int64_t)row0 + j;  // the lane's observation after the turn
    const bool own = act && o < G.N;
    const float yo = obs[wave][0][j];

    int par = 0;
    for (int64_t n0 = r0; n0 < r1; n0 += 32, par ^= 1) {
        const bool more = n0 + 32 < r1;  // (workgroup-uniform)
        if (more) fetch(par ^ 1);
        // forward: eta[32 rows][32 draws] over the Pp coefficients, two per MFMA
        glm_acc eta;
#pragma unroll
        for (int v = 0; v < 16; ++v) eta[v] = 0.0f;
        const float* bc = coef + h * kGpwLd + j;
#pragma unroll
        for (int k = 0; k < PT * 16; ++k)
            eta = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], bc[k * 2 * kGpwLd], eta, 0, 0, 0);
        // eta + intercept + offset in the accumulator layout (a lane is a draw),
        // turned through the patch
        const float icpt = ex[0][j];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int rb = 8 * g4 + 4 * h;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float e = eta[4 * g4 + u] + icpt;
                if (G.off) e = e + obs[wave][1][rb + u];
                pt[(rb + u) * kGpwLd + j] = e;
            }
        }
        gpw_wave_sync();
        // turned: the lane is observation j and takes draws 16 h .. 16 h + 15
        if (own) {
#pragma unroll 1
            for (int b = 0; b < 2; ++b) {
                const int d0 = 16 * h + kPwBatch * b;
                const int64_t left = r1 - (n0 + d0);
                const int kb = left >= kPwBatch ? kPwBatch : (left > 0 ? (int)left : 0);
                if (kb == 0) break;
                // one draw at a time (the sampler is emitted once); its replicate
                // enters a register window of the batch's values, newest last
                float x[kPwBatch];
#pragma unroll
                for (int k = 0; k < kPwBatch; ++k) x[k] = 0.0f;
#pragma unroll 1
                for (int k = 0; k < kb; ++k) {
                    const int d = d0 + k;
                    const float e = pt[j * kGpwLd + d];
                    const uint32_t chain = ectr[0][d], iter = ectr[1][d];
                    float y;
                    if constexpr (FAM == MC_GLM_NORMAL) {
                        y = pp_draw<false>(MC_DIST_NORMAL, e, ex[1][d], R.seed, chain, iter,
                                           (uint32_t)o);
                    } else if constexpr (FAM == MC_GLM_BERNOULLI_LOGIT) {
                        y = pp_draw_discrete(MC_DISCRETE_BERNOULLI, 0.0f, e, R.seed, chain, iter,
                                             (uint32_t)o);
                    } else {
                        y = pp_draw_discrete(MC_DISCRETE_POISSON, 0.0f, e, R.seed, chain, iter,
                                             (uint32_t)o);
                    }
                    if (yrep) yrep[(n0 + d) * (int64_t)G.N + o] = y;
                    // (a non-finite y compares false or is dropped here: BELOW and
                    // EQUAL count finite replicates only)
                    if (y - y == 0.0f && y < yo) below += 1.0;
                    if constexpr (FAM != MC_GLM_NORMAL) {
                        if (y - y == 0.0f && y == yo) equal += 1.0;
                    }
#pragma unroll
                    for (int i = 0; i + 1 < kPwBatch; ++i) x[i] = x[i + 1];
                    x[kPwBatch - 1] = y;
                }
                pw_moments(A, nfsum, x, kb);
            }
        }
        __syncthreads();  // every wave is done with coef / ex / ectr (and its patch)
        if (more) store();
        if (tid < kGlmChains) table(par);  // the tile after the next
        __syncthreads();
    }

    // ---- the upper half's draws join the lower half's, lower first (k_pp_merge's rules)
    const double un = gpw_from_upper(A.n), umean = gpw_from_upper(A.mean);
    const double um2 = gpw_from_upper(A.m2), unf = gpw_from_upper(A.nf);
    const double ubelow = gpw_from_upper(below);
    [[maybe_unused]] double uequal = 0.0;
    if constexpr (FAM != MC_GLM_NORMAL) uequal = gpw_from_upper(equal);
    if (h != 0 || !own) return;
    if (un > 0.0) {
        if (A.n > 0.0) {
            const double d = umean - A.mean;
            const double r = 1.0 / (A.n + un);
            A.mean += d * (un * r);
            A.m2 += um2 + d * d * (A.n * un * r);
        } else {
            A.mean = umean;
            A.m2 = um2;
        }
        A.n += un;
    }
    A.nf += unf;
    if (A.n == 0.0) A.mean = A.m2 = __builtin_nan("");
    const int64_t M = G.N;
    double* out = part + (int64_t)blockIdx.y * PP_COUNT * M + o;
    out[PP_N * M] = A.n + A.nf;
    out[PP_MEAN * M] = A.mean;
    out[PP_M2 * M] = A.m2;
    out[PP_BELOW * M] = below + ubelow;
    out[PP_NONFINITE * M] = A.nf;
    if constexpr (FAM != MC_GLM_NORMAL) {
        if (eqpart) eqpart[(int64_t)blockIdx.y * M + o] = equal + uequal;
    }
}

}  // namespace mc
