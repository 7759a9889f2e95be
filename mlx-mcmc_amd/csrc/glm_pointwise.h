// glm_pointwise.h — per-observation log-likelihood statistics of a design-matrix
// program over kept draws (mc_pointwise_stats on a program of
// mc_program_create_glm).
//
// Over all R = C * S draws the linear predictor is one GEMM with a long third
// dimension,  eta[N obs, R draws] = X[N, P] . B^T[P, R],  followed by the
// family's log density per entry and pointwise.h's f64 reduction over the draw
// axis.  The N x R matrix is never stored (unless the caller passes a matrix).
//
// k_glm_pointwise<FAM, PT>: grid (ceil(NT / 4), B draw blocks), 4 waves.
//   rows       wave w of workgroup x owns the 32-row tile 4 x + w for the whole
//              launch.  Its A operands — lane l's X^T[2 k + l / 32][row0 +
//              l % 32], k < 16 PT — stay in Pp / 2 registers (128 at PT = 8:
//              no instantiation needs scratch), so X is read once per draw
//              block.
//   draws      the four waves walk the same 32-draw tiles of block b.  A tile's
//              coefficients are read from the row-major [R][D] sample buffer
//              with consecutive lanes on consecutive coefficients of one draw
//              (coalesced) and stored transposed to LDS as coef[Pp][33] (the
//              pad: conflict-free both for this store and for the B operand
//              read coef[2 k + l / 32][l % 32]).  Beside them the draw's
//              intercept, scale and log scale (xf_apply / ex_log once per draw).
//              The stage is double-buffered through registers: the next tile's
//              global loads are issued before the current tile's MFMAs and are
//              written to LDS after its epilogue, between two barriers.
//   forward    k_glm_grad's loop: k ascending, two coefficients per
//              v_mfma_f32_32x32x2_f32.
//   values     in the accumulator layout (register v of lane l: row 8 (v / 4) +
//              4 (l / 32) + v % 4, draw l % 32), exactly as k_glm_grad forms lp:
//              + intercept, + offset, the family's device function; Poisson:
//              + the observation's normaliser -lgamma(y + 1) (one f32 add).
//   turn       through the wave's private LDS patch [32][33]: afterwards lane l
//              is observation l % 32 and holds draws 16 (l / 32) .. + 15 of the
//              tile, as two batches of kPwBatch for pw_lse / pw_moments.
//   output     lanes 32 .. 63 hand their accumulator to lanes 0 .. 31 (pw_merge,
//              lower half first); one partial per (draw block, observation), in
//              k_pointwise's layout: k_pw_merge merges the B partials unchanged.
// Rows past N, coefficients past P and draws past the block are zero operands
// or masked: nothing reads past an array and no such value is accumulated.
#pragma once
#include "glm.h"
#include "pointwise.h"

namespace mc {

constexpr int kGpwLd = 33;  // leading dimension of the LDS tiles (32 + 1 pad)

// LDS traffic between the lanes of one wave: order it without a workgroup barrier
MC_DEV void gpw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

MC_DEV double gpw_from_upper(double x) { return __shfl_down(x, 32); }

// The turn's second half: the wave's patch pt holds the values of its 32 rows
// under the 32 draws n0 .. n0 + 31 (row-major, leading dimension kGpwLd); the
// lane is observation j (o of N; own: a live one) and takes draws 16 h ..
// 16 h + 15, those before r1, as two batches of kPwBatch.
MC_DEV void gpw_turn(PwAcc& A, double& nfsum, const float* pt, int j, int h, int64_t n0, int64_t r1,
                     float* __restrict__ matrix, bool own, int64_t N, int64_t o) {
#pragma unroll 1
    for (int b = 0; b < 2; ++b) {
        const int d0 = 16 * h + kPwBatch * b;
        const int64_t left = r1 - (n0 + d0);
        const int kb = left >= kPwBatch ? kPwBatch : (left > 0 ? (int)left : 0);
        if (kb == 0) continue;
        // the batch's kb values at the end of the window, in draw order
        float x[kPwBatch];
#pragma unroll
        for (int k = 0; k < kPwBatch; ++k) {
            const int d = d0 + k - (kPwBatch - kb);
            x[k] = k >= kPwBatch - kb ? pt[j * kGpwLd + d] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kPwBatch; ++k) {
            if (k >= kPwBatch - kb) {
                const int d = d0 + k - (kPwBatch - kb);
                if (matrix && own) matrix[(n0 + d) * N + o] = x[k];
                pw_lse(A, x[k]);
            }
        }
        pw_moments(A, nfsum, x, kb);
    }
}

// The upper half's draws join the lower half's, lower first; lane (observation,
// h = 0) writes the partial of its draw block: out is the block's PW_MAX entry
// of the observation.
MC_DEV void gpw_finish(PwAcc& A, double nfsum, int h, bool own, double* __restrict__ out,
                       int64_t N) {
    if (A.nf > 0.0) {
        A.mean = nfsum;
        A.m2 = __builtin_nan("");
    }
    A.n = A.n + A.nf;
    PwAcc U;
    U.m = gpw_from_upper(A.m);
    U.s = gpw_from_upper(A.s);
    U.n = gpw_from_upper(A.n);
    U.mean = gpw_from_upper(A.mean);
    U.m2 = gpw_from_upper(A.m2);
    U.nf = gpw_from_upper(A.nf);
    if (h != 0 || !own) return;
    if (U.n > 0.0) pw_merge(A, U);  // (a block of fewer than 17 draws: no upper half)
    out[(int64_t)PW_MAX * N] = A.m;
    out[(int64_t)PW_SUMEXP * N] = A.s;
    out[(int64_t)PW_N * N] = A.n;
    out[(int64_t)PW_MEAN * N] = A.mean;
    out[(int64_t)PW_M2 * N] = A.m2;
    out[(int64_t)PW_NONFINITE * N] = A.nf;
}

template <int FAM, int PT>
__global__ void __launch_bounds__(256)
k_glm_pointwise(GlmDev G, const float* __restrict__ norm, int64_t R, int64_t per,
                const float* __restrict__ samples, double* __restrict__ part,
                float* __restrict__ matrix) {
    constexpr int Pp = 32 * PT;
    constexpr int NPRE = 4 * PT;  // staged coefficients per thread and tile
    __shared__ float coef[Pp * kGpwLd];
    __shared__ float ex[3][kGlmChains];      // per draw: intercept, scale, log scale
    __shared__ float obs[4][3][32];          // per wave: y, offset, normaliser of its rows
    __shared__ float patch[4][32 * kGpwLd];  // per wave: the turn
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const int t = blockIdx.x * 4 + wave;
    const bool act = t < G.NT;  // (an idle wave computes its workgroup's last tile, unwritten)
    const int row0 = (act ? t : G.NT - 1) * 32;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    const int64_t r1 = r0 + per < R ? r0 + per : R;
    const int64_t D = G.D;

    // ---- the stage: the next tile's global loads, then their LDS stores -----
    float pre[NPRE], pi = 0.0f, ps = 0.0f;
    bool plive = false;
    auto fetch = [&](int64_t n0) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = tid + 256 * i, jj = e / Pp, p = e % Pp;
            const int64_t n = n0 + jj;
            pre[i] = (p < G.P && n < r1) ? samples[n * D + G.boff + p] : 0.0f;
        }
        if (tid < kGlmChains) {
            const int64_t n = n0 + tid;
            plive = n < r1;
            if (G.ik == MC_OP_PSCALAR && plive) pi = samples[n * D + G.ipoff];
            if constexpr (FAM == MC_GLM_NORMAL) {
                if (G.sk != MC_OP_CONST && plive) ps = samples[n * D + G.spoff];
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
            float icpt = 0.0f, scale = 1.0f, logs = 0.0f;
            if (G.ik == MC_OP_CONST) icpt = G.ival;
            else if (G.ik == MC_OP_PSCALAR && plive) icpt = pi;
            if constexpr (FAM == MC_GLM_NORMAL) {
                if (G.sk == MC_OP_CONST) scale = G.sval;
                else if (plive) scale = xf_apply(G.sxf, ps);
                logs = ex_log(scale);
            }
            ex[0][tid] = icpt;
            ex[1][tid] = scale;
            ex[2][tid] = logs;
        }
    };
    fetch(r0);

    // ---- the wave's rows: y, offset, normaliser; its A operands --------------
    if (lane < 32) {
        obs[wave][0][lane] = G.y[row0 + lane];
        obs[wave][1][lane] = G.off ? G.off[row0 + lane] : 0.0f;
        obs[wave][2][lane] = FAM == MC_GLM_POISSON_LOG ? norm[row0 + lane] : 0.0f;
    }
    const float* xt = G.XT + (int64_t)h * G.Np + row0 + j;
    float a[PT * 16];
#pragma unroll
    for (int k = 0; k < PT * 16; ++k) a[k] = xt[(int64_t)(2 * k) * G.Np];
    store();
    __syncthreads();

    PwAcc A = {-(double)__builtin_inff(), 0.0, 0.0, 0.0, 0.0, 0.0};
    double nfsum = 0.0;
    float* pt = patch[wave];
    const int64_t o = (int64_t)row0 + j;  // the lane's observation after the turn
    const bool own = act && o < G.N;

    for (int64_t n0 = r0; n0 < r1; n0 += 32) {
        const bool more = n0 + 32 < r1;  // (workgroup-uniform)
        if (more) fetch(n0 + 32);
        // forward: eta[32 rows][32 draws] over the Pp coefficients, two per MFMA
        glm_acc eta;
#pragma unroll
        for (int v = 0; v < 16; ++v) eta[v] = 0.0f;
        const float* bc = coef + h * kGpwLd + j;
#pragma unroll
        for (int k = 0; k < PT * 16; ++k)
            eta = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], bc[k * 2 * kGpwLd], eta, 0, 0, 0);
        // the values, in the accumulator layout (a lane is a draw)
        const float icpt = ex[0][j], scale = ex[1][j], logs = ex[2][j];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int rb = 8 * g4 + 4 * h;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float e = eta[4 * g4 + u] + icpt;
                if (G.off) e = e + obs[wave][1][rb + u];
                const float yy = obs[wave][0][rb + u];
                float lp;
                if constexpr (FAM == MC_GLM_NORMAL) {
                    lp = ex_normal(G.c0, yy, e, scale, logs).lp;
                } else if constexpr (FAM == MC_GLM_BERNOULLI_LOGIT) {
                    lp = ex_bernoulli_lp(yy, e);
                } else {
                    lp = ex_poisson_lp(yy, e) + obs[wave][2][rb + u];
                }
                pt[(rb + u) * kGpwLd + j] = lp;
            }
        }
        gpw_wave_sync();
        gpw_turn(A, nfsum, pt, j, h, n0, r1, matrix, own, G.N, o);
        __syncthreads();  // every wave is done with coef / ex (and its patch)
        if (more) store();
        __syncthreads();
    }

    gpw_finish(A, nfsum, h, own, part + (int64_t)blockIdx.y * PW_COUNT * G.N + o, G.N);
}

}  // namespace mc

// ---- host side (run_glm_pointwise.hip) -------------------------------------------
// Draw blocks B and draws per block for R = C * S draws of a program of NT row
// tiles: enough workgroups to fill a device whatever it is (a constant target,
// not a query), whole 32-draw tiles per block and at least kGpwMinDraws of them
// so that a block's read of X (resident operands) is shared by many tiles.  A
// function of (R, NT) only; every block holds at least one draw.
inline constexpr int64_t kGpwTargetGroups = 4096;
inline constexpr int64_t kGpwMinDraws = 256;
inline constexpr int64_t kGpwMaxB = 1024;
inline void glm_pw_split(int64_t R, int64_t NT, int64_t* B, int64_t* per) {
    const int64_t groups = (NT + 3) / 4;
    int64_t b = (kGpwTargetGroups + groups - 1) / groups;
    b = std::min(b, std::max<int64_t>(1, R / kGpwMinDraws));
    b = std::max<int64_t>(1, std::min(b, kGpwMaxB));
    *per = ((R + b - 1) / b + 31) / 32 * 32;
    *B = (R + *per - 1) / *per;
}
