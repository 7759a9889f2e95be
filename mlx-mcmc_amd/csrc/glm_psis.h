// glm_psis.h — the tail selection and gather passes of PSIS-LOO on a
// design-matrix program (mc_glm_psis_loo on a program of mc_program_create_glm;
// DESIGN §3.24).
//
// k_psis_count and k_psis_gather (psis.h) give a thread one observation and at
// most five operands of a draw's row.  Here the per-draw value is a P-long dot
// product: over all R = C * S draws it is the GEMM of glm_pointwise.h,
// eta[N obs, R draws] = X[N, P] . B^T[P, R],  followed by the family's log
// density per entry — the bits k_glm_pointwise stores with a matrix — and the
// matrix is re-formed by every pass instead of stored.  k_psis_pick and
// k_psis_fit read a PsisWs only and run unchanged between and after these.
//
// Both kernels: grid (ceil(NT / 4), B draw blocks), 4 waves, glm_pw_split's
// blocks.
//   front end  glm_pointwise.h's, restated (glm_psis_walk): wave w of workgroup
//              x owns the 32-row tile 4 x + w, its X^T A operands resident in
//              Pp / 2 registers; a tile's coefficients are read coalesced into
//              registers before the current tile's MFMAs and written transposed
//              to coef[Pp][33] after its epilogue, the draw's intercept, scale
//              and log scale beside them; forward k ascending, two coefficients
//              per v_mfma_f32_32x32x2_f32; + intercept, + offset, the family's
//              function of eval.h, Poisson + the normaliser, in the accumulator
//              layout.
//   turn       through the wave's private LDS patch [32][33]: afterwards lane l
//              is observation row0 + l % 32 and holds draws 16 (l / 32) .. + 15
//              of the tile.  Each such draw's value goes to the kernel's sink in
//              draw order; draws past the block, rows past N and idle waves
//              reach no sink.
//   count      the sink is k_psis_count's: the key's digit in the observation's
//              bracket bumps sixteen register counters by a compare-and-add
//              chain (no register indexing, no LDS, no atomics), beside the
//              running smallest key.  The upper half's seventeen u32 join the
//              lower half's by __shfl_down(., 32): integer adds and a min do
//              not depend on order.  Lanes 0 .. 31 write cnt[(b 17 + j) M + o].
//   gather     a draw below the cutoff goes to the observation's slots of the
//              tail buffer, every other into an f64 sum of exp(lmin - x).  The
//              two halves of a wave hold the same observation and fill the
//              block's slot range from its two ends: the lower half upwards
//              from off[b][o], the upper half downwards from the range's end
//              (off[b + 1][o], or ntail[o] for the last block) minus one.  The
//              range holds exactly the block's tail draws, by the counts, so the
//              two never meet and exchange nothing; k_psis_fit sorts the keys,
//              so slot order is free.  Every store is tested against Mt.  The
//              upper half's rest and non-finite count join the lower's, lower
//              first.
// Integer counts and a fixed summation order: two calls give the same bits.
// Rows past N, coefficients past P and draws past the block are zero operands
// or masked: nothing reads past an array.
#pragma once
#include "glm_pointwise.h"
#include "psis.h"

namespace mc {

// The front end and the turn; sink(x) takes the lane's draws of its observation
// in draw order.  ROLL: the sink is emitted once and fed from the patch one draw
// at a time (the gather's f64 exponential), else sixteen times on a register
// batch read ahead of it (the count's compare-and-add chain).
template <int FAM, int PT, bool ROLL, class Sink>
MC_DEV void glm_psis_walk(const GlmDev& G, const float* __restrict__ norm, int64_t R, int64_t per,
                          const float* __restrict__ samples, bool own, Sink& sink) {
    constexpr int Pp = 32 * PT;
    constexpr int NPRE = 4 * PT;  // staged coefficients per thread and tile
    __shared__ float coef[Pp * kGpwLd];
    __shared__ float ex[3][kGlmChains];      // per draw: intercept, scale, log scale
    __shared__ float obs[4][3][32];          // per wave: y, offset, normaliser of its rows
    __shared__ float patch[4][32 * kGpwLd];  // per wave: the turn
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const int t = blockIdx.x * 4 + wave;
    // (an idle wave computes its workgroup's last tile, unwritten)
    const int row0 = (t < G.NT ? t : G.NT - 1) * 32;
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

    float* pt = patch[wave];
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
        // turned: the lane is observation j and takes draws 16 h .. 16 h + 15
        if (own) {
            const int64_t left = r1 - (n0 + 16 * h);
            const int kb = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
            const float* mine = pt + j * kGpwLd + 16 * h;
            if constexpr (ROLL) {
#pragma unroll 1
                for (int k = 0; k < kb; ++k) sink(mine[k]);
            } else {
                float x[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) x[k] = k < kb ? mine[k] : 0.0f;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < kb) sink(x[k]);
            }
        }
        __syncthreads();  // every wave is done with coef / ex (and its patch)
        if (more) store();
        __syncthreads();
    }
}

// One pass of the radix select (psis.h k_psis_count) over the draws of a block.
template <int FAM, int PT>
__global__ void __launch_bounds__(256)
k_glm_psis_count(GlmDev G, const float* __restrict__ norm, int64_t R, int64_t per,
                 const float* __restrict__ samples, int shift, int first,
                 const uint32_t* __restrict__ lo, uint32_t* __restrict__ cnt) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    const int64_t o = (int64_t)(t < G.NT ? t : G.NT - 1) * 32 + (lane & 31);
    const bool own = t < G.NT && o < G.N;
    const uint32_t base = (first || !own) ? 0u : lo[o];
    uint32_t c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] = 0u;
    uint32_t kmin = 0xffffffffu;
    auto sink = [&](float x) {
        const uint32_t key = psis_key(x);
        kmin = key < kmin ? key : kmin;
        // digit 0: below the bracket; d: in [lo + (d - 1) w, lo + d w); 17: above
        uint32_t d = (key - base) >> shift;
        d = key < base ? 0u : (d < 16u ? d : 16u) + 1u;
#pragma unroll
        for (int j = 0; j < 16; ++j) c[j] += d <= (uint32_t)j ? 1u : 0u;
    };
    glm_psis_walk<FAM, PT, false>(G, norm, R, per, samples, own, sink);
    // ---- the upper half's draws join the lower half's -------------------------
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] += __shfl_down(c[j], 32);
    const uint32_t umin = __shfl_down(kmin, 32);
    kmin = umin < kmin ? umin : kmin;
    if (lane >= 32 || !own) return;
    const int64_t M = G.N;
    uint32_t* out = cnt + (int64_t)blockIdx.y * kPsisSlots * M + o;
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j * M] = c[j];
    out[16 * M] = kmin;
}

// The draw loop once more (psis.h k_psis_gather): tails and the rest's sum.
template <int FAM, int PT>
__global__ void __launch_bounds__(256)
k_glm_psis_gather(GlmDev G, const float* __restrict__ norm, int64_t R, int64_t per,
                  const float* __restrict__ samples, uint32_t Mt, PsisWs W) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    const int64_t o = (int64_t)(t < G.NT ? t : G.NT - 1) * 32 + (lane & 31);
    const bool own = t < G.NT && o < G.N, upper = lane >= 32;
    const int64_t M = G.N, bo = (int64_t)blockIdx.y * M + o;
    uint32_t kcut = 0u, pos = 0u;
    double lmin = 0.0;
    if (own) {
        kcut = W.lo[o];
        lmin = (double)psis_unkey(W.kmin[o]);
        // the block's slots [off[b], end): the lower half fills upwards from the
        // first, the upper half downwards from the last
        const uint32_t end = blockIdx.y + 1 < gridDim.y ? W.off[bo + M] : W.ntail[o];
        pos = upper ? end - 1u : W.off[bo];
    }
    const uint32_t step = upper ? 0xffffffffu : 1u;  // (- 1 / + 1)
    float* __restrict__ slots = W.tail + o * (int64_t)Mt;
    double rest = 0.0;
    uint32_t nf = 0u;
    auto sink = [&](float v) {
        const uint32_t key = psis_key(v);
        const float x = psis_unkey(key);
        nf += x - x == 0.0f ? 0u : 1u;
        if (key < kcut) {
            // (pos < Mt by the counts, on both ends — a step below slot 0 wraps
            // above Mt; the test keeps a store inside the slots)
            if (pos < Mt) slots[pos] = x;
            pos += step;
        } else {
            rest += exp(lmin - (double)x);
        }
    };
    glm_psis_walk<FAM, PT, true>(G, norm, R, per, samples, own, sink);
    // ---- the upper half's sums join the lower half's, lower first -------------
    rest = rest + gpw_from_upper(rest);
    nf += __shfl_down(nf, 32);
    if (upper || !own) return;
    W.rest[bo] = rest;
    W.nf[bo] = nf;
}

}  // namespace mc
