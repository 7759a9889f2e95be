// glm_wide.h — k_glm_grad_wide: the design-matrix gradient (glm.h) for up to
// MC_GLM_WIDE_MAX_P = 1024 columns, and at fewer accumulator registers per lane
// for the widths k_glm_grad serves.
//
// k_glm_grad gives every wave its own row tiles and the WHOLE gradient block
// G[Pp][32 chains] in accumulator registers: 16 per 32 coefficients, 128 at
// P = 256, which is its cap.  Here the workgroup shares the row tiles and splits
// the COLUMNS of G over its four waves: a wave owns Pp / 4 coefficients, so
// Pp = 128 PTW and a lane holds 16 PTW accumulator registers (PTW <= 8).  Same
// grid (S row slices, chain blocks), 256 threads, GlmDev, (sc, sp) addressing,
// operand layouts and partial block as k_glm_grad.
//
// The slice's 32-row tiles t0 .. t1 are walked in rounds of four:
//   forward    wave w forms eta[32 rows][32 chains] of tile t0 + 4 round + w over
//              all Pp coefficients (A from X^T, B from the coefficients in LDS),
//              then intercept, offset and the family's functions of eval.h in the
//              accumulator layout, with the expressions, the masking of rows >= N
//              and the sums sl, sr, sd of k_glm_grad.  A wave whose tile is past
//              t1 computes nothing and writes zeros: every wave reaches every
//              barrier.
//   the corner the wave writes r = dl / d eta to the LDS buffer rbuf[round % 2]
//              [4 tiles][32 rows][32 chains]; one barrier; then every wave reads
//              all four tiles.  Two buffers by round parity: a wave may write
//              round n + 1 while another still reads round n, and the barrier of
//              round n + 1 orders the reads of round n before the writes of
//              round n + 2.
//              Row stride 32 floats, no padding, and row i of a tile stored at
//              i ^ ((i >> 2) & 1).  The backward pairs the ADJACENT rows 2m and
//              2m + 1 in one MFMA (k = 0 and k = 1): their two stored rows are
//              2m and 2m + 1 in some order, so the wave's 64 lanes read 64
//              consecutive floats, every bank once.  The forward's two half
//              waves write rows i and i + 4 (the accumulator layout); the swap
//              puts them an odd number of rows apart, in different halves of
//              the 64 banks, where plain rows would be 128 floats apart on the
//              same banks.
//   backward   wave w adds, for the round's tiles in row order and their row
//              pairs in order, X[rows 2m, 2m + 1][its columns]^T . r into
//              G[columns w PTW 32 .. (w + 1) PTW 32)[32 chains]: B from rbuf, A
//              = X[row 2m + l / 32][tile + l % 32] from the row-major X.  Tiles
//              past t1 are skipped (uniformly over the workgroup).
//   coefficients  Pp <= 256: [Pp][32] staged once.  Larger: the forward's K loop
//              runs over chunks of 256 coefficient rows (32 KB), each staged
//              between two barriers by all four waves in lockstep (the chunk's
//              first barrier of a round's first chunk is the round's own).
//   output     a wave's columns of G are complete when the loop ends: it writes
//              them straight to the partial block, no sum across waves.  sr, sd
//              and sl are added in wave order through LDS (the r buffer, free
//              by then) as in k_glm_grad; the block keeps the layout
//              [Pp + 4][32], so k_glm_finish, k_glm_hmc_step and
//              k_glm_nuts_step run on it unchanged.
// LDS: 32 KB of coefficients (16 KB at PTW = 1) and 32 KB of r, 64 KB in all
// (the three sums pass through the r buffer once the loop is done).
// A chain is one MFMA column and the order of every sum is fixed by (N, S)
// alone: the properties of glm.h's closing paragraph hold.  The sums of G run
// in another order than k_glm_grad's: the two kernels agree to rounding, not
// in bits.
#pragma once
#include "glm.h"

namespace mc {

constexpr int kGlmWideChunk = 256;  // coefficient rows of one LDS chunk

template <int FAM, int PTW>
__global__ void __launch_bounds__(256)
k_glm_grad_wide(GlmDev G, const float* q, int sc, int sp, int64_t C, int S, float* part) {
    constexpr int Pp = 128 * PTW;
    constexpr int CK = Pp < kGlmWideChunk ? Pp : kGlmWideChunk;
    constexpr int NCH = (Pp + CK - 1) / CK;
    __shared__ __attribute__((aligned(16))) float coef[CK * 32];
    __shared__ __attribute__((aligned(16))) float rbuf[2][4 * 1024];
    const int s = blockIdx.x, cb = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const float* qb = q + (int64_t)cb * kGlmChains * G.D;
    // rows [p0, p0 + rows) of the block's coefficients to LDS
    auto stage = [&](int p0, int rows) {
        for (int e = tid; e < rows * 32; e += 256) {
            const int p = p0 + (e >> 5), jj = e & 31;
            const bool ok = p < G.P && (int64_t)cb * kGlmChains + jj < C;
            coef[e] = ok ? qb[(int64_t)jj * sc + (int64_t)(G.boff + p) * sp] : 0.0f;
        }
    };
    const bool live = (int64_t)cb * kGlmChains + j < C;
    float icpt = 0.0f, scale = 1.0f, logs = 0.0f;
    if (G.ik == MC_OP_CONST) icpt = G.ival;
    else if (G.ik == MC_OP_PSCALAR && live) icpt = qb[(int64_t)j * sc + (int64_t)G.ipoff * sp];
    if constexpr (FAM == MC_GLM_NORMAL) {
        if (G.sk == MC_OP_CONST) scale = G.sval;
        else if (live) scale = xf_apply(G.sxf, qb[(int64_t)j * sc + (int64_t)G.spoff * sp]);
        logs = ex_log(scale);
    }
    if constexpr (NCH == 1) {
        stage(0, Pp);
        __syncthreads();
    }

    glm_acc acc[PTW];
#pragma unroll
    for (int pt = 0; pt < PTW; ++pt)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[pt][v] = 0.0f;
    float sl = 0.0f, sr = 0.0f, sd = 0.0f;
    const int t0 = (int)((int64_t)s * G.NT / S), t1 = (int)((int64_t)(s + 1) * G.NT / S);
    for (int tb = t0, par = 0; tb < t1; tb += 4, par ^= 1) {
        const int t = tb + wave;
        const bool mine = t < t1;
        const int row0 = t * 32;
        // forward: eta[32 rows][32 chains] over the Pp coefficients, two per MFMA
        glm_acc eta;
#pragma unroll
        for (int v = 0; v < 16; ++v) eta[v] = 0.0f;
        const float* xt = G.XT + (int64_t)h * G.Np + row0 + j;
        const float* bc = coef + h * 32 + j;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            constexpr int kLast = Pp - (NCH - 1) * CK;
            const int rows = c + 1 < NCH ? CK : kLast;
            if constexpr (NCH > 1) {
                // (the reads of the chunk before are done; a round's first chunk
                // follows the barrier of the round before)
                if (c > 0) __syncthreads();
                stage(c * CK, rows);
                __syncthreads();
            }
            if (mine) {
                const float* xc = xt + (int64_t)(c * CK) * G.Np;
#pragma unroll 8
                for (int k = 0; k < rows / 2; ++k)
                    eta = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[(int64_t)(2 * k) * G.Np],
                                                               bc[k * 64], eta, 0, 0, 0);
            }
        }
        // elementwise, in the accumulator layout; r to this round's buffer
        float* rw = rbuf[par] + wave * 1024 + j;
        if (mine) {
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
                    float e = eta[4 * g4 + u] + icpt;
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
                    // row i = 8 g4 + 4 h + u of the tile, stored at i ^ h
                    rw[(8 * g4 + 4 * h + (u ^ h)) * 32] = rr;
                }
            }
        } else {
#pragma unroll
            for (int v = 0; v < 16; ++v) rw[(2 * v + h) * 32] = 0.0f;
        }
        __syncthreads();
        // backward: G[this wave's columns] += X[rows 2m, 2m + 1][columns]^T . r
        const int nt = t1 - tb < 4 ? t1 - tb : 4;
        for (int i = 0; i < nt; ++i) {
            const float* rt = rbuf[par] + i * 1024 + j;
            const float* xr = G.X + (int64_t)((tb + i) * 32 + h) * G.Pp + wave * (PTW * 32) + j;
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float b = rt[(2 * m + (h ^ ((m >> 1) & 1))) * 32];
#pragma unroll
                for (int pt = 0; pt < PTW; ++pt)
                    acc[pt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                        xr[(int64_t)(2 * m) * G.Pp + pt * 32], b, acc[pt], 0, 0, 0);
            }
        }
    }

    // G: every wave its own columns, straight to the partial block
    float* out = part + ((int64_t)s * gridDim.y + cb) * (int64_t)((Pp + kGlmExtra) * 32);
#pragma unroll
    for (int pt = 0; pt < PTW; ++pt)
#pragma unroll
        for (int v = 0; v < 16; ++v)
            out[((wave * PTW + pt) * 32 + 8 * (v / 4) + 4 * h + (v % 4)) * 32 + j] = acc[pt][v];
    // the waves' sums of r, of the scale's cotangent and of l, in wave order
    sl = sl + __shfl_xor(sl, 32);
    sr = sr + __shfl_xor(sr, 32);
    sd = sd + __shfl_xor(sd, 32);
    __syncthreads();  // (the last round's reads of rbuf are done)
    float(*ex)[kGlmChains] = reinterpret_cast<float(*)[kGlmChains]>(rbuf[0]);
    for (int w = 0; w < 4; ++w) {
        if (wave == w && h == 0) {
            ex[0][j] = (w == 0) ? sr : ex[0][j] + sr;
            ex[1][j] = (w == 0) ? sd : ex[1][j] + sd;
            ex[2][j] = (w == 0) ? sl : ex[2][j] + sl;
        }
        __syncthreads();
    }
    if (tid < 3 * kGlmChains) out[Pp * 32 + tid] = ex[tid >> 5][tid & 31];
}

}  // namespace mc
