// glm_softmax.h — softmax (multinomial-logit) regression on a design matrix:
// sum_i log softmax(X_i B + a)[y_i] (include/mcmc355.h mc_glm_softmax).
//
// k_glm_softmax_grad<PT, KP>: k_glm_grad's two v_mfma_f32_32x32x2_f32 products
// (glm.h) with the (chain, class) pairs as their N dimension.  The 32 columns of
// a gradient block are CPB = 32 / KP chains times KP classes, class-minor: column
// n = cl KP + k is class k of chain gb CPB + cl (gb = blockIdx.y), KP = K rounded
// up to a power of two.  B[p, k] of a chain is row p, column n of the coefficient
// block, so the forward product gives eta[row, (chain, class)], the backward one
// G[p, (chain, class)] = dl / dB[p, k], and the accumulators cost PT x 16
// registers whatever K is.
//   staging    coef[p][n] = q[chain][boff + p K + k] for k < K and a live chain,
//              else 0; positions by the global chain, (c / 32) 32 D + (c % 32) sc +
//              d sp (a gradient block is not a block of 32 chains)
//   softmax    in the accumulator layout register v of lane l is (one row, column
//              l % 32): the KP classes of a (row, chain) pair are KP adjacent
//              lanes of one 32-lane half.  Padded classes take e = -inf; m = max
//              and s = sum exp(e - m) over the group by xor exchanges at distances
//              1 .. KP / 2 (ds_swizzle_b32 in its bit-mask mode: the xor mask is an
//              immediate, it stays inside a group of 32 lanes, touches no LDS
//              memory and needs no barrier and no address register, which is why
//              KP is a template parameter); lse = m + log s; the lane whose class is
//              the row's label adds e - lse to l; every lane forms r = [k == y] -
//              exp(e - lse): exactly 0 for a padded class, 0 for a row past N.
//              Both sides of an exchange add the same two values, so every lane of
//              a group holds the same m and s bits.
//   backward   r is the B operand as it stands: no LDS, no barrier between the
//              two products.
//   output     k_glm_grad's partial block [Pp + 4][32]: rows 0 .. Pp - 1 G, row Pp
//              the sum of r per column (dl / da_k), row Pp + 1 zero, row Pp + 2 the
//              column's share of l (the label's class column holds a row's term).
// Labels are checked when the program is made (0 .. K - 1, integers): there is no
// invalid-label path here.  The step kernels (glm.h) read chain c's partials in
// gradient block c / CPB (glm_part_of).
#pragma once
#include "glm.h"

namespace mc {

// the value of lane (l ^ DIST) of the same 32-lane half
template <int DIST>
MC_DEV float glm_xor_lane(float x) {
    return __builtin_bit_cast(
        float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x1f | (DIST << 10)));
}

// max / sum over the groups of KP adjacent lanes
template <int KP>
MC_DEV float glm_group_max(float x) {
    x = __builtin_fmaxf(x, glm_xor_lane<1>(x));
    if constexpr (KP > 2) x = __builtin_fmaxf(x, glm_xor_lane<2>(x));
    if constexpr (KP > 4) x = __builtin_fmaxf(x, glm_xor_lane<4>(x));
    if constexpr (KP > 8) x = __builtin_fmaxf(x, glm_xor_lane<8>(x));
    if constexpr (KP > 16) x = __builtin_fmaxf(x, glm_xor_lane<16>(x));
    return x;
}
template <int KP>
MC_DEV float glm_group_sum(float x) {
    x = x + glm_xor_lane<1>(x);
    if constexpr (KP > 2) x = x + glm_xor_lane<2>(x);
    if constexpr (KP > 4) x = x + glm_xor_lane<4>(x);
    if constexpr (KP > 8) x = x + glm_xor_lane<8>(x);
    if constexpr (KP > 16) x = x + glm_xor_lane<16>(x);
    return x;
}

template <int PT, int KP>
__global__ void __launch_bounds__(256)
k_glm_softmax_grad(GlmDev G, const float* q, int sc, int sp, int64_t C, int S, float* part) {
    static_assert(KP >= 2 && KP <= 32 && (KP & (KP - 1)) == 0, "KP: a power of two in 2 .. 32");
    constexpr int CPB = 32 / KP;
    extern __shared__ __attribute__((aligned(16))) float coef[];  // [PT * 32][32]
    __shared__ float ex[3][kGlmChains];
    const int s = blockIdx.x, gb = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const int K = G.K;
    // parameter d of global chain c
    auto at = [&](int64_t c, int d) {
        return q[(c >> 5) * 32 * G.D + (c & 31) * sc + (int64_t)d * sp];
    };
    for (int e = tid; e < PT * 1024; e += 256) {
        const int p = e >> 5, n = e & 31, k = n % KP;
        const int64_t c = (int64_t)gb * CPB + n / KP;
        const bool ok = p < G.P && k < K && c < C;
        coef[e] = ok ? at(c, G.boff + p * K + k) : 0.0f;
    }
    const int kc = j % KP;  // this lane's class, of chain gb CPB + j / KP
    const int64_t cj = (int64_t)gb * CPB + j / KP;
    const bool cls = kc < K;
    const float icpt = (G.aoff >= 0 && cls && cj < C) ? at(cj, G.aoff + kc) : 0.0f;
    const float kf = (float)kc;
    __syncthreads();

    glm_acc acc[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[pt][v] = 0.0f;
    float sl = 0.0f, sr = 0.0f;
    const int t0 = (int)((int64_t)s * G.NT / S), t1 = (int)((int64_t)(s + 1) * G.NT / S);
    for (int t = t0 + wave; t < t1; t += 4) {
        const int row0 = t * 32;
        // forward: eta[32 rows][32 (chain, class) pairs], two coefficients per MFMA
        glm_acc eta;
#pragma unroll
        for (int v = 0; v < 16; ++v) eta[v] = 0.0f;
        const float* xt = G.XT + (int64_t)h * G.Np + row0 + j;
        const float* bc = coef + h * 32 + j;
#pragma unroll 8
        for (int k = 0; k < PT * 16; ++k)
            eta = __builtin_amdgcn_mfma_f32_32x32x2f32(xt[(int64_t)(2 * k) * G.Np], bc[k * 64], eta,
                                                       0, 0, 0);
        // log-softmax over each group of KP lanes, in the accumulator layout
        glm_acc r;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int rb = row0 + 8 * g4 + 4 * h;
            const float4 yv = *reinterpret_cast<const float4*>(G.y + rb);
            const float ys[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int v = 4 * g4 + u;
                const float e = cls ? eta[v] + icpt : -__builtin_inff();
                const float m = glm_group_max<KP>(e);
                const float z = glm_group_sum<KP>(ex_exp(e - m));
                const float ll = e - (m + ex_log(z));
                const bool in = rb + u < G.N, hit = kf == ys[u];
                const float rr = in ? (hit ? 1.0f : 0.0f) - ex_exp(ll) : 0.0f;
                sl += (in && hit) ? ll : 0.0f;
                sr += rr;
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
                ex[1][j] = 0.0f;
                ex[2][j] = (w == 0) ? sl : ex[2][j] + sl;
            }
        }
        __syncthreads();
    }
    float* out = part + ((int64_t)s * gridDim.y + gb) * (int64_t)((PT * 32 + kGlmExtra) * 32);
    for (int e = tid; e < PT * 1024; e += 256) out[e] = coef[e];
    if (tid < 3 * kGlmChains) out[PT * 1024 + tid] = ex[tid >> 5][tid & 31];
}

}  // namespace mc
