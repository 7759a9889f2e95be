// glm_softmax_pointwise.h — per-observation log-likelihood statistics of a softmax
// regression program over kept draws (mc_pointwise_stats on a program of
// mc_program_create_glm_softmax).
//
// The value of observation i under draw r is log softmax(X_i B_r + a_r)[y_i].  Over
// all R = C * S draws the class logits are one GEMM with a long third dimension,
//     eta[N obs, R draws x K classes] = X[N, P] . B^T[P, R x K],
// followed by the log-softmax over each draw's K columns, the pick of the label's
// column and pointwise.h's f64 reduction over the draw axis.  Neither the N x R x K
// logits nor the N x R values are stored (unless the caller passes a matrix).
//
// k_glm_softmax_pointwise<PT, KP>: k_glm_pointwise's outer shape (glm_pointwise.h)
// with k_glm_softmax_grad's column packing (glm_softmax.h).  Grid (ceil(NT / 4),
// B draw blocks), 4 waves.
//   rows       wave w of workgroup x owns the 32-row tile 4 x + w for the whole
//              launch; its A operands stay in Pp / 2 registers, so X is read once
//              per draw block.
//   columns    the 32 columns of an MFMA tile are DPT = 32 / KP draws times KP
//              classes, class-minor: column n = dl KP + k is class k of the
//              tile's draw dl, KP = K rounded up to a power of two.  A macro-tile
//              of 32 draws is KP consecutive MFMA tiles.  At KP = 32 an MFMA tile
//              is one draw: the K logits of a draw are K columns of the product
//              whatever the packing, so that cost is the model's, not the layout's.
//   stage      per MFMA tile the DPT x P x K coefficients samples[n D + boff + p K
//              + k], consecutive lanes along (p, k) of one draw (a draw's B is
//              contiguous: coalesced but for the KP - K padded classes, which are
//              not read), stored to LDS as coef[p][n] with leading dimension 33;
//              padded classes, coefficients past P and draws past the block are 0.
//              Beside them the column's class intercept a_k (aoff >= 0).  Double-
//              buffered through registers as in k_glm_pointwise: the next tile's
//              global loads are issued before this tile's MFMAs and written to LDS
//              after its epilogue, between two barriers.
//   forward    k_glm_grad's loop: k ascending, two coefficients per
//              v_mfma_f32_32x32x2_f32.
//   softmax    in the accumulator layout (register v of lane l: row 8 (v / 4) +
//              4 (l / 32) + v % 4, column l % 32) the KP classes of a (row, draw)
//              pair are KP adjacent lanes: glm_group_max / glm_group_sum
//              (ds_swizzle xor exchanges; padded classes take -inf), ll = e - (m +
//              log z).  A NaN logit of any class makes z, and so every class's ll,
//              NaN (fmax drops a NaN from m; the sum keeps it).
//   compaction the one lane of a group whose class is the row's label writes ll to
//              the wave's private patch [32 rows][33] at column (the draw's index
//              in the macro-tile): one predicated LDS store per (row, draw).
//   turn       after the macro-tile's last MFMA tile (or the block's last): the
//              patch is k_glm_pointwise's, and so are gpw_turn, gpw_finish, the
//              partial layout and k_pw_merge.  Columns of draws past the block hold
//              stale values that the turn masks by the block's end.
// Rows past N (label 0 of the zero padding: computed, never written), coefficients
// past P, classes past K and draws past the block are zero operands or masked:
// nothing reads past an array and nothing masked is accumulated.  Labels were
// checked when the program was made: every (row, draw) has exactly one hit lane.
#pragma once
#include "glm_pointwise.h"
#include "glm_softmax.h"

namespace mc {

template <int PT, int KP>
__global__ void __launch_bounds__(256)
k_glm_softmax_pointwise(GlmDev G, int64_t R, int64_t per, const float* __restrict__ samples,
                        double* __restrict__ part, float* __restrict__ matrix) {
    static_assert(KP >= 2 && KP <= 32 && (KP & (KP - 1)) == 0, "KP: a power of two in 2 .. 32");
    constexpr int Pp = 32 * PT;
    constexpr int DPT = 32 / KP;  // draws per MFMA tile
    constexpr int NPRE = 4 * PT;  // staged coefficients per thread and MFMA tile
    __shared__ float coef[Pp * kGpwLd];
    __shared__ float ex[kGlmChains];         // per column: the class intercept
    __shared__ float obs[4][32];             // per wave: the labels of its rows
    __shared__ float patch[4][32 * kGpwLd];  // per wave: the macro-tile's values, the turn
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 31, h = lane >> 5;
    const int t = blockIdx.x * 4 + wave;
    const bool act = t < G.NT;  // (an idle wave computes its workgroup's last tile, unwritten)
    const int row0 = (act ? t : G.NT - 1) * 32;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    const int64_t r1 = r0 + per < R ? r0 + per : R;
    const int64_t D = G.D;
    const int K = G.K;

    // ---- the stage: the next MFMA tile's global loads, then their LDS stores --
    float pre[NPRE], pa = 0.0f;
    auto fetch = [&](int64_t n0) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = tid + 256 * i, dl = e / (Pp * KP), p = e % (Pp * KP) / KP, k = e % KP;
            const int64_t n = n0 + dl;
            pre[i] = (p < G.P && k < K && n < r1) ? samples[n * D + G.boff + p * K + k] : 0.0f;
        }
        if (tid < kGlmChains) {
            const int64_t n = n0 + tid / KP;
            const int k = tid % KP;
            pa = (G.aoff >= 0 && k < K && n < r1) ? samples[n * D + G.aoff + k] : 0.0f;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = tid + 256 * i, dl = e / (Pp * KP), p = e % (Pp * KP) / KP, k = e % KP;
            coef[p * kGpwLd + dl * KP + k] = pre[i];
        }
        if (tid < kGlmChains) ex[tid] = pa;
    };
    fetch(r0);

    // ---- the wave's rows: their labels; its A operands -------------------------
    if (lane < 32) obs[wave][lane] = G.y[row0 + lane];
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
    const int kc = j % KP, dj = j / KP;  // before the turn: the lane's class, of draw dj
    const bool cls = kc < K;
    const float kf = (float)kc;

    const int64_t nt = (r1 - r0 + DPT - 1) / DPT;  // MFMA tiles of the block
    for (int64_t T = 0; T < nt; ++T) {
        const bool more = T + 1 < nt;  // (workgroup-uniform)
        if (more) fetch(r0 + (T + 1) * DPT);
        // forward: eta[32 rows][DPT draws x KP classes], two coefficients per MFMA
        glm_acc eta;
#pragma unroll
        for (int v = 0; v < 16; ++v) eta[v] = 0.0f;
        const float* bc = coef + h * kGpwLd + j;
#pragma unroll
        for (int k = 0; k < PT * 16; ++k)
            eta = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], bc[k * 2 * kGpwLd], eta, 0, 0, 0);
        // log-softmax over each group of KP lanes; the label's lane keeps the value
        const int mt = (int)(T % KP);  // the MFMA tile's place in its macro-tile
        const float icpt = ex[j];
        float* pc = pt + mt * DPT + dj;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int rb = 8 * g4 + 4 * h;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float e = cls ? eta[4 * g4 + u] + icpt : -__builtin_inff();
                const float m = glm_group_max<KP>(e);
                const float z = glm_group_sum<KP>(ex_exp(e - m));
                const float ll = e - (m + ex_log(z));
                if (kf == obs[wave][rb + u]) pc[(rb + u) * kGpwLd] = ll;
            }
        }
        if (mt == KP - 1 || !more) {
            gpw_wave_sync();
            // turned: the lane is observation j and takes draws 16 h .. 16 h + 15
            gpw_turn(A, nfsum, pt, j, h, r0 + (T - mt) * DPT, r1, matrix, own, G.N, o);
        }
        __syncthreads();  // every wave is done with coef / ex (and its patch)
        if (more) store();
        __syncthreads();
    }

    gpw_finish(A, nfsum, h, own, part + (int64_t)blockIdx.y * PW_COUNT * G.N + o, G.N);
}

}  // namespace mc
