// rankdiag.h — rank-normalised split R-hat, bulk-ESS and tail-ESS (Vehtari,
// Gelman, Simpson, Carpenter and Buerkner 2021) of a [C, S, D] f32 sample
// buffer; the definition is stated in include/mcmc355.h (mc_rank_diag).
//
// A batch of Db elements is processed where the buffer lies.  Per element the
// N = 2C * n split draws (n = S / 2) lie column-contiguous in the workspace in
// position order p = j * n + i (split chain j, draw i).
//
//   k_rd_stage     transpose through LDS: coalesced rows of [C, S, D] in,
//                  columns y[e][p] and their order-preserving u32 keys (-0
//                  taken as +0) out; NaN flag per element (an integer OR).
//   k_rd_fold      the second ranking: keys of |y - median| (f32).
//   k_rd_sort_lds  (key, position) pairs of one element sorted in a
//                  workgroup's LDS: stable LSD radix sort, 4-bit digits.  Every
//                  thread owns a contiguous run of the pairs; its 16 counts go
//                  to cnt[digit][thread], whose exclusive scan in that order is
//                  the stable destination of each thread's first pair of a
//                  digit.  No atomics: a thread alone advances its counters.
//   k_rd_ghist /   the same sort across workgroups for a column that does not
//   k_rd_gscan /   fit: per pass a digit histogram per tile (integer LDS
//   k_rd_gscatter  atomics: counts are order-independent), an exclusive scan
//                  over [digit][tile] by one workgroup per element, and a
//                  stable scatter — the tile ranked in LDS as above, offset by
//                  the scanned base of its (digit, tile).
//   k_rd_rank      per sorted position the run of equal keys by two binary
//                  searches, r = (first + last) / 2 + 1, z = ndtri((r - 3/8) /
//                  (N + 1/4)) scattered back to position order; the pool's
//                  median, q05 and q95 straight from the sorted column
//                  (numpy's 'linear' rule on f32).
//   k_rd_acov      one workgroup per (element, quantity): waves take split
//                  chains sixteen at a time (held in LDS while n <= 1024), lanes
//                  stride over the draws, eight lags per pass; the chains' sums
//                  are added in chain order by one thread, which then advances
//                  the sequence rule (rd_geyer_*) and stops the loop.  f64
//                  throughout.
//   k_rd_final     NaN elements, the larger R-hat, the smaller tail ESS.
#pragma once

namespace mc {

constexpr int kRdLagBlock = 8;
constexpr int kRdThreads = 256;
constexpr int kRdAcovWaves = 16;                 // k_rd_acov: split chains in flight
constexpr int kRdDigits = 16;                    // 4-bit digits, 8 passes
constexpr int kRdCnt = kRdDigits * kRdThreads;   // cnt[digit][thread]
constexpr int kRdTileRun = 17;                   // pairs per thread of a global tile (odd:
                                                 // the threads' runs start on distinct banks)
constexpr int kRdTile = kRdThreads * kRdTileRun;
constexpr int64_t kRdLdsMaxN = 8192;             // largest column k_rd_sort_lds takes
constexpr int kRdStageE = 32, kRdStageP = 64;    // k_rd_stage tile: elements x positions

enum { RD_Q_BULK = 0, RD_Q_LO = 1, RD_Q_HI = 2, RD_Q_FOLD = 3 };

// ---------------------------------------------------------------------------
// The sequence rule of Stan's compute_effective_sample_size, as a stream: the
// caller hands over (rho_{t+1}, rho_{t+2}) for as long as rd_geyer_wants.  The
// monotone pass needs no stored sequence: a pair that is not the last one read
// contributes min(its sum, the previous pair's contribution), added when the
// next pair arrives.
// ---------------------------------------------------------------------------
struct RdGeyer {
    int64_t t;
    double even, odd;   // the last pair read
    double sum;         // of the pairs before it, after the monotone pass
    double prev;        // what the pair before it contributed
};
MC_HD void rd_geyer_init(RdGeyer& g, double rho1) {
    g.t = 1;
    g.even = 1.0;
    g.odd = rho1;
    g.sum = 0.0;
    g.prev = 0.0;
}
MC_HD bool rd_geyer_wants(const RdGeyer& g, int64_t n) {
    return g.t < n - 3 && g.even + g.odd > 0.0;
}
MC_HD void rd_geyer_push(RdGeyer& g, double even, double odd) {
    double pair = g.even + g.odd;
    if (g.t > 1 && pair > g.prev) pair = g.prev;
    g.sum += pair;
    g.prev = pair;
    g.even = even;
    g.odd = odd;
    g.t += 2;
}
MC_HD double rd_geyer_ess(const RdGeyer& g, int64_t N) {
    // r[max_t + 1]: the last even if positive; else what the first loop left
    // there (the even of a pair it wrote, 0 of one it did not)
    double last = 0.0;
    if (g.even > 0.0 || g.even + g.odd >= 0.0) last = g.even;
    double tau = -1.0 + 2.0 * g.sum + last;
    const double floor_ = 1.0 / log10((double)N);
    if (tau < floor_) tau = floor_;
    return (double)N / tau;
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------
struct RdWs {             // a batch's arrays (run_rankdiag.hip rd_carve)
    double* z;            // [Db, N] z-scores, position order
    double* tail;         // [Db, 2] ESS of the two indicators
    double* cmean;        // [Db, 3, 2C] split-chain means of z and the two indicators
    float* y;             // [Db, N] staged draws, position order
    float* q;             // [Db, 4] median, q05, q95, (unused)
    uint32_t* key[2];     // [Db, N] ping-pong keys
    uint32_t* pos[2];     // [Db, N] ping-pong positions
    uint32_t* hist;       // [Db, 16, tiles]
    uint32_t* flag;       // [Db, 4] NaN draw, NaN folded value, constant, (unused)
};
struct RdQuant {          // numpy's 'linear' percentile of N f32 values
    int64_t lo[2], hi[2];
    float g[2];
};

__device__ __forceinline__ uint32_t rd_key(float f) {
    if (f == 0.0f) f = 0.0f;   // -0 and +0 are equal
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rd_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// x[c, s, d0 + e] -> y[e][j * n + i], key[0][e][...]; grid (2C * tiles of n, tiles of Db)
__global__ __launch_bounds__(kRdThreads) void k_rd_stage(const float* __restrict__ x, int64_t S,
                                                         int64_t D, int64_t d0, int64_t Db,
                                                         int64_t n, int64_t N, RdWs W) {
    __shared__ float tile[kRdStageP][kRdStageE + 1];
    const int64_t tiles = (n + kRdStageP - 1) / kRdStageP;
    const int64_t j = blockIdx.x / tiles, i0 = (blockIdx.x - j * tiles) * kRdStageP;
    const int64_t e0 = (int64_t)blockIdx.y * kRdStageE;
    const int64_t c = j >> 1, s0 = (j & 1) ? S - n : 0;
    for (int idx = threadIdx.x; idx < kRdStageE * kRdStageP; idx += kRdThreads) {
        const int e = idx % kRdStageE, pp = idx / kRdStageE;
        if (i0 + pp < n && e0 + e < Db)
            tile[pp][e] = x[(c * S + s0 + i0 + pp) * D + d0 + e0 + e];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kRdStageE * kRdStageP; idx += kRdThreads) {
        const int pp = idx % kRdStageP, e = idx / kRdStageP;
        if (i0 + pp < n && e0 + e < Db) {
            const float v = tile[pp][e];
            const int64_t at = (e0 + e) * N + j * n + i0 + pp;
            W.y[at] = v;
            W.key[0][at] = rd_key(v);
            if (v != v) atomicOr(&W.flag[(e0 + e) * 4 + 0], 1u);
        }
    }
}

// key[0][e][p] = key(|y - median|); grid (ceil(N / 256), Db)
__global__ __launch_bounds__(kRdThreads) void k_rd_fold(int64_t N, RdWs W) {
    const int64_t e = blockIdx.y, p = (int64_t)blockIdx.x * kRdThreads + threadIdx.x;
    if (p >= N) return;
    const float v = fabsf(W.y[e * N + p] - W.q[e * 4 + 0]);
    W.key[0][e * N + p] = rd_key(v);
    if (v != v) atomicOr(&W.flag[e * 4 + 1], 1u);
}

// ---- the ranking of a run of pairs held in LDS -----------------------------
// Thread t owns pairs [lo, hi).  rd_count: its 16 digit counts to
// cnt[digit][t].  rd_scan: cnt becomes its exclusive prefix in [digit][thread]
// order (scan: 256 words of scratch).  A thread then walks its run again and
// takes cnt[digit][t]++ as each pair's stable rank.
__device__ __forceinline__ void rd_count(const uint32_t* __restrict__ keys, int lo, int hi,
                                         int shift, uint32_t* __restrict__ cnt) {
    uint32_t c[kRdDigits];
#pragma unroll
    for (int d = 0; d < kRdDigits; ++d) c[d] = 0u;
    for (int i = lo; i < hi; ++i) {
        const uint32_t dig = (keys[i] >> shift) & 15u;
#pragma unroll
        for (int d = 0; d < kRdDigits; ++d) c[d] += dig == (uint32_t)d ? 1u : 0u;
    }
#pragma unroll
    for (int d = 0; d < kRdDigits; ++d) cnt[d * kRdThreads + threadIdx.x] = c[d];
}
__device__ __forceinline__ void rd_scan(uint32_t* __restrict__ cnt, uint32_t* __restrict__ scan) {
    __syncthreads();
    const int t = threadIdx.x;
    uint32_t s = 0u;
#pragma unroll
    for (int k = 0; k < kRdDigits; ++k) s += cnt[t * kRdDigits + k];
    scan[t] = s;
    __syncthreads();
    for (int o = 1; o < kRdThreads; o <<= 1) {
        const uint32_t add = t >= o ? scan[t - o] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    uint32_t run = scan[t] - s;   // exclusive
#pragma unroll
    for (int k = 0; k < kRdDigits; ++k) {
        const uint32_t c = cnt[t * kRdDigits + k];
        cnt[t * kRdDigits + k] = run;
        run += c;
    }
    __syncthreads();
}

// dynamic LDS of k_rd_sort_lds for a column of N pairs
inline size_t rd_sort_lds_bytes(int64_t N) {
    return (size_t)(4 * N) * 4 + (size_t)(kRdCnt + kRdThreads) * 4;
}
// One workgroup per element: key[0] in, sorted key[0] / pos[0] out.
__global__ __launch_bounds__(kRdThreads) void k_rd_sort_lds(int64_t N64, RdWs W) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rd_lds[];
    const int N = (int)N64, t = threadIdx.x;
    uint32_t* kb[2] = {rd_lds, rd_lds + N};
    uint32_t* pb[2] = {rd_lds + 2 * N, rd_lds + 3 * N};
    uint32_t* cnt = rd_lds + 4 * N;
    uint32_t* scan = cnt + kRdCnt;
    uint32_t* gk = W.key[0] + (int64_t)blockIdx.x * N64;
    uint32_t* gp = W.pos[0] + (int64_t)blockIdx.x * N64;
    for (int i = t; i < N; i += kRdThreads) {
        kb[0][i] = gk[i];
        pb[0][i] = (uint32_t)i;
    }
    __syncthreads();
    const int run = ((N + kRdThreads - 1) / kRdThreads) | 1;
    const int lo = min(N, t * run), hi = min(N, lo + run);
    int cur = 0;
    for (int shift = 0; shift < 32; shift += 4) {
        const uint32_t* ki = kb[cur];
        const uint32_t* pi = pb[cur];
        uint32_t* ko = kb[cur ^ 1];
        uint32_t* po = pb[cur ^ 1];
        rd_count(ki, lo, hi, shift, cnt);
        rd_scan(cnt, scan);
        for (int i = lo; i < hi; ++i) {
            const uint32_t k = ki[i], dig = (k >> shift) & 15u;
            const uint32_t dst = cnt[dig * kRdThreads + t]++;
            ko[dst] = k;
            po[dst] = pi[i];
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int i = t; i < N; i += kRdThreads) {   // (8 passes: the result is in buffer 0)
        gk[i] = kb[0][i];
        gp[i] = pb[0][i];
    }
}

// ---- the same sort across workgroups ---------------------------------------
// grid (tiles, Db); hist[e][digit][tile]
__global__ __launch_bounds__(kRdThreads) void k_rd_ghist(int64_t N, int64_t tiles, int shift,
                                                         const uint32_t* __restrict__ kin,
                                                         uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[kRdDigits];
    if (threadIdx.x < kRdDigits) h[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t e = blockIdx.y, b = blockIdx.x, base = b * kRdTile;
    const int len = (int)min((int64_t)kRdTile, N - base);
    for (int i = threadIdx.x; i < len; i += kRdThreads)
        atomicAdd(&h[(kin[e * N + base + i] >> shift) & 15u], 1u);
    __syncthreads();
    if (threadIdx.x < kRdDigits) hist[(e * kRdDigits + threadIdx.x) * tiles + b] = h[threadIdx.x];
}
// one workgroup per element: hist[e] becomes its exclusive prefix
__global__ __launch_bounds__(kRdThreads) void k_rd_gscan(int64_t tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t scan[kRdThreads];
    const int t = threadIdx.x;
    const int64_t total = kRdDigits * tiles, run = (total + kRdThreads - 1) / kRdThreads;
    uint32_t* h = hist + (int64_t)blockIdx.x * total;
    const int64_t lo = min(total, t * run), hi = min(total, lo + run);
    uint32_t s = 0u;
    for (int64_t i = lo; i < hi; ++i) s += h[i];
    scan[t] = s;
    __syncthreads();
    for (int o = 1; o < kRdThreads; o <<= 1) {
        const uint32_t add = t >= o ? scan[t - o] : 0u;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    uint32_t acc = scan[t] - s;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t c = h[i];
        h[i] = acc;
        acc += c;
    }
}
// grid (tiles, Db): a tile's pairs to their places in the pass's output.
// first: positions are the indices themselves (pin is not read).
__global__ __launch_bounds__(kRdThreads) void k_rd_gscatter(int64_t N, int64_t tiles, int shift,
                                                            int first,
                                                            const uint32_t* __restrict__ kin,
                                                            const uint32_t* __restrict__ pin,
                                                            const uint32_t* __restrict__ hist,
                                                            uint32_t* __restrict__ kout,
                                                            uint32_t* __restrict__ pout) {
    __shared__ uint32_t kl[kRdTile], pl[kRdTile], cnt[kRdCnt], scan[kRdThreads];
    __shared__ uint32_t shiftd[kRdDigits];   // scanned base - the digit's start in the tile
    const int t = threadIdx.x;
    const int64_t e = blockIdx.y, b = blockIdx.x, base = b * kRdTile;
    const int len = (int)min((int64_t)kRdTile, N - base);
    for (int i = t; i < len; i += kRdThreads) {
        kl[i] = kin[e * N + base + i];
        pl[i] = first ? (uint32_t)(base + i) : pin[e * N + base + i];
    }
    __syncthreads();
    const int lo = min(len, t * kRdTileRun), hi = min(len, lo + kRdTileRun);
    rd_count(kl, lo, hi, shift, cnt);
    rd_scan(cnt, scan);
    if (t < kRdDigits)
        shiftd[t] = hist[(e * kRdDigits + t) * tiles + b] - cnt[t * kRdThreads];
    __syncthreads();
    for (int i = lo; i < hi; ++i) {
        const uint32_t k = kl[i], dig = (k >> shift) & 15u;
        const int64_t dst = (int64_t)(cnt[dig * kRdThreads + t]++ + shiftd[dig]);
        kout[e * N + dst] = k;
        pout[e * N + dst] = pl[i];
    }
}

// ---- ranks -------------------------------------------------------------------
__device__ __forceinline__ float rd_lerp(float a, float b, float g) {
    const float diff = b - a;
    float r = a + diff * g;
    if (g >= 0.5f) r = b - diff * (1.0f - g);
    return r;
}
// grid (ceil(N / 256), Db).  fold = 0: z of the draws, the pool statistics and
// the constant flag; 1: z of the folded values.  zout: NULL or the caller's
// [D, N] copy of the bulk z-scores, at this batch's first element.
__global__ __launch_bounds__(kRdThreads) void k_rd_rank(int64_t N, int fold, RdQuant Q, RdWs W,
                                                        double* __restrict__ zout) {
    const int64_t e = blockIdx.y, i = (int64_t)blockIdx.x * kRdThreads + threadIdx.x;
    const uint32_t* __restrict__ sk = W.key[0] + e * N;
    if (!fold && i == 0) {
        const float a = rd_unkey(sk[(N - 1) / 2]), b = rd_unkey(sk[N / 2]);
        W.q[e * 4 + 0] = (N & 1) ? a : (a + b) / 2.0f;
        W.q[e * 4 + 1] = rd_lerp(rd_unkey(sk[Q.lo[0]]), rd_unkey(sk[Q.lo[1]]), Q.g[0]);
        W.q[e * 4 + 2] = rd_lerp(rd_unkey(sk[Q.hi[0]]), rd_unkey(sk[Q.hi[1]]), Q.g[1]);
        W.flag[e * 4 + 2] = sk[0] == sk[N - 1] ? 1u : 0u;
    }
    if (i >= N) return;
    const uint32_t k = sk[i];
    int64_t first = i, last = i;
    if (i > 0 && sk[i - 1] == k) {          // the first index whose key is >= k
        int64_t lo = 0, hi = i - 1;         // sk[hi] == k
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (sk[mid] < k) lo = mid + 1; else hi = mid;
        }
        first = lo;
    }
    if (i + 1 < N && sk[i + 1] == k) {      // the last index whose key is <= k
        int64_t lo = i + 1, hi = N - 1;     // sk[lo] == k
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if (sk[mid] > k) hi = mid - 1; else lo = mid;
        }
        last = lo;
    }
    const double r = (double)(first + last) * 0.5 + 1.0;
    const double z = normcdfinv((r - 0.375) / ((double)N + 0.25));
    const int64_t p = W.pos[0][e * N + i];
    W.z[e * N + p] = z;
    if (!fold && zout) zout[e * N + p] = z;
}

// ---- moments, autocovariance, the sequence rule -----------------------------
__device__ __forceinline__ double rd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// grid (quantities, Db), quantity q0 + blockIdx.x: RD_Q_BULK z (R-hat and ESS),
// RD_Q_LO / RD_Q_HI the indicators 1[y <= q05], 1[y <= q95] formed from the
// staged column (ESS), RD_Q_FOLD z of the folded values (R-hat alone: lag 0).
// out: the caller's [MC_RD_COUNT, D] at this batch's first element.
// ST: n <= kRdAcovStageN, every wave holds its split chain in LDS for the nine
// reads a lag block makes of it (else they go to global memory: the shifted
// windows of sixteen chains do not stay in a CU's vector cache).  The same
// arithmetic in the same order either way.
constexpr int64_t kRdAcovStageN = 1024;
constexpr size_t kRdAcovFixedLds = (kRdAcovWaves * (kRdLagBlock + 1) + 2) * 8;
inline size_t rd_acov_lds_bytes(int64_t n) {
    return kRdAcovFixedLds + (n <= kRdAcovStageN ? (size_t)(kRdAcovWaves * n) * 8 : 0);
}
template <bool ST>
__global__ __launch_bounds__(64 * kRdAcovWaves) void k_rd_acov(int64_t m, int64_t n, int q0, RdWs W,
                                                        int64_t D, double* __restrict__ out,
                                                        int row_rhat_bulk, int row_rhat_folded,
                                                        int row_ess_bulk) {
    // all of the LDS is dynamic, every carve offset a multiple of 16 bytes
    extern __shared__ __attribute__((aligned(16))) double rd_acov_lds[];
    double (*part)[kRdLagBlock] = (double (*)[kRdLagBlock])rd_acov_lds;
    double* pmean = rd_acov_lds + kRdAcovWaves * kRdLagBlock;
    int& sdone = *(int*)(pmean + kRdAcovWaves);
    const int q = q0 + blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* sv = pmean + kRdAcovWaves + 2 + (ST ? (int64_t)w * n : 0);   // this wave's chain
    const int64_t e = blockIdx.y, N = m * n;
    const double* __restrict__ zc = W.z + e * N;
    const float* __restrict__ yc = W.y + e * N;
    const bool ind = q == RD_Q_LO || q == RD_Q_HI;
    const float thr = ind ? W.q[e * 4 + q] : 0.0f;
    auto val = [&](int64_t at) -> double {
        return ind ? (yc[at] <= thr ? 1.0 : 0.0) : zc[at];
    };
    const int nl = q == RD_Q_FOLD ? 1 : kRdLagBlock;
    // thread 0: chain-order sums, Welford over the chain means, the rule
    double asum[kRdLagBlock];
    double gmean = 0.0, gm2 = 0.0, Wv = 0.0, vp = 0.0;
    RdGeyer G;
    rd_geyer_init(G, 0.0);
    for (int64_t l0 = 0;; l0 += kRdLagBlock) {
#pragma unroll
        for (int t = 0; t < kRdLagBlock; ++t) asum[t] = 0.0;
        for (int64_t j0 = 0; j0 < m; j0 += kRdAcovWaves) {
            const int64_t j = j0 + w;
            double acc[kRdLagBlock];
#pragma unroll
            for (int t = 0; t < kRdLagBlock; ++t) acc[t] = 0.0;
            double mean = 0.0;
            if (ST) {
                if (j < m)
                    for (int64_t i = lane; i < n; i += 64) sv[i] = val(j * n + i);
                __syncthreads();
            }
            if (j < m) {
                const int64_t cb = j * n;
                auto rd = [&](int64_t i) -> double { return ST ? sv[i] : val(cb + i); };
                if (l0 == 0) {
                    double s = 0.0;
#pragma unroll 4
                    for (int64_t i = lane; i < n; i += 64) s += rd(i);
                    mean = rd_wave_sum(s) / (double)n;
                    if (lane == 0 && q != RD_Q_FOLD) W.cmean[(e * 3 + q) * m + j] = mean;
                } else {
                    mean = W.cmean[(e * 3 + q) * m + j];
                }
#pragma unroll 2
                for (int64_t i = lane; i + l0 < n; i += 64) {
                    const double v = rd(i) - mean;
#pragma unroll
                    for (int t = 0; t < kRdLagBlock; ++t) {
                        const int64_t ii = i + l0 + t;
                        if (t < nl && ii < n) acc[t] += v * (rd(ii) - mean);
                    }
                }
#pragma unroll
                for (int t = 0; t < kRdLagBlock; ++t) acc[t] = rd_wave_sum(acc[t]);
            }
            if (lane == 0) {
#pragma unroll
                for (int t = 0; t < kRdLagBlock; ++t) part[w][t] = acc[t];
                pmean[w] = mean;
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                for (int ww = 0; ww < kRdAcovWaves && j0 + ww < m; ++ww) {
#pragma unroll
                    for (int t = 0; t < kRdLagBlock; ++t) asum[t] += part[ww][t];
                    if (l0 == 0) {
                        const double dlt = pmean[ww] - gmean;
                        gmean += dlt / (double)(j0 + ww + 1);
                        gm2 += dlt * (pmean[ww] - gmean);
                    }
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            bool done = false;
            const double nm = (double)n * (double)m;
            if (l0 == 0) {
                const double a0 = asum[0] / nm;
                Wv = a0 * (double)n / (double)(n - 1);
                vp = ((double)(n - 1) / (double)n) * Wv + gm2 / (double)(m - 1);
                const double nan = __longlong_as_double(0x7ff8000000000000ll);
                const bool ok = Wv > 0.0;
                const double rhat = ok ? sqrt(vp / Wv) : nan;
                if (q == RD_Q_BULK) out[row_rhat_bulk * D + e] = rhat;
                if (q == RD_Q_FOLD) out[row_rhat_folded * D + e] = rhat;
                if (q == RD_Q_FOLD) done = true;
                if (!ok) {
                    if (q == RD_Q_BULK) out[row_ess_bulk * D + e] = nan;
                    if (ind) W.tail[e * 2 + (q - RD_Q_LO)] = nan;
                    done = true;
                }
            }
            if (!done) {
                // rho_t of this block's lags (lag 0 of the first block is not used)
                double rho[kRdLagBlock];
#pragma unroll
                for (int t = 0; t < kRdLagBlock; ++t) rho[t] = 1.0 - (Wv - asum[t] / nm) / vp;
                if (l0 == 0) rd_geyer_init(G, rho[1]);
#pragma unroll
                for (int t = 0; t < kRdLagBlock; t += 2) {
                    if (t == 0 && l0 == 0) continue;   // (rho_0, rho_1): the rule's start
                    if (rd_geyer_wants(G, n)) rd_geyer_push(G, rho[t], rho[t + 1]);
                }
                if (!rd_geyer_wants(G, n) || l0 + kRdLagBlock >= n) {
                    const double ess = rd_geyer_ess(G, N);
                    if (q == RD_Q_BULK) out[row_ess_bulk * D + e] = ess;
                    if (ind) W.tail[e * 2 + (q - RD_Q_LO)] = ess;
                    done = true;
                }
            }
            sdone = done ? 1 : 0;
        }
        __syncthreads();
        if (sdone) break;
    }
}

// one thread per element of the batch: out at this batch's first element
__global__ __launch_bounds__(kRdThreads) void k_rd_final(int64_t Db, int64_t D, RdWs W,
                                                         double* __restrict__ out, int row_rhat_bulk,
                                                         int row_rhat_folded, int row_rhat_rank,
                                                         int row_ess_bulk, int row_ess_tail,
                                                         int row_constant) {
    const int64_t e = (int64_t)blockIdx.x * kRdThreads + threadIdx.x;
    if (e >= Db) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double rb = out[row_rhat_bulk * D + e], rf = out[row_rhat_folded * D + e];
    double eb = out[row_ess_bulk * D + e];
    double t0 = W.tail[e * 2 + 0], t1 = W.tail[e * 2 + 1];
    if (W.flag[e * 4 + 1]) rf = nan;
    if (W.flag[e * 4 + 0]) rb = rf = eb = t0 = t1 = nan;
    out[row_rhat_bulk * D + e] = rb;
    out[row_rhat_folded * D + e] = rf;
    out[row_rhat_rank * D + e] = (rb != rb || rf != rf) ? nan : (rb > rf ? rb : rf);
    out[row_ess_bulk * D + e] = eb;
    out[row_ess_tail * D + e] = (t0 != t0 || t1 != t1) ? nan : (t0 < t1 ? t0 : t1);
    out[row_constant * D + e] = (!W.flag[e * 4 + 0] && W.flag[e * 4 + 2]) ? 1.0 : 0.0;
}

// n < 4: nothing is defined
__global__ __launch_bounds__(kRdThreads) void k_rd_fill(double* __restrict__ p, int64_t count,
                                                        double v) {
    const int64_t i = (int64_t)blockIdx.x * kRdThreads + threadIdx.x;
    if (i < count) p[i] = v;
}
#endif  // __HIPCC__

}  // namespace mc
