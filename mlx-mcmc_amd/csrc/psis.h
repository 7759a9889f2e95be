// psis.h — PSIS-LOO over kept draws on the pointwise view (mc_psis_loo; no
// reference counterpart: its README roadmap lists "Model comparison (WAIC,
// LOO)").  Vehtari, Gelman and Gabry (2017), "Practical Bayesian model
// evaluation using leave-one-out cross-validation and WAIC"; the tail fit is
// Zhang and Stephens (2009) with the PSIS paper's weakly informative prior.
//
// Per observation o, over the N = C * S draws, with l_s the f32 pointwise value
// pointwise.h's pw_elem_value forms (the bits k_pointwise forms; -0 taken as +0)
// and everything after the selection in f64 (include/mcmc355.h states the
// definition in full):
//   Mt    tail length, psis_tail_len(N, r_eff)
//   L     the (Mt + 1)-th smallest l (with multiplicity); lmin the smallest
//   tail  { s : l_s < L }, n <= Mt values (ties at the cutoff drop out)
//   fit   generalized Pareto (khat, sigma) of y_j = exp(lmin - t_j) - exp(lmin - L)
//   lw    smoothed log weights of the tail; lmin - l_s elsewhere
//   elpd  log((N - n) + sum_tail exp(t + lw - lmin)) - log(sum_tail exp(lw) +
//         sum_rest exp(lmin - l)) + lmin
// The N x M matrix is never stored: the draws are re-evaluated per pass.
//
//   k_psis_count  grid (tiles, B), k_pointwise's tiling and draw blocks, one
//                 observation per thread.  One pass of an exact radix select
//                 of L on the order-preserving u32 key of l, 4 bits a pass:
//                 inside the observation's current bracket [lo, lo + 16 w),
//                 w = 2^shift, a draw's digit d bumps the counters c_j of the
//                 pivots lo + j w it lies below (j = 0 .. 15: sixteen counters
//                 in registers, a compare-and-add chain on the digit — no
//                 register indexing, no LDS, no atomics).  Also the block's
//                 smallest key.  Writes 17 u32 per (block, observation).
//   k_psis_pick   one thread per observation sums the blocks' counters and
//                 moves lo to the last pivot with at most Mt draws below it.
//                 After the eighth pass (w = 1) lo is L's key; that pass also
//                 stores n and the blocks' tail offsets (a prefix over blocks).
//   k_psis_gather the draw loop once more: l_s < L goes to the observation's
//                 slots of the tail buffer at the block's offset, the others
//                 into the block's f64 partial of sum_rest exp(lmin - l);
//                 counts the block's non-finite draws.
//   k_psis_fit    one wavefront per observation: the tail's keys are sorted in
//                 LDS (bitonic, padded to a power of two with the largest key),
//                 y is formed in LDS, psis_fit and the sums of the elpd run
//                 with lane-strided partial sums and a butterfly (a fixed
//                 order), lane 0 writes the six outputs.
// Integer counts and a fixed summation order: two calls give the same bits.
// The split depends on (C, S, the program) only; nothing waits on another
// workgroup; no atomics.  No loop's trip count depends on a value of l.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "philox.h"  // MC_HD

constexpr int kPsisMaxTail = 2048;  // largest Mt: bounds k_psis_fit's LDS
constexpr int kPsisMaxM = 76;       // > 30 + sqrt(kPsisMaxTail) grid points of the fit
static_assert((kPsisMaxM - 30) * (kPsisMaxM - 30) > kPsisMaxTail, "kPsisMaxM");

enum { PSIS_ELPD = 0, PSIS_KHAT, PSIS_SIGMA, PSIS_CUTOFF, PSIS_MIN, PSIS_TAILN, PSIS_COUNT };

// Mt = min(ceil(min(N / 5, 3 sqrt(N / r_eff))), N - 1)
inline int64_t psis_tail_len(int64_t N, double r_eff) {
    const double a = (double)N / 5.0, b = 3.0 * sqrt((double)N / r_eff);
    const double t = ceil(a < b ? a : b);
    return t < (double)(N - 1) ? (int64_t)t : N - 1;
}

// The order-preserving key of an f32 (-0 as +0): a < b  <=>  key(a) < key(b)
// for every non-NaN pair; NaNs sort outside the infinities by their sign.
MC_HD uint32_t psis_key(float x) {
    if (x == 0.0f) x = 0.0f;
    uint32_t u;
    memcpy(&u, &x, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MC_HD float psis_unkey(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float x;
    memcpy(&x, &u, 4);
    return x;
}

// How a sum over j is shared: the host walks j alone; a wavefront strides it
// over its lanes and adds the lanes' partials in a butterfly.
struct PsisSerial {
    static constexpr int W = 1;
    MC_HD int lane() const { return 0; }
    MC_HD double sum(double x) const { return x; }
    MC_HD void sync() const {}
};

MC_HD double psis_inf() { return (double)__builtin_inff(); }
MC_HD double psis_nan() { return __builtin_nan(""); }

// Steps 5 of the definition: (khat, sigma) of the ascending exceedances
// y[0 .. n).  work holds 2 m doubles, m = 30 + floor(sqrt(n)) (every lane of a
// wavefront stores the same values).  n <= 4: khat = +inf, sigma = NaN.  The
// arithmetic is IEEE all the way: a degenerate tail (all y equal may put a grid
// point at b = 0, 0 / 0) gives NaN khat and sigma, which smooth nothing.
template <class R>
MC_HD void psis_fit(const R& red, const double* y, int n, double* work, double* khat,
                    double* sigma) {
    if (n <= 4) {
        *khat = psis_inf();
        *sigma = psis_nan();
        return;
    }
    const int m = 30 + (int)floor(sqrt((double)n));
    const double dn = (double)n;
    const double yq = y[(int)floor(dn / 4.0 + 0.5) - 1], yn = y[n - 1];
    double* b = work;
    double* ll = work + m;
    for (int i = 1; i <= m; ++i) {
        const double bi = (1.0 - sqrt((double)m / ((double)i - 0.5))) / (3.0 * yq) + 1.0 / yn;
        double s = 0.0;
        for (int j = red.lane(); j < n; j += R::W) s += log1p(-bi * y[j]);
        const double k = red.sum(s) / dn;
        b[i - 1] = bi;
        ll[i - 1] = dn * (log(-bi / k) - k - 1.0);
    }
    red.sync();
    double sw = 0.0, swb = 0.0;
    for (int i = red.lane(); i < m; i += R::W) {
        double s = 0.0;
        for (int j = 0; j < m; ++j) s += exp(ll[j] - ll[i]);
        const double w = 1.0 / s;
        sw += w;
        swb += w * b[i];
    }
    const double bbar = red.sum(swb) / red.sum(sw);
    double s = 0.0;
    for (int j = red.lane(); j < n; j += R::W) s += log1p(-bbar * y[j]);
    const double kbar = red.sum(s) / dn;
    red.sync();
    *sigma = -kbar / bbar;
    *khat = (dn * kbar + 5.0) / (dn + 10.0);
}

MC_HD bool psis_smooths(double khat, double sigma) { return khat - khat == 0.0 && sigma > 0.0; }

// Step 6: the smoothed log weight of the tail's j-th value in rank order
// (j = 1 .. n, decreasing l), e_c = exp(lmin - L).
MC_HD double psis_lw(int j, int n, double khat, double sigma, double ec) {
    const double l1 = log1p(-((double)j - 0.5) / (double)n);
    const double q = fabs(khat) < DBL_EPSILON ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
    const double lw = log(q + ec);
    return lw < 0.0 ? lw : (lw != lw ? lw : 0.0);
}

#if defined(__HIPCC__)
#include "pointwise.h"

namespace mc {

constexpr int kPsisSlots = 17;  // sixteen counters and the smallest key

struct PsisWave {
    static constexpr int W = 64;
    MC_DEV int lane() const { return (int)(threadIdx.x & 63); }
    MC_DEV double sum(double x) const {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
        return x;
    }
    MC_DEV void sync() const { __syncthreads(); }
};

// The workspace of a launch (offsets in bytes; M observations, B blocks).
struct PsisWs {
    double* rest;     // [B, M]  the blocks' sum_rest exp(lmin - l)
    uint32_t* cnt;    // [B, 17, M]
    uint32_t* off;    // [B, M]  the blocks' first tail slot
    uint32_t* nf;     // [B, M]  the blocks' non-finite draws
    uint32_t* lo;     // [M]     the bracket's lower key; L's key at the end
    uint32_t* kmin;   // [M]     the smallest key
    uint32_t* ntail;  // [M]     n
    float* tail;      // [M, Mt] as gathered (unsorted)
};

template <int NMAX, bool LG>
__global__ __launch_bounds__(kPwBlock) void k_psis_count(PwCtx P, int64_t N, int64_t per,
                                                         const float* __restrict__ samples,
                                                         int shift, int first,
                                                         const uint32_t* __restrict__ lo,
                                                         uint32_t* __restrict__ cnt) {
    const PwTile tile = P.tiles[blockIdx.x];
    const DevTerm T = load_term(cptr(P.terms) + __builtin_amdgcn_readfirstlane(tile.term));
    const int64_t i = tile.e0 + threadIdx.x;
    if (i >= T.n) return;  // (no barrier and no LDS below)
    const int64_t o = tile.o0 + threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    const int64_t r1 = r0 + per < N ? r0 + per : N;
    const int64_t D = P.D;
    const PwElem E = pw_elem<NMAX>(T, P, i);
    const uint32_t base = first ? 0u : lo[o];
    uint32_t c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] = 0u;
    uint32_t kmin = 0xffffffffu;
#pragma unroll 1
    for (int64_t r = r0; r < r1; ++r) {
        const uint32_t key = psis_key(pw_elem_value<NMAX, LG>(E, T, P, samples + r * D, i));
        kmin = key < kmin ? key : kmin;
        // digit 0: below the bracket; d: in [lo + (d - 1) w, lo + d w); 17: above
        uint32_t d = (key - base) >> shift;
        d = key < base ? 0u : (d < 16u ? d : 16u) + 1u;
#pragma unroll
        for (int j = 0; j < 16; ++j) c[j] += d <= (uint32_t)j ? 1u : 0u;
    }
    uint32_t* out = cnt + (int64_t)blockIdx.y * kPsisSlots * P.M + o;
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j * P.M] = c[j];
    out[16 * P.M] = kmin;
}

static __global__ __launch_bounds__(256) void k_psis_pick(int64_t M, int32_t B, uint32_t Mt,
                                                          int shift, int first, int last,
                                                          PsisWs W) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= M) return;
    uint32_t c[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] = 0u;
    uint32_t kmin = 0xffffffffu;
    for (int b = 0; b < B; ++b) {
        const uint32_t* p = W.cnt + (int64_t)b * kPsisSlots * M + o;
#pragma unroll
        for (int j = 0; j < 16; ++j) c[j] += p[j * M];
        const uint32_t k = p[16 * M];
        kmin = k < kmin ? k : kmin;
    }
    // the last pivot with at most Mt draws below it (c is non-decreasing in j;
    // c[0] <= Mt: the bracket holds the draw of rank Mt)
    uint32_t js = 0u, cs = c[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const bool take = c[j] <= Mt;
        js = take ? (uint32_t)j : js;
        cs = take ? c[j] : cs;
    }
    const uint32_t base = first ? 0u : W.lo[o];
    W.lo[o] = base + (js << shift);
    W.kmin[o] = kmin;
    if (last) {
        W.ntail[o] = cs;
        uint32_t acc = 0u;
        for (int b = 0; b < B; ++b) {
            W.off[(int64_t)b * M + o] = acc;
            acc += W.cnt[((int64_t)b * kPsisSlots + js) * M + o];
        }
    }
}

template <int NMAX, bool LG>
__global__ __launch_bounds__(kPwBlock) void k_psis_gather(PwCtx P, int64_t N, int64_t per,
                                                          const float* __restrict__ samples,
                                                          uint32_t Mt, PsisWs W) {
    const PwTile tile = P.tiles[blockIdx.x];
    const DevTerm T = load_term(cptr(P.terms) + __builtin_amdgcn_readfirstlane(tile.term));
    const int64_t i = tile.e0 + threadIdx.x;
    if (i >= T.n) return;  // (no barrier and no LDS below)
    const int64_t o = tile.o0 + threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    const int64_t r1 = r0 + per < N ? r0 + per : N;
    const int64_t D = P.D;
    const PwElem E = pw_elem<NMAX>(T, P, i);
    const uint32_t kcut = W.lo[o];
    const double lmin = (double)psis_unkey(W.kmin[o]);
    uint32_t pos = W.off[(int64_t)blockIdx.y * P.M + o];
    float* __restrict__ slots = W.tail + o * (int64_t)Mt;
    double rest = 0.0;
    uint32_t nf = 0u;
#pragma unroll 1
    for (int64_t r = r0; r < r1; ++r) {
        const uint32_t key = psis_key(pw_elem_value<NMAX, LG>(E, T, P, samples + r * D, i));
        const float x = psis_unkey(key);
        nf += x - x == 0.0f ? 0u : 1u;
        if (key < kcut) {
            // (pos < Mt by the counts; the test keeps a store inside the slots)
            if (pos < Mt) slots[pos] = x;
            ++pos;
        } else {
            rest += exp(lmin - (double)x);
        }
    }
    W.rest[(int64_t)blockIdx.y * P.M + o] = rest;
    W.nf[(int64_t)blockIdx.y * P.M + o] = nf;
}

// LDS: y [Mt] f64, the fit's grid [2 kPsisMaxM] f64, the keys [P] u32.
inline size_t psis_fit_lds(int64_t Mt, int64_t P) {
    return (size_t)(Mt + 2 * kPsisMaxM) * sizeof(double) + (size_t)P * sizeof(uint32_t);
}

static __global__ __launch_bounds__(64) void k_psis_fit(int64_t M, int64_t N, int32_t B,
                                                        int32_t Mt, int32_t P, PsisWs W,
                                                        double* __restrict__ out,
                                                        float* __restrict__ tail_out) {
    extern __shared__ double psis_lds[];
    double* y = psis_lds;
    double* work = y + Mt;
    uint32_t* keys = (uint32_t*)(work + 2 * kPsisMaxM);
    const PsisWave red;
    const int lane = red.lane();
    const int64_t o = blockIdx.x;
    int n = (int)W.ntail[o];
    n = n < Mt ? n : Mt;
    const uint32_t kcut = W.lo[o], kmin = W.kmin[o];
    const float* __restrict__ slots = W.tail + o * (int64_t)Mt;
    for (int k = lane; k < P; k += 64) keys[k] = k < n ? psis_key(slots[k]) : 0xffffffffu;
    __syncthreads();
    // bitonic network over P keys, ascending
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            for (int t = lane; t < (P >> 1); t += 64) {
                const int a = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
                const int bb = a | stride;
                const bool up = (a & size) == 0;
                const uint32_t ka = keys[a], kb = keys[bb];
                if ((ka > kb) == up) {
                    keys[a] = kb;
                    keys[bb] = ka;
                }
            }
            __syncthreads();
        }
    }
    if (tail_out) {
        float* __restrict__ to = tail_out + o * (int64_t)Mt;
        for (int k = lane; k < Mt; k += 64) to[k] = k < n ? psis_unkey(keys[k]) : __builtin_nanf("");
    }
    const double lmin = (double)psis_unkey(kmin), cut = (double)psis_unkey(kcut);
    const double ec = exp(lmin - cut);
    // ascending y: rank j = k + 1 is the (n - 1 - k)-th key
    for (int k = lane; k < n; k += 64) y[k] = exp(lmin - (double)psis_unkey(keys[n - 1 - k])) - ec;
    __syncthreads();
    double khat, sigma;
    psis_fit(red, y, n, work, &khat, &sigma);
    const bool smooth = psis_smooths(khat, sigma);
    double s1 = 0.0, s2 = 0.0;
    for (int k = lane; k < n; k += 64) {
        const double t = (double)psis_unkey(keys[n - 1 - k]);
        const double lw = smooth ? psis_lw(k + 1, n, khat, sigma, ec) : lmin - t;
        s1 += exp(t + lw - lmin);
        s2 += exp(lw);
    }
    s1 = red.sum(s1);
    s2 = red.sum(s2);
    double rest = 0.0;
    uint32_t nf = 0u;
    for (int b = 0; b < B; ++b) {
        rest += W.rest[(int64_t)b * M + o];
        nf += W.nf[(int64_t)b * M + o];
    }
    double elpd = (log((double)(N - n) + s1) - log(s2 + rest)) + lmin;
    if (nf > 0u) elpd = khat = sigma = psis_nan();
    if (lane == 0) {
        out[PSIS_ELPD * M + o] = elpd;
        out[PSIS_KHAT * M + o] = khat;
        out[PSIS_SIGMA * M + o] = sigma;
        out[PSIS_CUTOFF * M + o] = cut;
        out[PSIS_MIN * M + o] = lmin;
        out[PSIS_TAILN * M + o] = (double)n;
    }
}

}  // namespace mc
#endif  // __HIPCC__
