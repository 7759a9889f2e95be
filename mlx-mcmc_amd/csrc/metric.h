// metric.h — per-chain diagonal mass matrix M = diag(1 / minv) of the
// chain-per-workgroup samplers (k_hmc, k_nuts with MET) and of the register-only
// lane-resident NUTS kernel (k_nuts_lr with MET, nuts_lanes.h), and its windowed
// adaptation (Stan's scheme, per chain, inside the persistent kernel).
//
//   momentum   r_j = z_j * msqrt_j         msqrt_j = 1 / sqrt(minv_j), z as without a metric
//   velocity   v_j = minv_j * r_j
//   kinetic    0.5 sum r_j * v_j
//   drift      q_j += e * v_j              kicks and the U-turn test (on r) unchanged
// With minv = 1 every added product is an exact multiply by 1.0f: the draws of
// a run without a metric, bit for bit.
//
// Metric buffer (device memory, mc_metric_bytes; sections 256-byte aligned):
//   [MetricScalars x C][minv C x D][msqrt C x D][mean C x D][M2 C x D]   (f32)
// mean / M2 are the Welford accumulator of the current window (f32: a window
// holds at most a few thousand draws), n_window its count.  The state lives in
// the buffer, so a run may be cut into launches anywhere.
#pragma once
#include <stdint.h>
#include "internal.h"
#include "philox.h"

namespace mc {

// n_window: draws in the accumulator; n_updates: metric updates so far;
// da_origin: NUTS, the iteration at which dual averaging last restarted
typedef mc_metric_scalars MetricScalars;

// kernel argument of the MET instantiations
struct MetricDev {
    MetricScalars* sc;
    float* minv;
    float* msqrt;
    float* mean;
    float* m2;
    int32_t adapt;   // accumulate and update during warmup
    int32_t in_lds;  // LDS arena: minv and msqrt sit after it in LDS
};

// Stan's warmup schedule, a pure function of num_warmup W: a fast phase of
// `init` iterations, slow windows in [init, W - term), `term` fast iterations.
// base == 0: nothing is adapted (W < 20).
struct MetricSchedule {
    int64_t init, term, base;
};
MC_HD MetricSchedule metric_schedule(int64_t W) {
    MetricSchedule s = {75, 50, 25};
    if (W < 20) {
        s.init = s.term = s.base = 0;
    } else if (s.init + s.term + s.base > W) {
        s.init = 15 * W / 100;  // floor(0.15 W), floor(0.1 W)
        s.term = W / 10;
        s.base = W - s.init - s.term;
    }
    return s;
}
MC_HD bool metric_slow_phase(const MetricSchedule& s, int64_t W, int64_t it) {
    return s.base > 0 && it >= s.init && it < W - s.term;
}
// End (exclusive) of the window that holds the slow-phase iteration `it`:
// windows start at init with length base and double; a window is stretched to
// W - term when the one after it would not fit before W - term.
MC_HD int64_t metric_window_end(const MetricSchedule& s, int64_t W, int64_t it) {
    const int64_t stop = W - s.term;
    int64_t start = s.init, len = s.base;
    for (;;) {
        int64_t end = start + len;
        if (end + 2 * len > stop) end = stop;
        if (it < end || end >= stop) return end;
        start = end;
        len *= 2;
    }
}

#if defined(__HIPCC__)
template <bool MET>
__device__ __forceinline__ MetricDev metric_arg() {
    return MetricDev{};
}
template <bool MET>
__device__ __forceinline__ MetricDev metric_arg(const MetricDev& m) {
    return m;
}

// One element's share of a slow-phase warmup iteration: x enters the Welford
// accumulator (mean, m2) as draw number nf of the window; at the window's last
// iteration
//   var = M2 / (n - 1),  minv = (n / (n + 5)) var + 1e-3 (5 / (n + 5))
// replaces minv (a value that is not finite or not positive keeps the old one),
// msqrt follows and the accumulator is reset.  Returns true when minv / msqrt
// were replaced.  Shared by metric_adapt and the lane-resident k_nuts_lr.
__device__ __forceinline__ bool metric_update_element(float x, float nf, bool last, float& mean,
                                                      float& m2, float& minv, float& msqrt) {
    float mu = mean;
    const float d = x - mu;
    mu = mu + d / nf;
    const float s2 = m2 + d * (x - mu);
    if (!last) {
        mean = mu;
        m2 = s2;
        return false;
    }
    mean = 0.0f;
    m2 = 0.0f;
    const float var = s2 / (nf - 1.0f);
    const float v = (nf / (nf + 5.0f)) * var + 1e-3f * (5.0f / (nf + 5.0f));
    if (v > 0.0f && v < __builtin_inff()) {
        minv = v;
        msqrt = 1.0f / sqrtf(v);
        return true;
    }
    return false;
}

// One warmup iteration's adaptation work of chain c, after its accept / reject
// (q: the chain's current position; element j belongs to thread j % T).  In the
// slow phase q enters the Welford accumulator; at a window's last iteration the
// metric is replaced (metric_update_element).  minv / msqrt
// are the kernel's working copies (LDS or the buffer).  Returns true (for every
// thread of the group) when the metric was updated; the caller synchronises
// the group before the next momentum draw.
template <int T>
__device__ __forceinline__ bool metric_adapt(const MetricDev& M, MetricScalars& ms, int64_t c, int D,
                                             int64_t W, int64_t it, const float* q, float* minv,
                                             float* msqrt, int tid) {
    const MetricSchedule sch = metric_schedule(W);
    if (!metric_slow_phase(sch, W, it)) return false;
    ms.n_window += 1;
    const float nf = (float)ms.n_window;
    const bool last = it + 1 == metric_window_end(sch, W, it);
    float* mean = M.mean + c * D;
    float* m2 = M.m2 + c * D;
    for (int j = tid; j < D; j += T) {
        float mu = mean[j], s2 = m2[j], v = 0.0f, sq = 0.0f;  // (v, sq: set when replaced)
        if (metric_update_element(q[j], nf, last, mu, s2, v, sq)) {
            minv[j] = v;
            msqrt[j] = sq;
            if (M.in_lds) {
                M.minv[c * D + j] = v;
                M.msqrt[c * D + j] = sq;
            }
        }
        mean[j] = mu;
        m2[j] = s2;
    }
    if (last) {
        ms.n_window = 0;
        ms.n_updates += 1;
    }
    return last;
}
#endif

}  // namespace mc
