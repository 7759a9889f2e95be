// api.hip — libmcmc355.so: the device-facing entry points of
// include/mcmc355.h that are not sampler launches: batched log density and
// gradient, Distribution.log_prob, chain state, the diagonal metric buffer,
// RNG fill, diagnostics, mc_last_error / mc_abi_version.  (The program builder
// and slicing policy are in program.hip, the planners in plan_slices.hip and
// plan_lanes.hip, the sampler launches in run_hmc.hip, run_mh.hip,
// run_nuts.hip.)
#include "host.h"
#include "diag.h"  // (non-template kernels: this unit only)


// ---------------------------------------------------------------------------
// batched log density + gradient
// ---------------------------------------------------------------------------
template <int WPC, bool EX>
__global__ void __launch_bounds__(WPC >= 4 ? 64 * WPC : 256)
k_logp(DevCtx P, int64_t n_points, const float* q, float* logp, float* grad, int lds_floats) {
    constexpr int CPB = (WPC >= 4) ? 1 : 4 / WPC;
    constexpr int T = 64 * WPC;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lc = threadIdx.x / T;
    const int64_t c = (int64_t)blockIdx.x * CPB + lc;
    if (c >= n_points) return;
    Group<WPC> G;
    SegScratch S;
    G.tid = threadIdx.x % T;
    carve_group<WPC>(smem + (int64_t)lc * lds_floats, G, S);
    const float lp = eval_lp_grad<WPC, false, EX>(P, q + c * P.D, grad + c * P.D, G, S);
    if (G.tid == 0) logp[c] = lp;
}

template <int WPC, bool EX>
static int launch_logp(const mc_program* p, int64_t n, const float* q, float* lp, float* g,
                       hipStream_t st) {
    const int lds_floats = scratch_of(p);
    const size_t lds = (size_t)cpb_of(WPC) * lds_floats * 4;
    const int64_t grid = (n + cpb_of(WPC) - 1) / cpb_of(WPC);
    MC_HIP_TRY(allow_lds(k_logp<WPC, EX>, lds));
    hipLaunchKernelGGL((k_logp<WPC, EX>), dim3((unsigned)grid), dim3(block_of(WPC)), lds, st, ctx_of(p),
                       n, q, lp, g, lds_floats);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

extern "C" int mc_logp_grad(const mc_program* p, int64_t n_points, const float* q, float* logp,
                            float* grad, void* stream) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (n_points < 0) return fail(MC_ERR_INVALID, "n_points < 0");
    if (n_points == 0) return MC_OK;
    if (!q || !logp || !grad) return fail(MC_ERR_INVALID, "NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    switch (p->wpc) {
        case 1: return p->ex ? launch_logp<1, true>(p, n_points, q, logp, grad, st)
                             : launch_logp<1, false>(p, n_points, q, logp, grad, st);
        case 4: return p->ex ? launch_logp<4, true>(p, n_points, q, logp, grad, st)
                             : launch_logp<4, false>(p, n_points, q, logp, grad, st);
        default: return p->ex ? launch_logp<8, true>(p, n_points, q, logp, grad, st)
                              : launch_logp<8, false>(p, n_points, q, logp, grad, st);
    }
}

// ---------------------------------------------------------------------------
// elementwise Distribution.log_prob
// ---------------------------------------------------------------------------
__global__ void k_dist(int dist, float c0, int64_t n, const float* v, int vb, const float* m,
                       int mb, const float* s, int sb, float* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float vv = v[vb ? 0 : i];
        const float ss = s[sb ? 0 : i];
        const float mm = m[mb ? 0 : i];
        const float logs = logf(ss);
        const float lg = lgamma_norm(dist, mm, ss);
        out[i] = elem_eval(dist, c0, vv, mm, ss, logs, lg).lp;
    }
}

extern "C" int mc_dist_log_prob(int32_t dist, int64_t n, const float* v, int32_t vb,
                                const float* m, int32_t mb, const float* s, int32_t sb,
                                float* out, void* stream) {
    if (dist < MC_DIST_NORMAL || dist > MC_DIST_BETA)
        return fail(MC_ERR_INVALID, "unknown distribution %d", dist);
    if (n < 0) return fail(MC_ERR_INVALID, "n < 0");
    if (n == 0) return MC_OK;
    const bool need_m = dist == MC_DIST_NORMAL || dist == MC_DIST_GAMMA || dist == MC_DIST_BETA;
    if (!v || !s || !out || (need_m && !m)) return fail(MC_ERR_INVALID, "NULL operand");
    if (!need_m) mb = 1;  // the unused middle operand is read as element 0 of value
    const float c0 = dist_c0(dist);
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_dist, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dist,
                       c0, n, v, vb, m ? m : v, mb, s, sb, out);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

__global__ void k_discrete(int kind, int64_t n, const float* v, int vb, const float* t, int tb,
                           const float* e, int eb, float* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float y = v[vb ? 0 : i];
        const float eta = e[eb ? 0 : i];
        if (kind == MC_DISCRETE_BERNOULLI) out[i] = ex_bernoulli_lp(y, eta);
        else if (kind == MC_DISCRETE_BINOMIAL) out[i] = ex_binomial_lp(y, t[tb ? 0 : i], eta);
        else out[i] = ex_poisson_lp(y, eta);
    }
}

extern "C" int mc_discrete_log_prob(int32_t kind, int64_t n, const float* v, int32_t vb,
                                    const float* t, int32_t tb, const float* e, int32_t eb,
                                    float* out, void* stream) {
    if (kind < MC_DISCRETE_BERNOULLI || kind > MC_DISCRETE_POISSON)
        return fail(MC_ERR_INVALID, "unknown discrete distribution %d", kind);
    if (n < 0) return fail(MC_ERR_INVALID, "n < 0");
    if (n == 0) return MC_OK;
    const bool need_t = kind == MC_DISCRETE_BINOMIAL;
    if (!v || !e || !out || (need_t && !t)) return fail(MC_ERR_INVALID, "NULL operand");
    if (!need_t) tb = 1;  // the unused total is read as element 0 of value
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_discrete, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       kind, n, v, vb, need_t ? t : v, tb, e, eb, out);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// The Student-t nodes elementwise: ex_fwd's two cases on ex_student_t_lp (the
// function the tape calls), nu as the node constant.
__global__ void k_student_t(float nu, int half, int64_t n, const float* v, int vb, const float* m,
                            int mb, const float* s, int sb, float* out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float x = v[vb ? 0 : i];
        const float sc = s[sb ? 0 : i];
        if (half) out[i] = x >= 0.0f ? ex_student_t_lp(nu, x, sc) : -__builtin_inff();
        else out[i] = ex_student_t_lp(nu, x - m[mb ? 0 : i], sc);
    }
}

extern "C" int mc_student_t_log_prob(float df, int32_t half, int64_t n, const float* v,
                                     int32_t vb, const float* m, int32_t mb, const float* s,
                                     int32_t sb, float* out, void* stream) {
    if (!(df > 0.0f) || !(df < __builtin_inff()))
        return fail(MC_ERR_INVALID, "the degrees of freedom must be finite and positive (got %g)",
                    (double)df);
    if (n < 0) return fail(MC_ERR_INVALID, "n < 0");
    if (n == 0) return MC_OK;
    const bool need_m = half == 0;
    if (!v || !s || !out || (need_m && !m)) return fail(MC_ERR_INVALID, "NULL operand");
    if (!need_m) mb = 1;  // the unused loc is read as element 0 of value
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_student_t, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, df,
                       half != 0 ? 1 : 0, n, v, vb, need_m ? m : v, mb, s, sb, out);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// ---------------------------------------------------------------------------
// state
// ---------------------------------------------------------------------------
static int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

extern "C" int mc_state_offsets(const mc_program* p, int64_t C, int64_t* q_off, int64_t* g_off) {
    if (!p || C < 0) return fail(MC_ERR_INVALID, "bad arguments");
    const int64_t s = align256(C * (int64_t)sizeof(mc_chain_scalars));
    const int64_t qb = align256(C * p->D * 4);
    if (q_off) *q_off = s;
    if (g_off) *g_off = s + qb;
    return MC_OK;
}

extern "C" int64_t mc_state_bytes(const mc_program* p, int64_t C) {
    if (!p || C < 0) return -1;
    return align256(C * (int64_t)sizeof(mc_chain_scalars)) + 2 * align256(C * p->D * 4);
}

template <int WPC, bool EX>
__global__ void __launch_bounds__(WPC >= 4 ? 64 * WPC : 256)
k_init(DevCtx P, int64_t C, const float* q0, double eps0, float mu, mc_chain_scalars* scal,
       float* st_q, float* st_g, int lds_floats) {
    constexpr int CPB = (WPC >= 4) ? 1 : 4 / WPC;
    constexpr int T = 64 * WPC;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lc = threadIdx.x / T;
    const int64_t c = (int64_t)blockIdx.x * CPB + lc;
    if (c >= C) return;
    Group<WPC> G;
    SegScratch S;
    G.tid = threadIdx.x % T;
    carve_group<WPC>(smem + (int64_t)lc * lds_floats, G, S);
    const int D = P.D;
    for (int j = G.tid; j < D; j += T) st_q[c * D + j] = q0[c * D + j];
    const float lp = eval_lp_grad<WPC, false, EX>(P, q0 + c * D, st_g + c * D, G, S);
    if (G.tid == 0) {
        mc_chain_scalars sc = {};
        sc.step_size = eps0;
        sc.step_size_bar = 1.0;
        sc.h_bar = 0.0;
        sc.mu = mu;
        sc.logp = lp;
        sc.n_grad = 1;
        scal[c] = sc;
    }
}

template <int WPC, bool EX>
static int launch_init(const mc_program* p, int64_t C, const float* q0, double eps0,
                       void* state, hipStream_t st) {
    int64_t qo, go;
    mc_state_offsets(p, C, &qo, &go);
    char* b = (char*)state;
    const int lds_floats = scratch_of(p);
    const size_t lds = (size_t)cpb_of(WPC) * lds_floats * 4;
    const int64_t grid = (C + cpb_of(WPC) - 1) / cpb_of(WPC);
    const float mu = mc_logf_ref((float)(10.0 * eps0));  // nuts.py:63 mx.log(10 * step_size)
    MC_HIP_TRY(allow_lds(k_init<WPC, EX>, lds));
    hipLaunchKernelGGL((k_init<WPC, EX>), dim3((unsigned)grid), dim3(block_of(WPC)), lds, st,
                       ctx_of(p), C, q0, eps0, mu, (mc_chain_scalars*)b, (float*)(b + qo),
                       (float*)(b + go), lds_floats);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

extern "C" int mc_state_init(const mc_program* p, int64_t C, const float* q0, double eps0,
                             void* state, void* stream) {
    if (!p || C < 0 || (C > 0 && (!q0 || !state))) return fail(MC_ERR_INVALID, "bad arguments");
    if (C == 0) return MC_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (p->wpc) {
        case 1: return p->ex ? launch_init<1, true>(p, C, q0, eps0, state, st)
                             : launch_init<1, false>(p, C, q0, eps0, state, st);
        case 4: return p->ex ? launch_init<4, true>(p, C, q0, eps0, state, st)
                             : launch_init<4, false>(p, C, q0, eps0, state, st);
        default: return p->ex ? launch_init<8, true>(p, C, q0, eps0, state, st)
                              : launch_init<8, false>(p, C, q0, eps0, state, st);
    }
}

// ---------------------------------------------------------------------------
// diagonal metric buffer (metric.h)
// ---------------------------------------------------------------------------
extern "C" int32_t mc_metric_schedule(int64_t W, int64_t* ends, int32_t cap) {
    const MetricSchedule s = metric_schedule(W);
    int32_t n = 0;
    for (int64_t it = s.init; metric_slow_phase(s, W, it);) {
        const int64_t end = metric_window_end(s, W, it);
        if (ends && n < cap) ends[n] = end;
        ++n;
        it = end;
    }
    return n;
}

extern "C" int64_t mc_metric_bytes(const mc_program* p, int64_t C) {
    if (!p || C < 0) return -1;
    return metric_layout(p, C).total;
}

extern "C" int mc_metric_offsets(const mc_program* p, int64_t C, int64_t* minv_off,
                                 int64_t* msqrt_off, int64_t* mean_off, int64_t* m2_off) {
    if (!p || C < 0) return fail(MC_ERR_INVALID, "bad arguments");
    const MetricLayout L = metric_layout(p, C);
    if (minv_off) *minv_off = L.minv;
    if (msqrt_off) *msqrt_off = L.msqrt;
    if (mean_off) *mean_off = L.mean;
    if (m2_off) *m2_off = L.m2;
    return MC_OK;
}

extern "C" int mc_metric_init(const mc_program* p, int64_t C, const float* inv_mass, int32_t bcast,
                              void* metric, void* stream) {
    if (!p || C < 0 || (C > 0 && !metric)) return fail(MC_ERR_INVALID, "bad arguments");
    if (C == 0) return MC_OK;
    const int64_t D = p->D;
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> in;
    if (inv_mass) {
        in.resize((size_t)((bcast ? 1 : C) * D));
        if (p->host_only) {
            std::memcpy(in.data(), inv_mass, in.size() * 4);
        } else {
            MC_HIP_TRY(hipMemcpyAsync(in.data(), inv_mass, in.size() * 4, hipMemcpyDeviceToHost, st));
            MC_HIP_TRY(hipStreamSynchronize(st));
        }
        for (size_t i = 0; i < in.size(); ++i)
            if (!(in[i] > 0.0f) || !std::isfinite(in[i]))
                return fail(MC_ERR_INVALID, "inverse mass entry %lld (chain %lld, element %lld) is "
                            "%g: every entry must be finite and positive", (long long)i,
                            (long long)(i / (size_t)D), (long long)(i % (size_t)D), (double)in[i]);
    }
    const MetricLayout L = metric_layout(p, C);
    std::vector<char> buf((size_t)L.total, 0);  // scalars and accumulator zero
    float* minv = (float*)(buf.data() + L.minv);
    float* msqrt = (float*)(buf.data() + L.msqrt);
    for (int64_t c = 0; c < C; ++c)
        for (int64_t j = 0; j < D; ++j) {
            const float v = inv_mass ? in[(size_t)((bcast ? 0 : c * D) + j)] : 1.0f;
            minv[c * D + j] = v;
            msqrt[c * D + j] = 1.0f / std::sqrt(v);
        }
    if (p->host_only) {
        std::memcpy(metric, buf.data(), buf.size());
    } else {
        MC_HIP_TRY(hipMemcpyAsync(metric, buf.data(), buf.size(), hipMemcpyHostToDevice, st));
        MC_HIP_TRY(hipStreamSynchronize(st));
    }
    return MC_OK;
}




// ---------------------------------------------------------------------------
// RNG fill (test hook and Distribution.sample)
// ---------------------------------------------------------------------------
__global__ void k_rng(uint64_t seed, uint32_t chain, uint32_t iter, uint32_t tag, uint32_t sub,
                      uint32_t index0, int64_t n, int mode, void* out) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * blockDim.x) {
        const mc_u32x4 r = mc_draw(seed, chain, iter, tag, sub, index0 + (uint32_t)e);
        if (mode == 0) {
            uint32_t* o = (uint32_t*)out + 4 * e;
            o[0] = r.x;
            o[1] = r.y;
            o[2] = r.z;
            o[3] = r.w;
        } else if (mode == 1) {
            float* o = (float*)out + 4 * e;
            o[0] = mc_u01_f32(r.x);
            o[1] = mc_u01_f32(r.y);
            o[2] = mc_u01_f32(r.z);
            o[3] = mc_u01_f32(r.w);
        } else {
            float* o = (float*)out + 4 * e;
            mc_box_muller(r.x, r.y, &o[0], &o[1]);
            mc_box_muller(r.z, r.w, &o[2], &o[3]);
        }
    }
}

extern "C" int mc_rng_fill(uint64_t seed, uint32_t chain, uint32_t iter, uint32_t tag,
                           uint32_t sub, uint32_t index0, int64_t n, int32_t mode, void* out,
                           void* stream) {
    if (n < 0 || (n > 0 && !out) || mode < 0 || mode > 2)
        return fail(MC_ERR_INVALID, "bad arguments");
    if (n == 0) return MC_OK;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_rng, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, seed,
                       chain, iter, tag, sub, index0, n, mode, out);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}


// ---------------------------------------------------------------------------
// diagnostics (diag.h)
// ---------------------------------------------------------------------------
static int check_csd(int64_t C, int64_t S, int64_t D, const void* x) {
    if (C < 1 || S < 1 || D < 1) return fail(MC_ERR_INVALID, "C, S and D must be >= 1");
    if (!x) return fail(MC_ERR_INVALID, "samples is NULL");
    return MC_OK;
}

extern "C" int mc_series_stats(int64_t C, int64_t S, int64_t D, const float* samples,
                               int32_t max_lag, double* stats, void* stream) {
    if (int rc = check_csd(C, S, D, samples)) return rc;
    if (!stats) return fail(MC_ERR_INVALID, "stats is NULL");
    if (max_lag < 1) return fail(MC_ERR_INVALID, "max_lag must be >= 1");
    const int32_t lmax = (int32_t)std::min<int64_t>(S / 2, max_lag);
    const int64_t blocks = (C * D + 255) / 256;
    hipLaunchKernelGGL(k_series_stats, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       samples, C, S, D, lmax, stats);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

extern "C" int mc_stats_reduce(int64_t C, int64_t S, int64_t D, const double* stats,
                               const double* center, int64_t m_total, double* out, void* stream) {
    if (int rc = check_csd(C, S, D, stats)) return rc;
    if (!out) return fail(MC_ERR_INVALID, "out is NULL");
    if (center && (S < 4 || m_total < 2))
        return fail(MC_ERR_INVALID, "split R-hat needs S >= 4 draws and >= 2 half chains");
    hipLaunchKernelGGL(k_stats_reduce, dim3((unsigned)((D + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, stats, C, S, D, center ? 1 : 0, center, m_total, out);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

extern "C" int mc_rhat(int64_t D, int64_t m_total, int64_t S, const double* spread, double* rhat,
                       void* stream) {
    if (D < 1 || !spread || !rhat) return fail(MC_ERR_INVALID, "bad mc_rhat arguments");
    if (S < 4 || m_total < 2)
        return fail(MC_ERR_INVALID, "split R-hat needs S >= 4 draws and >= 2 half chains");
    hipLaunchKernelGGL(k_rhat, dim3((unsigned)((D + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, spread, D, m_total, S / 2, rhat);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

extern "C" int mc_pool_moments(int64_t C, int64_t S, int64_t D, const double* stats, int64_t off,
                               int64_t len, double* out, void* stream) {
    if (int rc = check_csd(C, S, D, stats)) return rc;
    if (off < 0 || len < 1 || off + len > D || !out)
        return fail(MC_ERR_INVALID, "element range [%lld, %lld) outside [0, %lld)", (long long)off,
                    (long long)(off + len), (long long)D);
    hipLaunchKernelGGL(k_pool_moments, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, C, S, D,
                       off, len, out);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

extern "C" int64_t mc_select_workspace_bytes(int32_t nk) {
    if (nk < 1 || nk > kSelMaxTargets) return -1;
    return (int64_t)nk * (int64_t)(sizeof(SelState) + 256 * sizeof(unsigned long long)) + 16;
}

extern "C" int mc_select(int64_t C, int64_t S, int64_t D, const float* samples, int64_t off,
                         int64_t len, int32_t nk, const int64_t* k, float* out, void* ws,
                         int64_t ws_bytes, void* stream) {
    if (int rc = check_csd(C, S, D, samples)) return rc;
    if (off < 0 || len < 1 || off + len > D)
        return fail(MC_ERR_INVALID, "element range outside [0, D)");
    if (nk < 1 || nk > kSelMaxTargets || !k || !out)
        return fail(MC_ERR_INVALID, "nk must be in [1, %d] with k and out set", kSelMaxTargets);
    if (!ws || ws_bytes < mc_select_workspace_bytes(nk))
        return fail(MC_ERR_INVALID, "workspace too small (need %lld bytes)",
                    (long long)mc_select_workspace_bytes(nk));
    const int64_t rows = C * S, n = rows * len;
    SelTargets tg{};
    tg.nk = nk;
    for (int i = 0; i < nk; ++i) {
        if (k[i] < 0 || k[i] >= n)
            return fail(MC_ERR_INVALID, "rank %lld outside [0, %lld)", (long long)k[i], (long long)n);
        tg.k[i] = k[i];
    }
    hipStream_t st = (hipStream_t)stream;
    SelState* stt = (SelState*)ws;
    unsigned long long* hist = (unsigned long long*)(stt + nk);
    uint32_t* nanf = (uint32_t*)(hist + nk * 256);
    hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(256), 0, st, tg, stt, hist, nanf);
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 1023) / 1024, 2048);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_sel_hist, dim3(blocks), dim3(256), 0, st, samples, rows, D, off, len,
                           nk, shift, stt, hist, nanf);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(64), 0, st, nk, shift, stt, hist, nanf,
                           shift == 0 ? out : nullptr);
    }
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// Host evaluations of the samplers' Box-Muller and uniform log (philox.h:
// the same code the kernels run), for the CPU tests against libm / the oracle.
extern "C" int mc_box_muller_host(const uint32_t* words, int64_t n, float* out) {
    if (n < 0 || (n > 0 && (!words || !out))) return fail(MC_ERR_INVALID, "bad arguments");
    for (int64_t i = 0; i < n; ++i) mc_box_muller(words[2 * i], words[2 * i + 1], &out[2 * i], &out[2 * i + 1]);
    return MC_OK;
}
extern "C" int mc_logf_unit_host(const float* x, int64_t n, float* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(MC_ERR_INVALID, "bad arguments");
    for (int64_t i = 0; i < n; ++i) out[i] = mc_logf_unit(x[i]);
    return MC_OK;
}

extern "C" const char* mc_last_error(void) { return g_last_error.c_str(); }
extern "C" int32_t mc_abi_version(void) { return MC_ABI_VERSION; }
