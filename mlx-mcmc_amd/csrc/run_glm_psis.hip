// run_glm_psis.hip — PSIS-LOO of a design-matrix program (csrc/glm_psis.h):
// mc_glm_psis_workspace_bytes, mc_glm_psis_loo and the measurement hook
// mc_debug_glm_psis_times.  The program is one of
// mc_program_create_glm without prior terms, with its pointwise view enabled
// (the Poisson normaliser); mc_psis_* (run_psis.hip, on a term view such a
// program does not have) keep declining it.  The select's pick and the fit are
// psis.h's kernels on psis_carve's workspace, M = N observations and
// glm_pw_split's draw blocks.
#include "host.h"
#include "glm_psis.h"

namespace {

// The geometry of a launch, validated.
struct GpsPlan {
    const GlmPlan* g;
    int64_t R, Mt, P, B, per;
};
int gps_plan(const mc_program* p, int64_t C, int64_t S, double r_eff, GpsPlan* out) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (!is_glm(p))
        return fail(MC_ERR_UNSUPPORTED, "glm psis: the program is not a design-matrix "
                    "(X @ beta) program of mc_program_create_glm; mc_psis_loo takes every "
                    "other likelihood");
    const GlmPlan* g = p->glm;
    if (g->softmax)
        return fail(MC_ERR_UNSUPPORTED, "glm psis: a softmax program "
                    "(mc_program_create_glm_softmax) is not taken: the select and gather kernels "
                    "form one linear predictor per draw, not K class logits");
    if (g->wide)
        return fail(MC_ERR_UNSUPPORTED,
                    "glm psis: a program of mc_program_create_glm_wide (glm_kernel=\"wide\") is "
                    "not taken: the select and gather kernels keep their X^T operands in "
                    "registers and take at most %d columns on a program of mc_program_create_glm",
                    MC_GLM_MAX_P);
    if (g->dev.n_priors > 0)
        return fail(MC_ERR_UNSUPPORTED,
                    "glm psis: this design-matrix program carries %d prior term%s; a "
                    "likelihood is passed alone (exactly one sum of Family(X @ beta ...)"
                    ".log_prob(y)): priors belong to no observation", g->dev.n_priors,
                    g->dev.n_priors == 1 ? "" : "s");
    if (!g->d_norm)
        return fail(MC_ERR_INVALID, "glm psis: call mc_program_enable_pointwise first");
    if (C < 1 || S < 1) return fail(MC_ERR_INVALID, "glm psis: C and S must be >= 1");
    if (C > (int64_t)UINT32_MAX / S)
        return fail(MC_ERR_UNSUPPORTED, "glm psis: C * S exceeds the 32-bit draw counters");
    if (!(r_eff > 0.0) || r_eff - r_eff != 0.0)
        return fail(MC_ERR_INVALID, "glm psis: r_eff must be positive and finite");
    if ((int64_t)g->dev.N > (int64_t)INT32_MAX)
        return fail(MC_ERR_UNSUPPORTED, "glm psis: %lld observations exceed the fit kernel's grid",
                    (long long)g->dev.N);
    out->g = g;
    out->R = C * S;
    out->Mt = psis_tail_len(out->R, r_eff);
    if (out->Mt > kPsisMaxTail)
        return fail(MC_ERR_UNSUPPORTED, "glm psis: a tail of %lld draws exceeds kPsisMaxTail = %d "
                    "(the fit kernel's LDS)", (long long)out->Mt, kPsisMaxTail);
    out->P = 1;
    while (out->P < out->Mt) out->P <<= 1;
    glm_pw_split(out->R, g->dev.NT, &out->B, &out->per);
    return MC_OK;
}

template <int FAM>
void launch_count(int PT, dim3 grid, hipStream_t st, const mc::GlmDev& G, const float* norm,
                  int64_t R, int64_t per, const float* samples, int shift, int first,
                  const uint32_t* lo, uint32_t* cnt) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, G, norm, R, per, samples, shift, first,
                           lo, cnt);
    };
    if (PT == 1) go(mc::k_glm_psis_count<FAM, 1>);
    else if (PT == 2) go(mc::k_glm_psis_count<FAM, 2>);
    else if (PT == 4) go(mc::k_glm_psis_count<FAM, 4>);
    else go(mc::k_glm_psis_count<FAM, 8>);
}

template <int FAM>
void launch_gather(int PT, dim3 grid, hipStream_t st, const mc::GlmDev& G, const float* norm,
                   int64_t R, int64_t per, const float* samples, uint32_t Mt,
                   const mc::PsisWs& W) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, G, norm, R, per, samples, Mt, W);
    };
    if (PT == 1) go(mc::k_glm_psis_gather<FAM, 1>);
    else if (PT == 2) go(mc::k_glm_psis_gather<FAM, 2>);
    else if (PT == 4) go(mc::k_glm_psis_gather<FAM, 4>);
    else go(mc::k_glm_psis_gather<FAM, 8>);
}

}  // namespace

extern "C" int64_t mc_glm_psis_workspace_bytes(const mc_program* p, int64_t C, int64_t S,
                                               double r_eff) {
    GpsPlan L;
    const int rc = gps_plan(p, C, S, r_eff, &L);
    return rc != MC_OK ? rc : mc::psis_carve(L.g->dev.N, L.B, L.Mt, nullptr, nullptr);
}

namespace {

constexpr int kGpsStages = 18;  // eight (count, pick) pairs, the gather, the fit

// ev: NULL, or kGpsStages + 1 events recorded before the first launch and after
// every stage (mc_debug_glm_psis_times).
int gps_run(const mc_program* p, int64_t C, int64_t S, double r_eff, const float* samples,
            double* out, float* tail, void* ws, int64_t ws_bytes, void* hip_stream,
            hipEvent_t* ev) {
    GpsPlan L;
    const int rc = gps_plan(p, C, S, r_eff, &L);
    if (rc != MC_OK) return rc;
    if (!samples || !out) return fail(MC_ERR_INVALID, "glm psis: NULL samples / out");
    const mc::GlmDev& G = L.g->dev;
    const int64_t M = G.N;
    const int64_t need = mc::psis_carve(M, L.B, L.Mt, nullptr, nullptr);
    if (!ws || ws_bytes < need)
        return fail(MC_ERR_INVALID, "glm psis: the workspace needs %lld bytes", (long long)need);
    if (((uintptr_t)ws & 7) != 0)
        return fail(MC_ERR_INVALID, "glm psis: the workspace is unaligned");
    mc::PsisWs W;
    mc::psis_carve(M, L.B, L.Mt, ws, &W);
    hipStream_t st = (hipStream_t)hip_stream;
    const float* norm = L.g->d_norm;
    const int PT = L.g->PT;
    const dim3 grid((unsigned)((G.NT + 3) / 4), (unsigned)L.B);
    const dim3 ogrid((unsigned)((M + 255) / 256));
    int stage = 0;
    auto mark = [&]() { return ev ? hipEventRecord(ev[stage++], st) : hipSuccess; };
    MC_HIP_TRY(mark());
    // the eight passes of the select, most significant digit first
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 28 - 4 * pass, first = pass == 0, last = pass == 7;
        if (G.family == MC_GLM_NORMAL)
            launch_count<MC_GLM_NORMAL>(PT, grid, st, G, norm, L.R, L.per, samples, shift, first,
                                        W.lo, W.cnt);
        else if (G.family == MC_GLM_BERNOULLI_LOGIT)
            launch_count<MC_GLM_BERNOULLI_LOGIT>(PT, grid, st, G, norm, L.R, L.per, samples, shift,
                                                 first, W.lo, W.cnt);
        else
            launch_count<MC_GLM_POISSON_LOG>(PT, grid, st, G, norm, L.R, L.per, samples, shift,
                                             first, W.lo, W.cnt);
        MC_HIP_TRY(hipGetLastError());
        MC_HIP_TRY(mark());
        hipLaunchKernelGGL(mc::k_psis_pick, ogrid, dim3(256), 0, st, M, (int32_t)L.B,
                           (uint32_t)L.Mt, shift, first, last, W);
        MC_HIP_TRY(hipGetLastError());
        MC_HIP_TRY(mark());
    }
    if (G.family == MC_GLM_NORMAL)
        launch_gather<MC_GLM_NORMAL>(PT, grid, st, G, norm, L.R, L.per, samples, (uint32_t)L.Mt, W);
    else if (G.family == MC_GLM_BERNOULLI_LOGIT)
        launch_gather<MC_GLM_BERNOULLI_LOGIT>(PT, grid, st, G, norm, L.R, L.per, samples,
                                              (uint32_t)L.Mt, W);
    else
        launch_gather<MC_GLM_POISSON_LOG>(PT, grid, st, G, norm, L.R, L.per, samples,
                                          (uint32_t)L.Mt, W);
    MC_HIP_TRY(hipGetLastError());
    MC_HIP_TRY(mark());
    hipLaunchKernelGGL(mc::k_psis_fit, dim3((unsigned)M), dim3(64), mc::psis_fit_lds(L.Mt, L.P), st,
                       M, L.R, (int32_t)L.B, (int32_t)L.Mt, (int32_t)L.P, W, out, tail);
    MC_HIP_TRY(hipGetLastError());
    MC_HIP_TRY(mark());
    return MC_OK;
}

}  // namespace

extern "C" int mc_glm_psis_loo(const mc_program* p, int64_t C, int64_t S, double r_eff,
                               const float* samples, double* out, float* tail, void* ws,
                               int64_t ws_bytes, void* hip_stream) {
    return gps_run(p, C, S, r_eff, samples, out, tail, ws, ws_bytes, hip_stream, nullptr);
}

// Measurement hook: one mc_glm_psis_loo (no tail_dev) with an event after every
// stage; synchronises on the last.  ms[18]: count and pick of the eight passes
// alternating, the gather, the fit.
extern "C" int mc_debug_glm_psis_times(const mc_program* p, int64_t C, int64_t S, double r_eff,
                                       const float* samples, double* out, void* ws,
                                       int64_t ws_bytes, void* hip_stream, float* ms) {
    if (!ms) return fail(MC_ERR_INVALID, "glm psis: NULL ms");
    hipEvent_t ev[kGpsStages + 1] = {};
    for (hipEvent_t& e : ev) MC_HIP_TRY(hipEventCreate(&e));
    int rc = gps_run(p, C, S, r_eff, samples, out, nullptr, ws, ws_bytes, hip_stream, ev);
    if (rc == MC_OK && hipEventSynchronize(ev[kGpsStages]) != hipSuccess)
        rc = fail(MC_ERR_HIP, "glm psis: the timed launch failed");
    for (int i = 0; i < kGpsStages && rc == MC_OK; ++i)
        if (hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]) != hipSuccess)
            rc = fail(MC_ERR_HIP, "glm psis: hipEventElapsedTime failed");
    for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
    return rc;
}
