// run_glm_pointwise.hip — the pointwise view of a design-matrix program and the
// launches of csrc/glm_pointwise.h (a softmax program: those of
// csrc/glm_softmax_pointwise.h): what mc_program_num_elements,
// mc_program_enable_pointwise, mc_pointwise_workspace_bytes and
// mc_pointwise_stats (run_pointwise.hip) do on a program of
// mc_program_create_glm or mc_program_create_glm_softmax.  The view lives in the
// GlmPlan, never in mc_program::pw: the PSIS and predictive units, written
// against a PwCtx, see no view on such a program and decline it by name (and
// mc_glm_psis_* / mc_glm_predictive* decline a softmax program by its plan,
// enabled or not).
#include "host.h"
#include "glm_pointwise.h"
#include "glm_softmax_pointwise.h"

#include <cmath>

int64_t glm_pw_elements(const mc_program* p) { return p->glm->dev.N; }

// The view: the per-observation normaliser -lgamma(y + 1) of the Poisson
// family (what the sampler folds into lp_const as one sum), from the f32 y in
// float64, rounded once to f32; 0 outside the support (the value is -inf
// there) and for the other families (a softmax program's kernel does not read
// it: there the view only marks the program as enabled).  X, X^T, y and the
// offset are the plan's.
int glm_pw_enable(mc_program* p) {
    GlmPlan* g = p->glm;
    if (g->d_norm) return MC_OK;
    if (g->wide)
        return fail(MC_ERR_UNSUPPORTED,
                    "pointwise: a program of mc_program_create_glm_wide (glm_kernel=\"wide\") has no "
                    "pointwise view: k_glm_pointwise keeps its X^T operands in registers and takes "
                    "at most %d columns on a program of mc_program_create_glm", MC_GLM_MAX_P);
    if (g->dev.n_priors > 0)
        return fail(MC_ERR_UNSUPPORTED,
                    "pointwise: this design-matrix program carries %d prior term%s; a "
                    "likelihood is passed alone (exactly one sum of Family(X @ beta ...)"
                    ".log_prob(y)): priors belong to no observation", g->dev.n_priors,
                    g->dev.n_priors == 1 ? "" : "s");
    const size_t Np = (size_t)g->dev.Np;
    std::vector<float> y(Np, 0.0f), norm(Np, 0.0f);
    if (g->dev.family == MC_GLM_POISSON_LOG) {
        MC_HIP_TRY(hipMemcpy(y.data(), g->d_y, Np * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < g->dev.N; ++i) {
            const double v = (double)y[(size_t)i];
            const bool count = v >= 0.0 && std::isfinite(v) && v == std::floor(v);
            norm[(size_t)i] = count ? (float)-std::lgamma(v + 1.0) : 0.0f;
        }
    }
    float* d = nullptr;
    if (hipMalloc((void**)&d, Np * sizeof(float)) != hipSuccess)
        return fail(MC_ERR_NOMEM, "pointwise: device allocation of %zu bytes failed",
                    Np * sizeof(float));
    const hipError_t e = hipMemcpy(d, norm.data(), Np * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(MC_ERR_HIP, "pointwise view upload failed: %s", hipGetErrorString(e));
    }
    g->d_norm = d;
    return MC_OK;
}

int64_t glm_pw_workspace_bytes(const mc_program* p, int64_t C, int64_t S) {
    const GlmPlan* g = p->glm;
    if (C < 1 || S < 1) return fail(MC_ERR_INVALID, "pointwise: C and S must be >= 1");
    if (!g->d_norm)
        return fail(MC_ERR_INVALID, "pointwise: call mc_program_enable_pointwise first");
    if (C > INT64_MAX / S) return fail(MC_ERR_INVALID, "pointwise: C * S overflows");
    int64_t B, per;
    glm_pw_split(C * S, g->dev.NT, &B, &per);
    return B > 1 ? B * mc::PW_COUNT * (int64_t)g->dev.N * (int64_t)sizeof(double) : 0;
}

namespace {

template <int FAM>
void launch_family(int PT, dim3 grid, hipStream_t st, const mc::GlmDev& G, const float* norm,
                   int64_t R, int64_t per, const float* samples, double* part, float* matrix) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, G, norm, R, per, samples, part, matrix);
    };
    if (PT == 1) go(mc::k_glm_pointwise<FAM, 1>);
    else if (PT == 2) go(mc::k_glm_pointwise<FAM, 2>);
    else if (PT == 4) go(mc::k_glm_pointwise<FAM, 4>);
    else go(mc::k_glm_pointwise<FAM, 8>);
}

template <int PT>
int launch_softmax(int Kp, dim3 grid, hipStream_t st, const mc::GlmDev& G, int64_t R, int64_t per,
                   const float* samples, double* part, float* matrix) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, G, R, per, samples, part, matrix);
        return MC_OK;
    };
    switch (Kp) {
        case 2: return go(mc::k_glm_softmax_pointwise<PT, 2>);
        case 4: return go(mc::k_glm_softmax_pointwise<PT, 4>);
        case 8: return go(mc::k_glm_softmax_pointwise<PT, 8>);
        case 16: return go(mc::k_glm_softmax_pointwise<PT, 16>);
        case 32: return go(mc::k_glm_softmax_pointwise<PT, 32>);
        default: return fail(MC_ERR_INVALID, "k_glm_softmax_pointwise has no instantiation Kp = %d",
                             Kp);
    }
}

}  // namespace

int glm_pw_stats(const mc_program* p, int64_t C, int64_t S, const float* samples, double* stats,
                 float* matrix, void* ws, int64_t ws_bytes, hipStream_t st) {
    const GlmPlan* g = p->glm;
    if (!g->d_norm)
        return fail(MC_ERR_INVALID, "pointwise: call mc_program_enable_pointwise first");
    if (C < 1 || S < 1) return fail(MC_ERR_INVALID, "pointwise: C and S must be >= 1");
    if (C > INT64_MAX / S) return fail(MC_ERR_INVALID, "pointwise: C * S overflows");
    if (!samples || !stats) return fail(MC_ERR_INVALID, "pointwise: NULL samples / stats");
    const int64_t R = C * S, N = g->dev.N;
    int64_t B, per;
    glm_pw_split(R, g->dev.NT, &B, &per);
    const int64_t need = B > 1 ? B * mc::PW_COUNT * N * (int64_t)sizeof(double) : 0;
    if (need > 0 && (!ws || ws_bytes < need))
        return fail(MC_ERR_INVALID, "pointwise: the workspace needs %lld bytes",
                    (long long)need);
    // one block of draws: its partial is the result
    double* part = B > 1 ? (double*)ws : stats;
    const dim3 grid((unsigned)((g->dev.NT + 3) / 4), (unsigned)B);
    if (g->softmax) {
        auto go = [&](auto launch) {
            return launch(g->dev.Kp, grid, st, g->dev, R, per, samples, part, matrix);
        };
        const int rc = g->PT == 1   ? go(launch_softmax<1>)
                       : g->PT == 2 ? go(launch_softmax<2>)
                       : g->PT == 4 ? go(launch_softmax<4>)
                                    : go(launch_softmax<8>);
        if (rc != MC_OK) return rc;
    } else if (g->dev.family == MC_GLM_NORMAL)
        launch_family<MC_GLM_NORMAL>(g->PT, grid, st, g->dev, g->d_norm, R, per, samples, part,
                                     matrix);
    else if (g->dev.family == MC_GLM_BERNOULLI_LOGIT)
        launch_family<MC_GLM_BERNOULLI_LOGIT>(g->PT, grid, st, g->dev, g->d_norm, R, per, samples,
                                              part, matrix);
    else
        launch_family<MC_GLM_POISSON_LOG>(g->PT, grid, st, g->dev, g->d_norm, R, per, samples,
                                          part, matrix);
    MC_HIP_TRY(hipGetLastError());
    if (B > 1) {
        hipLaunchKernelGGL(mc::k_pw_merge, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st,
                           (const double*)part, N, (int32_t)B, stats);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}
