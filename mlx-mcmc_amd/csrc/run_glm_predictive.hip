// run_glm_predictive.hip — posterior predictive replicates of a design-matrix
// program (csrc/glm_predictive.h): mc_glm_predictive_workspace_bytes and
// mc_glm_predictive.  The program is one of mc_program_create_glm without prior
// terms (a likelihood passed alone); mc_predictive* (run_predictive.hip, on a
// term view such a program does not have) keep declining it.
#include "host.h"
#include "glm_predictive.h"

namespace {

// The geometry of a launch, validated: S' = ceil(S / thin) processed iterations
// per chain, B blocks of `per` processed draws — a function of (C * S', NT) only.
struct GppPlan {
    const GlmPlan* g;
    int64_t Sp, Np, B, per;
    bool ties;  // a count family: EQUAL is counted (a sixth f64 per block and observation)
};
int gpp_plan(const mc_program* p, int64_t C, int64_t S, int64_t thin, GppPlan* out) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (!is_glm(p))
        return fail(MC_ERR_UNSUPPORTED, "glm predictive: the program is not a design-matrix "
                    "(X @ beta) program of mc_program_create_glm; mc_predictive takes every "
                    "other likelihood");
    const GlmPlan* g = p->glm;
    if (g->softmax)
        return fail(MC_ERR_UNSUPPORTED, "glm predictive: a softmax program "
                    "(mc_program_create_glm_softmax) is not taken: k_glm_predictive forms one "
                    "linear predictor per draw, not K class logits");
    if (g->wide)
        return fail(MC_ERR_UNSUPPORTED,
                    "glm predictive: a program of mc_program_create_glm_wide (glm_kernel=\"wide\") "
                    "is not taken: k_glm_predictive keeps its X^T operands in registers and takes "
                    "at most %d columns on a program of mc_program_create_glm", MC_GLM_MAX_P);
    if (g->dev.n_priors > 0)
        return fail(MC_ERR_UNSUPPORTED,
                    "glm predictive: this design-matrix program carries %d prior term%s; a "
                    "likelihood is passed alone (exactly one sum of Family(X @ beta ...)"
                    ".log_prob(y)): priors have no replicate", g->dev.n_priors,
                    g->dev.n_priors == 1 ? "" : "s");
    if (C < 1 || S < 1 || thin < 1)
        return fail(MC_ERR_INVALID, "glm predictive: C, S and thin must be >= 1");
    if (C > INT64_MAX / S) return fail(MC_ERR_INVALID, "glm predictive: C * S overflows");
    out->g = g;
    out->Sp = (S + thin - 1) / thin;
    out->Np = C * out->Sp;
    out->ties = g->dev.family != MC_GLM_NORMAL;
    glm_pw_split(out->Np, g->dev.NT, &out->B, &out->per);
    return MC_OK;
}
int64_t gpp_need(const GppPlan& L) {
    return L.B > 1 ? L.B * (mc::PP_COUNT + (L.ties ? 1 : 0)) * (int64_t)L.g->dev.N *
                         (int64_t)sizeof(double)
                   : 0;
}

template <int FAM>
void launch_family(int PT, dim3 grid, hipStream_t st, const mc::GlmDev& G, const mc::PpRun& R,
                   const float* samples, double* part, double* eqpart, float* yrep) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, G, R, samples, part, eqpart, yrep);
    };
    if (PT == 1) go(mc::k_glm_predictive<FAM, 1>);
    else if (PT == 2) go(mc::k_glm_predictive<FAM, 2>);
    else if (PT == 4) go(mc::k_glm_predictive<FAM, 4>);
    else go(mc::k_glm_predictive<FAM, 8>);
}

}  // namespace

extern "C" int64_t mc_glm_predictive_workspace_bytes(const mc_program* p, int64_t C, int64_t S,
                                                     int64_t thin) {
    GppPlan L;
    const int rc = gpp_plan(p, C, S, thin, &L);
    return rc != MC_OK ? rc : gpp_need(L);
}

extern "C" int mc_glm_predictive(const mc_program* p, int64_t C, int64_t S, int64_t thin,
                                 uint64_t seed, int64_t chain_offset, int64_t iter_offset,
                                 const float* samples, double* stats, double* equal, float* yrep,
                                 void* ws, int64_t ws_bytes, void* hip_stream) {
    GppPlan L;
    const int rc = gpp_plan(p, C, S, thin, &L);
    if (rc != MC_OK) return rc;
    if (!samples || !stats) return fail(MC_ERR_INVALID, "glm predictive: NULL samples / stats");
    if (equal && !L.ties)
        return fail(MC_ERR_UNSUPPORTED, "glm predictive: the count of ties needs the Bernoulli "
                    "or Poisson family (pass equal = NULL)");
    if (chain_offset < 0 || chain_offset + C > (int64_t)UINT32_MAX)
        return fail(MC_ERR_INVALID, "glm predictive: chain ids must fit in 32 bits");
    if (iter_offset < 0 || iter_offset + S > (int64_t)UINT32_MAX)
        return fail(MC_ERR_INVALID, "glm predictive: iteration ids must fit in 32 bits");
    const int64_t need = gpp_need(L);
    if (need > 0 && (!ws || ws_bytes < need))
        return fail(MC_ERR_INVALID, "glm predictive: the workspace needs %lld bytes",
                    (long long)need);
    hipStream_t st = (hipStream_t)hip_stream;
    const mc::GlmDev& G = L.g->dev;
    const int64_t N = G.N;
    mc::PpRun R;
    R.S = S;
    R.Sp = L.Sp;
    R.thin = thin;
    R.Np = L.Np;
    R.per = L.per;
    R.seed = seed;
    R.chain0 = (uint32_t)chain_offset;
    R.iter0 = (uint32_t)iter_offset;
    // one block of draws: its partial is the result
    double* part = L.B > 1 ? (double*)ws : stats;
    double* eqpart = !equal ? nullptr : L.B > 1 ? (double*)ws + L.B * mc::PP_COUNT * N : equal;
    const dim3 grid((unsigned)((G.NT + 3) / 4), (unsigned)L.B);
    if (G.family == MC_GLM_NORMAL)
        launch_family<MC_GLM_NORMAL>(L.g->PT, grid, st, G, R, samples, part, eqpart, yrep);
    else if (G.family == MC_GLM_BERNOULLI_LOGIT)
        launch_family<MC_GLM_BERNOULLI_LOGIT>(L.g->PT, grid, st, G, R, samples, part, eqpart, yrep);
    else
        launch_family<MC_GLM_POISSON_LOG>(L.g->PT, grid, st, G, R, samples, part, eqpart, yrep);
    MC_HIP_TRY(hipGetLastError());
    if (L.B > 1) {
        hipLaunchKernelGGL(mc::k_pp_merge, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st,
                           (const double*)part, N, (int32_t)L.B, stats, (const double*)eqpart,
                           equal);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}
