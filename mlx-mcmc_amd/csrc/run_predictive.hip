// run_predictive.hip — posterior predictive replicates on the pointwise view
// of a program (csrc/predictive.h): mc_predictive_draw and
// mc_predictive_draw_discrete / mc_predictive_draw_student_t (the scalar
// definitions, host only),
// mc_predictive_workspace_bytes, mc_predictive, mc_predictive_eq.
#include "host.h"
#include "predictive.h"
#include "pw_view.h"

namespace {

bool pp_sampled(int dist) { return dist >= MC_DIST_NORMAL && dist <= MC_DIST_BETA; }

// The view and the geometry of a launch, validated: S' = ceil(S / thin)
// processed iterations per chain, B blocks of `per` processed draws.
struct PpPlan {
    const PwView* v;
    int64_t Sp, Np, B, per;
    bool gb;
    int nmax;  // 0: no expression sampler; 16 / 32: the largest one's node bound
    bool ties;  // a count term: EQUAL is counted (a sixth f64 per block and observation)
};
int pp_plan(const mc_program* p, int64_t C, int64_t S, int64_t thin, PpPlan* out) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    const PwView* v = (const PwView*)p->pw;
    if (!v) return fail(MC_ERR_INVALID, "predictive: call mc_program_enable_pointwise first");
    if (C < 1 || S < 1 || thin < 1)
        return fail(MC_ERR_INVALID, "predictive: C, S and thin must be >= 1");
    if (C > INT64_MAX / S) return fail(MC_ERR_INVALID, "predictive: C * S overflows");
    bool gb = false;
    int nmax = 0;
    bool ties = false;
    for (size_t t = 0; t < p->pw_terms.size(); ++t) {
        const int dist = p->pw_terms[t].dist;
        // an expression term whose root is a count or Student-t node (internal.h
        // PwSampler)
        if (dist == MC_DIST_EXPR && t < p->pw_samplers.size() && p->pw_samplers[t].kind >= 0) {
            nmax = std::max(nmax, p->pw_terms[t].expr_n > 16 ? 32 : 16);
            ties |= p->pw_samplers[t].kind < PW_SAMPLER_STUDENT_T;
            continue;
        }
        if (!pp_sampled(dist))
            return fail(MC_ERR_UNSUPPORTED, "predictive: term %zu (%s) has no sampling "
                        "distribution", t, dist == MC_DIST_EXPR ? "an expression term"
                        : dist == MC_DIST_IDENTITY ? "an identity term" : "unknown");
        gb |= dist == MC_DIST_GAMMA || dist == MC_DIST_BETA;
    }
    if (v->M > (int64_t)UINT32_MAX)
        return fail(MC_ERR_UNSUPPORTED, "predictive: %lld observations exceed the 32-bit "
                    "counter index", (long long)v->M);
    out->v = v;
    out->Sp = (S + thin - 1) / thin;
    out->Np = C * out->Sp;
    out->gb = gb;
    out->nmax = nmax;
    out->ties = ties;
    pw_split(out->Np, v->ntiles, &out->B, &out->per);
    return MC_OK;
}
int64_t pp_need(const PpPlan& L) {
    // (the five fields per block; with count terms the ties' count as well)
    return L.B > 1 ? L.B * (PP_COUNT + (L.ties ? 1 : 0)) * L.v->M * (int64_t)sizeof(double)
                   : 0;
}

}  // namespace

extern "C" int mc_predictive_draw(int dist, float loc_or_alpha, float scale_or_rate_or_beta,
                                  uint64_t seed, uint32_t chain, uint32_t iter, uint32_t obs,
                                  float* out) {
    if (!out) return fail(MC_ERR_INVALID, "predictive: out is NULL");
    if (!pp_sampled(dist))
        return fail(MC_ERR_UNSUPPORTED, "predictive: distribution %d has no sampling "
                    "distribution", dist);
    *out = pp_draw<true>(dist, loc_or_alpha, scale_or_rate_or_beta, seed, chain, iter, obs);
    return MC_OK;
}

extern "C" int mc_predictive_draw_discrete(int kind, float total, float eta, uint64_t seed,
                                           uint32_t chain, uint32_t iter, uint32_t obs,
                                           float* out) {
    if (!out) return fail(MC_ERR_INVALID, "predictive: out is NULL");
    if (kind < MC_DISCRETE_BERNOULLI || kind > MC_DISCRETE_POISSON)
        return fail(MC_ERR_INVALID, "predictive: unknown discrete distribution %d", kind);
    *out = pp_draw_discrete(kind, total, eta, seed, chain, iter, obs);
    return MC_OK;
}

extern "C" int mc_predictive_draw_student_t(float df, float loc, float scale, int half,
                                            uint64_t seed, uint32_t chain, uint32_t iter,
                                            uint32_t obs, float* out) {
    if (!out) return fail(MC_ERR_INVALID, "predictive: out is NULL");
    *out = pp_student_t(df, loc, scale, half != 0, seed, chain, iter, obs);
    return MC_OK;
}

extern "C" int32_t mc_program_num_count_terms(const mc_program* p) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    int32_t n = 0;
    for (const PwSampler& sd : p->pw_samplers)
        n += sd.kind >= 0 && sd.kind < PW_SAMPLER_STUDENT_T ? 1 : 0;
    return n;
}

extern "C" int64_t mc_predictive_workspace_bytes(const mc_program* p, int64_t C, int64_t S,
                                                 int64_t thin) {
    PpPlan L;
    const int rc = pp_plan(p, C, S, thin, &L);
    return rc != MC_OK ? rc : pp_need(L);
}

extern "C" int mc_predictive(const mc_program* p, int64_t C, int64_t S, int64_t thin,
                             uint64_t seed, int64_t chain_offset, int64_t iter_offset,
                             const float* samples, double* stats, float* yrep, void* ws,
                             int64_t ws_bytes, void* hip_stream) {
    return mc_predictive_eq(p, C, S, thin, seed, chain_offset, iter_offset, samples, stats,
                            nullptr, yrep, ws, ws_bytes, hip_stream);
}

extern "C" int mc_predictive_eq(const mc_program* p, int64_t C, int64_t S, int64_t thin,
                                uint64_t seed, int64_t chain_offset, int64_t iter_offset,
                                const float* samples, double* stats, double* equal, float* yrep,
                                void* ws, int64_t ws_bytes, void* hip_stream) {
    PpPlan L;
    const int rc = pp_plan(p, C, S, thin, &L);
    if (rc != MC_OK) return rc;
    if (!samples || !stats) return fail(MC_ERR_INVALID, "predictive: NULL samples / stats");
    if (equal && !L.ties)
        return fail(MC_ERR_UNSUPPORTED, "predictive: the count of ties needs a likelihood with "
                    "a count term (pass equal = NULL)");
    if (chain_offset < 0 || chain_offset + C > (int64_t)UINT32_MAX)
        return fail(MC_ERR_INVALID, "predictive: chain ids must fit in 32 bits");
    if (iter_offset < 0 || iter_offset + S > (int64_t)UINT32_MAX)
        return fail(MC_ERR_INVALID, "predictive: iteration ids must fit in 32 bits");
    const int64_t need = pp_need(L);
    if (need > 0 && (!ws || ws_bytes < need))
        return fail(MC_ERR_INVALID, "predictive: the workspace needs %lld bytes",
                    (long long)need);
    hipStream_t st = (hipStream_t)hip_stream;
    const PwCtx X = pw_ctx_of(p, L.v);
    PpRun R;
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
    double* eqpart = !equal ? nullptr
                     : L.B > 1 ? (double*)ws + L.B * PP_COUNT * L.v->M : equal;
    const dim3 grid((unsigned)L.v->ntiles, (unsigned)L.B);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kPwBlock), 0, st, X, R, samples, part, yrep,
                           (const PwSampler*)L.v->d_samplers, eqpart);
    };
    // programs with count or Student-t terms run the NMAX > 0 kernel (it
    // carries every sampler); everything else the kernels without that path
    const int nmax = L.nmax;
    if (nmax > 16) launch(k_predictive<true, 32>);
    else if (nmax > 0) launch(k_predictive<true, 16>);
    else if (L.gb) launch(k_predictive<true, 0>);
    else launch(k_predictive<false, 0>);
    MC_HIP_TRY(hipGetLastError());
    if (L.B > 1) {
        hipLaunchKernelGGL(k_pp_merge, dim3((unsigned)((L.v->M + 255) / 256)), dim3(256), 0, st,
                           (const double*)part, L.v->M, (int32_t)L.B, stats,
                           (const double*)eqpart, equal);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}
