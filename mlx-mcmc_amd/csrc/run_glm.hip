// run_glm.hip — launches of the design-matrix kernels (glm.h): mc_logp_grad,
// mc_state_init and mc_hmc_run of a program made by mc_program_create_glm,
// mc_program_create_glm_wide (the gradient then runs on glm_wide.h's kernel) or
// mc_program_create_glm_softmax (on glm_softmax.h's, whose gradient blocks hold
// CPB = 32 / Kp chains: the partial blocks are counted by glm_grad_blocks).
//
// mc_hmc_run enqueues, per iteration, one k_glm_hmc_step for the iteration
// start, then per leapfrog step one k_glm_grad and one k_glm_hmc_step, in stream
// order: the kernel boundary is the exchange of the per-slice partials (a
// [P + 4][32] block per slice and chain block, not the few-float records of the
// exchange kernels).  As k_hmc, an iteration reuses the current position's
// gradient for its first half kick: L gradient launches and L + 1 step
// launches.  No host synchronisation and no allocation inside the call.
#include "launch.h"
#include "glm_wide.h"
#include "glm_softmax.h"

static int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

// workspace of an HMC run of C chains: the proposal and its momentum,
// chain-minor [blocks][D][32]; H_init per chain; the partial blocks
struct GlmWs {
    int64_t q, p, h0, part, total;
};
static GlmWs glm_ws(const mc_program* p, int64_t C, int S) {
    const int64_t blocks = (C + kGlmChains - 1) / kGlmChains;
    const int64_t vec = align256(blocks * p->D * kGlmChains * 4);
    GlmWs w;
    w.q = 0;
    w.p = vec;
    w.h0 = 2 * vec;
    w.part = w.h0 + align256(blocks * kGlmChains * 4);
    w.total = w.part + align256((int64_t)S * glm_grad_blocks(p->glm, C) *
                                glm_block_floats(p->glm) * 4);
    return w;
}

int64_t glm_hmc_workspace_bytes(const mc_program* p, int64_t C) {
    return glm_ws(p, C, glm_plan_slices(p->glm, C)).total;
}

template <int FAM, int PT>
static int launch_grad_pt(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S,
                          float* part, hipStream_t st) {
    const int64_t blocks = (C + kGlmChains - 1) / kGlmChains;
    const size_t lds = (size_t)PT * 1024 * 4;
    hipLaunchKernelGGL((k_glm_grad<FAM, PT>), dim3((unsigned)S, (unsigned)blocks), dim3(256), lds,
                       st, g->dev, q, sc, sp, C, S, part);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}
template <int FAM>
static int launch_grad_fam(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S,
                           float* part, hipStream_t st) {
    switch (g->PT) {
        case 1: return launch_grad_pt<FAM, 1>(g, q, sc, sp, C, S, part, st);
        case 2: return launch_grad_pt<FAM, 2>(g, q, sc, sp, C, S, part, st);
        case 4: return launch_grad_pt<FAM, 4>(g, q, sc, sp, C, S, part, st);
        default: return launch_grad_pt<FAM, 8>(g, q, sc, sp, C, S, part, st);
    }
}
template <int FAM, int PTW>
static int launch_wide_ptw(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S,
                           float* part, hipStream_t st) {
    const int64_t blocks = (C + kGlmChains - 1) / kGlmChains;
    hipLaunchKernelGGL((k_glm_grad_wide<FAM, PTW>), dim3((unsigned)S, (unsigned)blocks), dim3(256), 0,
                       st, g->dev, q, sc, sp, C, S, part);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}
template <int FAM>
static int launch_wide_fam(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S,
                           float* part, hipStream_t st) {
    switch (g->PTW) {
        case 1: return launch_wide_ptw<FAM, 1>(g, q, sc, sp, C, S, part, st);
        case 2: return launch_wide_ptw<FAM, 2>(g, q, sc, sp, C, S, part, st);
        case 3: return launch_wide_ptw<FAM, 3>(g, q, sc, sp, C, S, part, st);
        case 4: return launch_wide_ptw<FAM, 4>(g, q, sc, sp, C, S, part, st);
        case 6: return launch_wide_ptw<FAM, 6>(g, q, sc, sp, C, S, part, st);
        case 8: return launch_wide_ptw<FAM, 8>(g, q, sc, sp, C, S, part, st);
        default: return fail(MC_ERR_INVALID, "k_glm_grad_wide has no instantiation PTW = %d", g->PTW);
    }
}
template <int PT, int KP>
static int launch_softmax_kp(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S,
                             float* part, hipStream_t st) {
    const int64_t blocks = glm_grad_blocks(g, C);
    const size_t lds = (size_t)PT * 1024 * 4;
    hipLaunchKernelGGL((k_glm_softmax_grad<PT, KP>), dim3((unsigned)S, (unsigned)blocks), dim3(256),
                       lds, st, g->dev, q, sc, sp, C, S, part);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}
template <int PT>
static int launch_softmax_pt(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S,
                             float* part, hipStream_t st) {
    switch (g->dev.Kp) {
        case 2: return launch_softmax_kp<PT, 2>(g, q, sc, sp, C, S, part, st);
        case 4: return launch_softmax_kp<PT, 4>(g, q, sc, sp, C, S, part, st);
        case 8: return launch_softmax_kp<PT, 8>(g, q, sc, sp, C, S, part, st);
        case 16: return launch_softmax_kp<PT, 16>(g, q, sc, sp, C, S, part, st);
        case 32: return launch_softmax_kp<PT, 32>(g, q, sc, sp, C, S, part, st);
        default: return fail(MC_ERR_INVALID, "k_glm_softmax_grad has no instantiation Kp = %d",
                             g->dev.Kp);
    }
}
// k_glm_grad, k_glm_grad_wide on a wide plan or k_glm_softmax_grad on a softmax
// plan, at the positions q (strides sc, sp: glm.h) of C chains, S slices
static int launch_grad(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S,
                       float* part, hipStream_t st) {
    if (g->softmax) {
        switch (g->PT) {
            case 1: return launch_softmax_pt<1>(g, q, sc, sp, C, S, part, st);
            case 2: return launch_softmax_pt<2>(g, q, sc, sp, C, S, part, st);
            case 4: return launch_softmax_pt<4>(g, q, sc, sp, C, S, part, st);
            default: return launch_softmax_pt<8>(g, q, sc, sp, C, S, part, st);
        }
    }
    if (g->wide) {
        switch (g->dev.family) {
            case MC_GLM_NORMAL: return launch_wide_fam<MC_GLM_NORMAL>(g, q, sc, sp, C, S, part, st);
            case MC_GLM_BERNOULLI_LOGIT:
                return launch_wide_fam<MC_GLM_BERNOULLI_LOGIT>(g, q, sc, sp, C, S, part, st);
            default: return launch_wide_fam<MC_GLM_POISSON_LOG>(g, q, sc, sp, C, S, part, st);
        }
    }
    switch (g->dev.family) {
        case MC_GLM_NORMAL: return launch_grad_fam<MC_GLM_NORMAL>(g, q, sc, sp, C, S, part, st);
        case MC_GLM_BERNOULLI_LOGIT:
            return launch_grad_fam<MC_GLM_BERNOULLI_LOGIT>(g, q, sc, sp, C, S, part, st);
        default: return launch_grad_fam<MC_GLM_POISSON_LOG>(g, q, sc, sp, C, S, part, st);
    }
}

// One gradient launch and its reduce, in chunks of kGlmScratchBlocks gradient
// blocks (32 chains each, CPB on a softmax plan) on the program's scratch
// (stream order makes the reuse safe).
template <bool INIT>
static int glm_eval(const mc_program* p, int64_t n, const float* q, float* lp, float* grad,
                    double eps0, mc_chain_scalars* scal, float* st_q, hipStream_t st) {
    const GlmPlan* g = p->glm;
    const int S = glm_plan_slices(g, n);
    const int64_t chunk = (int64_t)kGlmScratchBlocks * (g->softmax ? g->dev.CPB : kGlmChains);
    const float mu = mc_logf_ref((float)(10.0 * eps0));  // nuts.py:63, as k_init
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t nc = std::min(chunk, n - c0);
        const int64_t blocks = (nc + kGlmChains - 1) / kGlmChains;
        const float* qc = q + c0 * p->D;
        const int rc = launch_grad(g, qc, p->D, 1, nc, S, g->d_scratch, st);
        if (rc != MC_OK) return rc;
        const GlmPart R = {g->d_scratch, glm_grad_blocks(g, nc) * glm_block_floats(g), S, 0};
        hipLaunchKernelGGL((k_glm_finish<INIT>), dim3((unsigned)blocks), dim3(256), 0, st, g->dev,
                           nc, qc, R, lp ? lp + c0 : nullptr, grad + c0 * p->D, eps0, mu,
                           scal ? scal + c0 : nullptr, st_q ? st_q + c0 * p->D : nullptr);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}

int glm_launch_grad(const GlmPlan* g, const float* q, int sc, int sp, int64_t C, int S, float* part,
                    hipStream_t st) {
    return launch_grad(g, q, sc, sp, C, S, part, st);
}

int glm_logp_grad(const mc_program* p, int64_t n, const float* q, float* lp, float* g,
                  hipStream_t st) {
    return glm_eval<false>(p, n, q, lp, g, 0.0, nullptr, nullptr, st);
}

int glm_state_init(const mc_program* p, int64_t C, const float* q0, double eps0, void* state,
                   hipStream_t st) {
    int64_t qo, go;
    mc_state_offsets(p, C, &qo, &go);
    char* b = (char*)state;
    return glm_eval<true>(p, C, q0, nullptr, (float*)(b + go), eps0, (mc_chain_scalars*)b,
                          (float*)(b + qo), st);
}

int glm_hmc_run(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                const mc_trace* tr, void* ws, int64_t ws_bytes, hipStream_t st) {
    const GlmPlan* g = p->glm;
    const int64_t C = cfg->num_chains;
    const int S = glm_plan_slices(g, C);
    const GlmWs W = glm_ws(p, C, S);
    if (ws == nullptr || ws_bytes < W.total)
        return fail(MC_ERR_INVALID, "workspace too small: need %lld bytes", (long long)W.total);
    ws_forget(ws);
    RunState R = run_state(p, cfg, state);
    const TraceDev td = trace_of(tr);
    char* b = (char*)ws;
    float* qT = (float*)(b + W.q);
    float* pT = (float*)(b + W.p);
    float* H0 = (float*)(b + W.h0);
    float* part = (float*)(b + W.part);
    const int64_t blocks = (C + kGlmChains - 1) / kGlmChains;
    const GlmPart RP = {part, glm_grad_blocks(g, C) * glm_block_floats(g), S, 0};
    const int L = cfg->num_leapfrog_steps;
    auto step = [&](int phase, int64_t it) {
        hipLaunchKernelGGL((k_glm_hmc_step<0>), dim3((unsigned)blocks), dim3(256), 0, st, g->dev, R.A,
                           phase, it, R.scalars, R.q, R.g, samples, td, qT, pT, H0, RP);
        return hipGetLastError();
    };
    for (int64_t it = cfg->iter_begin; it < cfg->iter_begin + cfg->iter_count; ++it) {
        MC_HIP_TRY(step(GLM_START, it));
        for (int l = 0; l < L; ++l) {
            // the proposal, chain-minor: strides (1, 32)
            const int rc = launch_grad(g, qT, 1, kGlmChains, C, S, part, st);
            if (rc != MC_OK) return rc;
            if (l + 1 < L) MC_HIP_TRY(step(GLM_INTERIOR, it));
        }
        MC_HIP_TRY(step(GLM_END, it));
    }
    return MC_OK;
}
