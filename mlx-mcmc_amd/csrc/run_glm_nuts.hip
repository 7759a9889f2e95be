// run_glm_nuts.hip — mc_nuts_run_glm: NUTS of a design-matrix program on the
// kernels of glm.h and glm_nuts.h.
//
// A window is one k_glm_nuts_step START launch and then ticks, each one
// k_glm_grad launch at the chains' pending positions and one k_glm_nuts_step
// launch.  How many ticks a window needs — the largest per-chain total of
// leaves — is known only on the device, so the ticks are enqueued in batches
// of T; after each batch a one-wave kernel adds the chain blocks' counts of
// chains that are not done, the word is copied to a pinned host word the
// program owns, and the stream is synchronised.  THIS IS THE ONE ENTRY OF THE
// LIBRARY THAT SYNCHRONISES INSIDE THE CALL (it cannot be captured into a graph).
// The loop ends at zero chains left; iter_count * 2^max_tree_depth ticks, which
// no run can need, end it with an internal error.  No allocation in the call.
#include "launch.h"
#include "glm.h"
#include "glm_nuts.h"

static int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

// Ticks per batch.  The ticks enqueued after the last chain finished are T / 2
// on average and the host's poll costs one stream round trip per T ticks; 32
// keeps both small against windows of hundreds of leaves.
// MC_GLM_NUTS_BATCH in the environment overrides it (measurements).
static int nuts_glm_batch() {
    static const int t = [] {
        const char* e = std::getenv("MC_GLM_NUTS_BATCH");
        const int v = e ? std::atoi(e) : 0;
        return v >= 1 && v <= 4096 ? v : 32;
    }();
    return t;
}

// workspace: the pending positions qT [blocks][D][32]; the arena
// [blocks][nuts_arena_vectors + 1][D][32]; the walk state [blocks][words][32];
// the blocks' counts and the total; the partial blocks
struct GlmNutsWs {
    int64_t q, arena, words, cnt, part, total;
};
static GlmNutsWs glm_nuts_ws(const mc_program* p, int64_t C, int max_depth, int S) {
    const int64_t blocks = (C + kGlmChains - 1) / kGlmChains;
    const int64_t vec = blocks * p->D * kGlmChains * 4;
    GlmNutsWs w;
    w.q = 0;
    w.arena = align256(vec);
    w.words = w.arena + align256((nuts_arena_vectors(max_depth) + 1) * vec);
    w.cnt = w.words + align256(blocks * kGlmNutsWords * kGlmChains * 4);
    w.part = w.cnt + align256((blocks + 1) * 4);
    w.total = w.part + align256((int64_t)S * blocks * glm_block_floats(p->glm) * 4);
    return w;
}

static int64_t g_ticks = 0, g_polls = 0;  // mc_debug_glm_nuts_stats
extern "C" int mc_debug_glm_nuts_stats(int64_t* ticks, int64_t* polls) {
    if (ticks) *ticks = g_ticks;
    if (polls) *polls = g_polls;
    g_ticks = g_polls = 0;
    return MC_OK;
}

extern "C" int64_t mc_nuts_glm_workspace_bytes(const mc_program* p, int64_t C, int32_t max_depth) {
    if (!is_glm(p) || p->glm->softmax || C < 0 || max_depth < 0 || max_depth > kMaxTreeDepth)
        return -1;
    return glm_nuts_ws(p, C, max_depth, glm_plan_slices(p->glm, C)).total;
}

extern "C" int mc_nuts_run_glm(const mc_program* p, const mc_run_config* cfg, void* state,
                               float* samples, const mc_trace* tr, void* ws, int64_t ws_bytes,
                               void* stream) {
    int rc = check_cfg(p, cfg, state);
    if (rc) return rc;
    if (!is_glm(p))
        return fail(MC_ERR_UNSUPPORTED, "mc_nuts_run_glm runs design-matrix (X @ beta) programs "
                    "(mc_program_create_glm) only: mc_nuts_run runs this one");
    if (p->glm->softmax)
        return fail(MC_ERR_UNSUPPORTED, "mc_nuts_run_glm: a softmax program "
                    "(mc_program_create_glm_softmax) runs under mc_hmc_run only: k_glm_nuts_step "
                    "reads one column per chain, not the class-packed gradient blocks");
    if (cfg->max_tree_depth < 0 || cfg->max_tree_depth > kMaxTreeDepth)
        return fail(MC_ERR_UNSUPPORTED, "max_tree_depth must be in [0, %d]", kMaxTreeDepth);
    const GlmPlan* g = p->glm;
    const int64_t C = cfg->num_chains;
    const int S = glm_plan_slices(g, C);
    const int MAXJ = cfg->max_tree_depth;
    const GlmNutsWs W = glm_nuts_ws(p, C, MAXJ, S);
    if (ws == nullptr || ws_bytes < W.total)
        return fail(MC_ERR_INVALID, "mc_nuts_run_glm: workspace too small: need %lld bytes",
                    (long long)W.total);
    if (C == 0 || cfg->iter_count == 0) return MC_OK;
    ws_forget(ws);
    hipStream_t st = (hipStream_t)stream;
    RunState R = run_state(p, cfg, state);
    const TraceDev td = trace_of(tr);
    char* b = (char*)ws;
    float* qT = (float*)(b + W.q);
    float* arena = (float*)(b + W.arena);
    uint32_t* words = (uint32_t*)(b + W.words);
    int32_t* cnt = (int32_t*)(b + W.cnt);
    float* part = (float*)(b + W.part);
    const int64_t blocks = (C + kGlmChains - 1) / kGlmChains;
    int32_t* d_left = cnt + blocks;
    const GlmPart RP = {part, blocks * glm_block_floats(g), S, 0};
    auto step = [&](int phase) {
        hipLaunchKernelGGL((k_glm_nuts_step<0>), dim3((unsigned)blocks), dim3(256), 0, st, g->dev,
                           R.A, phase, R.scalars, R.q, R.g, samples, td, qT, arena, words, cnt, RP);
        return hipGetLastError();
    };
    MC_HIP_TRY(step(GLM_NUTS_START));
    if (MAXJ == 0) return MC_OK;  // (START ran the window: no iteration has a leaf)
    const int T = nuts_glm_batch();
    const int64_t cap = cfg->iter_count << MAXJ;
    for (int64_t ticks = 0; ticks < cap;) {
        const int tb = (int)std::min<int64_t>(T, cap - ticks);
        for (int t = 0; t < tb; ++t) {
            rc = glm_launch_grad(g, qT, 1, kGlmChains, C, S, part, st);
            if (rc != MC_OK) return rc;
            MC_HIP_TRY(step(GLM_NUTS_TICK));
        }
        ticks += tb;
        hipLaunchKernelGGL((k_glm_nuts_left<0>), dim3(1), dim3(64), 0, st, cnt, blocks, d_left);
        MC_HIP_TRY(hipGetLastError());
        MC_HIP_TRY(hipMemcpyAsync(g->h_left, d_left, 4, hipMemcpyDeviceToHost, st));
        MC_HIP_TRY(hipStreamSynchronize(st));
        g_ticks += tb;
        g_polls += 1;
        if (*g->h_left == 0) return MC_OK;
    }
    return fail(MC_ERR_TIMEOUT, "mc_nuts_run_glm: internal error: %d chains not done after the %lld "
                "ticks no window of %lld iterations at depth %d can need", (int)*g->h_left,
                (long long)cap, (long long)cfg->iter_count, MAXJ);
}
