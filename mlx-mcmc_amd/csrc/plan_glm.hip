// plan_glm.hip — design-matrix programs (include/mcmc355.h mc_glm and
// mc_glm_softmax): validation,
// the padded device copies of X, X^T, y and the offset, the prior table, and the
// row-slice plan of the MFMA kernels (glm.h; the launches are in run_glm.hip).
#include "host.h"
#include "glm.h"

#include <cmath>

static int ceil32(int64_t x) { return (int)((x + 31) / 32 * 32); }

// Row slices of a launch of C chains: the explicit count, or enough that
// slices x gradient blocks (32 chains, CPB on a softmax plan) cover the CUs, at
// most 64 and at most one 32-row tile per wave (4 tiles per slice).
int glm_plan_slices(const GlmPlan* g, int64_t C) {
    if (g->slices > 0) return g->slices;
    const int64_t blocks = std::max<int64_t>(1, glm_grad_blocks(g, C));
    const int64_t cus = std::max(1, device_cus());
    int64_t S = (cus + blocks - 1) / blocks;
    S = std::min<int64_t>(S, std::max(1, g->dev.NT / 4));
    return (int)std::max<int64_t>(1, std::min<int64_t>(S, kGlmMaxSlices));
}

static void glm_describe(GlmPlan* g) {
    static const char* fam[] = {"normal", "bernoulli-logit", "poisson-log"};
    char buf[400];
    if (g->softmax) {
        std::snprintf(buf, sizeof buf,
                      "design-matrix softmax regression (categorical-logit): N = %d, P = %d, K = %d "
                      "on k_glm_softmax_grad / k_glm_hmc_step: Kp = %d class columns per chain, CPB = "
                      "%d chains per gradient block of 32 columns, %d coefficient tile%s of 32 (%d "
                      "accumulator registers per lane), %s row slices per gradient block", g->dev.N,
                      g->dev.P, g->dev.K, g->dev.Kp, g->dev.CPB, g->PT, g->PT == 1 ? "" : "s",
                      16 * g->PT, g->slices > 0 ? std::to_string(g->slices).c_str() : "automatic");
        g->note = buf;
        return;
    }
    if (g->wide) {
        std::snprintf(buf, sizeof buf,
                      "design-matrix GLM (%s): N = %d, P = %d on k_glm_grad_wide / k_glm_hmc_step: 32 "
                      "chains per block, %d columns per wave (%d coefficient tile%s of 32, %d "
                      "accumulator registers per lane), coefficients %s, %s row slices per chain "
                      "block", fam[g->dev.family], g->dev.N, g->dev.P, 32 * g->PTW, g->PTW,
                      g->PTW == 1 ? "" : "s", 16 * g->PTW,
                      g->dev.Pp > 256 ? "staged in chunks of 256 rows" : "resident in LDS",
                      g->slices > 0 ? std::to_string(g->slices).c_str() : "automatic");
        g->note = buf;
        return;
    }
    std::snprintf(buf, sizeof buf,
                  "design-matrix GLM (%s): N = %d, P = %d on k_glm_grad / k_glm_hmc_step: 32 chains "
                  "per block, %d coefficient tile%s of 32 (%d accumulator registers per lane), %s "
                  "row slices per chain block", fam[g->dev.family], g->dev.N, g->dev.P, g->PT,
                  g->PT == 1 ? "" : "s", 16 * g->PT,
                  g->slices > 0 ? std::to_string(g->slices).c_str() : "automatic");
    g->note = buf;
}

void glm_free(mc_program* p) {
    GlmPlan* g = p->glm;
    if (!g) return;
    for (void* d : {(void*)g->d_X, (void*)g->d_XT, (void*)g->d_y, (void*)g->d_off,
                    (void*)g->d_priors, (void*)g->d_scratch, (void*)g->d_norm})
        if (d) (void)hipFree(d);
    if (g->h_left) (void)hipHostFree(g->h_left);
    delete g;
    p->glm = nullptr;
}

int glm_set_slices(mc_program* p, int32_t S) {
    p->glm->slices = S;
    glm_describe(p->glm);
    return MC_OK;
}
int32_t glm_num_slices(const mc_program* p) {
    return p->glm->slices > 0 ? p->glm->slices : glm_plan_slices(p->glm, kGlmChains);
}
const char* glm_note(const mc_program* p) { return p->glm->note.c_str(); }

extern "C" int32_t mc_program_glm_slices(const mc_program* p, int64_t num_chains) {
    if (!p) return -1;
    return is_glm(p) ? glm_plan_slices(p->glm, num_chains) : 0;
}
extern "C" int32_t mc_program_glm_chain_block(const mc_program* p) {
    if (!p) return -1;
    return is_glm(p) ? kGlmChains : 0;
}

template <typename T>
static int upload(const std::vector<T>& h, T** d) {
    if (hipMalloc((void**)d, std::max<size_t>(1, h.size()) * sizeof(T)) != hipSuccess)
        return fail(MC_ERR_NOMEM, "device allocation of %zu bytes failed", h.size() * sizeof(T));
    if (!h.empty())
        MC_HIP_TRY(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return MC_OK;
}

// PTW of a wide plan: the first instantiation of k_glm_grad_wide (run_glm.hip)
// whose 128 PTW columns hold P
static int wide_ptw(int64_t P) {
    for (int ptw : {1, 2, 3, 4, 6, 8})
        if (128 * ptw >= P) return ptw;
    return 0;
}

// the prior table: fused terms on parameters with constant arguments
static int glm_priors(const mc_term* priors, int32_t n_priors, int32_t n_params,
                      std::vector<GlmPrior>& pri) {
    for (int32_t k = 0; k < n_priors; ++k) {
        const mc_term& t = priors[k];
        const bool dist_ok = (t.dist >= MC_DIST_NORMAL && t.dist <= MC_DIST_IDENTITY);
        const bool val_ok = (t.value.kind == MC_OP_PSCALAR && t.n == 1) || t.value.kind == MC_OP_PVEC;
        const bool args_ok = (t.loc.kind == MC_OP_CONST || t.loc.kind == MC_OP_NONE) &&
                             (t.scale.kind == MC_OP_CONST || t.scale.kind == MC_OP_NONE);
        if (!dist_ok || !val_ok || !args_ok || t.affine != 0)
            return fail(MC_ERR_UNSUPPORTED,
                        "design-matrix GLM: term %d beside the X @ beta likelihood is not a fused "
                        "prior whose value is a parameter, with constant arguments", k);
        if (t.n < 1 || t.value.param_offset < 0 || t.value.param_offset + t.n > n_params)
            return fail(MC_ERR_INVALID, "design-matrix GLM: prior %d: parameter range out of range",
                        k);
        if (t.value.transform < MC_XF_NONE || t.value.transform > MC_XF_LOG)
            return fail(MC_ERR_INVALID, "design-matrix GLM: prior %d: unknown transform", k);
        GlmPrior g;
        g.dist = t.dist;
        g.poff = t.value.param_offset;
        g.n = (int32_t)t.n;
        g.xf = t.value.transform;
        g.weight = t.weight;
        g.c0 = dist_c0(t.dist);
        g.m = t.loc.kind == MC_OP_CONST ? t.loc.value : 0.0f;
        g.s = t.scale.kind == MC_OP_CONST ? t.scale.value : 1.0f;
        g.logs = logf(g.s);
        g.lg = lgamma_norm(t.dist, g.m, g.s);
        pri.push_back(g);
    }
    return MC_OK;
}

// The program around a plan whose shape (dev.family, N, P, Np, Pp, the parameter
// offsets) is filled in: the zero-padded device copies X [Np][Pp], X^T [Pp][Np],
// y and the offset [Np], the prior table and the scratch.  Takes the plan over.
static int glm_build(GlmPlan* g, int32_t n_params, float lp_const, const float* xs, const float* ys,
                     const float* offs, const std::vector<GlmPrior>& pri, mc_program** out) {
    GlmDev& d = g->dev;
    const int64_t N = d.N, P = d.P, Np = d.Np, Pp = d.Pp;
    std::vector<float> X((size_t)(Np * Pp), 0.0f), XT((size_t)(Np * Pp), 0.0f), y((size_t)Np, 0.0f),
        off;
    for (int64_t i = 0; i < N; ++i)
        for (int64_t k = 0; k < P; ++k) {
            X[(size_t)(i * Pp + k)] = xs[i * P + k];
            XT[(size_t)(k * Np + i)] = xs[i * P + k];
        }
    std::copy(ys, ys + N, y.begin());
    if (offs) {
        off.assign((size_t)Np, 0.0f);
        std::copy(offs, offs + N, off.begin());
    }

    mc_program* p = new mc_program();
    p->D = n_params;
    p->lp_const = lp_const;
    p->sl.S = 1;
    p->glm = g;
    d.NT = (int32_t)(Np / 32);
    d.D = n_params;
    d.c0 = c_log_norm();
    d.lp_const = lp_const;
    d.n_priors = (int32_t)pri.size();
    int rc = upload(X, &g->d_X);
    if (rc == MC_OK) rc = upload(XT, &g->d_XT);
    if (rc == MC_OK) rc = upload(y, &g->d_y);
    if (rc == MC_OK && !off.empty()) rc = upload(off, &g->d_off);
    if (rc == MC_OK) rc = upload(pri, &g->d_priors);
    if (rc == MC_OK &&
        hipMalloc((void**)&g->d_scratch, (size_t)kGlmMaxSlices * kGlmScratchBlocks *
                                             glm_block_floats(g) * 4) != hipSuccess)
        rc = fail(MC_ERR_NOMEM, "device allocation of the GLM scratch failed");
    if (rc == MC_OK && hipHostMalloc((void**)&g->h_left, 64, hipHostMallocDefault) != hipSuccess)
        rc = fail(MC_ERR_NOMEM, "pinned host allocation of the GLM NUTS counter failed");
    if (rc != MC_OK) {
        const std::string err = g_last_error;
        mc_program_destroy(p);
        g_last_error = err;
        return rc;
    }
    d.X = g->d_X;
    d.XT = g->d_XT;
    d.y = g->d_y;
    d.off = g->d_off;
    d.priors = g->d_priors;
    glm_describe(g);
    *out = p;
    return MC_OK;
}

static int create_glm(bool wide, const mc_glm* glm, const mc_term* priors, int32_t n_priors,
                      int32_t n_params, float lp_const, const float* data, int64_t n_data,
                      mc_program** out) {
    if (!glm || !out) return fail(MC_ERR_INVALID, "NULL glm / out");
    if (n_params < 1) return fail(MC_ERR_INVALID, "n_params must be >= 1");
    if (n_priors < 0 || (n_priors > 0 && !priors)) return fail(MC_ERR_INVALID, "priors");
    if (n_data < 0 || (n_data > 0 && !data)) return fail(MC_ERR_INVALID, "data");
    if (glm->family < MC_GLM_NORMAL || glm->family > MC_GLM_POISSON_LOG)
        return fail(MC_ERR_INVALID, "unknown GLM family %d", glm->family);
    const int64_t N = glm->n, P = glm->p;
    if (N < 1 || P < 1) return fail(MC_ERR_INVALID, "a design matrix needs N >= 1 and P >= 1");
    if (wide && P > MC_GLM_WIDE_MAX_P)
        return fail(MC_ERR_UNSUPPORTED,
                    "design-matrix GLM on the column-split kernel: P = %lld columns, at most %d "
                    "(a wave holds a quarter of the gradient of a block of 32 chains in accumulator "
                    "registers, 16 per 32 coefficients)", (long long)P, MC_GLM_WIDE_MAX_P);
    if (!wide && P > MC_GLM_MAX_P)
        return fail(MC_ERR_UNSUPPORTED,
                    "design-matrix GLM: P = %lld columns, at most %d (the gradient of a block of 32 "
                    "chains lives in accumulator registers, 16 per 32 coefficients); "
                    "mc_program_create_glm_wide (glm_kernel=\"wide\") splits the columns over the "
                    "waves and takes up to %d", (long long)P, MC_GLM_MAX_P, MC_GLM_WIDE_MAX_P);
    const int PTW = wide ? wide_ptw(P) : 0;
    int PT = 1;
    while (32 * PT < P) PT *= 2;
    if (wide) PT = 4 * PTW;
    const int64_t Np = (N + 31) / 32 * 32, Pp = 32 * PT;
    if (Np * Pp >= ((int64_t)1 << 31))
        return fail(MC_ERR_UNSUPPORTED,
                    "design-matrix GLM: N * P = %lld x %lld (padded %lld x %lld) does not fit a "
                    "32-bit index", (long long)N, (long long)P, (long long)Np, (long long)Pp);
    auto in_pool = [&](int64_t off, int64_t n) { return off >= 0 && off <= n_data - n; };
    if (!in_pool(glm->x_pool, N * P) || !in_pool(glm->y_pool, N) ||
        (glm->offset_pool >= 0 && !in_pool(glm->offset_pool, N)))
        return fail(MC_ERR_INVALID, "design-matrix GLM: data range out of pool");
    if (glm->beta_offset < 0 || glm->beta_offset + P > n_params)
        return fail(MC_ERR_INVALID, "design-matrix GLM: beta range out of the parameters");
    auto pscalar_ok = [&](const mc_operand& o) {
        return o.param_offset >= 0 && o.param_offset < n_params;
    };
    const mc_operand& ic = glm->intercept;
    if (!(ic.kind == MC_OP_NONE || ic.kind == MC_OP_CONST ||
          (ic.kind == MC_OP_PSCALAR && ic.transform == MC_XF_NONE && pscalar_ok(ic))))
        return fail(MC_ERR_UNSUPPORTED, "design-matrix GLM: the intercept is a constant or an "
                    "untransformed scalar parameter");
    const mc_operand& sc = glm->scale;
    if (glm->family == MC_GLM_NORMAL &&
        !(sc.kind == MC_OP_CONST ||
          (sc.kind == MC_OP_PSCALAR && pscalar_ok(sc) &&
           (sc.transform == MC_XF_NONE || sc.transform == MC_XF_EXP))))
        return fail(MC_ERR_UNSUPPORTED, "design-matrix GLM: the normal family's scale is a "
                    "constant, a scalar parameter or mx.exp of one");
    std::vector<GlmPrior> pri;
    const int prc = glm_priors(priors, n_priors, n_params, pri);
    if (prc != MC_OK) return prc;

    GlmPlan* g = new GlmPlan();
    g->PT = PT;
    g->wide = wide;
    g->PTW = PTW;
    GlmDev& d = g->dev;
    d.family = glm->family;
    d.N = (int32_t)N;
    d.P = (int32_t)P;
    d.Np = (int32_t)Np;
    d.Pp = (int32_t)Pp;
    d.boff = glm->beta_offset;
    d.ik = ic.kind;
    d.ipoff = ic.param_offset;
    d.ival = ic.value;
    d.sk = glm->family == MC_GLM_NORMAL ? sc.kind : MC_OP_NONE;
    d.spoff = sc.param_offset;
    d.sxf = sc.transform;
    d.sval = sc.value;
    return glm_build(g, n_params, lp_const, data + glm->x_pool, data + glm->y_pool,
                     glm->offset_pool >= 0 ? data + glm->offset_pool : nullptr, pri, out);
}

extern "C" int mc_program_create_glm(const mc_glm* glm, const mc_term* priors, int32_t n_priors,
                                     int32_t n_params, float lp_const, const float* data,
                                     int64_t n_data, mc_program** out) {
    return create_glm(false, glm, priors, n_priors, n_params, lp_const, data, n_data, out);
}

extern "C" int mc_program_create_glm_wide(const mc_glm* glm, const mc_term* priors, int32_t n_priors,
                                          int32_t n_params, float lp_const, const float* data,
                                          int64_t n_data, mc_program** out) {
    return create_glm(true, glm, priors, n_priors, n_params, lp_const, data, n_data, out);
}

// Softmax regression (include/mcmc355.h mc_glm_softmax): the class-packed plan of
// glm_softmax.h.  Every check runs before any device work.
extern "C" int mc_program_create_glm_softmax(const mc_glm_softmax* glm, const mc_term* priors,
                                             int32_t n_priors, int32_t n_params, float lp_const,
                                             const float* data, int64_t n_data, mc_program** out) {
    if (!glm || !out) return fail(MC_ERR_INVALID, "NULL glm / out");
    if (n_params < 1) return fail(MC_ERR_INVALID, "n_params must be >= 1");
    if (n_priors < 0 || (n_priors > 0 && !priors)) return fail(MC_ERR_INVALID, "priors");
    if (n_data < 0 || (n_data > 0 && !data)) return fail(MC_ERR_INVALID, "data");
    const int64_t N = glm->n, P = glm->p, K = glm->k;
    if (N < 1 || P < 1) return fail(MC_ERR_INVALID, "a design matrix needs N >= 1 and P >= 1");
    if (K < 2 || K > MC_GLM_SOFTMAX_MAX_K)
        return fail(MC_ERR_UNSUPPORTED,
                    "design-matrix softmax regression: K = %lld classes, from 2 to %d (the classes "
                    "of a chain are adjacent columns of one 32-column gradient block; one class is "
                    "a constant log density)", (long long)K, MC_GLM_SOFTMAX_MAX_K);
    if (P > MC_GLM_MAX_P)
        return fail(MC_ERR_UNSUPPORTED,
                    "design-matrix softmax regression: P = %lld columns, at most %d whatever K is "
                    "(the gradient of a block of 32 (chain, class) columns lives in accumulator "
                    "registers, 16 per 32 coefficients)", (long long)P, MC_GLM_MAX_P);
    int PT = 1, Kp = 2;
    while (32 * PT < P) PT *= 2;
    while (Kp < K) Kp *= 2;
    const int64_t Np = (N + 31) / 32 * 32, Pp = 32 * PT;
    if (Np * Pp >= ((int64_t)1 << 31))
        return fail(MC_ERR_UNSUPPORTED,
                    "design-matrix softmax regression: N * P = %lld x %lld (padded %lld x %lld) "
                    "does not fit a 32-bit index", (long long)N, (long long)P, (long long)Np,
                    (long long)Pp);
    auto in_pool = [&](int64_t off, int64_t n) { return off >= 0 && off <= n_data - n; };
    if (!in_pool(glm->x_pool, N * P) || !in_pool(glm->y_pool, N))
        return fail(MC_ERR_INVALID, "design-matrix softmax regression: data range out of pool");
    if (glm->beta_offset < 0 || glm->beta_offset + P * K > n_params)
        return fail(MC_ERR_INVALID, "design-matrix softmax regression: the [P, K] coefficient "
                    "range is out of the parameters");
    if (glm->icpt_offset >= 0 && glm->icpt_offset + K > n_params)
        return fail(MC_ERR_INVALID, "design-matrix softmax regression: the K class intercepts are "
                    "out of the parameters");
    const float* ys = data + glm->y_pool;
    for (int64_t i = 0; i < N; ++i)
        if (!(ys[i] >= 0.0f && ys[i] < (float)K && ys[i] == std::floor(ys[i])))
            return fail(MC_ERR_INVALID, "design-matrix softmax regression: label %lld is %g, not "
                        "an integer in 0 .. %lld", (long long)i, (double)ys[i], (long long)(K - 1));
    std::vector<GlmPrior> pri;
    const int prc = glm_priors(priors, n_priors, n_params, pri);
    if (prc != MC_OK) return prc;
    GlmPlan* g = new GlmPlan();
    g->PT = PT;
    g->softmax = true;
    GlmDev& d = g->dev;
    d.family = MC_GLM_CATEGORICAL_LOGIT;
    d.N = (int32_t)N;
    d.P = (int32_t)P;
    d.Np = (int32_t)Np;
    d.Pp = (int32_t)Pp;
    d.boff = glm->beta_offset;
    d.ik = d.sk = MC_OP_NONE;
    d.K = (int32_t)K;
    d.Kp = Kp;
    d.CPB = 32 / Kp;
    d.aoff = glm->icpt_offset >= 0 ? glm->icpt_offset : -1;
    return glm_build(g, n_params, lp_const, data + glm->x_pool, ys, nullptr, pri, out);
}
