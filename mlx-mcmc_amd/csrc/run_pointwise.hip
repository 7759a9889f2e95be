// run_pointwise.hip — the pointwise view of a program and the launches of
// csrc/pointwise.h (mc_program_num_elements, mc_program_enable_pointwise,
// mc_pointwise_workspace_bytes, mc_pointwise_stats).
#include "host.h"
#include "pointwise.h"
#include "pw_view.h"

namespace {

template <typename T>
hipError_t pw_upload(T** dst, const T* src, size_t n) {
    hipError_t e = hipMalloc((void**)dst, std::max<size_t>(1, n) * sizeof(T));
    if (e != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    return hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice);
}

int64_t pw_elements(const mc_program* p) {
    int64_t m = 0;
    for (const DevTerm& t : p->pw_terms) m += t.n;
    return m;
}

}  // namespace

void pw_free(mc_program* p) {
    PwView* v = (PwView*)p->pw;
    if (!v) return;
    if (v->d_terms) (void)hipFree(v->d_terms);
    if (v->d_nodes) (void)hipFree(v->d_nodes);
    if (v->d_data) (void)hipFree(v->d_data);
    if (v->d_index) (void)hipFree(v->d_index);
    if (v->d_tiles) (void)hipFree(v->d_tiles);
    if (v->d_samplers) (void)hipFree(v->d_samplers);
    delete v;
    p->pw = nullptr;
}

extern "C" int64_t mc_program_num_elements(const mc_program* p) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    return pw_elements(p);
}

extern "C" int mc_program_enable_pointwise(mc_program* p) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (p->pw) return MC_OK;
    if (p->host_only)
        return fail(MC_ERR_INVALID, "a host-only program has no device tables");
    int max_nodes = 0;
    bool lg = false;
    for (size_t t = 0; t < p->pw_terms.size(); ++t) {
        const DevTerm& T = p->pw_terms[t];
        if (T.dist < MC_DIST_NORMAL || T.dist > MC_DIST_EXPR)
            return fail(MC_ERR_UNSUPPORTED, "pointwise: term %zu has a distribution (%d) the "
                        "pointwise kernel does not evaluate", t, T.dist);
        if (T.dist == MC_DIST_EXPR) {
            if (T.expr_n < 1 || T.expr_n > kExMaxNodes ||
                (size_t)T.expr_base + T.expr_n > p->rnodes.size())
                return fail(MC_ERR_UNSUPPORTED, "pointwise: term %zu is an expression of %d "
                            "nodes (1 .. %d are evaluated)", t, T.expr_n, kExMaxNodes);
            max_nodes = std::max(max_nodes, T.expr_n);
        } else if (T.dist == MC_DIST_GAMMA || T.dist == MC_DIST_BETA) {
            // (eval_term's rule: constant shapes keep the precomputed clg)
            const int k1 = T.op[1].kind, k2 = T.op[2].kind;
            const bool vec1 = k1 == MC_OP_DATA || k1 == MC_OP_PVEC || k1 == MC_OP_GATHER;
            const bool vec2 = k2 == MC_OP_DATA || k2 == MC_OP_PVEC || k2 == MC_OP_GATHER;
            const bool per_elem = T.dist == MC_DIST_GAMMA ? vec1 : (vec1 || vec2);
            lg |= per_elem || k1 == MC_OP_PSCALAR || k2 == MC_OP_PSCALAR;
        }
    }
    // tiles never straddle a term: the term is uniform in a workgroup
    std::vector<PwTile> tiles;
    int64_t o = 0;
    for (size_t t = 0; t < p->pw_terms.size(); ++t) {
        const int64_t n = p->pw_terms[t].n;
        for (int64_t e = 0; e < n; e += kPwBlock) tiles.push_back(PwTile{e, o + e, (int32_t)t, 0});
        o += n;
    }
    if (tiles.empty()) return fail(MC_ERR_INVALID, "pointwise: the program has no terms");
    if (tiles.size() > (size_t)INT32_MAX)
        return fail(MC_ERR_UNSUPPORTED, "pointwise: %zu tiles exceed the grid", tiles.size());
    PwView* v = new PwView();
    p->pw = v;
    v->ntiles = (int32_t)tiles.size();
    v->M = o;
    v->max_nodes = max_nodes;
    v->lg = lg;
    hipError_t e = pw_upload(&v->d_terms, p->pw_terms.data(), p->pw_terms.size());
    if (e == hipSuccess) e = pw_upload(&v->d_nodes, p->rnodes.data(), p->rnodes.size());
    if (e == hipSuccess) e = pw_upload(&v->d_data, p->h_data.data(), (size_t)p->pw_n_data);
    if (e == hipSuccess) e = pw_upload(&v->d_index, p->h_index.data(), (size_t)p->pw_n_index);
    if (e == hipSuccess) e = pw_upload(&v->d_tiles, tiles.data(), tiles.size());
    if (e == hipSuccess)
        e = pw_upload(&v->d_samplers, p->pw_samplers.data(), p->pw_samplers.size());
    if (e != hipSuccess) {
        pw_free(p);
        return fail(e == hipErrorOutOfMemory ? MC_ERR_NOMEM : MC_ERR_HIP,
                    "pointwise view upload failed: %s", hipGetErrorString(e));
    }
    return MC_OK;
}

extern "C" int64_t mc_pointwise_workspace_bytes(const mc_program* p, int64_t C, int64_t S) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (C < 1 || S < 1) return fail(MC_ERR_INVALID, "pointwise: C and S must be >= 1");
    const PwView* v = (const PwView*)p->pw;
    if (!v) return fail(MC_ERR_INVALID, "pointwise: call mc_program_enable_pointwise first");
    int64_t B, per;
    pw_split(C * S, v->ntiles, &B, &per);
    return B > 1 ? B * PW_COUNT * v->M * (int64_t)sizeof(double) : 0;
}

extern "C" int mc_pointwise_stats(const mc_program* p, int64_t C, int64_t S, const float* samples,
                                  double* stats, float* matrix, void* ws, int64_t ws_bytes,
                                  void* hip_stream) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    const PwView* v = (const PwView*)p->pw;
    if (!v) return fail(MC_ERR_INVALID, "pointwise: call mc_program_enable_pointwise first");
    if (C < 1 || S < 1) return fail(MC_ERR_INVALID, "pointwise: C and S must be >= 1");
    if (C > INT64_MAX / S) return fail(MC_ERR_INVALID, "pointwise: C * S overflows");
    if (!samples || !stats) return fail(MC_ERR_INVALID, "pointwise: NULL samples / stats");
    const int64_t N = C * S;
    int64_t B, per;
    pw_split(N, v->ntiles, &B, &per);
    const int64_t need = B > 1 ? B * PW_COUNT * v->M * (int64_t)sizeof(double) : 0;
    if (need > 0 && (!ws || ws_bytes < need))
        return fail(MC_ERR_INVALID, "pointwise: the workspace needs %lld bytes",
                    (long long)need);
    hipStream_t st = (hipStream_t)hip_stream;
    const PwCtx X = pw_ctx_of(p, v);
    // one block of draws: its partial is the result
    double* part = B > 1 ? (double*)ws : stats;
    const dim3 grid((unsigned)v->ntiles, (unsigned)B);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(kPwBlock), 0, st, X, N, per, samples, part, matrix);
    };
    if (v->max_nodes > 16) launch(k_pointwise<32, true>);
    else if (v->max_nodes > 0) launch(k_pointwise<16, true>);
    else if (v->lg) launch(k_pointwise<0, true>);
    else launch(k_pointwise<0, false>);
    MC_HIP_TRY(hipGetLastError());
    if (B > 1) {
        hipLaunchKernelGGL(k_pw_merge, dim3((unsigned)((v->M + 255) / 256)), dim3(256), 0, st,
                           (const double*)part, v->M, (int32_t)B, stats);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}
