// run_psis.hip — PSIS-LOO on the pointwise view of a program (csrc/psis.h):
// mc_psis_tail_len, mc_psis_fit_host (the scalar definition of the fit, host
// only), mc_psis_workspace_bytes, mc_psis_loo.
#include "host.h"
#include "psis.h"
#include "pw_view.h"

namespace {

// The view and the geometry of a launch, validated.
struct PsisPlan {
    const PwView* v;
    int64_t N, Mt, P, B, per;
};
int psis_plan(const mc_program* p, int64_t C, int64_t S, double r_eff, PsisPlan* out) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    const PwView* v = (const PwView*)p->pw;
    if (!v) return fail(MC_ERR_INVALID, "psis: call mc_program_enable_pointwise first");
    if (C < 1 || S < 1) return fail(MC_ERR_INVALID, "psis: C and S must be >= 1");
    if (C > (int64_t)UINT32_MAX / S)
        return fail(MC_ERR_UNSUPPORTED, "psis: C * S exceeds the 32-bit draw counters");
    if (!(r_eff > 0.0) || r_eff - r_eff != 0.0)
        return fail(MC_ERR_INVALID, "psis: r_eff must be positive and finite");
    if (v->M > (int64_t)INT32_MAX)
        return fail(MC_ERR_UNSUPPORTED, "psis: %lld observations exceed the fit kernel's grid",
                    (long long)v->M);
    out->v = v;
    out->N = C * S;
    out->Mt = psis_tail_len(out->N, r_eff);
    if (out->Mt > kPsisMaxTail)
        return fail(MC_ERR_UNSUPPORTED, "psis: a tail of %lld draws exceeds kPsisMaxTail = %d "
                    "(the fit kernel's LDS)", (long long)out->Mt, kPsisMaxTail);
    out->P = 1;
    while (out->P < out->Mt) out->P <<= 1;
    pw_split(out->N, v->ntiles, &out->B, &out->per);
    return MC_OK;
}

// The workspace's arrays in order (f64 first; every size a multiple of 4 bytes).
int64_t psis_carve(const PsisPlan& L, void* ws, mc::PsisWs* W) {
    const int64_t M = L.v->M, B = L.B;
    char* p = (char*)ws;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        char* r = p ? p + at : nullptr;
        at += bytes;
        return r;
    };
    mc::PsisWs w;
    w.rest = (double*)take(B * M * 8);
    w.cnt = (uint32_t*)take(B * mc::kPsisSlots * M * 4);
    w.off = (uint32_t*)take(B * M * 4);
    w.nf = (uint32_t*)take(B * M * 4);
    w.lo = (uint32_t*)take(M * 4);
    w.kmin = (uint32_t*)take(M * 4);
    w.ntail = (uint32_t*)take(M * 4);
    w.tail = (float*)take(M * std::max<int64_t>(L.Mt, 1) * 4);
    if (W) *W = w;
    return at;
}

}  // namespace

extern "C" int64_t mc_psis_tail_len(int64_t N, double r_eff) {
    if (N < 1) return fail(MC_ERR_INVALID, "psis: N must be >= 1");
    if (!(r_eff > 0.0) || r_eff - r_eff != 0.0)
        return fail(MC_ERR_INVALID, "psis: r_eff must be positive and finite");
    return psis_tail_len(N, r_eff);
}

extern "C" int mc_psis_fit_host(const float* tail_desc, int64_t n, float cutoff, float lmin,
                                double* khat, double* sigma, double* lw_out) {
    if (n < 0 || n > INT32_MAX) return fail(MC_ERR_INVALID, "psis: bad tail length");
    if (!khat || !sigma || (n > 0 && !tail_desc))
        return fail(MC_ERR_INVALID, "psis: NULL tail / khat / sigma");
    const double lm = (double)lmin, ec = exp(lm - (double)cutoff);
    std::vector<double> y((size_t)n);
    for (int64_t j = 0; j < n; ++j) y[(size_t)j] = exp(lm - (double)tail_desc[j]) - ec;
    std::vector<double> work(2 * (size_t)(31 + (int64_t)sqrt((double)n)));
    psis_fit(PsisSerial(), y.data(), (int)n, work.data(), khat, sigma);
    if (lw_out) {
        const bool smooth = psis_smooths(*khat, *sigma);
        for (int64_t j = 0; j < n; ++j)
            lw_out[j] = smooth ? psis_lw((int)j + 1, (int)n, *khat, *sigma, ec)
                               : lm - (double)tail_desc[j];
    }
    return MC_OK;
}

extern "C" int64_t mc_psis_workspace_bytes(const mc_program* p, int64_t C, int64_t S,
                                           double r_eff) {
    PsisPlan L;
    const int rc = psis_plan(p, C, S, r_eff, &L);
    return rc != MC_OK ? rc : psis_carve(L, nullptr, nullptr);
}

extern "C" int mc_psis_loo(const mc_program* p, int64_t C, int64_t S, double r_eff,
                           const float* samples, double* out, float* tail, void* ws,
                           int64_t ws_bytes, void* hip_stream) {
    PsisPlan L;
    const int rc = psis_plan(p, C, S, r_eff, &L);
    if (rc != MC_OK) return rc;
    if (!samples || !out) return fail(MC_ERR_INVALID, "psis: NULL samples / out");
    const int64_t need = psis_carve(L, nullptr, nullptr);
    if (!ws || ws_bytes < need)
        return fail(MC_ERR_INVALID, "psis: the workspace needs %lld bytes", (long long)need);
    if (((uintptr_t)ws & 7) != 0) return fail(MC_ERR_INVALID, "psis: the workspace is unaligned");
    mc::PsisWs W;
    psis_carve(L, ws, &W);
    hipStream_t st = (hipStream_t)hip_stream;
    const PwView* v = L.v;
    const PwCtx X = pw_ctx_of(p, v);
    const dim3 grid((unsigned)v->ntiles, (unsigned)L.B);
    const dim3 ogrid((unsigned)((v->M + 255) / 256));
    // the eight passes of the select, most significant digit first
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 28 - 4 * pass, first = pass == 0, last = pass == 7;
        auto count = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(mc::kPwBlock), 0, st, X, L.N, L.per, samples,
                               shift, first, (const uint32_t*)W.lo, W.cnt);
        };
        if (v->max_nodes > 16) count(mc::k_psis_count<32, true>);
        else if (v->max_nodes > 0) count(mc::k_psis_count<16, true>);
        else if (v->lg) count(mc::k_psis_count<0, true>);
        else count(mc::k_psis_count<0, false>);
        MC_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(mc::k_psis_pick, ogrid, dim3(256), 0, st, v->M, (int32_t)L.B,
                           (uint32_t)L.Mt, shift, first, last, W);
        MC_HIP_TRY(hipGetLastError());
    }
    auto gather = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(mc::kPwBlock), 0, st, X, L.N, L.per, samples,
                           (uint32_t)L.Mt, W);
    };
    if (v->max_nodes > 16) gather(mc::k_psis_gather<32, true>);
    else if (v->max_nodes > 0) gather(mc::k_psis_gather<16, true>);
    else if (v->lg) gather(mc::k_psis_gather<0, true>);
    else gather(mc::k_psis_gather<0, false>);
    MC_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mc::k_psis_fit, dim3((unsigned)v->M), dim3(64),
                       mc::psis_fit_lds(L.Mt, L.P), st, v->M, L.N, (int32_t)L.B, (int32_t)L.Mt,
                       (int32_t)L.P, W, out, tail);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}
