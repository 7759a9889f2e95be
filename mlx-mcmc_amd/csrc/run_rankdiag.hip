// run_rankdiag.hip — rank-normalised R-hat, bulk- and tail-ESS (csrc/rankdiag.h):
// mc_rank_diag_workspace_bytes, mc_rank_diag, mc_geyer_ess_host (the sequence
// rule on the host), mc_debug_rank_path.
#include "host.h"
#include "rankdiag.h"

namespace {

int g_rank_path = 0;  // mc_debug_rank_path

// What one batch may take of the workspace.  A constant: the batch size is a
// function of (C, S, D) alone.
constexpr int64_t kRdWsCap = 512ll << 20;
constexpr int64_t kRdMaxBatch = 32768;  // (elements are a grid's y dimension)

struct RdPlan {
    int64_t C, S, D, n, m, N, tiles, Db;
    bool lds;  // k_rd_sort_lds takes a column
};
int64_t rd_elem_bytes(int64_t N, int64_t tiles, int64_t m) {
    return N * (8 + 4 + 4 * 4) + tiles * mc::kRdDigits * 4 + 3 * m * 8 + 2 * 8 + 4 * 4 + 4 * 4;
}
int rd_plan(int64_t C, int64_t S, int64_t D, RdPlan* P) {
    if (C < 1 || S < 1 || D < 0) return fail(MC_ERR_INVALID, "rank_diag: C, S >= 1 and D >= 0");
    P->C = C;
    P->S = S;
    P->D = D;
    P->n = S / 2;
    if (C > ((int64_t)1 << 30)) return fail(MC_ERR_UNSUPPORTED, "rank_diag: too many chains");
    P->m = 2 * C;
    if (P->n > 0 && P->m > (int64_t)INT32_MAX / P->n)
        return fail(MC_ERR_UNSUPPORTED, "rank_diag: %lld split draws per element exceed 2^31 - 1",
                    (long long)P->m * (long long)P->n);
    P->N = P->m * P->n;
    P->tiles = (P->N + mc::kRdTile - 1) / mc::kRdTile;
    P->lds = g_rank_path != 1 && P->N <= mc::kRdLdsMaxN;
    const int64_t per =
        rd_elem_bytes(std::max<int64_t>(P->N, 1), std::max<int64_t>(P->tiles, 1), P->m);
    int64_t Db = std::max<int64_t>(1, kRdWsCap / per);
    Db = std::min(Db, kRdMaxBatch);
    if (g_rank_path == 2) Db = std::min<int64_t>(Db, 3);
    P->Db = std::max<int64_t>(1, std::min(Db, D));
    // the stage kernel's grid: split chains x tiles of n
    if (P->n >= 4 && P->m * ((P->n + mc::kRdStageP - 1) / mc::kRdStageP) > (int64_t)INT32_MAX)
        return fail(MC_ERR_UNSUPPORTED, "rank_diag: the stage grid exceeds 2^31 - 1 workgroups");
    return MC_OK;
}

// The workspace's arrays in order (f64 first; every size a multiple of 8 bytes).
int64_t rd_carve(const RdPlan& P, void* ws, mc::RdWs* W) {
    char* p = (char*)ws;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        char* r = p ? p + at : nullptr;
        at += (bytes + 7) / 8 * 8;
        return r;
    };
    const int64_t Db = P.Db, N = std::max<int64_t>(P.N, 1), T = std::max<int64_t>(P.tiles, 1);
    mc::RdWs w;
    w.z = (double*)take(Db * N * 8);
    w.tail = (double*)take(Db * 2 * 8);
    w.cmean = (double*)take(Db * 3 * P.m * 8);
    w.y = (float*)take(Db * N * 4);
    w.q = (float*)take(Db * 4 * 4);
    for (int k = 0; k < 2; ++k) w.key[k] = (uint32_t*)take(Db * N * 4);
    for (int k = 0; k < 2; ++k) w.pos[k] = (uint32_t*)take(Db * N * 4);
    w.hist = (uint32_t*)take(Db * mc::kRdDigits * T * 4);
    w.flag = (uint32_t*)take(Db * 4 * 4);
    if (W) *W = w;
    return at;
}

// numpy's 'linear' percentile of N values in f32 (diagnostics._percentile_ranks)
void rd_pct(int64_t N, float q, int64_t* lo, float* g) {
    const float q32 = q / 100.0f;
    const float vi = (float)(N - 1) * q32;
    if (vi >= (float)(N - 1)) {
        lo[0] = lo[1] = N - 1;
        *g = 0.0f;
        return;
    }
    const float prev = std::floor(vi);
    lo[0] = (int64_t)prev;
    lo[1] = std::min<int64_t>(lo[0] + 1, N - 1);
    *g = vi - prev;
}

// k_rd_acov over `nq` quantities from q0 of every element of the batch
int rd_acov(const RdPlan& P, int64_t nb, int q0, int nq, const mc::RdWs& W, double* o,
            hipStream_t st) {
    const size_t lds = mc::rd_acov_lds_bytes(P.n);
    auto go = [&](auto kernel) {
        MC_HIP_TRY(allow_lds(kernel, lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)nq, (unsigned)nb), dim3(64 * mc::kRdAcovWaves),
                           lds, st, P.m, P.n, q0, W, P.D, o, MC_RD_RHAT_BULK, MC_RD_RHAT_FOLDED,
                           MC_RD_ESS_BULK);
        MC_HIP_TRY(hipGetLastError());
        return (int)MC_OK;
    };
    return P.n <= mc::kRdAcovStageN ? go(mc::k_rd_acov<true>) : go(mc::k_rd_acov<false>);
}

// (key, position) pairs of every element of the batch, sorted: key[0] in,
// key[0] / pos[0] out
int rd_sort(const RdPlan& P, int64_t nb, const mc::RdWs& W, hipStream_t st) {
    if (P.lds) {
        const size_t lds = mc::rd_sort_lds_bytes(P.N);
        MC_HIP_TRY(allow_lds(mc::k_rd_sort_lds, lds));
        hipLaunchKernelGGL(mc::k_rd_sort_lds, dim3((unsigned)nb), dim3(mc::kRdThreads), lds, st,
                           P.N, W);
        MC_HIP_TRY(hipGetLastError());
        return MC_OK;
    }
    const dim3 grid((unsigned)P.tiles, (unsigned)nb);
    for (int pass = 0; pass < 8; ++pass) {
        const int a = pass & 1, b = a ^ 1;  // 8 passes: the result is in buffer 0
        hipLaunchKernelGGL(mc::k_rd_ghist, grid, dim3(mc::kRdThreads), 0, st, P.N, P.tiles,
                           4 * pass, (const uint32_t*)W.key[a], W.hist);
        MC_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(mc::k_rd_gscan, dim3((unsigned)nb), dim3(mc::kRdThreads), 0, st,
                           P.tiles, W.hist);
        MC_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(mc::k_rd_gscatter, grid, dim3(mc::kRdThreads), 0, st, P.N, P.tiles,
                           4 * pass, pass == 0 ? 1 : 0, (const uint32_t*)W.key[a],
                           (const uint32_t*)W.pos[a], (const uint32_t*)W.hist, W.key[b], W.pos[b]);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}

int rd_fill(double* p, int64_t count, double v, hipStream_t st) {
    for (int64_t at = 0; at < count; at += (int64_t)1 << 38) {  // (a grid's x dimension)
        const int64_t len = std::min(count - at, (int64_t)1 << 38);
        hipLaunchKernelGGL(mc::k_rd_fill, dim3((unsigned)((len + mc::kRdThreads - 1) / mc::kRdThreads)),
                           dim3(mc::kRdThreads), 0, st, p + at, len, v);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}

}  // namespace

extern "C" int mc_debug_rank_path(int path) {
    const int was = g_rank_path;
    if (path >= 0 && path <= 2) g_rank_path = path;
    return was;
}

extern "C" int mc_geyer_ess_host(const double* rho, int64_t n, int64_t N, double* ess) {
    if (!rho || !ess) return fail(MC_ERR_INVALID, "geyer_ess: NULL rho / ess");
    if (n < 4 || N < n) return fail(MC_ERR_INVALID, "geyer_ess: n >= 4 and N >= n");
    mc::RdGeyer G;
    mc::rd_geyer_init(G, rho[0]);
    while (mc::rd_geyer_wants(G, n)) {
        const int64_t t = G.t;  // rho_{t+1}, rho_{t+2}
        mc::rd_geyer_push(G, rho[t], rho[t + 1]);
    }
    *ess = mc::rd_geyer_ess(G, N);
    return MC_OK;
}

extern "C" int64_t mc_rank_diag_workspace_bytes(int64_t C, int64_t S, int64_t D) {
    RdPlan P;
    const int rc = rd_plan(C, S, D, &P);
    return rc != MC_OK ? rc : rd_carve(P, nullptr, nullptr);
}

extern "C" int mc_rank_diag(int64_t C, int64_t S, int64_t D, const float* samples, double* out,
                            double* z, void* ws, int64_t ws_bytes, void* hip_stream) {
    RdPlan P;
    const int rc0 = rd_plan(C, S, D, &P);
    if (rc0 != MC_OK) return rc0;
    if (D == 0) return MC_OK;
    if (!samples || !out) return fail(MC_ERR_INVALID, "rank_diag: NULL samples / out");
    hipStream_t st = (hipStream_t)hip_stream;
    const double nan = std::nan("");
    if (P.n < 4) {  // nothing is defined
        int rc = rd_fill(out, (int64_t)MC_RD_CONSTANT * D, nan, st);
        if (rc == MC_OK) rc = rd_fill(out + (int64_t)MC_RD_CONSTANT * D, D, 0.0, st);
        if (rc == MC_OK && z && P.N > 0) rc = rd_fill(z, D * P.N, nan, st);
        return rc;
    }
    const int64_t need = rd_carve(P, nullptr, nullptr);
    if (!ws || ws_bytes < need)
        return fail(MC_ERR_INVALID, "rank_diag: the workspace needs %lld bytes", (long long)need);
    if (((uintptr_t)ws & 7) != 0)
        return fail(MC_ERR_INVALID, "rank_diag: the workspace is unaligned");
    mc::RdWs W;
    rd_carve(P, ws, &W);
    mc::RdQuant Q;
    rd_pct(P.N, 5.0f, Q.lo, &Q.g[0]);
    rd_pct(P.N, 95.0f, Q.hi, &Q.g[1]);
    const int64_t ptiles = (P.n + mc::kRdStageP - 1) / mc::kRdStageP;
    const dim3 blk(mc::kRdThreads);
    for (int64_t d0 = 0; d0 < D; d0 += P.Db) {
        const int64_t nb = std::min(P.Db, D - d0);
        double* o = out + d0;
        const dim3 cols((unsigned)((P.N + mc::kRdThreads - 1) / mc::kRdThreads), (unsigned)nb);
        MC_HIP_TRY(hipMemsetAsync(W.flag, 0, (size_t)nb * 4 * 4, st));
        hipLaunchKernelGGL(mc::k_rd_stage,
                           dim3((unsigned)(P.m * ptiles),
                                (unsigned)((nb + mc::kRdStageE - 1) / mc::kRdStageE)),
                           blk, 0, st, samples, S, D, d0, nb, P.n, P.N, W);
        MC_HIP_TRY(hipGetLastError());
        int rc = rd_sort(P, nb, W, st);
        if (rc != MC_OK) return rc;
        hipLaunchKernelGGL(mc::k_rd_rank, cols, blk, 0, st, P.N, 0, Q, W,
                           z ? z + d0 * P.N : nullptr);
        MC_HIP_TRY(hipGetLastError());
        rc = rd_acov(P, nb, mc::RD_Q_BULK, 3, W, o, st);
        if (rc != MC_OK) return rc;
        // the folded values: a second ranking in the same workspace
        hipLaunchKernelGGL(mc::k_rd_fold, cols, blk, 0, st, P.N, W);
        MC_HIP_TRY(hipGetLastError());
        rc = rd_sort(P, nb, W, st);
        if (rc != MC_OK) return rc;
        hipLaunchKernelGGL(mc::k_rd_rank, cols, blk, 0, st, P.N, 1, Q, W, (double*)nullptr);
        MC_HIP_TRY(hipGetLastError());
        rc = rd_acov(P, nb, mc::RD_Q_FOLD, 1, W, o, st);
        if (rc != MC_OK) return rc;
        hipLaunchKernelGGL(mc::k_rd_final, dim3((unsigned)((nb + mc::kRdThreads - 1) / mc::kRdThreads)),
                           blk, 0, st, nb, D, W, o, MC_RD_RHAT_BULK, MC_RD_RHAT_FOLDED,
                           MC_RD_RHAT_RANK, MC_RD_ESS_BULK, MC_RD_ESS_TAIL, MC_RD_CONSTANT);
        MC_HIP_TRY(hipGetLastError());
    }
    return MC_OK;
}
