// pw_view.h — the host side of the pointwise view of a program, shared by the
// units that launch on it (run_pointwise.hip builds it; run_predictive.hip
// reuses it as built).  Include after host.h and pointwise.h.
#pragma once

// Device tables of the pointwise view (mc_program::pw).
struct PwView {
    DevTerm* d_terms = nullptr;
    DevExprNode* d_nodes = nullptr;
    float* d_data = nullptr;
    int32_t* d_index = nullptr;
    PwTile* d_tiles = nullptr;
    PwSampler* d_samplers = nullptr;  // one per term (internal.h; predictive.h reads them)
    int32_t ntiles = 0;
    int64_t M = 0;
    int32_t max_nodes = 0;  // largest expression term (0: fused terms only)
    bool lg = false;        // a Gamma / Beta term whose normaliser follows the draw
};

inline PwCtx pw_ctx_of(const mc_program* p, const PwView* v) {
    PwCtx X;
    X.terms = v->d_terms;
    X.nodes = v->d_nodes;
    X.data = v->d_data;
    X.index = v->d_index;
    X.tiles = v->d_tiles;
    X.M = v->M;
    X.D = p->D;
    X.ntiles = v->ntiles;
    return X;
}

// Draw blocks B and draws per block for N = C * S draws over `ntiles` tiles:
// enough workgroups to fill the device whatever it is (a constant target, not
// a query), at least 32 draws per block so that a partial's 48 bytes per
// observation stay small beside the block's work.  A function of (N, ntiles)
// only; every block holds at least one draw.
inline constexpr int64_t kPwTargetGroups = 4096;
inline constexpr int64_t kPwMinDraws = 32;
inline constexpr int64_t kPwMaxB = 1024;
inline void pw_split(int64_t N, int64_t ntiles, int64_t* B, int64_t* per) {
    int64_t b = (kPwTargetGroups + ntiles - 1) / std::max<int64_t>(1, ntiles);
    b = std::min(b, std::max<int64_t>(1, N / kPwMinDraws));
    b = std::max<int64_t>(1, std::min(b, kPwMaxB));
    *per = (N + b - 1) / b;
    *B = (N + *per - 1) / *per;
}
