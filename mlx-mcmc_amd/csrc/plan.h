// plan.h — the slice and lane planners in stages (plan_slices.hip,
// plan_lanes.hip), for the slicing policy (program.hip):
//   partition_program  validated terms -> SlPartition: the broadcast parameters,
//                      each private parameter's and element's slice, the
//                      bundles, the scalar terms
//   tile_slices        SlPartition -> SlicePlan: the term interpreter's run,
//                      lane and combine tables (sliced.h)
//   plan_lanes         SlPartition -> LanePlan: parameters to (lane, slot),
//                      elements tiled per (slot, lane) (lanes.h)
#pragma once
#include "host.h"

// The parameter / element partition of a program over S slices.
struct SlPartition {
    int S = 1, Pmax = 0, Dsh = 0, nitems = 0;  // Pmax: most private parameters in a slice
    std::vector<int> shxf;                // per shared ordinal: mc_transform_kind
    std::vector<int> sterm_raw;           // per scalar term: LrSterm::raw bits
    std::vector<SlTerm> sterms;           // the scalar terms (niter: element count)
    std::vector<int> ppr;                 // per term: slot of its per-element parameter, or -1
    std::vector<char> shared, scalar;     // per parameter / per term
    std::vector<int> jsh;                 // per parameter: shared ordinal, or -1
    std::vector<int> owner, lidx;         // per private parameter: its slice, its slot there
    std::vector<std::vector<int>> priv;   // per slice: its private parameters
    std::vector<int> shl;                 // shared parameters by ordinal
    std::vector<std::vector<std::vector<int64_t>>> elems;  // [slice][term] element ids
    // grouped expression terms (host.h expr_term_class): per term its distinct
    // parameter vectors' offsets and its element -> group map (empty: not
    // grouped); per parameter the lowest member of its bundle (itself: alone)
    // and its position in the bundle
    std::vector<std::vector<int32_t>> gvec, gmap;
    std::vector<int> bfirst, bpos;
    bool grouped = false;
};

int partition_program(const mc_program* p, int S, SlPartition& part);
int tile_slices(const mc_program* p, const SlPartition& part, SlicePlan& P);
int plan_slices(const mc_program* p, int S, SlicePlan& P, SlPartition& part);
// MC_ERR_UNSUPPORTED (with L.why) when the program does not take the lane layout
int plan_lanes(const mc_program* p, const SlPartition& part, LanePlan& L);
void free_slices(SlicePlan& P);
void free_lanes(LanePlan& L);

inline int64_t pp_index(const DevTerm& t, int a, int64_t i, const std::vector<int32_t>& ip) {
    const DevOperand& o = t.op[a];
    return o.kind == MC_OP_PVEC ? (int64_t)o.poff + i : (int64_t)o.poff + ip[o.pool + i];
}
// The parameter whose owner takes element i of grouped expression term t.
inline int gx_param(const SlPartition& part, int t, int64_t i) {
    return part.bfirst[part.gvec[t][0] + part.gmap[t][(size_t)i]];
}
// Only constants and broadcast parameters: evaluated once per chain after
// every exchange, not split into slices (an expression term is sliced by element).
inline bool is_scalar_term(const DevTerm& t) {
    for (int a = 0; a < 3; ++a) {
        const int k = t.op[a].kind;
        if (k != MC_OP_CONST && k != MC_OP_PSCALAR && k != MC_OP_NONE) return false;
    }
    return t.dist != MC_DIST_EXPR;
}
// The fields a planned term has on both layouts (SlTerm, LrTerm), the rest zero.
template <typename Term>
inline void fill_term(Term& st, const DevTerm& rt, int pp, const std::vector<int>& jsh) {
    std::memset(&st, 0, sizeof(st));
    st.dist = rt.dist;
    st.pp = pp;
    st.weight = rt.weight;
    st.c0 = rt.c0;
    st.clg = rt.clg;
    if (rt.op[2].kind == MC_OP_CONST) {
        const float c = rt.op[2].cval;
        st.clogs = (float)std::log((double)c);
        st.cinv = 1.0f / c;
        st.cinv2 = 1.0f / (c * c);
    }
    for (int a = 0; a < 3; ++a) {  // operand kinds (SK_*)
        const DevOperand& o = rt.op[a];
        switch (o.kind) {
            case MC_OP_CONST: st.kind[a] = SK_CONST; st.cval[a] = o.cval; break;
            case MC_OP_PSCALAR: st.kind[a] = SK_SHARED; st.jsh[a] = jsh[o.poff]; break;
            case MC_OP_DATA: st.kind[a] = SK_DATA; break;
            case MC_OP_PVEC:
            case MC_OP_GATHER: st.kind[a] = SK_PP; break;
            default: st.kind[a] = SK_NONE; break;
        }
    }
    // moment sums for Normal / HalfNormal with a broadcast scale, else the
    // per-element formula
    st.mode = (st.kind[2] == SK_DATA || st.kind[2] == SK_PP ||
               (rt.dist != MC_DIST_NORMAL && rt.dist != MC_DIST_HALFNORMAL)) ? 1 : 0;
}

// ---- device copies of the host tables ----------------------------------------
template <typename T>
inline hipError_t upload(T** dst, const std::vector<T>& v) {
    hipError_t e = hipMalloc(dst, v.size() * sizeof(T));
    if (e == hipSuccess) e = hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}
inline hipError_t upload_slices(SlicePlan& Q) {
    hipError_t e = upload(&Q.d_terms, Q.terms);
    if (e == hipSuccess && !Q.sterms.empty()) e = upload(&Q.d_sterms, Q.sterms);
    if (e == hipSuccess) e = upload(&Q.d_data, Q.data);
    if (e == hipSuccess) e = upload(&Q.d_index, Q.index);
    if (e == hipSuccess) e = upload(&Q.d_blocks, Q.blocks);
    if (e == hipSuccess) e = upload(&Q.d_gidx, Q.gidx);
    return e;
}
inline hipError_t upload_lanes(LanePlan& LP) {
    hipError_t e = upload(&LP.d_terms, LP.terms);
    if (e == hipSuccess) e = upload(&LP.d_data, LP.data);
    if (e == hipSuccess) e = upload(&LP.d_blocks, LP.blocks);
    if (e == hipSuccess) e = upload(&LP.d_gidx, LP.gidx);
    if (e == hipSuccess && !LP.sterms.empty()) e = upload(&LP.d_sterms, LP.sterms);
    if (e == hipSuccess && !LP.rng.empty()) e = upload(&LP.d_rng, LP.rng);
    if (e == hipSuccess && !LP.mom.empty()) e = upload(&LP.d_mom, LP.mom);
    return e;
}
inline int upload_failed(hipError_t e, const char* what) {
    return fail(e == hipErrorOutOfMemory ? MC_ERR_NOMEM : MC_ERR_HIP, "%s upload failed: %s", what,
                hipGetErrorString(e));
}
