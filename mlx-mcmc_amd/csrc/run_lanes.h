// run_lanes.h — the lane-resident HMC launch (k_hmc_lf / k_hmc_lr), included by
// run_lanes_rs{1,2,4}.hip: one translation unit per register-slot count, so
// the instantiations compile in parallel.
#pragma once
#include "launch.h"
#include "lanes_fast_nc.h"

// The launches of kernel pair k (NW waves per workgroup; X1: one slice)
template <int NW, bool X1, typename K>
inline int hmc_lr_exchange(const char* name, K& k, const mc_program* p, const mc_run_config* cfg,
                           void* state, float* samples, const mc_trace* tr, void* ws,
                           hipStream_t st, bool fast = false) {
    RunState R = run_state(p, cfg, state);
    const LrCtx ctx = lrctx_of(p);
    const TraceDev td = trace_of(tr);
    constexpr int NB = 2 * NW;
    ExchangeLaunch d;
    d.name = name;
    d.threads = 64 * NW;
    d.chains = NB;
    d.S = p->lr.S;
    // (k_hmc_lf keeps only the scalar terms in LDS: its steps read no observation)
    d.lds = fast ? p->lr.sterms.size() * sizeof(LrSterm) : lr_base_lds_bytes(p);
    d.blocks_per_launch = lr_groups_per_launch(p, cfg->num_chains);  // (X1: all of them)
    d.clear_bytes = sl_workspace_bytes(p, cfg->num_chains);
    d.tags_per_launch = (uint64_t)cfg->iter_count * cfg->num_leapfrog_steps + 1;
    d.restart_tags = false;
    d.coresident = !X1;
    int* status = (int*)ws;
    unsigned long long* xch = (unsigned long long*)((char*)ws + kSlStatusBytes);
    return run_exchange(d, k, cfg->num_chains, ws, st, R.A,
                        [&](int64_t g0, int64_t ng, int64_t grid, bool xl, uint32_t base) {
        return k.launch(xl, grid, d.threads, d.lds, st, ctx, R.A, g0 * NB, ng, R.scalars, R.q, R.g,
                        samples, td, xch, status, base);
    });
}

template <int RS, int NSH, int NW, bool X1>
inline int launch_hmc_lr(const mc_program* p, const mc_run_config* cfg, void* state,
                         float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    if (p->lr.has_expr) {  // LS_EXPR terms: only the JIT-compiled k_hmc_lr runs the plan
        ModulePair k{p, "mc::k_hmc_lr<" + std::to_string(RS) + ", " + std::to_string(NSH) + ", " +
                            std::to_string(NW) + ", " + (X1 ? "true" : "false")};
        const int rc = k.load();
        if (rc != MC_OK) return rc;
        if (k.f == nullptr) return kLanesNoJit;
        return hmc_lr_exchange<NW, X1>("lane-resident HMC (expression JIT)", k, p, cfg, state,
                                       samples, tr, ws, st);
    }
    const bool fast = p->lr.fast && lanes_fast_enabled();
    auto kern = fast ? k_hmc_lf<RS, NSH, NW, X1, -1> : k_hmc_lr<RS, NSH, NW, X1>;
    // the same with L2-resident records (host.h xcd_round_robin): the generic
    // kernel and the compile-time forms (the run-time form keeps sc1 records)
    auto kern_xl = (fast || X1) ? kern : k_hmc_lr<RS, NSH, NW, X1, true>;
    const bool forms = lanes_forms_enabled();
    if constexpr (NSH == 3) {  // the compile-time forms (one instantiation each)
        constexpr int HIER = LF_SW | LF_SWS | LF_DIR | LF_DM | LF_DS;
        if (fast && forms && p->lr.form == HIER) {
            kern = k_hmc_lf<RS, lf_nroles(HIER), NW, X1, HIER>;
            kern_xl = X1 ? kern : k_hmc_lf<RS, lf_nroles(HIER), NW, X1, HIER, true>;
            // the launch constants of the common layout, compiled in: one
            // lane per private parameter, no transformed shared parameter
            // at one register slot per lane (the bench shapes; every other
            // combination reads them at run time, above: few instantiations)
            if constexpr (RS == 1) {
                constexpr int PLAIN = LFS_REP1 | LFS_NOXF;
                if (p->lr.rep == 1 && p->lr.has_xf == 0) {
                    kern = k_hmc_lf<RS, lf_nroles(HIER), NW, X1, HIER, false, PLAIN>;
                    kern_xl =
                        X1 ? kern : k_hmc_lf<RS, lf_nroles(HIER), NW, X1, HIER, true, PLAIN>;
                }
            }
        }
        if (fast && forms && p->lr.form == LF_DIR) {
            kern = k_hmc_lf<RS, lf_nroles(LF_DIR), NW, X1, LF_DIR>;
            kern_xl = X1 ? kern : k_hmc_lf<RS, lf_nroles(LF_DIR), NW, X1, LF_DIR, true>;
        }
    }
    auto k = static_pair(kern, kern_xl);
    return hmc_lr_exchange<NW, X1>("lane-resident HMC", k, p, cfg, state, samples, tr, ws, st,
                                   fast);
}

// The dense launch (mc_program::lrd; lanes_fast.h DN): one workgroup per chain
// pair — or per chain (lanes_fast_nc.h k_hmc_lfc, NC = 1) while the launch has no more
// chains than the device has CUs — no exchange workspace, tags, co-residency
// check or status word: the grid is the pairs (chains), however many the
// device holds at once.  One slice: the X1 kernel (a wave per workgroup, always
// a pair); DS slices: DS waves exchanging through LDS, which by the plan's
// choice of DS have 2 register slots.
template <int RS>
inline int launch_hmc_dense(const mc_program* p, const mc_run_config* cfg, void* state,
                            float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    constexpr int HIER = LF_SW | LF_SWS | LF_DIR | LF_DM | LF_DS;
    constexpr int PLAIN = LFS_REP1 | LFS_NOXF;
    constexpr int NSH = lf_nroles(HIER);
    const LanePlan& L = p->lrd;
    RunState R = run_state(p, cfg, state);
    const LrCtx ctx = lrctx_of(p, L);
    const TraceDev td = trace_of(tr);
    ws_forget(ws);  // (no status word: mc_workspace_status has nothing to read)
    // chains per workgroup: the one-wave kernel always runs a pair; the 4- and
    // 8-wave kernels one chain while each then has a CU (host.h hmc_dense_chains)
    const int nc = L.S == 1 ? 2 : hmc_dense_chains(cfg->num_chains, device_cus(), L.dense_chains);
    const int64_t groups = (cfg->num_chains + nc - 1) / nc;
    const size_t sterm_bytes = L.sterms.size() * sizeof(LrSterm);
    // block-wide draws (LrCtx::blk_rng): per iteration parity every chain's
    // normals, 4 per Philox block, and the accept logs (padded to a float4)
    const size_t draw_bytes =
        L.blk_rng ? (size_t)2 * (4 * nc * ((p->D + 3) / 4) + 4) * 4 : 0;
    auto go = [&](auto kern, int waves) {
        // (the record lines, per parity: lanes_fast_nc.h lfc_line_floats)
        const size_t lds = sterm_bytes + draw_bytes +
                           (waves > 1 ? (size_t)2 * lfc_line_floats(nc, waves) * 4 : 0);
        hipLaunchKernelGGL(kern, dim3((unsigned)groups), dim3(64 * waves), lds, st, ctx, R.A,
                           (int64_t)0, groups, R.scalars, R.q, R.g, samples, td,
                           (unsigned long long*)nullptr, (int*)nullptr, (uint32_t)0);
        MC_HIP_TRY(hipGetLastError());
        return MC_OK;
    };
    if (L.S == 1) return go(k_hmc_lf<RS, NSH, 1, true, HIER, false, PLAIN>, 1);
    if constexpr (RS == 2) {
        if (L.S == 4)
            return nc == 1 ? go(k_hmc_lfc<2, NSH, 4, false, HIER, false, PLAIN, 4, 1>, 4)
                           : go(k_hmc_lf<2, NSH, 4, false, HIER, false, PLAIN, 4>, 4);
        if (L.S == 8)
            return nc == 1 ? go(k_hmc_lfc<2, NSH, 8, false, HIER, false, PLAIN, 8, 1>, 8)
                           : go(k_hmc_lf<2, NSH, 8, false, HIER, false, PLAIN, 8>, 8);
    }
    return fail(MC_ERR_UNSUPPORTED, "dense HMC: no kernel for %d slices at %d slots", L.S, RS);
}

// NSH (3 or 4 shared parameters) x waves per workgroup (one slice: 1 wave and
// no exchange; <= 8 slices: 4; else 8)
template <int RS>
inline int hmc_lanes_dispatch(const mc_program* p, const mc_run_config* cfg, void* state,
                              float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    const bool w4 = lr_nw(p) == 4, x1 = p->lr.S == 1;
    return dispatch_nsh(p, [&](auto N) {
        constexpr int NSH = decltype(N)::value;
        return x1 ? launch_hmc_lr<RS, NSH, 1, true>(p, cfg, state, samples, tr, ws, st)
             : w4 ? launch_hmc_lr<RS, NSH, 4, false>(p, cfg, state, samples, tr, ws, st)
                  : launch_hmc_lr<RS, NSH, 8, false>(p, cfg, state, samples, tr, ws, st);
    });
}
