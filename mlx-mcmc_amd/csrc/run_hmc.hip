// run_hmc.hip — HMC launches (k_hmc_lf, k_hmc_lr, k_hmc_sl, k_hmc) and mc_hmc_run.
#include "launch.h"

extern "C" int mc_workspace_release(const void* ws) {
    if (ws) ws_forget(ws);
    return MC_OK;
}

extern "C" int mc_debug_exchange_fault(int on) {
    g_exchange_fault = on ? 1 : 0;
    return MC_OK;
}

// Exchange groups (blocks, counted by slice 0) launched on the workspace
// since it was last cleared that were found on one XCD (L2-resident
// publishes) / not (sliced.h xcd_agree): the status area's words 8 and 9.
extern "C" int mc_debug_workspace_xcd(const void* ws, int32_t* local, int32_t* remote) {
    if (!ws) return fail(MC_ERR_INVALID, "workspace is NULL");
    int32_t w[2] = {0, 0};
    MC_HIP_TRY(hipMemcpy(w, (const int32_t*)ws + 8, sizeof(w), hipMemcpyDeviceToHost));
    if (local) *local = w[0];
    if (remote) *remote = w[1];
    return MC_OK;
}

// host.h: the device deals workgroups round-robin over its XCDs (probe)
static __global__ void k_xcc_probe(uint32_t* out) {
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    if (threadIdx.x == 0) out[blockIdx.x] = x;
}
bool xcd_round_robin(int64_t grid, int S) {
    if (g_xcd_local < 0) g_xcd_local = env_on("MC_XCD_LOCAL");
    if (g_xcd_local == 0 || S < 2 || grid % 8 != 0 || (grid / 8) % S != 0) return false;
    static std::mutex mu;
    static std::map<std::pair<int, int64_t>, bool> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const auto key = std::make_pair(dev, grid);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    bool ok = false;
    uint32_t* d = nullptr;
    if (hipMalloc(&d, grid * sizeof(uint32_t)) == hipSuccess) {
        std::vector<uint32_t> h((size_t)grid, 0xFFFFFFFFu);
        hipLaunchKernelGGL(k_xcc_probe, dim3((unsigned)grid), dim3(64), 0, 0, d);
        if (hipGetLastError() == hipSuccess &&
            hipMemcpy(h.data(), d, grid * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess) {
            ok = true;
            for (int64_t b = 8; b < grid && ok; ++b) ok = h[b] == h[b % 8];
        }
        (void)hipFree(d);
    }
    (void)hipGetLastError();
    cache[key] = ok;
    return ok;
}

extern "C" int mc_debug_xcd_local(int on) {
    g_xcd_local = on < 0 ? -1 : (on ? 1 : 0);
    return MC_OK;
}

extern "C" int mc_debug_lanes_fast(int on) {
    g_lanes_fast = on ? 1 : 0;
    return MC_OK;
}

extern "C" int mc_debug_lanes_forms(int on) {
    g_lanes_forms = on ? 1 : 0;
    return MC_OK;
}

template <int NB>
static int launch_hmc_sl(const mc_program* p, const mc_run_config* cfg, void* state,
                         float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    if (!interp_ok(p))
        return fail(MC_ERR_UNSUPPORTED, "the term interpreter does not run transformed operands "
                    "or affine locs");
    RunState R = run_state(p, cfg, state);
    const SlCtx ctx = slctx_of(p);
    const TraceDev td = trace_of(tr);
    ExchangeLaunch d;
    d.name = "sliced HMC";
    d.threads = kSlLanes * NB / 2;
    d.chains = NB;
    d.S = p->sl.S;
    d.lds = (size_t)SlLayout<NB>(ctx).total * 4;
    d.blocks_per_launch = sl_groups_per_launch(p, cfg->num_chains);
    d.clear_bytes = sl_workspace_bytes(p, cfg->num_chains);
    d.tags_per_launch = 0;
    // the kernel takes no tag base: its tags restart at 1 in every launch, so
    // the granules (and, first, the status word) are cleared ahead of each, and
    // the lane-resident kernel must clear again after it
    d.restart_tags = true;
    d.coresident = true;
    int* status = (int*)ws;
    unsigned long long* xch = (unsigned long long*)((char*)ws + kSlStatusBytes);
    auto k = static_pair(k_hmc_sl<NB>, k_hmc_sl<NB>);  // (no L2-resident variant)
    return run_exchange(d, k, cfg->num_chains, ws, st, R.A,
                        [&](int64_t g0, int64_t ng, int64_t grid, bool xl, uint32_t) {
        return k.launch(xl, grid, d.threads, d.lds, st, ctx, R.A, g0 * NB, ng, R.scalars, R.q, R.g,
                        samples, td, xch, status);
    });
}

extern "C" int mc_workspace_status(const mc_program* p, const void* ws, int64_t bytes,
                                   void* stream) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (!ws || !ws_has_status(ws)) return MC_OK;  // the last launch on ws had no exchange
    if (bytes < kSlStatusBytes) return fail(MC_ERR_INVALID, "bad workspace");
    int v = 0;
    MC_HIP_TRY(hipMemcpyAsync(&v, ws, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    MC_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (v != 0) {
        ws_forget(ws);  // the next launch clears the status word and the granules
        if (v == 2) {
            // the placement probe was wrong for this device: later launches in
            // this process use the agent-scope exchange (as MC_XCD_LOCAL=0);
            // the launch that failed skipped work and has to be redone
            g_xcd_local = 0;
            return fail(MC_ERR_UNSUPPORTED,
                        "sliced launch: an exchange group's workgroups were not on one XCD, which "
                        "its L2-resident records need (the device's workgroup placement differs "
                        "from its probe); the L2-resident exchange is now off in this process: "
                        "redo the launch from the chains' state before it");
        }
        return fail(MC_ERR_TIMEOUT, "sliced HMC: a cross-workgroup exchange timed out");
    }
    return MC_OK;
}

extern "C" int64_t mc_hmc_workspace_bytes(const mc_program* p, int64_t C) {
    if (!p || C < 0) return -1;
    // (a lanes1 program runs L = 0 configurations on the unsliced kernel, and
    // so does a sliced program with transformed operands, which the term
    // interpreter does not take: mc_hmc_run)
    const int64_t x = (lanes1(p) || sliced(p)) ? sl_workspace_bytes(p, C) : 0;
    if (sliced(p) && interp_ok(p)) return x;
    if (hmc_use_lds(p)) return x;
    return std::max(x, C * 5 * (int64_t)dpad_of(p->D) * 4);
}

// MET: the metric instantiation (metric.h) on the buffer `metric`; minv and
// msqrt join the arena in LDS when the two extra vectors still fit its budget
// (the arena decision itself, and so the workspace, is the one without a metric)
template <int WPC, bool LDS, bool EX, bool MET>
static int launch_hmc(const mc_program* p, const mc_run_config* cfg, void* state,
                      float* samples, const mc_trace* tr, float* ws, hipStream_t st, void* metric,
                      int adapt) {
    RunState R = run_state(p, cfg, state);
    RunArgs& A = R.A;
    A.dpad = dpad_of(p->D);
    A.lds_floats = (int32_t)hmc_lds_floats(p, LDS);
    A.scratch_floats = scratch_of(p);
    bool ml = false;
    if constexpr (MET) {
        ml = LDS && cpb_of(WPC) * (A.lds_floats + 2 * (int64_t)A.dpad) * 4 <= kLdsArenaBudget;
        if (ml) A.lds_floats += 2 * A.dpad;
    }
    const size_t lds = (size_t)cpb_of(WPC) * A.lds_floats * 4;
    const int64_t grid = (cfg->num_chains + cpb_of(WPC) - 1) / cpb_of(WPC);
    // (EX: the program's expression terms compiled, jit.hip)
    const std::string jit = !EX ? "" : "mc::k_hmc<" + std::to_string(WPC) + ", " +
                                           (LDS ? "true" : "false") +
                                           (MET ? ", true, true, mc::MetricDev>" : ", true>");
    auto go = [&](auto kern, auto... met) {
        return launch_tape(p, kern, jit, grid, block_of(WPC), lds, st, ctx_of(p), A, R.scalars,
                           R.q, R.g, samples, trace_of(tr), ws, met...);
    };
    if constexpr (MET)
        return go(k_hmc<WPC, LDS, EX, true, MetricDev>,
                  metricdev_of(p, cfg->num_chains, metric, adapt, ml));
    else
        return go(k_hmc<WPC, LDS, EX>);
}

// A run that takes an exchange kernel (sliced or lane-resident).  L = 0 with
// transformed operands: the interpreter (k_hmc_sl) declines them, so such a
// run takes the chain-per-workgroup tape (as lanes1 does)
static bool hmc_exchange_route(const mc_program* p, const mc_run_config* cfg) {
    const bool sl_tape = sliced(p) && !use_lanes(p, cfg) && !interp_ok(p);
    return (sliced(p) && !sl_tape) || (lanes1(p) && use_lanes(p, cfg));
}

// What mc_hmc_run and mc_hmc_run_metric check first (met: the metric entry)
static int hmc_validate(const mc_program* p, const mc_run_config* cfg, void* state, bool met,
                        const void* metric) {
    int rc = check_cfg(p, cfg, state);
    if (rc) return rc;
    if (met && !metric) return fail(MC_ERR_INVALID, "metric buffer is NULL");
    if (cfg->num_leapfrog_steps < 0) return fail(MC_ERR_INVALID, "num_leapfrog_steps < 0");
    return MC_OK;
}

// ... and where both end: k_hmc on the tape (metric: the MET instantiation)
template <bool MET>
static int hmc_tape(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                    const mc_trace* tr, void* ws, int64_t ws_bytes, void* stream, void* metric,
                    int adapt) {
    ws_forget(ws);
    const bool lds = hmc_use_lds(p);
    const int64_t need = mc_hmc_workspace_bytes(p, cfg->num_chains);
    if (!lds && (ws == nullptr || ws_bytes < need))
        return fail(MC_ERR_INVALID, "workspace too small: need %lld bytes", (long long)need);
    return dispatch_tape(p, lds, [&](auto W, auto L, auto E) {
        return launch_hmc<decltype(W)::value, decltype(L)::value, decltype(E)::value, MET>(
            p, cfg, state, samples, tr, (float*)ws, (hipStream_t)stream, metric, adapt);
    });
}

extern "C" int mc_hmc_run(const mc_program* p, const mc_run_config* cfg, void* state,
                          float* samples, const mc_trace* tr, void* ws, int64_t ws_bytes,
                          void* stream) {
    int rc = hmc_validate(p, cfg, state, false, nullptr);
    if (rc) return rc;
    if (cfg->num_chains == 0 || cfg->iter_count == 0) return MC_OK;
    if (hmc_exchange_route(p, cfg)) {
        const int64_t need = sl_workspace_bytes(p, cfg->num_chains);
        if (ws == nullptr || ws_bytes < need)
            return fail(MC_ERR_INVALID, "workspace too small: need %lld bytes", (long long)need);
        if (device_cus() <= 0) return fail(MC_ERR_HIP, "no HIP device");
        hipStream_t st = (hipStream_t)stream;
        if (use_lanes(p, cfg) && hmc_dense_route(p)) {
            switch (p->lrd.rs) {
                case 1: return hmc_dense_rs1(p, cfg, state, samples, tr, ws, st);
                case 2: return hmc_dense_rs2(p, cfg, state, samples, tr, ws, st);
                default: return hmc_dense_rs4(p, cfg, state, samples, tr, ws, st);
            }
        }
        if (!use_lanes(p, cfg))
            return sl_nb_for(p, cfg->num_chains) == 16
                       ? launch_hmc_sl<16>(p, cfg, state, samples, tr, ws, st)
                       : launch_hmc_sl<8>(p, cfg, state, samples, tr, ws, st);
        switch (p->lr.rs) {  // (one translation unit per slot count: run_lanes_rs*.hip)
            case 1: rc = hmc_lanes_rs1(p, cfg, state, samples, tr, ws, st); break;
            case 2: rc = hmc_lanes_rs2(p, cfg, state, samples, tr, ws, st); break;
            default: rc = hmc_lanes_rs4(p, cfg, state, samples, tr, ws, st); break;
        }
        // an expression program without its JIT-compiled lane kernel (the
        // JIT off or failed): the tape below
        if (rc != kLanesNoJit) return rc;
    }
    return hmc_tape<false>(p, cfg, state, samples, tr, ws, ws_bytes, stream, nullptr, 0);
}

extern "C" int mc_hmc_run_metric(const mc_program* p, const mc_run_config* cfg, void* state,
                                 float* samples, const mc_trace* tr, void* ws, int64_t ws_bytes,
                                 void* metric, int32_t adapt, void* stream) {
    int rc = hmc_validate(p, cfg, state, true, metric);
    if (rc) return rc;
    if (hmc_exchange_route(p, cfg))
        return fail(MC_ERR_UNSUPPORTED,
                    "a metric runs on the chain-per-workgroup kernel k_hmc only and this program "
                    "is planned onto a sliced or lane-resident kernel: "
                    "mc_program_set_slices(prog, 1) keeps it on k_hmc");
    if (cfg->num_chains == 0 || cfg->iter_count == 0) return MC_OK;
    return hmc_tape<true>(p, cfg, state, samples, tr, ws, ws_bytes, stream, metric, adapt);
}

#ifdef MC_STAMPS
MC_STAMPS_EXPORT(mc_debug_stamps, mc_debug_stamps_wg)
#endif
