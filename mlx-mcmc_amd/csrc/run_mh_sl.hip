// run_mh_sl.hip — the sliced Metropolis-Hastings launch (k_mh_sl, mh_sliced.h)
// for programs sliced onto the fast-form lane layout.
#include "run_mh_sl.h"

// The launches of kernel pair k
template <typename K>
static int mh_sl_exchange(const char* name, K& k, const mc_program* p, const mc_run_config* cfg,
                          float scale, void* state, float* samples, const mc_trace* tr, void* ws,
                          hipStream_t st) {
    RunState R = run_state(p, cfg, state);
    const LrCtx ctx = lrctx_of(p);
    const TraceDev td = trace_of(tr);
    ExchangeLaunch d;
    d.name = name;
    d.threads = 64 * kNslWaves;
    d.chains = kNslWaves;
    d.S = p->lr.S;
    d.lds = lr_base_lds_bytes(p);
    d.blocks_per_launch = 0;  // what the device holds: the workspace has lines for every block
    d.clear_bytes = kSlStatusBytes + mh_sl_line_bytes(p, cfg->num_chains);
    d.tags_per_launch = (uint64_t)cfg->iter_count + 1;  // one exchange per iteration
    d.restart_tags = false;
    d.coresident = true;
    int* status = (int*)ws;
    unsigned long long* xch = (unsigned long long*)((char*)ws + kSlStatusBytes);
    return run_exchange(d, k, cfg->num_chains, ws, st, R.A,
                        [&](int64_t g0, int64_t ng, int64_t grid, bool xl, uint32_t base) {
        return k.launch(xl, grid, d.threads, d.lds, st, ctx, R.A, scale, g0 * kNslWaves, ng,
                        R.scalars, R.q, samples, td, xch, status, base);
    });
}

template <int RS, int NSH, int OCC, int FORM>
static int launch_mh_sl(const mc_program* p, const mc_run_config* cfg, float scale, void* state,
                        float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    auto kern = k_mh_sl<RS, NSH, kNslWaves, OCC, FORM>;
    // the compile-time form also with L2-resident records (host.h xcd_round_robin)
    auto kern_xl = kern;
    if constexpr (FORM >= 0) kern_xl = k_mh_sl<RS, NSH, kNslWaves, OCC, FORM, true>;
    auto k = static_pair(kern, kern_xl);
    return mh_sl_exchange("sliced MH", k, p, cfg, scale, state, samples, tr, ws, st);
}

// The run-time form compiled with the program's expression terms (jit.hip);
// kLanesNoJit when the JIT is off or the compilation failed.
template <int RS, int NSH>
static int launch_mh_sl_jit(const mc_program* p, const mc_run_config* cfg, float scale,
                            void* state, float* samples, const mc_trace* tr, void* ws,
                            hipStream_t st) {
    ModulePair k{p, "mc::k_mh_sl<" + std::to_string(RS) + ", " + std::to_string(NSH) + ", " +
                        std::to_string(kNslWaves) + ", 2, -1"};
    const int rc = k.load();
    if (rc != MC_OK) return rc;
    if (k.f == nullptr) return kLanesNoJit;
    return mh_sl_exchange("sliced MH (expression JIT)", k, p, cfg, scale, state, samples, tr, ws,
                          st);
}

int mh_sliced_run(const mc_program* p, const mc_run_config* cfg, float scale, void* state,
                  float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    if (!p->lr.fast)  // expression terms (LanePlan::nuts_expr): the JIT-compiled form
        return dispatch_lanes(p, [&](auto R, auto N) {
            return launch_mh_sl_jit<decltype(R)::value, decltype(N)::value>(p, cfg, scale, state,
                                                                            samples, tr, ws, st);
        });
    constexpr int HIER = LF_SW | LF_SWS | LF_DIR | LF_DM | LF_DS;
    const bool hier = p->lr.form == HIER && lanes_forms_enabled();
    const bool o4 = nuts_sl_occ(p) == 4;
    return dispatch_rs(p, [&](auto R) {
        constexpr int RS = decltype(R)::value;
        if (hier)  // (NSH = 3 alone, at either occupancy; the run-time form at 2 only)
            return o4 ? launch_mh_sl<RS, 3, 4, HIER>(p, cfg, scale, state, samples, tr, ws, st)
                      : launch_mh_sl<RS, 3, 2, HIER>(p, cfg, scale, state, samples, tr, ws, st);
        return dispatch_nsh(p, [&](auto N) {
            return launch_mh_sl<RS, decltype(N)::value, 2, -1>(p, cfg, scale, state, samples, tr,
                                                               ws, st);
        });
    });
}
