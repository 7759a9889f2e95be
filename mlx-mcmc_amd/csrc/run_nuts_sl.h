// run_nuts_sl.h — the sliced NUTS launch (k_nuts_sl, nuts_sliced.h), included
// by run_nuts_sl.hip (the compile-time hierarchical form) and
// run_nuts_sl_rt.hip (the run-time form): two translation units so the
// instantiations compile in parallel.
#pragma once
#include "launch.h"

// chains (waves) per workgroup of k_nuts_sl
constexpr int kNslWaves = 8;

// LDS bytes of a k_nuts_sl workgroup: the slice block and scalar terms, then
// per wave the first-leaf arena and the shared parameters' arena rows
inline size_t nuts_sl_lds_bytes(const mc_program* p, int max_depth) {
    return lr_base_lds_bytes(p) +
           (size_t)kNslWaves *
               ((size_t)nuts_sl_first_floats(p->lr.rs, max_depth) +
                (size_t)nuts_sl_shared_rows(max_depth) * 4) * 4;
}

// waves per SIMD the kernel is compiled for: with more than 8 slices two
// workgroups share a CU (4 waves per SIMD, <= 128 VGPRs), so 256 chains of 16
// slices run at once (4096 waves); with <= 8 one workgroup per CU (2 waves
// per SIMD).  Large shape, 256 chains, 16 slices: 21.7 M leaf-steps/s at 4
// waves per SIMD, 14.3 M at 2 (two launches of 128 chains); 8 slices at 2:
// 18.5 M.  MC_NUTS_SL_OCC=2|4 overrides.
inline int nuts_sl_occ(const mc_program* p) {
    if (const char* e = std::getenv("MC_NUTS_SL_OCC")) {
        const int v = std::atoi(e);
        if (v == 2 || v == 4) return v;
    }
    return p->lr.S > 8 ? 4 : 2;
}

// exchange lines (both parities) for every chain block of C chains, then the
// XCD check's slots (16 granules per slice of a block)
inline int64_t nuts_sl_line_bytes(const mc_program* p, int64_t C) {
    const int64_t groups = (C + kNslWaves - 1) / kNslWaves;
    return 2 * groups * kNslWaves * (int64_t)p->lr.S * kNslLine * 8 +
           groups * (int64_t)p->lr.S * 16 * 8;
}

// The launches of kernel pair k
template <typename K>
inline int nuts_sl_exchange(const char* name, K& k, const mc_program* p, const mc_run_config* cfg,
                            void* state, float* samples, const mc_trace* tr, void* ws,
                            hipStream_t st) {
    RunState R = run_state(p, cfg, state);
    const LrCtx ctx = lrctx_of(p);
    const TraceDev td = trace_of(tr);
    const int maxj = cfg->max_tree_depth;
    const int64_t lines = nuts_sl_line_bytes(p, cfg->num_chains);
    ExchangeLaunch d;
    d.name = name;
    d.threads = 64 * kNslWaves;
    d.chains = kNslWaves;
    d.S = p->lr.S;
    d.lds = nuts_sl_lds_bytes(p, maxj);
    d.blocks_per_launch = 0;  // what the device holds: the workspace has lines for every block
    d.clear_bytes = kSlStatusBytes + lines;
    // tags: one per leaf, at most iter_count * 2^maxj leaves per chain
    d.tags_per_launch = (uint64_t)cfg->iter_count * (1ull << maxj) + 1;
    d.restart_tags = false;
    d.coresident = true;
    int* status = (int*)ws;
    unsigned long long* xch = (unsigned long long*)((char*)ws + kSlStatusBytes);
    float* pool = (float*)((char*)ws + kSlStatusBytes + lines);
    return run_exchange(d, k, cfg->num_chains, ws, st, R.A,
                        [&](int64_t g0, int64_t ng, int64_t grid, bool xl, uint32_t base) {
        return k.launch(xl, grid, d.threads, d.lds, st, ctx, R.A, g0 * kNslWaves, ng, R.scalars,
                        R.q, R.g, samples, td, xch, pool, status, base);
    });
}

template <int RS, int NSH, int OCC, int FORM>
inline int launch_nuts_sl(const mc_program* p, const mc_run_config* cfg, void* state,
                          float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    auto kern = k_nuts_sl<RS, NSH, kNslWaves, OCC, FORM>;
    // the compile-time form also with L2-resident records (host.h xcd_round_robin)
    auto kern_xl = kern;
    if constexpr (FORM >= 0) kern_xl = k_nuts_sl<RS, NSH, kNslWaves, OCC, FORM, true>;
    auto k = static_pair(kern, kern_xl);
    return nuts_sl_exchange("sliced NUTS", k, p, cfg, state, samples, tr, ws, st);
}

// The run-time form compiled with the program's expression terms (jit.hip):
// kLanesNoJit when the JIT is off or the compilation failed (the caller runs
// the program on the tape).
template <int RS, int NSH, int OCC>
inline int launch_nuts_sl_jit(const mc_program* p, const mc_run_config* cfg, void* state,
                              float* samples, const mc_trace* tr, void* ws, hipStream_t st) {
    ModulePair k{p, "mc::k_nuts_sl<" + std::to_string(RS) + ", " + std::to_string(NSH) + ", " +
                        std::to_string(kNslWaves) + ", " + std::to_string(OCC) + ", -1"};
    const int rc = k.load();
    if (rc != MC_OK) return rc;
    if (k.f == nullptr) return kLanesNoJit;
    return nuts_sl_exchange("sliced NUTS (expression JIT)", k, p, cfg, state, samples, tr, ws, st);
}

// the compile-time hierarchical form (run_nuts_sl.hip) and the run-time form
// (run_nuts_sl_rt.hip)
int nuts_sl_hier(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                 const mc_trace* tr, void* ws, hipStream_t st);
int nuts_sl_rt(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
               const mc_trace* tr, void* ws, hipStream_t st);

// The sliced NUTS kernel runs programs the automatic plan slices (S >= 2)
// onto the fast-form lane layout (k_hmc_lf's programs), unless
// MC_NUTS_SLICED=0 in the environment or mc_debug_nuts_variant(0) (A/B and
// tests: k_nuts on the tape), the slice kernel is forced to the interpreter,
// max_tree_depth is outside [1, kNslMaxDepth] or the LDS arenas do not fit.
inline int g_nuts_sliced = -1;  // mc_debug_nuts_sliced; -1: MC_NUTS_SLICED
inline bool nuts_sliced_enabled() {
    if (g_nuts_sliced < 0) g_nuts_sliced = env_on("MC_NUTS_SLICED");
    return g_nuts_sliced == 1;
}
// A program with expression terms (LanePlan::nuts_expr) runs the JIT-compiled
// run-time form (their element code exists only compiled per program): not
// while the JIT is off or after its compilation failed (the tape runs it).
inline bool use_nuts_sliced(const mc_program* p, int max_depth) {
    const bool expr = p->lr.nuts_expr && jit_enabled() && jit_error(p).empty();
    return nuts_sliced_enabled() && p->sl.S >= 2 && p->lr.ok && (p->lr.fast || expr) &&
           lanes_fast_enabled() && p->lr.S >= 2 && p->lr.S <= kLrSlices &&
           p->slice_kernel != 1 && max_depth >= 1 && max_depth <= kNslMaxDepth &&
           nuts_sl_lds_bytes(p, max_depth) <= (size_t)kSlLdsBudget;
}
// status word, exchange lines, then the candidate pool of every chain
inline int64_t nuts_sl_workspace_bytes(const mc_program* p, int64_t C, int max_depth) {
    const int64_t groups = (C + kNslWaves - 1) / kNslWaves;
    return kSlStatusBytes + nuts_sl_line_bytes(p, C) +
           groups * kNslWaves * (int64_t)p->lr.S * nuts_sl_pool_floats(p->lr.rs, max_depth) * 4;
}
