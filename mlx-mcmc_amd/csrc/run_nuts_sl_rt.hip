// run_nuts_sl_rt.hip — sliced NUTS, run-time form (k_nuts_sl<..., FORM = -1>):
// fast-form programs whose slices differ in their terms or share roles.
#include "run_nuts_sl.h"

int nuts_sl_rt(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
               const mc_trace* tr, void* ws, hipStream_t st) {
    if (!p->lr.fast) {  // expression terms (LanePlan::nuts_expr): the JIT-compiled form
        // (2 waves per SIMD: at 16 slices 4 — every chain block of 256 chains
        // resident in one launch — measured no faster on the N = 100 K GLMs,
        // logistic 4.30 vs 4.25 M leaf-steps/s, two-predictor 8.97 vs 8.18;
        // MC_NUTS_SL_OCC=4 selects it: this path's own rule, 4 only when asked
        // for, where nuts_sl_occ defaults to 4 above 8 slices)
        const char* oe = std::getenv("MC_NUTS_SL_OCC");
        const bool o4 = oe && std::atoi(oe) == 4;
        return dispatch_lanes(p, [&](auto R, auto N) {
            constexpr int RS = decltype(R)::value, NSH = decltype(N)::value;
            return o4 ? launch_nuts_sl_jit<RS, NSH, 4>(p, cfg, state, samples, tr, ws, st)
                      : launch_nuts_sl_jit<RS, NSH, 2>(p, cfg, state, samples, tr, ws, st);
        });
    }
    return dispatch_lanes(p, [&](auto R, auto N) {
        return launch_nuts_sl<decltype(R)::value, decltype(N)::value, 2, -1>(p, cfg, state, samples,
                                                                             tr, ws, st);
    });
}
