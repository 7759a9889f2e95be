// run_nuts_lr_met.hip — k_nuts_lr<RS, 3, 2, PW, MET>: the register-only
// lane-resident NUTS kernel with a per-chain diagonal metric (nuts_lanes.h),
// RS in {1, 2, 4}, with and without the draw wave.
#include "run_nuts_lr_met.h"

int nuts_lr_met_launch(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                       const mc_trace* tr, void* metric, int adapt, const NutsLrShape& sh,
                       hipStream_t st) {
    // (minv / msqrt live in the lanes' registers: nothing of the metric in LDS)
    const MetricDev M = metricdev_of(p, cfg->num_chains, metric, adapt, false);
    RunState R = run_state(p, cfg, state);
    return dispatch_rs(p, [&](auto R_) {  // (register-only: NSH = 3 alone)
        constexpr int RS = decltype(R_)::value;
        auto kern = sh.pw ? k_nuts_lr<RS, 3, 2, true, true, MetricDev>
                          : k_nuts_lr<RS, 3, 2, false, true, MetricDev>;
        return launch_tape(p, kern, "", cfg->num_chains, sh.threads, sh.lds, st, lrctx_of(p), R.A,
                           R.scalars, R.q, R.g, samples, trace_of(tr), M);
    });
}
