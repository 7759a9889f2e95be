// run_nuts_lr_met.hip — k_nuts_lr<RS, 3, 2, PW, MET>: the register-only
// lane-resident NUTS kernel with a per-chain diagonal metric (nuts_lanes.h),
// RS in {1, 2, 4}, with and without the draw wave.
#include "run_nuts_lr_met.h"

template <int RS>
static int launch_rs(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                     const mc_trace* tr, const MetricDev& M, size_t lds, bool pw, hipStream_t st) {
    int64_t qo, go;
    mc_state_offsets(p, cfg->num_chains, &qo, &go);
    char* b = (char*)state;
    RunArgs A;
    std::memset(&A, 0, sizeof(A));
    A.cfg = *cfg;
    auto kern = pw ? k_nuts_lr<RS, 3, 2, true, true, MetricDev>
                   : k_nuts_lr<RS, 3, 2, false, true, MetricDev>;
    MC_HIP_TRY(allow_lds(kern, lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)cfg->num_chains), dim3(pw ? 128 : 64), lds, st,
                       lrctx_of(p), A, (mc_chain_scalars*)b, (float*)(b + qo), (float*)(b + go),
                       samples, trace_of(tr), M);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

int nuts_lr_met_launch(const mc_program* p, const mc_run_config* cfg, void* state, float* samples,
                       const mc_trace* tr, void* metric, int adapt, size_t lds, bool pw,
                       hipStream_t st) {
    // (minv / msqrt live in the lanes' registers: nothing of the metric in LDS)
    const MetricDev M = metricdev_of(p, cfg->num_chains, metric, adapt, false);
    switch (p->lr.rs) {
        case 1: return launch_rs<1>(p, cfg, state, samples, tr, M, lds, pw, st);
        case 2: return launch_rs<2>(p, cfg, state, samples, tr, M, lds, pw, st);
        default: return launch_rs<4>(p, cfg, state, samples, tr, M, lds, pw, st);
    }
}
