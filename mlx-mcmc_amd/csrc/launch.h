// launch.h — the host side of a sampler launch, shared by the run_* units
// (host only: the expression JIT does not embed it).  run_state: the prologue
// every launcher starts with.  launch_tape: one chain-per-workgroup launch,
// with its JIT attempt.  ExchangeLaunch / run_exchange: the launches of a
// kernel whose workgroups exchange records (k_hmc_sl, k_hmc_lr / k_hmc_lf,
// k_nuts_sl, k_mh_sl), on a kernel pair compiled into the library
// (StaticPair) or by the expression JIT (ModulePair).
#pragma once
#include "host.h"
#include "jit.h"

// The state pointers of a run and a zeroed RunArgs holding its configuration.
struct RunState {
    mc_chain_scalars* scalars;
    float *q, *g;
    RunArgs A;
};
inline RunState run_state(const mc_program* p, const mc_run_config* cfg, void* state) {
    int64_t qo, go;
    mc_state_offsets(p, cfg->num_chains, &qo, &go);
    char* b = (char*)state;
    RunState R;
    R.scalars = (mc_chain_scalars*)b;
    R.q = (float*)(b + qo);
    R.g = (float*)(b + go);
    std::memset(&R.A, 0, sizeof(R.A));
    R.A.cfg = *cfg;
    return R;
}

// One launch of a kernel without an exchange: `jit_name` (a name expression,
// "" for none) compiled with the program's expression terms when the JIT has
// it (jit.hip), else `kernel`.  The arguments are converted to the kernel's
// parameter types for either.
template <typename... KA, typename... A>
inline int launch_tape(const mc_program* p, void (*kernel)(KA...), const std::string& jit_name,
                       int64_t grid, int block, size_t lds, hipStream_t st, const A&... a) {
    if (!jit_name.empty()) {
        std::tuple<std::decay_t<KA>...> v(a...);
        bool used = false;
        const int rc = std::apply([&](auto&... x) {
            void* args[] = {(void*)&x...};
            return jit_launch(p, jit_name, (unsigned)grid, block, lds, st, args, &used);
        }, v);
        if (rc != MC_OK || used) return rc;
    }
    MC_HIP_TRY(allow_lds(kernel, lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), lds, st, std::decay_t<KA>(a)...);
    MC_HIP_TRY(hipGetLastError());
    return MC_OK;
}

// ---- exchange launches --------------------------------------------------------
// What run_exchange needs to know of a kernel whose workgroups wait for each
// other's records (host.h: "sliced launches").
struct ExchangeLaunch {
    const char* name;   // for the co-residency error text ("sliced NUTS")
    int threads;        // per workgroup
    int chains;         // per chain block
    int S;              // workgroups (slices) per chain block
    size_t lds;         // dynamic LDS bytes
    // chain blocks per launch, or 0: as many as the device holds of this
    // kernel, capacity / S (k_nuts_sl, k_mh_sl; the HMC kernels size their
    // workspace for one workgroup per CU: sl / lr_groups_per_launch)
    int64_t blocks_per_launch;
    int64_t clear_bytes;       // of the workspace: status word and exchange lines
    uint64_t tags_per_launch;  // exchange tags a launch may use
    // false: tags continue on the workspace across launches (ws_reserve: it is
    // cleared only when the library first sees it); true: they restart at 1 in
    // every launch, so the workspace is forgotten and the lines cleared ahead
    // of each (k_hmc_sl: it takes no tag base)
    bool restart_tags;
    // false: one slice, no exchange (k_hmc_lr / k_hmc_lf with X1) — no
    // capacity check, no fault hook, no L2-resident variant
    bool coresident;
};

// A kernel and its L2-resident variant (host.h xcd_round_robin; the same
// pointer twice when it has none), compiled into the library.
template <typename... KA>
struct StaticPair {
    void (*k)(KA...);
    void (*kxl)(KA...);
    int prepare(size_t lds) const {
        MC_HIP_TRY(allow_lds(k, lds));
        if (kxl != k) MC_HIP_TRY(allow_lds(kxl, lds));
        return MC_OK;
    }
    int64_t capacity(int threads, size_t lds) const { return resident_capacity(k, threads, lds); }
    bool has_xl() const { return kxl != k; }
    template <typename... A>
    int launch(bool xl, int64_t grid, int threads, size_t lds, hipStream_t st, const A&... a) const {
        const hipError_t e = launch_exchange(xl ? kxl : k, grid, threads, lds, st, a...);
        MC_HIP_TRY(e);
        return MC_OK;
    }
};
template <typename... KA>
inline StaticPair<KA...> static_pair(void (*k)(KA...), void (*kxl)(KA...)) {
    return {k, kxl};
}

// The same pair compiled by the expression JIT: `name` is the kernel's name
// expression up to its last template argument, XL.
struct ModulePair {
    const mc_program* p;
    std::string name;
    hipFunction_t f = nullptr, fxl = nullptr;
    // f stays nullptr (and MC_OK) when the JIT is off or the compilation failed
    int load() { return jit_function(p, name + ", false>", &f); }
    // GAP: module kernels launch without the attribute allow_lds sets, and
    // nothing here refuses more than the default 64 KB of dynamic LDS (the
    // tape's JIT launch of k_nuts is gated on it, run_nuts.hip; the lane
    // layout's LDS may exceed it).  DESIGN §7.
    int prepare(size_t) const { return MC_OK; }
    // not cached (a hipFunction_t dies with its program, so its value is no
    // key); 0 when the query fails
    int64_t capacity(int threads, size_t lds) const {
        int n = 0;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, threads, lds) != hipSuccess)
            n = 0;
        return (int64_t)n * device_cus();
    }
    bool has_xl() const { return true; }  // (loaded at the first launch that wants it)
    // the arguments must have the kernel's parameter types exactly
    template <typename... A>
    int launch(bool xl, int64_t grid, int threads, size_t lds, hipStream_t st, A... a) {
        hipFunction_t k = f;
        if (xl) {
            if (fxl == nullptr) {
                const int rc = jit_function(p, name + ", true>", &fxl);
                if (rc != MC_OK) return rc;
            }
            if (fxl != nullptr) k = fxl;
        }
        void* args[] = {(void*)&a...};
        MC_HIP_TRY(hipModuleLaunchKernel(k, (unsigned)grid, 1, 1, threads, 1, 1, (unsigned)lds, st,
                                         args, nullptr));
        return MC_OK;
    }
};

// Run C chains of exchange kernel pair k on workspace ws: the co-residency
// check, the workspace's tags and clearing, then one launch per group of chain
// blocks the device holds at once, each through launch(g0, ng, grid, use_xl,
// base) — chain blocks [g0, g0 + ng), grid workgroups, the L2-resident variant
// or not, base = the launch's first tag - 1 — which owns the kernel's
// argument list.
template <typename K, typename F>
inline int run_exchange(const ExchangeLaunch& d, K& k, int64_t C, void* ws, hipStream_t st,
                        RunArgs& A, F&& launch) {
    int rc = k.prepare(d.lds);
    if (rc != MC_OK) return rc;
    const int64_t groups = (C + d.chains - 1) / d.chains;
    int64_t gpl = d.blocks_per_launch;
    if (d.coresident) {
        const int64_t cap = k.capacity(d.threads, d.lds);
        if (gpl == 0) {
            if (cap < d.S)
                return fail(MC_ERR_UNSUPPORTED,
                            "%s: a chain block's %d workgroups must be co-resident, the device "
                            "holds %lld of this kernel", d.name, d.S, (long long)cap);
            gpl = std::min(groups, cap / d.S);
        } else if (cap < std::min(gpl, groups) * d.S) {
            return fail(MC_ERR_UNSUPPORTED,
                        "%s: %lld workgroups must be co-resident, the device holds %lld of this "
                        "kernel", d.name, (long long)(std::min(gpl, groups) * d.S), (long long)cap);
        }
        A.fault = g_exchange_fault;
    }
    const int64_t nlaunch = (groups + gpl - 1) / gpl;
    uint32_t base = 0;
    if (d.restart_tags)
        ws_forget(ws);  // a kernel whose tags continue must clear again
    else if (ws_reserve(ws, d.tags_per_launch * (uint64_t)nlaunch, (uint64_t)d.clear_bytes, &base))
        MC_HIP_TRY(hipMemsetAsync(ws, 0, d.clear_bytes, st));
    ws_mark_status(ws);
    for (int64_t g0 = 0; g0 < groups; g0 += gpl) {
        const int64_t ng = std::min(gpl, groups - g0);
        if (d.restart_tags)  // the lines and, ahead of the first launch, the status word
            MC_HIP_TRY(hipMemsetAsync(g0 == 0 ? ws : (void*)((char*)ws + kSlStatusBytes), 0,
                                      g0 == 0 ? d.clear_bytes : d.clear_bytes - kSlStatusBytes, st));
        const int64_t grid = ng * d.S;
        const bool xl = d.coresident && k.has_xl() && xcd_round_robin(grid, d.S);
        rc = launch(g0, ng, grid, xl, base);
        if (rc != MC_OK) return rc;
        base += (uint32_t)d.tags_per_launch;
    }
    return MC_OK;
}
