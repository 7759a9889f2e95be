// program.hip — the program builder (mc_program_create*: validation, the
// chain-per-workgroup tape's segment tiling, pass and barrier planning), the
// slicing policy (which slice count and kernel a program runs on, through the
// planners of plan.h) and the program queries and host-only test hooks of
// include/mcmc355.h.
#include "plan.h"
#include "jit.h"

static thread_local bool g_program_host_only;
static bool is_vec_kind(int k) { return k == MC_OP_DATA || k == MC_OP_PVEC || k == MC_OP_GATHER; }
static bool is_acc_vec(int k) { return k == MC_OP_PVEC || k == MC_OP_GATHER; }

static int choose_wpc(int64_t max_n) {
    if (max_n <= 512) return 1;
    if (max_n <= 16384) return 4;
    return 8;
}

// Segment-tiled layout of a term sorted by its primary (non-injective) gather
// index; see DevTerm in internal.h.  Runs of equal index ("segments") are
// split into at most ceil(len / Lt) near-equal virtual segments so that a
// chain group of T threads has ~2T lanes of work even for few, long groups;
// with >= 2T segments nothing is split and each lane writes its group's
// gradient directly.
// prim_pool: index-pool offset of the sorted primary index; others: the
// term's other vector operands, tiled beside it (DATA copied, PVEC turned
// into identity gathers, GATHER indices copied); tsplit: with fewer groups
// than that, runs are split into ~tsplit virtual segments; nprim: partials per
// virtual segment (an expression term keeps one per gathered leaf), so that
// nprim x (virtual segments) fit the evaluator's 4T segment-partial floats.
static int build_segments_ops(DevTerm& dt, int64_t prim_pool, const std::vector<DevOperand*>& others,
                              int64_t tsplit, int nprim, std::vector<float>& dpool,
                              std::vector<int32_t>& ipool, int T) {
    const int64_t n = dt.n;
    const int64_t ip = prim_pool;
    std::vector<int64_t> sstart;
    std::vector<int32_t> sk;
    for (int64_t i = 0; i < n; ++i)
        if (i == 0 || ipool[ip + i] != ipool[ip + i - 1]) {
            sstart.push_back(i);
            sk.push_back(ipool[ip + i]);
        }
    const int64_t G = (int64_t)sstart.size();
    sstart.push_back(n);
    // split only when there are fewer groups than tsplit (then <= 2 tsplit
    // virtual segments); otherwise each lane owns whole groups
    struct V {
        int32_t k;
        int64_t start;
        int32_t len;
    };
    std::vector<V> vs;
    std::vector<int32_t> comb;
    bool split = false;
    auto plan_runs = [&](int64_t Lt) {
        vs.clear();
        comb.clear();
        split = false;
        for (int64_t g = 0; g < G; ++g) {
            const int64_t len = sstart[g + 1] - sstart[g];
            const int64_t pieces = (Lt == INT64_MAX) ? 1 : (len + Lt - 1) / Lt;
            if (pieces > 1) split = true;
            const int64_t base = len / pieces, rem = len % pieces;
            comb.push_back(sk[g]);
            comb.push_back((int32_t)vs.size());
            comb.push_back((int32_t)pieces);
            int64_t st = sstart[g];
            for (int64_t pc = 0; pc < pieces; ++pc) {
                const int64_t pl = base + (pc < rem ? 1 : 0);
                if (pl > INT32_MAX) return fail(MC_ERR_UNSUPPORTED, "segment too long");
                vs.push_back({sk[g], st, (int32_t)pl});
                st += pl;
            }
        }
        return MC_OK;
    };
    int rc = plan_runs((G >= tsplit) ? INT64_MAX : std::max<int64_t>(1, (n + tsplit - 1) / tsplit));
    if (rc) return rc;
    // the split's partial rows (nprim per virtual segment) must fit the
    // evaluator's 4T floats of segment scratch; tsplit keeps them within it,
    // and should a plan not, the runs stay whole (no hard error)
    if (split && (int64_t)vs.size() * nprim > 4 * (int64_t)T) {
        rc = plan_runs(INT64_MAX);
        if (rc) return rc;
    }
    const int64_t nv = (int64_t)vs.size();
    const int64_t ntiles = (nv + 63) / 64;
    std::vector<int32_t> tiles(3 * ntiles), lanes(2 * nv);
    int64_t total = 0;
    for (int64_t t = 0; t < ntiles; ++t) {
        int32_t lmax = 0, lmin = INT32_MAX;
        for (int l = 0; l < 64; ++l) {
            const int64_t v = t * 64 + l;
            if (v >= nv) break;  // lanes past the end are masked off in-kernel
            lmax = std::max(lmax, vs[v].len);
            lmin = std::min(lmin, vs[v].len);
        }
        const int32_t lpad = (lmax + 3) / 4 * 4;
        if (total > INT32_MAX - 64 * (int64_t)lpad)
            return fail(MC_ERR_UNSUPPORTED, "segmented term too large");
        tiles[3 * t] = (int32_t)total;
        tiles[3 * t + 1] = lpad;
        tiles[3 * t + 2] = lmin;
        total += 64 * (int64_t)lpad;
    }
    for (int64_t v = 0; v < nv; ++v) {
        lanes[2 * v] = vs[v].k;
        lanes[2 * v + 1] = vs[v].len;
    }
    // parameter slices become identity gathers so that they can be tiled too
    for (DevOperand* dp : others) {
        DevOperand& d = *dp;
        if (d.kind != MC_OP_PVEC) continue;
        const int64_t base = (int64_t)ipool.size();
        for (int64_t i = 0; i < n; ++i) ipool.push_back((int32_t)i);
        d.kind = MC_OP_GATHER;
        d.pool = base;
        d.unique = 1;
    }
    // tiled copies of every other vector operand (and an affine loc's data x)
    for (DevOperand* dp : others) {
        DevOperand& d = *dp;
        if (d.kind != MC_OP_DATA && d.kind != MC_OP_GATHER) continue;
        if (d.kind == MC_OP_DATA) {
            while (dpool.size() % 64) dpool.push_back(0.0f);
            const int64_t base = (int64_t)dpool.size();
            dpool.resize(base + total, 0.0f);
            for (int64_t v = 0; v < nv; ++v) {
                const int64_t t = v / 64, l = v % 64;
                for (int32_t u = 0; u < vs[v].len; ++u)
                    dpool[base + tiles[3 * t] + (u >> 2) * 256 + l * 4 + (u & 3)] =
                        dpool[d.pool + vs[v].start + u];
            }
            d.pool = base;
        } else {
            while (ipool.size() % 64) ipool.push_back(0);
            const int64_t base = (int64_t)ipool.size();
            ipool.resize(base + total, 0);
            for (int64_t v = 0; v < nv; ++v) {
                const int64_t t = v / 64, l = v % 64;
                for (int32_t u = 0; u < vs[v].len; ++u)
                    ipool[base + tiles[3 * t] + (u >> 2) * 256 + l * 4 + (u & 3)] =
                        ipool[d.pool + vs[v].start + u];
            }
            d.pool = base;
        }
    }
    dt.ntiles = (int32_t)ntiles;
    dt.nvirt = (int32_t)nv;
    dt.ncomb = split ? (int32_t)G : 0;
    dt.tile_base = (int64_t)ipool.size();
    ipool.insert(ipool.end(), tiles.begin(), tiles.end());
    while (ipool.size() % 2) ipool.push_back(0);  // lane records are read as int2
    dt.lane_base = (int64_t)ipool.size();
    ipool.insert(ipool.end(), lanes.begin(), lanes.end());
    dt.comb_base = (int64_t)ipool.size();
    if (split) ipool.insert(ipool.end(), comb.begin(), comb.end());
    return MC_OK;
}

static int build_segments(DevTerm& dt, std::vector<float>& dpool, std::vector<int32_t>& ipool,
                          int T) {
    const int a = dt.primary;
    std::vector<DevOperand*> others;
    for (int b = 0; b < 3; ++b)
        if (b != a) others.push_back(&dt.op[b]);
    if (dt.affine) others.push_back(&dt.ax);
    return build_segments_ops(dt, dt.op[a].pool, others, T, 1, dpool, ipool, T);
}

static int sl_lds_bytes(const mc_program* p, int nb) {
    const SlCtx c = slctx_of(p);
    return 4 * (nb == 16 ? SlLayout<16>(c).total : SlLayout<8>(c).total);
}

// Element count of a program (the planner's size measure).
static int64_t program_elements(const mc_program* p) {
    int64_t n = 0;
    for (const DevTerm& t : p->raw) n += t.n;
    return n;
}
// The automatic slice count.  Programs of 2 K - 8 K elements are sliced (4
// ways) only when the lane-resident kernel takes them (measured at 256
// chains: the D = 100 / N = 10 k and D = 10 / N = 1 k hierarchical models run
// 2.1x / 1.7x faster than on the chain-per-workgroup kernel); smaller ones
// stay unsliced (a per-step exchange costs more than the whole evaluation).
// 8 - 64 K elements: 8 slices (one wave per SIMD, every CU busy at 256
// chains; the D = 100 / N = 10 k model: 165 -> 185 M steps/s against 4
// slices, 79 M with 16, profiles/r4/slices).
static int auto_slices(const mc_program* p) {
    if ((has_expr(p) && !expr_lanes_ok(p)) || (has_affine(p) && !affine_lanes_ok(p)) ||
        (has_transform(p) && !transform_on_shared_only(p)))
        return 1;
    const int64_t n = program_elements(p);
    if (n >= 65536) return 16;
    if (n >= 8192) return 8;
    if (n >= kLrAutoMinElements) return 4;
    return 1;
}

// The lane planner declined (LanePlan::why): drop its partial tables, keep the
// reason and note it.  Returns the reason.
static const std::string& decline_lanes(mc_program* p) {
    const std::string why = p->lr.why;
    free_lanes(p->lr);
    p->lr.why = why;
    p->note = "lane-resident kernel: " + why;
    return p->lr.why;
}

// Plan an unsliced program onto the lane-resident kernel (one slice).
static int plan_lanes1(mc_program* p) {
    free_lanes(p->lr);
    // expression programs below the slicing threshold stay on the tape (the
    // one-slice lane kernel is not measured on them)
    if (has_expr(p))
        return fail(MC_ERR_UNSUPPORTED, "lane-resident kernel: an unsliced expression program "
                    "runs on the tape");
    SlicePlan P;
    SlPartition part;
    // (the tile stage's tables are not used here, only its status: known
    // slack, DESIGN.md "planner stages")
    const int rc = plan_slices(p, 1, P, part);
    if (rc != MC_OK) {
        p->note = "lane-resident kernel: " + g_last_error;
        return rc;
    }
    if (plan_lanes(p, part, p->lr) != MC_OK)
        return fail(MC_ERR_UNSUPPORTED, "lane-resident kernel: %s", decline_lanes(p).c_str());
    p->note.clear();
    const hipError_t e = upload_lanes(p->lr);
    if (e != hipSuccess) {
        free_lanes(p->lr);
        return upload_failed(e, "lane plan");
    }
    return MC_OK;
}

// The dense HMC plan (mc_program::lrd), beside an automatic program-level plan
// that is fast-form with the hierarchical compile-time form and no transformed
// shared parameter: the same planner passes at one lane per parameter on DS
// slices.  A step of k_hmc_lf reads no observation (lanes_fast.h lf_moments),
// so nothing is gained by spreading a chain pair's sweep over workgroups: a
// pair runs in one.  DS = 1 — one wave, no exchange — when the private
// parameters fit a wave's 64 lanes x 4 slots; else the fewer of 4 and 8 waves
// that hold them at two slots per lane, exchanging through LDS (measured on
// D = 1000: 8 waves x 2 slots 244 M leapfrog-steps/s, 4 x 4 219 M, the 16
// exchanging workgroups 239 M).  More than 1024 private
// parameters keep the exchange kernels: 16 waves of one workgroup would need
// the kernel in 128 VGPRs.  MC_HMC_DENSE=0 in the environment turns the
// route off (A/B against the exchange kernels).  The plan's data tables are
// uploaded with it though the kernel reads only the direct term's length
// table of them: known slack.
static void plan_hmc_dense(mc_program* p) {
    constexpr int HIER = LF_SW | LF_SWS | LF_DIR | LF_DM | LF_DS;
    if (!env_on("MC_HMC_DENSE")) return;
    if (!p->lr.ok || !p->lr.fast || p->lr.form != HIER || p->lr.has_xf || p->lr.has_expr) return;
    const int priv = p->D - p->lr.Dsh;
    int DS = 1;
    if (priv > 64 * kLrMaxSlots) {
        DS = (priv + 3) / 4 <= 128 ? 4 : 8;
        if ((priv + DS - 1) / DS > 128) return;
    }
    SlicePlan P;
    SlPartition part;
    LanePlan& L = p->lrd;
    L.rep_cap = 1;
    const bool ok = plan_slices(p, DS, P, part) == MC_OK && plan_lanes(p, part, L) == MC_OK &&
                    L.fast && L.form == HIER && L.rep == 1 && L.S == DS && !L.has_xf &&
                    (DS == 1 || L.rs == 2) && upload_lanes(L) == hipSuccess;
    if (!ok) {
        free_lanes(L);
        return;
    }
    // Without a lane RNG plan (plan_lanes.hip plan_lane_rng: a slice with more
    // than 62 (chain, block) jobs — 124 private parameters: every 8 x 2 plan)
    // the workgroup draws each Philox block once and hands the normals out
    // through LDS (lanes_fast.h draw_block) instead of every lane drawing a
    // block per normal it needs.  (Of the one-wave kernels the four-slot one
    // alone: lanes_fast.h BDRAW.)  MC_HMC_DENSE_RNG=0 keeps the per-lane draws
    // (A/B; the draws are the same bits either way).
    L.blk_rng = L.rng.empty() && (DS > 1 || L.rs == 4) && env_on("MC_HMC_DENSE_RNG");
    // MC_HMC_DENSE_CHAINS=1|2 fixes the chains per workgroup of the 4- and
    // 8-slice launches (host.h hmc_dense_chains; A/B, tests), read here so that
    // programs of both routes can live in one process
    const char* nc = std::getenv("MC_HMC_DENSE_CHAINS");
    L.dense_chains = (nc && (nc[0] == '1' || nc[0] == '2') && nc[1] == 0) ? nc[0] - '0' : 0;
}

static int set_slices(mc_program* p, int32_t S);
extern "C" int mc_program_set_slices(mc_program* p, int32_t S) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (S < 0 || S > 64) return fail(MC_ERR_INVALID, "num_slices must be in [0, 64]");
    free_lanes(p->lrd);
    const int rc = set_slices(p, S);
    // an explicit slice count always runs the program-level kernels
    if (rc == MC_OK && S == 0) {
        const std::string err = g_last_error;  // (a declined dense plan is no error)
        plan_hmc_dense(p);
        g_last_error = err;
    }
    return rc;
}

// 1 when HMC launches of the program take the dense route (run_hmc.hip), with
// its slices (waves per chain pair) and register slots per lane; else 0
extern "C" int32_t mc_program_hmc_dense(const mc_program* p, int32_t* slices, int32_t* slots) {
    if (!p) return -1;
    const bool on = hmc_dense_route(p);
    if (slices) *slices = on ? p->lrd.S : 0;
    if (slots) *slots = on ? p->lrd.rs : 0;
    return on ? 1 : 0;
}

// Test hook: how the dense HMC route draws.  0: HMC launches run the
// program-level plan; 1: the dense plan has a lane RNG plan; 2: it has none
// and the workgroup draws block-wide; 3: none, per-lane draws
// (MC_HMC_DENSE_RNG=0).  -1 on a null program.
extern "C" int32_t mc_debug_hmc_dense_rng(const mc_program* p) {
    if (!p) return -1;
    if (!hmc_dense_route(p)) return 0;
    if (!p->lrd.rng.empty()) return 1;
    return p->lrd.blk_rng ? 2 : 3;
}

// The chains per workgroup (1 | 2) of a dense HMC launch of `num_chains` chains
// of the program on the current device (host.h hmc_dense_chains, with the
// override the plan was made under); 0 when HMC launches do not take the dense
// route or take its one-wave kernel (a chain pair per wave); -1 on a null
// program or without a device.
extern "C" int32_t mc_program_hmc_dense_chains(const mc_program* p, int64_t num_chains) {
    if (!p) return -1;
    if (!hmc_dense_route(p) || p->lrd.S < 2) return 0;
    if (p->lrd.dense_chains) return p->lrd.dense_chains;
    const int cus = device_cus();
    return cus > 0 ? hmc_dense_chains(num_chains, cus, 0) : -1;
}

// Test hook: the rule itself, a pure function of the launch's chains, the
// device's CU count and the override (0: none).
extern "C" int32_t mc_debug_hmc_dense_chains(int64_t num_chains, int32_t cus, int32_t forced) {
    return hmc_dense_chains(num_chains, cus, forced);
}

// Test hook: the moment constants (c, R, Q, n) of the program-level lane plan
// (host table; LanePlan::mom), [S][kLrMaxSlots][64][4] floats.  Returns the
// number of floats, or a negative error code.
extern "C" int64_t mc_debug_lane_moments(const mc_program* p, float* out, int64_t n_out) {
    if (!p) return -(int64_t)fail(MC_ERR_INVALID, "program is NULL");
    if (!p->lr.ok) return -(int64_t)fail(MC_ERR_UNSUPPORTED, "the program has no lane plan");
    const int64_t n = (int64_t)p->lr.mom.size();
    if (out) {
        if (n_out < n) return -(int64_t)fail(MC_ERR_INVALID, "out holds %lld floats", (long long)n);
        std::copy(p->lr.mom.begin(), p->lr.mom.end(), out);
    }
    return n;
}

static int set_slices(mc_program* p, int32_t S) {
    const bool automatic = (S == 0);
    if (automatic) S = auto_slices(p);
    free_slices(p->sl);
    free_lanes(p->lr);
    p->note.clear();
    if (S <= 1) {
        // automatic: the lane-resident kernel with one slice when the program
        // qualifies (1.4-4.5x k_hmc on D = 2..100 models at 64-1024 chains,
        // scripts/bench_unsliced.py); an explicit 1 keeps k_hmc
        if (automatic && p->slice_kernel != 1) (void)plan_lanes1(p);
        return MC_OK;
    }
    SlicePlan P;
    SlPartition part;
    int rc = plan_slices(p, S, P, part);
    if (rc == MC_OK) {
        p->sl = P;  // host tables; geometry below needs them in place
        auto fit = [&]() {
            return sl_lds_bytes(p, 16) <= kSlLdsBudget ? 16
                 : (sl_lds_bytes(p, 8) <= kSlLdsBudget ? 8 : 0);
        };
        p->sl.nb_max = fit();
        if (p->sl.nb_max == 0)
            rc = fail(MC_ERR_UNSUPPORTED, "slice state (%d bytes) exceeds the LDS budget",
                      sl_lds_bytes(p, 8));
    }
    if (rc != MC_OK) {
        free_slices(p->sl);
        if (!automatic) return rc;
        p->note = "data slicing: " + g_last_error;
        return MC_OK;  // automatic: stay on the unsliced kernels
    }
    hipError_t e = upload_slices(p->sl);
    if (e != hipSuccess) {
        free_slices(p->sl);
        return upload_failed(e, "slice");
    }
    // the lane-resident layout of the same slices, when the program qualifies
    if (plan_lanes(p, part, p->lr) == MC_OK) {
        e = upload_lanes(p->lr);
        if (e != hipSuccess) {
            free_lanes(p->lr);
            free_slices(p->sl);
            return upload_failed(e, "slice");
        }
    } else {
        const std::string& why = decline_lanes(p);
        if (!interp_ok(p)) {  // the term interpreter has no transforms / affine locs
            free_slices(p->sl);
            if (!automatic)
                return fail(MC_ERR_UNSUPPORTED, "lane-resident kernel: %s (a program with "
                            "transformed operands or affine locs is sliced onto it only)",
                            why.c_str());
            return MC_OK;
        }
        if (automatic && program_elements(p) < 16384) {  // only worth it on the lanes kernel
            free_slices(p->sl);
            if (p->slice_kernel != 1) (void)plan_lanes1(p);
            return MC_OK;
        }
    }
    return MC_OK;
}

extern "C" int mc_program_set_slice_kernel(mc_program* p, int32_t kernel) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (kernel < 0 || kernel > 2) return fail(MC_ERR_INVALID, "slice kernel must be 0, 1 or 2");
    if (p->sl.S < 2) {
        // an unsliced program: 0 and 2 run it on the lane-resident kernel with
        // one slice (no exchange) — 0 when it qualifies, 2 or an error; 1 keeps
        // the chain-per-workgroup kernel (k_hmc)
        free_lanes(p->lr);
        if (kernel != 1) {
            const int rc = plan_lanes1(p);
            if (rc != MC_OK && kernel == 2) return rc;
        }
        p->slice_kernel = kernel;
        return MC_OK;
    }
    if (kernel == 2 && !p->lr.ok)
        return fail(MC_ERR_UNSUPPORTED, "lane-resident kernel: %s", p->lr.why.c_str());
    if (kernel == 1 && !interp_ok(p))
        return fail(MC_ERR_UNSUPPORTED, "the term interpreter does not run transformed operands "
                    "(mx.exp / mx.log), identity terms or affine locs");
    p->slice_kernel = kernel;
    return MC_OK;
}

extern "C" int32_t mc_program_slice_kernel(const mc_program* p) {
    if (!p) return -1;
    // expression terms on the lane layout run there only with their JIT-compiled
    // kernel: without it (off, or its compilation failed) the tape runs them
    if (p->lr.ok && p->lr.has_expr && p->slice_kernel != 1 &&
        (!jit_enabled() || !jit_error(p).empty()))
        return 0;
    if (p->sl.S < 2) return (p->lr.ok && p->lr.S == 1) ? 2 : 0;
    if (p->slice_kernel == 1 || !p->lr.ok) return 1;
    return 2;
}

extern "C" int32_t mc_program_lanes_fast(const mc_program* p) {
    if (!p) return -1;
    const int32_t k = mc_program_slice_kernel(p);
    return (k == 2 && p->lr.fast && lanes_fast_enabled()) ? 1 : 0;
}

extern "C" int32_t mc_program_lane_slots(const mc_program* p) {
    if (!p) return -1;
    return p->lr.ok ? p->lr.rs : 0;
}

extern "C" int32_t mc_program_lane_rep(const mc_program* p) {
    if (!p) return -1;
    return p->lr.ok ? p->lr.rep : 0;
}

extern "C" int32_t mc_program_lane_bundle(const mc_program* p) {
    if (!p) return -1;
    return p->lr.ok ? p->lr.bundle : 0;
}

extern "C" int32_t mc_program_num_slices(const mc_program* p) { return p ? p->sl.S : -1; }

extern "C" const char* mc_program_kernel_note(const mc_program* p) {
    if (!p) return "";
    const std::string je = jit_error(p);
    if (!je.empty()) {  // (the interpreter runs the expression terms)
        static thread_local std::string buf;
        buf = "expression JIT: compilation failed, the interpreter runs: " + je;
        return buf.c_str();
    }
    return (mc_program_slice_kernel(p) == 2) ? "" : p->note.c_str();
}

extern "C" int mc_program_create(const mc_term* terms, int32_t n_terms, int32_t n_params,
                                 float lp_const, const float* data, int64_t n_data,
                                 const int32_t* index, int64_t n_index, mc_program** out) {
    // the non-affine entry point ignores mc_term.affine (it was reserved0
    // before affine locs existed, and callers were free to leave it unset)
    if (n_terms < 0 || (n_terms > 0 && !terms)) return fail(MC_ERR_INVALID, "terms");
    std::vector<mc_term> t(terms, terms + n_terms);
    for (mc_term& x : t) x.affine = 0;
    return mc_program_create_affine(t.data(), n_terms, nullptr, 0, n_params, lp_const, data,
                                    n_data, index, n_index, out);
}

extern "C" int mc_program_create_affine(const mc_term* terms, int32_t n_terms,
                                        const mc_affine* affines, int32_t n_affines,
                                        int32_t n_params, float lp_const, const float* data,
                                        int64_t n_data, const int32_t* index, int64_t n_index,
                                        mc_program** out) {
    if (n_terms < 0 || (n_terms > 0 && !terms)) return fail(MC_ERR_INVALID, "bad term array");
    for (int32_t t = 0; t < n_terms; ++t)
        if (terms[t].dist == MC_DIST_EXPR)
            return fail(MC_ERR_INVALID, "term %d: expression terms need mc_program_create_expr", t);
    return mc_program_create_expr(terms, n_terms, affines, n_affines, nullptr, 0, nullptr, 0,
                                  n_params, lp_const, data, n_data, index, n_index, out);
}

// Validate and lay out one expression term (MC_DIST_EXPR): its nodes are
// appended to `gnodes` (dt.expr_base ..), a non-injective gather orders the
// term into the segment-tiled layout (build_segments_ops, whole runs), and
// vector leaves with overlapping parameter ranges deposit in different passes.
static int build_expr_term(int32_t t, const mc_term& src, const mc_expr* exprs, int32_t n_exprs,
                           const mc_expr_node* nodes, int32_t n_nodes, int32_t n_params,
                           int64_t n_data, int64_t n_index, std::vector<float>& dpool,
                           std::vector<int32_t>& ipool, std::vector<DevExprNode>& gnodes,
                           std::vector<DevExprNode>& rnodes, DevTerm& dt, int wpc) {
    // (leaf ranges are checked against the caller's pools, n_data / n_index:
    // dpool / ipool already hold the library's own tiled copies of earlier terms)
    if (src.affine < 1 || src.affine > n_exprs)
        return fail(MC_ERR_INVALID, "term %d: expression index %d out of range", t, src.affine);
    if (src.value.kind != MC_OP_NONE || src.loc.kind != MC_OP_NONE || src.scale.kind != MC_OP_NONE)
        return fail(MC_ERR_INVALID, "term %d: an expression term takes no value / loc / scale", t);
    const mc_expr& ex = exprs[src.affine - 1];
    if (ex.count < 1 || ex.count > kExMaxNodes)
        return fail(MC_ERR_UNSUPPORTED, "term %d: an expression holds 1 .. %d nodes (got %d)", t,
                    kExMaxNodes, ex.count);
    if (ex.first < 0 || (int64_t)ex.first + ex.count > n_nodes)
        return fail(MC_ERR_INVALID, "term %d: expression nodes out of range", t);
    const int64_t n = src.n;
    const int nn = ex.count;
    std::vector<DevExprNode> en(nn);
    std::vector<int> nonunique;  // non-injective gather leaves
    for (int k = 0; k < nn; ++k) {
        const mc_expr_node& s = nodes[ex.first + k];
        DevExprNode& d = en[k];
        std::memset(&d, 0, sizeof(d));
        d.op = s.op;
        d.a = s.a;
        d.b = s.b;
        d.c = s.c;
        d.leaf.kind = MC_OP_NONE;
        d.leaf.slot = -1;
        if (s.op < MC_EX_LEAF || s.op > MC_EX_HALF_STUDENT_T_LP || s.op == 28 ||
            s.op == 31)  // (28, 31: not assigned)
            return fail(MC_ERR_INVALID, "term %d node %d: unknown op %d", t, k, s.op);
        if (s.op == MC_EX_LEAF) {
            const mc_operand& o = s.leaf;
            d.leaf.kind = o.kind;
            d.leaf.poff = o.param_offset;
            d.leaf.pool = o.pool_offset;
            d.leaf.cval = o.value;
            d.leaf.unique = 1;
            d.leaf.xf = MC_XF_NONE;
            if (o.transform != MC_XF_NONE)
                return fail(MC_ERR_INVALID, "term %d node %d: expression leaves take no transform "
                            "(exp / log are nodes)", t, k);
            switch (o.kind) {
                case MC_OP_CONST:
                    break;
                case MC_OP_PSCALAR:
                    if (o.param_offset < 0 || o.param_offset >= n_params)
                        return fail(MC_ERR_INVALID, "term %d node %d: param %d out of range", t, k,
                                    o.param_offset);
                    break;
                case MC_OP_DATA:
                    if (o.pool_offset < 0 || o.pool_offset + n > n_data)
                        return fail(MC_ERR_INVALID, "term %d node %d: data range out of pool", t, k);
                    break;
                case MC_OP_PVEC:
                    if (o.param_offset < 0 || (int64_t)o.param_offset + n > n_params)
                        return fail(MC_ERR_INVALID, "term %d node %d: param slice out of range", t,
                                    k);
                    break;
                case MC_OP_GATHER: {
                    if (o.pool_offset < 0 || o.pool_offset + n > n_index)
                        return fail(MC_ERR_INVALID, "term %d node %d: index range out of pool", t,
                                    k);
                    std::vector<int32_t> v(ipool.begin() + o.pool_offset,
                                           ipool.begin() + o.pool_offset + n);
                    for (int32_t x : v)
                        if (x < 0 || (int64_t)o.param_offset + x >= n_params)
                            return fail(MC_ERR_INVALID,
                                        "term %d node %d: gather index %d out of range", t, k, x);
                    std::sort(v.begin(), v.end());
                    d.leaf.unique = (std::adjacent_find(v.begin(), v.end()) == v.end()) ? 1 : 0;
                    if (!d.leaf.unique) nonunique.push_back(k);
                    break;
                }
                default:
                    return fail(MC_ERR_INVALID, "term %d node %d: bad leaf kind %d", t, k, o.kind);
            }
            d.a = d.b = d.c = -1;
            continue;
        }
        // arity: which arguments the op reads
        bool ua = true, ub = false, uc = false;
        switch (s.op) {
            case MC_EX_ADD: case MC_EX_SUB: case MC_EX_MUL: case MC_EX_DIV: case MC_EX_POW:
            case MC_EX_GT: case MC_EX_GE: case MC_EX_LT: case MC_EX_LE:
            case MC_EX_BERNOULLI_LOGIT_LP: case MC_EX_POISSON_LOG_LP: case MC_EX_LOGADDEXP:
                ub = true;
                break;
            case MC_EX_NORMAL_LP: case MC_EX_WHERE: case MC_EX_GAMMA_LP: case MC_EX_BETA_LP:
            case MC_EX_BINOMIAL_LOGIT_LP: case MC_EX_PICK: case MC_EX_STUDENT_T_LP:
                ub = uc = true;
                break;
            case MC_EX_HALFNORMAL_LP: case MC_EX_EXPONENTIAL_LP: case MC_EX_HALF_STUDENT_T_LP:
                uc = true;
                break;
            default:
                break;
        }
        auto arg_ok = [&](int x, bool used) { return used ? (x >= 0 && x < k) : x == -1; };
        if (!arg_ok(s.a, ua) || !arg_ok(s.b, ub) || !arg_ok(s.c, uc))
            return fail(MC_ERR_INVALID, "term %d node %d: bad arguments (%d, %d, %d) for op %d", t,
                        k, s.a, s.b, s.c, s.op);
        if (s.op == MC_EX_WHERE &&
            !(en[s.a].op == MC_EX_LEAF &&
              (en[s.a].leaf.kind == MC_OP_CONST || en[s.a].leaf.kind == MC_OP_DATA)) &&
            !(en[s.a].op >= MC_EX_GT && en[s.a].op <= MC_EX_LE))
            return fail(MC_ERR_UNSUPPORTED, "term %d node %d: a where mask must be data, a "
                        "constant or a comparison", t, k);
        // the count nodes' y (and the Binomial's n): data or a constant
        if (s.op >= MC_EX_BERNOULLI_LOGIT_LP && s.op <= MC_EX_POISSON_LOG_LP) {
            auto fixed = [&](int x) {
                return en[x].op == MC_EX_LEAF &&
                       (en[x].leaf.kind == MC_OP_CONST || en[x].leaf.kind == MC_OP_DATA);
            };
            static const char* const names[] = {"Bernoulli", "Binomial", "Poisson"};
            const char* nm = names[s.op - MC_EX_BERNOULLI_LOGIT_LP];
            if (!fixed(s.a))
                return fail(MC_ERR_UNSUPPORTED, "term %d node %d: the %s node's count y must be "
                            "data or a constant", t, k, nm);
            if (s.op == MC_EX_BINOMIAL_LOGIT_LP && !fixed(s.b))
                return fail(MC_ERR_UNSUPPORTED, "term %d node %d: the Binomial node's total n "
                            "must be data or a constant", t, k);
        }
        // MC_EX_PICK: the label y is data or a constant, the class the node's own
        // constant (the one non-leaf node that reads its leaf field)
        if (s.op == MC_EX_PICK) {
            if (!(en[s.a].op == MC_EX_LEAF &&
                  (en[s.a].leaf.kind == MC_OP_CONST || en[s.a].leaf.kind == MC_OP_DATA)))
                return fail(MC_ERR_UNSUPPORTED, "term %d node %d: the pick node's label y must be "
                            "data or a constant", t, k);
            d.leaf.cval = s.leaf.value;
        }
        // the Student-t nodes: nu is the node's own constant, finite and positive
        if (s.op == MC_EX_STUDENT_T_LP || s.op == MC_EX_HALF_STUDENT_T_LP) {
            const float nu = s.leaf.value;
            if (!(nu > 0.0f) || !(nu < __builtin_inff()))
                return fail(MC_ERR_INVALID, "term %d node %d: the Student-t node's degrees of "
                            "freedom must be finite and positive (got %g)", t, k, (double)nu);
            d.leaf.cval = nu;
        }
        // the distribution nodes' f32 normalisers (elem_normal / elem_halfnormal)
        if (s.op == MC_EX_NORMAL_LP) d.leaf.cval = dist_c0(MC_DIST_NORMAL);
        if (s.op == MC_EX_HALFNORMAL_LP) d.leaf.cval = dist_c0(MC_DIST_HALFNORMAL);
    }
    dt.dist = MC_DIST_EXPR;
    dt.n = n;
    dt.weight = src.weight;
    dt.affine = 0;
    dt.wave_task = -1;
    dt.primary = -1;
    // a non-injective gather: every such leaf through the same index values
    int64_t prim_pool = -1;
    if (!nonunique.empty()) {
        const int64_t p0 = en[nonunique[0]].leaf.pool;
        for (size_t r = 0; r < nonunique.size(); ++r) {
            const int k = nonunique[r];
            const int64_t pk = en[k].leaf.pool;
            if (pk != p0 && !std::equal(ipool.begin() + pk, ipool.begin() + pk + n,
                                        ipool.begin() + p0))
                return fail(MC_ERR_UNSUPPORTED, "term %d: an expression gathers through two "
                            "different non-injective index arrays", t);
            en[k].prim = 1 + (int)r;  // 1 + its row of split-run partials
        }
        prim_pool = p0;
        dt.primary = 0;  // (a flag for expression terms: segmented)
    }
    // passes: accumulating vector leaves with overlapping parameter ranges
    // deposit in different sweeps (ranges before any tiling)
    {
        std::vector<std::vector<std::pair<int64_t, int64_t>>> pr;  // per pass
        for (int k = 0; k < nn; ++k) {
            DevExprNode& d = en[k];
            if (d.op != MC_EX_LEAF || !is_acc_vec(d.leaf.kind)) continue;
            int64_t lo, hi;
            if (d.leaf.kind == MC_OP_PVEC) {
                lo = d.leaf.poff;
                hi = d.leaf.poff + n - 1;
            } else {
                const int32_t* ix = ipool.data() + d.leaf.pool;
                lo = d.leaf.poff + *std::min_element(ix, ix + n);
                hi = d.leaf.poff + *std::max_element(ix, ix + n);
            }
            int placed = -1;
            for (size_t ps = 0; ps < pr.size() && placed < 0; ++ps) {
                bool clash = false;
                for (auto& r : pr[ps])
                    if (!(hi < r.first || r.second < lo)) clash = true;
                if (!clash) placed = (int)ps;
            }
            if (placed < 0) {
                placed = (int)pr.size();
                pr.emplace_back();
            }
            pr[placed].push_back({lo, hi});
            d.pass = placed;
        }
        if (pr.size() > 16)
            return fail(MC_ERR_UNSUPPORTED, "term %d: more than 16 overlapping vector leaves", t);
        dt.npass = std::max<int>(1, (int)pr.size());
    }
    // (the nodes as validated: the slice / lane planners tile a gathered term
    // themselves, from the caller's pools in element order)
    rnodes.insert(rnodes.end(), en.begin(), en.end());
    if (prim_pool >= 0) {
        // order the term by the index (stable), then tile it by runs
        bool sorted = true;
        for (int64_t i = 1; i < n && sorted; ++i) sorted = ipool[prim_pool + i - 1] <= ipool[prim_pool + i];
        if (!sorted) {
            std::vector<int64_t> perm(n);
            std::iota(perm.begin(), perm.end(), 0);
            std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) {
                return ipool[prim_pool + x] < ipool[prim_pool + y];
            });
            std::map<std::pair<int, int64_t>, int64_t> moved;  // (kind, old pool) -> new pool
            for (int k = 0; k < nn; ++k) {
                DevOperand& d = en[k].leaf;
                if (en[k].op != MC_EX_LEAF) continue;
                if (d.kind == MC_OP_DATA || d.kind == MC_OP_GATHER) {
                    const auto key = std::make_pair((int)d.kind, d.pool);
                    auto it = moved.find(key);
                    if (it != moved.end()) {
                        d.pool = it->second;
                        continue;
                    }
                    int64_t base;
                    if (d.kind == MC_OP_DATA) {
                        base = (int64_t)dpool.size();
                        for (int64_t i = 0; i < n; ++i) dpool.push_back(dpool[d.pool + perm[i]]);
                    } else {
                        base = (int64_t)ipool.size();
                        for (int64_t i = 0; i < n; ++i) ipool.push_back(ipool[d.pool + perm[i]]);
                    }
                    moved[key] = base;
                    d.pool = base;
                } else if (d.kind == MC_OP_PVEC) {
                    const int64_t base = (int64_t)ipool.size();
                    for (int64_t i = 0; i < n; ++i) ipool.push_back((int32_t)perm[i]);
                    d.kind = MC_OP_GATHER;
                    d.pool = base;
                    d.unique = 1;
                }
            }
            prim_pool = en[nonunique[0]].leaf.pool;
        }
        std::vector<DevOperand*> others;
        for (int k = 0; k < nn; ++k)
            if (en[k].op == MC_EX_LEAF && !en[k].prim && is_vec_kind(en[k].leaf.kind))
                others.push_back(&en[k].leaf);
        // long runs split as the fused terms' are, with one partial row per
        // gathered leaf (nprim rows of <= 2 tsplit virtual segments: 4T floats)
        const int T = 64 * wpc;
        const int nprim = (int)nonunique.size();
        const int64_t tsplit = std::max<int64_t>(1, std::min<int64_t>(T, 2 * T / nprim));
        const int rc = build_segments_ops(dt, prim_pool, others, tsplit, nprim, dpool, ipool, T);
        if (rc) return rc;
    }
    dt.expr_base = (int32_t)gnodes.size();
    dt.expr_n = nn;
    gnodes.insert(gnodes.end(), en.begin(), en.end());
    return MC_OK;
}

// The sampler descriptor of an expression term (internal.h PwSampler) from its
// validated nodes.
static PwSampler expr_sampler(const DevExprNode* N, int nn) {
    PwSampler sd = kPwNoSampler;
    auto student_node = [](int op) {
        return op == MC_EX_STUDENT_T_LP || op == MC_EX_HALF_STUDENT_T_LP;
    };
    auto count_node = [&](int op) {  // (a node with a sampler: count or Student-t)
        return (op >= MC_EX_BERNOULLI_LOGIT_LP && op <= MC_EX_POISSON_LOG_LP) ||
               student_node(op);
    };
    auto fixed_leaf = [&](int k) {
        return N[k].op == MC_EX_LEAF &&
               (N[k].leaf.kind == MC_OP_CONST || N[k].leaf.kind == MC_OP_DATA);
    };
    int node = -1;
    const DevExprNode& r = N[nn - 1];
    if (count_node(r.op)) node = nn - 1;
    else if (r.op == MC_EX_ADD && count_node(N[r.a].op) && fixed_leaf(r.b)) node = r.a;
    else if (r.op == MC_EX_ADD && count_node(N[r.b].op) && fixed_leaf(r.a)) node = r.b;
    if (node < 0) return sd;
    const DevExprNode& d = N[node];
    if (student_node(d.op)) {  // y the value, tot the loc (-1: half form), eta the scale
        sd.kind = d.op == MC_EX_STUDENT_T_LP ? PW_SAMPLER_STUDENT_T : PW_SAMPLER_HALF_STUDENT_T;
        sd.node = node;
        sd.y = d.a;
        sd.tot = d.b;
        sd.eta = d.c;
        sd.nu = d.leaf.cval;
        return sd;
    }
    sd.kind = d.op - MC_EX_BERNOULLI_LOGIT_LP;  // mc_discrete_kind, in op order
    sd.node = node;
    sd.y = d.a;
    sd.tot = d.op == MC_EX_BINOMIAL_LOGIT_LP ? d.b : -1;
    sd.eta = d.op == MC_EX_BINOMIAL_LOGIT_LP ? d.c : d.b;
    return sd;
}

extern "C" int mc_program_create_expr(const mc_term* terms, int32_t n_terms,
                                      const mc_affine* affines, int32_t n_affines,
                                      const mc_expr* exprs, int32_t n_exprs,
                                      const mc_expr_node* nodes, int32_t n_nodes,
                                      int32_t n_params, float lp_const, const float* data,
                                      int64_t n_data, const int32_t* index, int64_t n_index,
                                      mc_program** out) {
    if (!out) return fail(MC_ERR_INVALID, "out is NULL");
    if (n_affines < 0 || (n_affines > 0 && !affines))
        return fail(MC_ERR_INVALID, "bad affine array");
    if (n_exprs < 0 || (n_exprs > 0 && !exprs)) return fail(MC_ERR_INVALID, "bad expression array");
    if (n_nodes < 0 || (n_nodes > 0 && !nodes)) return fail(MC_ERR_INVALID, "bad node array");
    *out = nullptr;
    if (n_params <= 0) return fail(MC_ERR_INVALID, "n_params must be positive (got %d)", n_params);
    if (n_terms < 0 || (n_terms > 0 && !terms)) return fail(MC_ERR_INVALID, "bad term array");
    if (n_data < 0 || (n_data > 0 && !data)) return fail(MC_ERR_INVALID, "bad data pool");
    if (n_index < 0 || (n_index > 0 && !index)) return fail(MC_ERR_INVALID, "bad index pool");

    std::vector<float> dpool(data, data + n_data);
    std::vector<int32_t> ipool(index, index + n_index);
    std::vector<DevTerm> dts, raws, pws;  // pws: the pointwise view (host.h pw_terms)
    std::vector<PwSampler> pwsd;          // and its samplers (host.h pw_samplers)
    std::vector<DevExprNode> gnodes, rnodes;
    int64_t max_n = 0;
    for (int32_t t = 0; t < n_terms; ++t) max_n = std::max<int64_t>(max_n, terms[t].n);
    const int wpc = choose_wpc(max_n);

    for (int32_t t = 0; t < n_terms; ++t) {
        const mc_term& src = terms[t];
        if (src.dist < MC_DIST_NORMAL || src.dist > MC_DIST_EXPR)
            return fail(MC_ERR_INVALID, "term %d: unknown distribution %d", t, src.dist);
        if (src.n < 1) return fail(MC_ERR_INVALID, "term %d: n must be >= 1", t);
        const int64_t n = src.n;
        DevTerm dt;
        std::memset(&dt, 0, sizeof(dt));
        if (src.dist == MC_DIST_EXPR) {
            const int rc = build_expr_term(t, src, exprs, n_exprs, nodes, n_nodes, n_params,
                                           n_data, n_index, dpool, ipool, gnodes, rnodes, dt,
                                           wpc);
            if (rc) return rc;
            raws.push_back(dt);
            pws.push_back(dt);
            pwsd.push_back(expr_sampler(rnodes.data() + dt.expr_base, dt.expr_n));
            dts.push_back(dt);
            continue;
        }
        dt.dist = src.dist;
        dt.n = n;
        dt.weight = src.weight;
        dt.c0 = dist_c0(src.dist);
        const mc_operand* ops[5] = {&src.value, &src.loc, &src.scale, nullptr, nullptr};
        int nops = 3;
        if (src.affine != 0) {
            if (src.affine < 0 || src.affine > n_affines)
                return fail(MC_ERR_INVALID, "term %d: affine index %d out of range", t,
                            src.affine);
            if (src.dist != MC_DIST_NORMAL)
                return fail(MC_ERR_UNSUPPORTED, "term %d: an affine loc needs a Normal term", t);
            const mc_affine& af = affines[src.affine - 1];
            if (af.slope.kind != MC_OP_CONST && af.slope.kind != MC_OP_PSCALAR)
                return fail(MC_ERR_UNSUPPORTED, "term %d: affine slope must be a constant or a "
                            "scalar parameter", t);
            if (af.x.kind != MC_OP_DATA && af.x.kind != MC_OP_PVEC && af.x.kind != MC_OP_GATHER)
                return fail(MC_ERR_UNSUPPORTED, "term %d: affine x must be data, a parameter "
                            "vector or a gather", t);
            ops[3] = &af.slope;
            ops[4] = &af.x;
            nops = 5;
            dt.affine = 1;
        }
        for (int a = 0; a < nops; ++a) {
            const mc_operand& o = *ops[a];
            DevOperand& d = a < 3 ? dt.op[a] : (a == 3 ? dt.ab : dt.ax);
            d.kind = o.kind;
            d.poff = o.param_offset;
            d.pool = o.pool_offset;
            d.cval = o.value;
            d.unique = 1;
            d.xf = o.transform;
            if (o.transform < MC_XF_NONE || o.transform > MC_XF_LOG)
                return fail(MC_ERR_INVALID, "term %d op %d: unknown transform %d", t, a,
                            o.transform);
            if (o.transform != MC_XF_NONE && o.kind != MC_OP_PSCALAR && o.kind != MC_OP_PVEC &&
                o.kind != MC_OP_GATHER)
                return fail(MC_ERR_INVALID, "term %d op %d: a transform applies to parameter "
                            "operands only", t, a);
            const bool need =
                !(a == 1 && (src.dist == MC_DIST_HALFNORMAL || src.dist == MC_DIST_EXPONENTIAL)) &&
                !(src.dist == MC_DIST_IDENTITY && (a == 1 || a == 2));
            if (!need) {
                if (o.kind != MC_OP_NONE && o.kind != MC_OP_CONST)
                    return fail(MC_ERR_INVALID, "term %d: %s takes no %s operand", t,
                                src.dist == MC_DIST_HALFNORMAL
                                    ? "HalfNormal"
                                    : (src.dist == MC_DIST_EXPONENTIAL ? "Exponential"
                                                                       : "an identity term"),
                                a == 1 ? "loc" : "scale");
                d.kind = MC_OP_NONE;
                d.xf = MC_XF_NONE;
                continue;
            }
            switch (o.kind) {
                case MC_OP_CONST:
                    break;
                case MC_OP_PSCALAR:
                    if (o.param_offset < 0 || o.param_offset >= n_params)
                        return fail(MC_ERR_INVALID, "term %d op %d: param %d out of range", t, a,
                                    o.param_offset);
                    break;
                case MC_OP_DATA:
                    if (o.pool_offset < 0 || o.pool_offset + n > n_data)
                        return fail(MC_ERR_INVALID, "term %d op %d: data range out of pool", t, a);
                    break;
                case MC_OP_PVEC:
                    if (o.param_offset < 0 || (int64_t)o.param_offset + n > n_params)
                        return fail(MC_ERR_INVALID, "term %d op %d: param slice out of range", t,
                                    a);
                    break;
                case MC_OP_GATHER: {
                    if (o.pool_offset < 0 || o.pool_offset + n > n_index)
                        return fail(MC_ERR_INVALID, "term %d op %d: index range out of pool", t,
                                    a);
                    std::vector<int32_t> v(ipool.begin() + o.pool_offset,
                                           ipool.begin() + o.pool_offset + n);
                    for (int32_t x : v)
                        if (x < 0 || (int64_t)o.param_offset + x >= n_params)
                            return fail(MC_ERR_INVALID,
                                        "term %d op %d: gather index %d out of range", t, a, x);
                    std::sort(v.begin(), v.end());
                    d.unique = (std::adjacent_find(v.begin(), v.end()) == v.end()) ? 1 : 0;
                    break;
                }
                default:
                    return fail(MC_ERR_INVALID, "term %d op %d: bad operand kind %d", t, a,
                                o.kind);
            }
        }
        if (dt.affine) {
            // a non-injective gather only as the loc itself (alpha[group] + b * x,
            // the segmented path), with a data x
            for (int k = 0; k < 5; ++k) {
                const DevOperand* d = k < 3 ? &dt.op[k] : (k == 3 ? &dt.ab : &dt.ax);
                if (d->kind == MC_OP_GATHER && !d->unique && !(k == 1 && dt.ax.kind == MC_OP_DATA))
                    return fail(MC_ERR_UNSUPPORTED, "term %d: an affine-loc term gathers through "
                                "a non-injective index only in its loc, with a data x", t);
            }
            if (dt.op[1].kind == MC_OP_NONE)
                return fail(MC_ERR_INVALID, "term %d: affine loc without a loc operand", t);
        }
        // the non-injective gather, if any, orders the term
        int primary = -1;
        for (int a = 0; a < 3; ++a) {
            if (dt.op[a].kind == MC_OP_GATHER && !dt.op[a].unique) {
                if (primary >= 0)
                    return fail(MC_ERR_UNSUPPORTED,
                                "term %d gathers through two non-injective index arrays", t);
                primary = a;
            }
        }
        dt.primary = primary;
        DevTerm pwt = dt;  // the caller's element order and pools
        if (primary >= 0) {
            const int64_t ip = dt.op[primary].pool;
            bool sorted = true;
            for (int64_t i = 1; i < n && sorted; ++i) sorted = ipool[ip + i - 1] <= ipool[ip + i];
            if (!sorted) {
                std::vector<int64_t> perm(n);
                std::iota(perm.begin(), perm.end(), 0);
                std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) {
                    return ipool[ip + x] < ipool[ip + y];
                });
                for (int a = 0; a < 4; ++a) {
                    if (a == 3 && !dt.affine) break;
                    DevOperand& d = a < 3 ? dt.op[a] : dt.ax;  // (an affine x is data)
                    if (d.kind == MC_OP_DATA) {
                        const int64_t base = (int64_t)dpool.size();
                        for (int64_t i = 0; i < n; ++i) dpool.push_back(dpool[d.pool + perm[i]]);
                        d.pool = base;
                    } else if (d.kind == MC_OP_GATHER) {
                        const int64_t base = (int64_t)ipool.size();
                        for (int64_t i = 0; i < n; ++i) ipool.push_back(ipool[d.pool + perm[i]]);
                        d.pool = base;
                    } else if (d.kind == MC_OP_PVEC) {
                        const int64_t base = (int64_t)ipool.size();
                        for (int64_t i = 0; i < n; ++i) ipool.push_back((int32_t)perm[i]);
                        d.kind = MC_OP_GATHER;
                        d.pool = base;
                        d.unique = 1;
                    }
                }
            }
        }
        // constant-shape normalisers (every layout reads them: the sliced
        // planners copy them from the validated terms)
        dt.clogs = (dt.op[2].kind == MC_OP_CONST) ? (float)std::log((double)dt.op[2].cval) : 0.0f;
        dt.clg = 0.0f;
        if ((dt.dist == MC_DIST_GAMMA && dt.op[1].kind == MC_OP_CONST) ||
            (dt.dist == MC_DIST_BETA && dt.op[1].kind == MC_OP_CONST &&
             dt.op[2].kind == MC_OP_CONST))
            dt.clg = lgamma_norm(dt.dist, dt.op[1].cval, dt.op[2].cval);
        raws.push_back(dt);
        pwt.clogs = dt.clogs;
        pwt.clg = dt.clg;
        pws.push_back(pwt);
        pwsd.push_back(kPwNoSampler);
        // pass planning: accumulating vector operands with overlapping parameter
        // ranges go to different sweeps
        int64_t lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            const DevOperand& d = dt.op[a];
            lo[a] = hi[a] = -1;
            if (d.kind == MC_OP_PVEC) {
                lo[a] = d.poff;
                hi[a] = d.poff + n - 1;
            } else if (d.kind == MC_OP_GATHER) {
                int32_t mn = ipool[d.pool], mx = ipool[d.pool];
                for (int64_t i = 1; i < n; ++i) {
                    mn = std::min(mn, ipool[d.pool + i]);
                    mx = std::max(mx, ipool[d.pool + i]);
                }
                lo[a] = d.poff + mn;
                hi[a] = d.poff + mx;
            }
        }
        uint32_t masks[3] = {PASS_LP, 0, 0};
        int npass = 1;
        for (int a = 0; a < 3; ++a) {
            const uint32_t bit = 1u << a;
            if (dt.op[a].kind == MC_OP_PSCALAR) {
                masks[0] |= bit;
                continue;
            }
            if (!is_acc_vec(dt.op[a].kind)) continue;
            int placed = -1;
            for (int ps = 0; ps < npass && placed < 0; ++ps) {
                bool clash = false;
                for (int b = 0; b < a; ++b)
                    if ((masks[ps] & (1u << b)) && is_acc_vec(dt.op[b].kind) &&
                        !(hi[a] < lo[b] || hi[b] < lo[a]))
                        clash = true;
                if (!clash) placed = ps;
            }
            if (placed < 0) placed = npass++;
            masks[placed] |= bit;
        }
        if (dt.affine) {
            // the slope's and x's cotangents accumulate in the loc's sweep:
            // x must not overlap another accumulating operand of the term
            const bool acc = dt.ab.kind == MC_OP_PSCALAR || is_acc_vec(dt.ax.kind);
            bool has_loc = false;
            for (int ps = 0; ps < npass; ++ps) has_loc |= (masks[ps] & PASS_LOC) != 0;
            if (acc && !has_loc) masks[0] |= PASS_LOC;
            if (is_acc_vec(dt.ax.kind)) {
                int64_t xl, xh;
                if (dt.ax.kind == MC_OP_PVEC) {
                    xl = dt.ax.poff;
                    xh = dt.ax.poff + n - 1;
                } else {
                    int32_t mn = ipool[dt.ax.pool], mx = ipool[dt.ax.pool];
                    for (int64_t i = 1; i < n; ++i) {
                        mn = std::min(mn, ipool[dt.ax.pool + i]);
                        mx = std::max(mx, ipool[dt.ax.pool + i]);
                    }
                    xl = dt.ax.poff + mn;
                    xh = dt.ax.poff + mx;
                }
                for (int a = 0; a < 3; ++a)
                    if (is_acc_vec(dt.op[a].kind) && !(xh < lo[a] || hi[a] < xl))
                        return fail(MC_ERR_UNSUPPORTED, "term %d: the affine x overlaps operand "
                                    "%d's parameters", t, a);
            }
        }
        dt.npass = npass;
        dt.pass_masks = masks[0] | (masks[1] << 4) | (masks[2] << 8);
        dt.wave_task = -1;
        dt.prim_poff = primary >= 0 ? dt.op[primary].poff : 0;
        if (primary >= 0) {
            const int rc = build_segments(dt, dpool, ipool, 64 * wpc);
            if (rc) return rc;
        }
        dts.push_back(dt);
    }

    // broadcast-parameter cotangent slots and their fixed-order finalize list
    int32_t nslot = 0;
    std::vector<std::pair<int32_t, int32_t>> uses;  // (param, slot)
    for (DevTerm& dt : dts) {
        for (int a = 0; a < 3; ++a)
            if (dt.op[a].kind == MC_OP_PSCALAR) {
                dt.op[a].slot = nslot;
                uses.push_back({dt.op[a].poff, nslot});
                ++nslot;
            }
        if (dt.affine && dt.ab.kind == MC_OP_PSCALAR) {
            dt.ab.slot = nslot;
            uses.push_back({dt.ab.poff, nslot});
            ++nslot;
        }
        if (dt.dist == MC_DIST_EXPR)
            for (int k = 0; k < dt.expr_n; ++k) {
                DevExprNode& d = gnodes[dt.expr_base + k];
                if (d.op != MC_EX_LEAF || d.leaf.kind != MC_OP_PSCALAR) continue;
                d.leaf.slot = nslot;
                uses.push_back({d.leaf.poff, nslot});
                ++nslot;
            }
    }
    std::stable_sort(uses.begin(), uses.end(),
                     [](const std::pair<int32_t, int32_t>& x,
                        const std::pair<int32_t, int32_t>& y) { return x.first < y.first; });
    std::vector<int32_t> fin_hdr, fin_ids;
    for (size_t i = 0; i < uses.size();) {
        size_t j = i;
        while (j < uses.size() && uses[j].first == uses[i].first) ++j;
        fin_hdr.push_back(uses[i].first);
        fin_hdr.push_back((int32_t)fin_ids.size());
        fin_hdr.push_back((int32_t)(j - i));
        for (size_t k = i; k < j; ++k) fin_ids.push_back(uses[k].second);
        i = j;
    }
    const int64_t sfin_base = (int64_t)ipool.size();
    ipool.push_back((int32_t)(fin_hdr.size() / 3));
    ipool.insert(ipool.end(), fin_hdr.begin(), fin_hdr.end());
    ipool.insert(ipool.end(), fin_ids.begin(), fin_ids.end());
    // small terms whose only cotangents are broadcast parameters run as wave
    // tasks: one wave each, round robin, concurrently with the other waves
    {
        int next = 0;
        for (DevTerm& dt : dts) {
            bool vec_param = false;
            for (int a = 0; a < 3; ++a)
                if (dt.op[a].kind == MC_OP_PVEC || dt.op[a].kind == MC_OP_GATHER) vec_param = true;
            if (dt.affine && (dt.ax.kind == MC_OP_PVEC || dt.ax.kind == MC_OP_GATHER))
                vec_param = true;
            if (dt.dist == MC_DIST_EXPR)
                for (int k = 0; k < dt.expr_n; ++k)
                    if (gnodes[dt.expr_base + k].op == MC_EX_LEAF &&
                        is_acc_vec(gnodes[dt.expr_base + k].leaf.kind))
                        vec_param = true;
            if (dt.primary < 0 && dt.npass == 1 && dt.n <= 64 && !vec_param)
                dt.wave_task = (next++) % wpc;
        }
    }
    // evaluate all-wave terms first and the wave tasks last: a wave task only
    // writes its own cotangent slots, so its position is free, and at the end
    // it overlaps the other waves' share of the last all-wave term
    std::stable_partition(dts.begin(), dts.end(),
                          [](const DevTerm& dt) { return dt.wave_task < 0; });
    // barriers between terms whose gradient writes overlap (vector operands)
    {
        std::vector<std::pair<int64_t, int64_t>> open_ranges;
        for (DevTerm& dt : dts) {
            std::vector<std::pair<int64_t, int64_t>> mine;
            if (dt.dist == MC_DIST_EXPR)
                for (int k = 0; k < dt.expr_n; ++k) {
                    const DevExprNode& d = gnodes[dt.expr_base + k];
                    if (d.op != MC_EX_LEAF) continue;
                    if (d.leaf.kind == MC_OP_PVEC)
                        mine.push_back({d.leaf.poff, d.leaf.poff + dt.n - 1});
                    else if (d.leaf.kind == MC_OP_GATHER)
                        mine.push_back({0, (int64_t)n_params - 1});
                }
            for (int a = 0; a < 4; ++a) {
                if (a == 3 && !dt.affine) break;
                const DevOperand& d = a < 3 ? dt.op[a] : dt.ax;
                if (d.kind == MC_OP_PVEC) {
                    mine.push_back({d.poff, d.poff + dt.n - 1});
                } else if (d.kind == MC_OP_GATHER) {
                    // conservative: the whole parameter vector
                    mine.push_back({0, (int64_t)n_params - 1});
                }
            }
            bool clash = false;
            for (auto& r : mine)
                for (auto& o : open_ranges)
                    if (!(r.second < o.first || o.second < r.first)) clash = true;
            dt.sync_before = clash ? 1 : 0;
            if (clash) open_ranges.clear();
            open_ranges.insert(open_ranges.end(), mine.begin(), mine.end());
        }
    }

    // expression leaves address the pools with 32-bit offsets (eval.h reads
    // them into lanes): every offset, tiled copies included, lies below the
    // pools' final sizes, so bounding those bounds them all
    if (!gnodes.empty() && (dpool.size() > (size_t)INT32_MAX || ipool.size() > (size_t)INT32_MAX))
        return fail(MC_ERR_UNSUPPORTED,
                    "expression terms: the data / index pools (%zu / %zu elements) exceed the "
                    "2^31 elements their 32-bit leaf offsets address", dpool.size(), ipool.size());
    mc_program* p = new mc_program();
    p->D = n_params;
    p->nslots = nslot + 1;
    p->sfin_base = sfin_base;
    p->lp_const = lp_const;
    p->max_n = max_n;
    p->wpc = wpc;
    p->terms = dts;
    p->raw = raws;
    p->nodes = gnodes;
    p->rnodes = rnodes;
    p->pw_terms = pws;
    p->pw_samplers = pwsd;
    p->pw_n_data = n_data;
    p->pw_n_index = n_index;
    p->ex = !gnodes.empty();
    p->h_data = dpool;
    p->h_index = ipool;
    if (g_program_host_only) {  // test hook: the host tables only (no device)
        p->host_only = true;
        *out = p;
        return MC_OK;
    }
    hipError_t e = hipSuccess;
    if (!dts.empty()) e = upload(&p->d_terms, dts);
    if (e == hipSuccess && !gnodes.empty()) e = upload(&p->d_nodes, gnodes);
    if (e == hipSuccess && !dpool.empty()) e = upload(&p->d_data, dpool);
    if (e == hipSuccess && !ipool.empty()) e = upload(&p->d_index, ipool);
    if (e != hipSuccess) {
        mc_program_destroy(p);
        return upload_failed(e, "program");
    }
    {
        const int rc = mc_program_set_slices(p, 0);
        if (rc != MC_OK) {
            mc_program_destroy(p);
            return rc;
        }
    }
    *out = p;
    return MC_OK;
}

// Test hook without a device: the slice and lane plans of a host-only program
// (mc_debug_program_host_only) with S slices, host tables only (no upload),
// so the lane-resident expression source can be generated and compiled on a
// machine without a GPU (mc_debug_expr_jit_source / _compile with a
// "mc::k_hmc_lr<...>" kernel).  Returns the planner's status; MC_OK with
// lr.has_expr set when the program's expression terms took the lane layout.
static int lane_plan_host(mc_program* p, int32_t S, SlicePlan& P, bool& sliced) {
    sliced = false;  // the slice planner took the program (P holds its plan)
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (S < 1 || S > kLrSlices) return fail(MC_ERR_INVALID, "S must be in [1, %d]", kLrSlices);
    free_lanes(p->lr);
    SlPartition part;
    int rc = plan_slices(p, S, P, part);
    if (rc != MC_OK) return rc;
    sliced = true;
    rc = plan_lanes(p, part, p->lr);
    if (rc != MC_OK) return fail(rc, "lane-resident kernel: %s", p->lr.why.c_str());
    return MC_OK;
}
extern "C" int mc_debug_lane_plan_host(mc_program* p, int32_t S) {
    SlicePlan P;
    bool sliced;
    return lane_plan_host(p, S, P, sliced);
}

// Test hook: the same plans as mc_debug_lane_plan_host, one 64-bit FNV-1a
// digest per host table (include/mcmc355.h lists them), over the tables' bytes:
// the term structs hold 4-byte fields only, so they have no padding.
static_assert(sizeof(SlTerm) == 4 * 31 && alignof(SlTerm) == 4, "SlTerm: 4-byte fields only");
static_assert(sizeof(LrTerm) == 4 * (30 + 2 * kLrMaxSlots + kLrExprData) && alignof(LrTerm) == 4,
              "LrTerm: 4-byte fields only");
static_assert(sizeof(LrSterm) == 4 * 16 && alignof(LrSterm) == 4, "LrSterm: 4-byte fields only");
static uint64_t fnv1a(const void* data, size_t n) {
    const unsigned char* b = (const unsigned char*)data;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
template <typename T>
static uint64_t digest(const T& x) { return fnv1a(&x, sizeof(T)); }
template <typename T>
static uint64_t digest(const std::vector<T>& v) { return fnv1a(v.data(), v.size() * sizeof(T)); }
extern "C" int mc_debug_plan_digest(mc_program* p, int32_t S, uint64_t* out, int32_t n_out) {
    constexpr int kSlice = 13, kLane = 24;
    if (!out || n_out < kSlice + kLane) return fail(MC_ERR_INVALID, "out holds %d digests", kSlice + kLane);
    std::fill(out, out + n_out, (uint64_t)0);
    SlicePlan P;
    bool sliced;
    const int rc = lane_plan_host(p, S, P, sliced);
    if (!sliced) return rc;
    const uint64_t sl[kSlice] = {digest(P.S), digest(P.Lp), digest(P.Pmax), digest(P.Dsh),
                                 digest(P.nitems), digest(P.sdata_floats), digest(P.combine),
                                 digest(P.terms), digest(P.sterms), digest(P.data),
                                 digest(P.index), digest(P.blocks), digest(P.gidx)};
    std::copy(sl, sl + kSlice, out);
    if (rc != MC_OK) return rc;  // (only the lane planner declined)
    const LanePlan& L = p->lr;
    const uint64_t ln[kLane] = {digest(L.ok), digest(L.rs), digest(L.rep), digest(L.S),
                                digest(L.Dsh), digest(L.nitems), digest(L.sdata_floats),
                                digest(L.shl), digest(L.shxf), digest(L.shid), digest(L.n_generic),
                                digest(L.fast), digest(L.form), digest(L.has_xf),
                                digest(L.has_expr), digest(L.nuts_expr), digest(L.bundle),
                                digest(L.terms), digest(L.data), digest(L.blocks), digest(L.gidx),
                                digest(L.sterms), digest(L.rng), digest(L.gx_off)};
    std::copy(ln, ln + kLane, out + kSlice);
    return MC_OK;
}

// Test hook (mc_debug_program_host_only): programs built after it is set keep
// their host tables only — no device upload, no slice plan — for host-side
// checks without a GPU (the expression JIT's code generation and compilation,
// mc_debug_expr_jit_compile).  Such a program must not be launched.
extern "C" int mc_debug_program_host_only(int on) {
    g_program_host_only = on != 0;
    return MC_OK;
}

extern "C" int mc_program_destroy(mc_program* p) {
    if (!p) return MC_OK;
    jit_free(p);
    pw_free(p);
    free_slices(p->sl);
    free_lanes(p->lr);
    free_lanes(p->lrd);
    if (p->d_terms) (void)hipFree(p->d_terms);
    if (p->d_nodes) (void)hipFree(p->d_nodes);
    if (p->d_data) (void)hipFree(p->d_data);
    if (p->d_index) (void)hipFree(p->d_index);
    delete p;
    return MC_OK;
}

extern "C" int32_t mc_program_num_params(const mc_program* p) { return p ? p->D : -1; }
extern "C" int32_t mc_program_waves_per_chain(const mc_program* p) { return p ? p->wpc : -1; }

// Test hook: the tape plan of one term, in evaluation order (host tables).
extern "C" int mc_debug_term_plan(const mc_program* p, int32_t term, int32_t* out, int32_t n_out) {
    if (!p) return fail(MC_ERR_INVALID, "program is NULL");
    if (!out || n_out < 10) return fail(MC_ERR_INVALID, "out holds 10 values");
    if (term < 0 || (size_t)term >= p->terms.size())
        return fail(MC_ERR_INVALID, "term %d out of range (the program has %zu)", term,
                    p->terms.size());
    const DevTerm& T = p->terms[term];
    const int32_t v[10] = {T.dist, (int32_t)std::min<int64_t>(T.n, INT32_MAX), T.primary, T.npass,
                           (int32_t)T.pass_masks, T.wave_task, T.ncomb, T.ntiles, T.nvirt,
                           T.sync_before};
    std::copy(v, v + 10, out);
    return MC_OK;
}
