// plan_lanes.hip — the lane-resident layout planner (lanes.h): deal every
// slice's private parameters to (lane, slot), longest first onto the least
// loaded lane with a free slot, and tile each term's elements per (slot,
// lane).  Declines with MC_ERR_UNSUPPORTED (and LanePlan::why) when the
// program does not qualify; the term interpreter (k_hmc_sl) then runs it.
#include "plan.h"

void free_lanes(LanePlan& L) {
    if (L.d_terms) (void)hipFree(L.d_terms);
    if (L.d_data) (void)hipFree(L.d_data);
    if (L.d_blocks) (void)hipFree(L.d_blocks);
    if (L.d_gidx) (void)hipFree(L.d_gidx);
    if (L.d_sterms) (void)hipFree(L.d_sterms);
    if (L.d_rng) (void)hipFree(L.d_rng);
    if (L.d_mom) (void)hipFree(L.d_mom);
    L = LanePlan();
}

static int no(LanePlan& L, const char* why) {
    L.why = why;
    return MC_ERR_UNSUPPORTED;
}

// The compile-time form of a fast-form plan (lanes_fast.h LF_* bits): every
// slice holds the same swept / direct terms with the same shared operands,
// the shared roles (swept scale, direct loc, direct scale) are distinct
// parameters and every shared parameter has one; -1 otherwise, or when the
// form has no compiled kernel (k_hmc_lf<..., -1> reads it at run time).
static int lanes_form(const LanePlan& L, int nT) {
    int form = -2, o_sw = -1, o_dm = -1, o_ds = -1;
    for (int s = 0; s < L.S; ++s) {
        const int nsw = (int)(L.blocks[4 * s + 3] & 255), ndir = (int)((L.blocks[4 * s + 3] >> 8) & 255);
        const LrTerm* t = &L.terms[(size_t)s * nT];
        int f = 0, a = -1, b = -1, c = -1;
        if (nsw > 0) {
            f |= LF_SW;
            if (t[0].kind[2] == SK_SHARED) f |= LF_SWS, a = t[0].jsh[2];
        }
        if (ndir > 0) {
            const LrTerm& u = t[nsw];
            f |= LF_DIR;
            if (u.kind[1] == SK_SHARED) f |= LF_DM, b = u.jsh[1];
            if (u.kind[2] == SK_SHARED) f |= LF_DS, c = u.jsh[2];
        }
        if (form == -2) {
            form = f, o_sw = a, o_dm = b, o_ds = c;
        } else if (f != form || a != o_sw || b != o_dm || c != o_ds) {
            return -1;
        }
    }
    if (form < 0) return -1;
    const int roles = lf_nroles(form);
    if (roles != L.Dsh) return -1;
    if ((o_sw >= 0 && (o_sw == o_dm || o_sw == o_ds)) || (o_dm >= 0 && o_dm == o_ds)) return -1;
    return (form == (LF_SW | LF_SWS | LF_DIR | LF_DM | LF_DS) || form == LF_DIR) ? form : -1;
}

// The lane RNG plan of k_hmc_lf (lanes_fast.h lf_rng_*).  A wave's draws per
// iteration are the momentum normals of its two chains' private parameters
// (normal g % 4 of Philox block g / 4, the tape kernels' mapping), of the
// lanes' shared parameters (lane 2 k + c: parameter k of chain c), and one
// accept uniform per chain.  Every lane of a slice holds the same parameters
// in every wave, so the distinct (chain, block) pairs can be dealt to lanes
// once: lane i computes one Philox block and both Box-Muller pairs of it, two
// more lanes the chains' accept draws (their first Box-Muller log is the
// accept log), and each lane fetches its normals from the lanes that hold
// them — one Philox block and two Box-Muller pairs per lane and iteration
// instead of three blocks and three pairs, plus two blocks and logs per lane
// for the accept.  Per lane four words:
//   x: job (0 none, 1 / 2 momentum block of chain 0 / 1, 3 / 4 accept draw
//      of chain 0 / 1) | block << 3
//   y: slots 0, 1: source lane of chain 0, chain 1 (6 bits each) and the
//      component (2 bits), per slot 14 bits
//   z: slots 2, 3 likewise
//   w: the accept lane of chain 0 << 8 | of chain 1 << 14 | 1 << 30 (valid)
// (the blocks of every shared parameter of both chains are among the jobs;
// a lane finds its shared parameter's block lane once per launch)
// Empty when more than 62 distinct blocks are needed (the kernel then draws
// per lane).
static void plan_lane_rng(LanePlan& L, int S) {
    if (const char* e = std::getenv("MC_LANES_RNG"))  // 0: per-lane draws (A/B)
        if (std::atoi(e) == 0) return;
    std::vector<int32_t> rng((size_t)S * 64 * 4, 0);
    for (int s = 0; s < S; ++s) {
        std::map<std::pair<int, int32_t>, int> lane_of_block;  // (chain, block) -> lane
        std::vector<std::pair<int, int32_t>> jobs;
        auto job = [&](int c, int32_t b) {
            const auto key = std::make_pair(c, b);
            auto it = lane_of_block.find(key);
            if (it != lane_of_block.end()) return it->second;
            const int l = (int)jobs.size();
            jobs.push_back(key);
            lane_of_block[key] = l;
            return l;
        };
        int32_t* R = &rng[(size_t)s * 64 * 4];
        for (int j = 0; j < 64; ++j) {
            for (int r = 0; r < L.rs && r < kLrMaxSlots; ++r) {
                const int32_t g = L.gidx[((size_t)s * kLrMaxSlots + r) * 64 + j];
                if (g < 0) continue;
                if (g >= (1 << 28)) return;  // (block << 3 must fit the word)
                const int l0 = job(0, g >> 2), l1 = job(1, g >> 2);
                const int32_t v = l0 | (l1 << 6) | ((g & 3) << 12);
                R[4 * j + 1 + (r >> 1)] |= v << (14 * (r & 1));
            }
            if (j < 2 * L.Dsh) {  // every shared parameter k = j / 2 of chain j % 2 (the
                                  // kernel finds its block's lane: lane layouts differ)
                const int32_t g = L.shl[j >> 1];
                if (g >= (1 << 28)) return;
                (void)job(j & 1, g >> 2);
            }
        }
        if ((int)jobs.size() + 2 > 64) return;  // (no plan: per-lane draws)
        const int acc0 = (int)jobs.size(), acc1 = acc0 + 1;
        for (size_t i = 0; i < jobs.size(); ++i)
            R[4 * i] = (jobs[i].first + 1) | (jobs[i].second << 3);
        R[4 * acc0] = 3;
        R[4 * acc1] = 4;
        for (int j = 0; j < 64; ++j) R[4 * j + 3] |= (acc0 << 8) | (acc1 << 14) | (1 << 30);
    }
    L.rng.swap(rng);
}

// One slice's private parameters -> (lane group, slot): whole bundles (a
// parameter alone: a bundle of one), heaviest first onto the least loaded
// lane group with free consecutive slots for all its members.  ln / sl per
// position in part.priv[s]; false when a bundle finds no lane.
static bool deal(const mc_program* p, const SlPartition& part, int s, int rs, int ngroups,
                 std::vector<int>& ln, std::vector<int>& sl) {
    const std::vector<int>& pv = part.priv[s];
    std::vector<int64_t> cost(pv.size(), 0);
    std::vector<int> lpos(p->D, -1);
    for (size_t k = 0; k < pv.size(); ++k) lpos[pv[k]] = (int)k;
    for (int t = 0; t < (int)p->raw.size(); ++t) {
        if (part.scalar[t]) continue;
        if (part.ppr[t] >= 0)
            for (int64_t i : part.elems[s][t])
                cost[lpos[pp_index(p->raw[t], part.ppr[t], i, p->h_index)]]++;
        else if (!part.gmap[t].empty())
            for (int64_t i : part.elems[s][t]) cost[lpos[gx_param(part, t, i)]]++;
    }
    // (a bundle's members follow its first in priv[s], partition_program)
    std::vector<int> items, width;
    std::vector<int64_t> icost;
    for (size_t k = 0; k < pv.size(); ++k) {
        if (part.bfirst[pv[k]] == pv[k]) {
            items.push_back((int)k);
            width.push_back(1);
            icost.push_back(cost[k]);
        } else {
            ++width.back();
            icost.back() += cost[k];
        }
    }
    std::vector<int> ord(items.size());
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return icost[a] > icost[b]; });
    std::vector<int64_t> load(ngroups, 0);
    std::vector<int> used(ngroups, 0);
    ln.assign(pv.size(), -1);
    sl.assign(pv.size(), -1);
    for (int it : ord) {
        int best = -1;
        for (int l = 0; l < ngroups; ++l)
            if (used[l] + width[it] <= rs && (best < 0 || load[l] < load[best])) best = l;
        if (best < 0) return false;
        for (int m = 0; m < width[it]; ++m) {
            ln[items[it] + m] = best;
            sl[items[it] + m] = used[best]++;
        }
        load[best] += icost[it];
    }
    return true;
}

// Register slots L.rs, replication L.rep, and the bundle geometry of grouped
// expression terms (L.bundle, L.gx_off).
static int lane_geometry(const mc_program* p, const SlPartition& part, LanePlan& L) {
    const std::vector<DevTerm>& raw = p->raw;
    const int nT = (int)raw.size(), S = part.S;
    if (S > kLrSlices) return no(L, "more than 16 slices");
    if (part.Dsh > kLrMaxShared) return no(L, "more than 4 broadcast parameters");
    int rs = 1;
    for (int s = 0; s < S; ++s) {
        const int need = ((int)part.priv[s].size() + 63) / 64;
        if (need > kLrMaxSlots) return no(L, "more than 256 private parameters in a slice");
        rs = std::max(rs, need);
    }
    if (rs == 3) rs = 4;
    if (part.grouped) {  // the slots every slice's bundles need (whole bundles per lane)
        std::vector<int> ln, sl;
        for (;;) {
            bool fit = true;
            for (int s = 0; s < S && fit; ++s) fit = deal(p, part, s, rs, 64, ln, sl);
            if (fit) break;
            if (rs >= kLrMaxSlots)
                return no(L, "the bundles of private parameters do not fit the lanes' register slots");
            rs = rs == 1 ? 2 : 4;
        }
    }
    // replication (lanes.h LrCtx::rep): with at most 32 private parameters per
    // slice, each is dealt to a group of `rep` lanes (the largest power of two
    // <= 16 that still fits every parameter) and its elements are split over
    // the group: a lone wave's sweep runs n / rep elements instead of n (the
    // README "Small" shape: 7 groups of ~143 observations, 7 busy lanes of 64).
    // MC_LANES_REP=<k> caps it (1: off; A/B and tests).
    int rep = 1;
    if (rs == 1 && !part.grouped) {  // (a plan with grouped expression terms: rep = 1)
        size_t maxp = 1;
        for (int s = 0; s < S; ++s) maxp = std::max(maxp, part.priv[s].size());
        int np2 = 1;
        while ((size_t)np2 < maxp) np2 <<= 1;
        rep = std::max(1, std::min(16, 64 / np2));
        if (const char* e = std::getenv("MC_LANES_REP")) {
            const int cap = std::atoi(e);
            while (rep > 1 && rep > cap) rep >>= 1;
        }
        while (L.rep_cap > 0 && rep > L.rep_cap) rep >>= 1;
    }
    for (int t = 0; t < nT; ++t) {
        if (part.scalar[t] || part.ppr[t] < 0) continue;
        for (int64_t i = 0; i < raw[t].n; ++i)
            if (part.shared[pp_index(raw[t], part.ppr[t], i, p->h_index)])
                return no(L, "a per-element operand reads a broadcast parameter");
    }
    // the widest bundle a grouped expression term reads, and each gathered
    // leaf's slot offset inside its bundle: one value per leaf over all elements
    L.bundle = 0;
    L.gx_off.assign(p->rnodes.size(), -1);
    if (part.grouped) {
        std::vector<int> bwidth(p->D, 0);
        for (int j = 0; j < p->D; ++j) bwidth[part.bfirst[j]]++;
        for (int t = 0; t < nT; ++t) {
            if (part.gmap[t].empty()) continue;
            for (int k = 0; k < raw[t].expr_n; ++k) {
                const DevExprNode& d = p->rnodes[raw[t].expr_base + k];
                if (d.op != MC_EX_LEAF || (d.leaf.kind != MC_OP_PVEC && d.leaf.kind != MC_OP_GATHER))
                    continue;
                int32_t& off = L.gx_off[raw[t].expr_base + k];
                for (int32_t g : part.gmap[t]) {
                    const int j = d.leaf.poff + g;
                    L.bundle = std::max(L.bundle, bwidth[part.bfirst[j]]);
                    if (off >= 0 && off != part.bpos[j])
                        return no(L, "a gathered leaf sits at different slots of its elements' bundles");
                    off = part.bpos[j];
                }
            }
        }
    }
    L.rs = rs;
    L.rep = rep;
    return MC_OK;
}

// The form of term t on the lanes: the specialised signature, an affine loc,
// a per-element data scale, an expression term's fields.
static int classify_lane_term(const mc_program* p, const SlPartition& part, int t, LrTerm& lt,
                              LanePlan& L) {
    const DevTerm& rt = p->raw[t];
    fill_term(lt, rt, part.ppr[t], part.jsh);
    lt.sig = LS_GENERIC;
    if (rt.dist == MC_DIST_NORMAL && lt.mode == 0) {
        const int a = lt.kind[0], b = lt.kind[1], c = lt.kind[2];
        if (a == SK_DATA && b == SK_PP) lt.sig = c == SK_SHARED ? LS_DATA_PP_SH : LS_DATA_PP_C;
        else if (a == SK_PP && b == SK_SHARED && c == SK_SHARED) lt.sig = LS_PP_SH_SH;
        else if (a == SK_PP && b == SK_CONST && c == SK_CONST) lt.sig = LS_PP_C_C;
        else if (a == SK_PP && b == SK_DATA && c == SK_SHARED) lt.sig = LS_PP_DATA_SH;
        else if (a == SK_DATA && b == SK_SHARED && c == SK_SHARED) lt.sig = LS_DATA_SH_SH;
    }
    // an affine loc (loc + b * x over data x): lanes.h lr_affine_term
    if (rt.affine) {
        if (rt.dist != MC_DIST_NORMAL || lt.mode != 0 || lt.kind[0] != SK_DATA ||
            rt.ax.kind != MC_OP_DATA)
            return no(L, "an affine loc the lane kernels do not take");
        lt.sig = LS_AFF;
        lt.kb = rt.ab.kind == MC_OP_PSCALAR ? SK_SHARED : SK_CONST;
        lt.jb = rt.ab.kind == MC_OP_PSCALAR ? part.jsh[rt.ab.poff] : 0;
        lt.cb = rt.ab.kind == MC_OP_CONST ? rt.ab.cval : 0.0f;
    }
    // Normal with a per-element data scale, one of value / loc private
    // (theta ~ N(m, s_i), y_i ~ N(theta_g, s_i)): lanes.h lr_dscale_term
    if (rt.dist == MC_DIST_NORMAL && lt.kind[2] == SK_DATA && lt.pp >= 0 && lt.pp <= 1 &&
        lt.kind[lt.pp] == SK_PP && lt.kind[1 - lt.pp] != SK_PP &&
        lt.kind[1 - lt.pp] != SK_NONE && !rt.affine)
        lt.sig = LS_DSCALE;
    // an expression term (a chunk term: its data leaves tiled by tile_lane_term)
    if (rt.dist == MC_DIST_EXPR) {
        lt.sig = LS_EXPR;
        lt.expr_base = rt.expr_base;
        lt.expr_n = rt.expr_n;
        L.has_expr = 1;
        // a grouped term: tiled by the (lane, first slot) of its
        // elements' bundles; its vectors' slot offsets inside them
        lt.kb = (int32_t)part.gvec[t].size();
    }
    return MC_OK;
}

// Element lists per (slot, lane), in element order
typedef std::vector<std::vector<int64_t>> LaneLists;
static void lane_lists(const mc_program* p, const SlPartition& part, int s, int t, int rep,
                       const std::vector<int>& lane_of, const std::vector<int>& slot_of_p,
                       LaneLists& lists, int32_t& nslot) {
    const std::vector<int64_t>& E = part.elems[s][t];
    const bool grouped = !part.gmap[t].empty();
    lists.assign((size_t)kLrMaxSlots * 64, {});
    nslot = 1;
    if (part.ppr[t] < 0 && !grouped) {
        // chunk term: contiguous near-equal chunks over the lanes (slot 0)
        const int64_t nE = (int64_t)E.size(), nch = std::min<int64_t>(64, nE);
        int64_t f = 0;
        for (int64_t c = 0; c < nch; ++c) {
            const int64_t len = nE / nch + (c < nE % nch ? 1 : 0);
            for (int64_t u = 0; u < len; ++u) lists[(size_t)c].push_back(E[f + u]);
            f += len;
        }
        return;
    }
    for (int64_t i : E) {  // (a grouped expression term: by its bundle's first parameter)
        const int64_t g = grouped ? gx_param(part, t, i)
                                  : pp_index(p->raw[t], part.ppr[t], i, p->h_index);
        const int r = slot_of_p[g];
        lists[(size_t)r * 64 + lane_of[g]].push_back(i);
        nslot = std::max(nslot, r + 1);
    }
    // a replicated parameter's elements: near-equal contiguous
    // chunks over its group (a lone element stays with the leader; a plan
    // with grouped expression terms has rep = 1)
    if (rep > 1)
        for (int r = 0; r < nslot; ++r)
            for (int l0 = 0; l0 < 64; l0 += rep) {
                std::vector<int64_t> all;
                all.swap(lists[(size_t)r * 64 + l0]);
                const int64_t n = (int64_t)all.size();
                int64_t f = 0;
                for (int x = 0; x < rep; ++x) {
                    const int64_t len = n / rep + (x < n % rep ? 1 : 0);
                    lists[(size_t)r * 64 + l0 + x].assign(all.begin() + f, all.begin() + f + len);
                    f += len;
                }
            }
}

// Append one tiled array of `tot` floats to the block: set(dst, offset in the
// array, element) for every element of the lists, at (u >> 2) * 256 + 4 * lane
// + (u & 3) of its slot's tile.  Returns the array's offset in `data`.
template <typename F>
static int64_t tile_lane_array(std::vector<float>& data, const LrTerm& lt, const LaneLists& lists,
                               int64_t tot, F&& set) {
    while (data.size() % 4) data.push_back(0.0f);
    const int64_t base = (int64_t)data.size();
    data.resize(base + tot, 0.0f);
    for (int r = 0; r < lt.nslot; ++r)
        for (int l = 0; l < 64; ++l) {
            const std::vector<int64_t>& li = lists[(size_t)r * 64 + l];
            for (size_t u = 0; u < li.size(); ++u) {
                const int64_t o = lt.toff[r] + (u >> 2) * 256 + 4 * l + (u & 3);
                set(data[base + o], o, li[u]);
            }
        }
    return base;
}

// One term's tiles in the slice block that starts at blk0: its data operands,
// an expression's data leaves, the run lengths.  maxlen: its longest run.
static int tile_lane_term(const mc_program* p, int t, const LaneLists& lists, int64_t blk0,
                          LrTerm& lt, LanePlan& L, int32_t& maxlen) {
    const DevTerm& rt = p->raw[t];
    const std::vector<float>& dp = p->h_data;
    int64_t tot = 0;
    std::vector<int32_t> lens((size_t)lt.nslot * 64, 0);
    for (int r = 0; r < lt.nslot; ++r) {
        int64_t lmax = 0, lmin = INT64_MAX;
        for (int l = 0; l < 64; ++l) {
            const int64_t n = (int64_t)lists[(size_t)r * 64 + l].size();
            if (n > INT32_MAX / 256) return no(L, "a lane run is too long");
            lens[(size_t)r * 64 + l] = (int32_t)n;
            lmax = std::max(lmax, n);
            if (n > 0) lmin = std::min(lmin, n);
        }
        if (tot > INT32_MAX / 4) return no(L, "slice data too large");
        lt.toff[r] = (int32_t)tot;
        lt.lmin4[r] = lmax > 0 ? (int32_t)(lmin / 4) : 0;
        tot += 64 * ((lmax + 3) / 4 * 4);
    }
    auto copy_from = [&](int64_t src) {
        return [&dp, src](float& dst, int64_t, int64_t e) { dst = dp[src + e]; };
    };
    for (int a = 0; a < 4; ++a) {  // (a = 3: an affine term's x)
        if (a < 3 ? lt.kind[a] != SK_DATA : lt.sig != LS_AFF) continue;
        const int64_t base = tile_lane_array(L.data, lt, lists, tot,
                                             copy_from(a < 3 ? rt.op[a].pool : rt.ax.pool));
        if (a < 3) lt.doff[a] = (int32_t)(base - blk0);
        else lt.xoff = (int32_t)(base - blk0);
    }
    if (lt.sig == LS_EXPR) {  // the data leaves' arrays, in node order (one tile each)
        int e = 0;
        std::vector<int64_t> seen;
        for (int k = 0; k < rt.expr_n; ++k) {
            const DevExprNode& d = p->rnodes[rt.expr_base + k];
            if (d.op != MC_EX_LEAF || d.leaf.kind != MC_OP_DATA) continue;
            if (std::find(seen.begin(), seen.end(), d.leaf.pool) != seen.end()) continue;
            seen.push_back(d.leaf.pool);
            if (e >= kLrExprData) return no(L, "an expression with too many data leaves");
            lt.eoff[e++] =
                (int32_t)(tile_lane_array(L.data, lt, lists, tot, copy_from(d.leaf.pool)) - blk0);
        }
    }
    if (lt.sig == LS_DSCALE) {
        // the scale tile becomes 1/s^2 and the private operand's (free)
        // tile holds f32 log s, per element, as the constant-scale
        // terms' cinv2 / clogs
        const int64_t sb = blk0 + lt.doff[2];
        std::vector<float>& data = L.data;
        lt.doff[lt.pp] = (int32_t)(tile_lane_array(data, lt, lists, tot,
                                                   [&data, sb](float& dst, int64_t o, int64_t) {
            const float sc = data[sb + o];
            dst = (float)std::log((double)sc);
            data[sb + o] = 1.0f / (sc * sc);
        }) - blk0);
    }
    const int64_t lo = (int64_t)L.data.size();
    L.data.resize(lo + lens.size());
    std::memcpy(&L.data[lo], lens.data(), lens.size() * 4);
    lt.len_off = (int32_t)(lo - blk0);
    maxlen = 0;
    for (int32_t x : lens) maxlen = std::max(maxlen, x);
    return MC_OK;
}

// The moment constants of slice s's first swept term `lt` (block at blk0), per
// (slot, lane) run exactly as the tile holds it (with rep > 1: a lane's own
// part of the run): n its element count, c = (float) mean(x),
// R = (float) sum (x - c), Q = (float) sum (x - c)^2 — float64 sums in element
// order, rounded once (c and R contain no multiply: the bits do not depend on
// the host compiler's contraction).  An empty run: zeros.  lanes_fast.h
// lf_moments forms both moment sums at any position from them.
static void lane_moments(LanePlan& L, int s, int64_t blk0, const LrTerm& lt) {
    const float* base = &L.data[blk0 + lt.doff[0]];
    const int32_t* lens = (const int32_t*)&L.data[blk0 + lt.len_off];
    for (int r = 0; r < lt.nslot && r < kLrMaxSlots; ++r)
        for (int l = 0; l < 64; ++l) {
            const int64_t n = lens[r * 64 + l];
            if (n <= 0) continue;
            const float* x = base + lt.toff[r] + 4 * l;
            auto at = [&](int64_t u) { return (double)x[(u >> 2) * 256 + (u & 3)]; };
            double sum = 0.0, sr = 0.0, sq = 0.0;
            for (int64_t u = 0; u < n; ++u) sum += at(u);
            const float c = (float)(sum / (double)n);
            for (int64_t u = 0; u < n; ++u) sr += at(u) - (double)c;
            for (int64_t u = 0; u < n; ++u) {
                const double d = at(u) - (double)c;
                sq += d * d;
            }
            float* m = &L.mom[(((size_t)s * kLrMaxSlots + r) * 64 + l) * 4];
            m[0] = c;
            m[1] = (float)sr;
            m[2] = (float)sq;
            m[3] = (float)n;
        }
}

// The scalar terms, compact (LDS copy in every workgroup).  Returns the number
// of them k_hmc_lf cannot take.
static int lane_sterms(const SlPartition& part, LanePlan& L) {
    uint32_t own_mask = 0;
    int lf_generic = 0;
    for (size_t it = 0; it < part.sterms.size(); ++it) {
        const SlTerm& st = part.sterms[it];
        LrSterm x;
        std::memset(&x, 0, sizeof(x));
        x.raw = part.sterm_raw[it];
        x.dist = st.dist;
        x.kinds = st.kind[0] | (st.kind[1] << 4) | (st.kind[2] << 8);
        x.jsh = st.jsh[0] | (st.jsh[1] << 4) | (st.jsh[2] << 8);  // (0 unless SK_SHARED)
        x.c0 = st.c0;
        for (int a = 0; a < 3; ++a) x.cval[a] = st.cval[a];
        x.clogs = st.clogs;
        x.clg = st.clg;
        x.wn = st.weight * (float)st.niter;
        // one "own" prior per shared parameter (lanes.h LrOwn)
        x.own = st.kind[0] == SK_SHARED &&
                (st.dist == MC_DIST_NORMAL || st.dist == MC_DIST_HALFNORMAL) &&
                (st.kind[1] == SK_CONST || st.kind[1] == SK_NONE) && st.kind[2] == SK_CONST &&
                !(own_mask >> st.jsh[0] & 1) && !(x.raw & 1);
        if (x.own) own_mask |= 1u << st.jsh[0];
        x.cinv = st.kind[2] == SK_CONST ? 1.0f / st.cval[2] : 0.0f;
        if (!x.own) ++L.n_generic;
        // an identity term over a raw shared parameter (its log-Jacobian):
        // k_hmc_lf adds it in the holder lane (LrCtx::shid); k_hmc_lr runs it
        // with the other generic scalar terms
        const bool raw_id = st.dist == MC_DIST_IDENTITY && st.kind[0] == SK_SHARED &&
                            ((x.raw & 1) || L.shxf[st.jsh[0]] == MC_XF_NONE);
        if (raw_id) L.shid[st.jsh[0]] += x.wn;
        else if (!x.own) ++lf_generic;
        L.sterms.push_back(x);
    }
    return lf_generic;
}

int plan_lanes(const mc_program* p, const SlPartition& part, LanePlan& L) {
    const int nT = (int)p->raw.size(), S = part.S;
    if (int rc = lane_geometry(p, part, L)) return rc;
    const int rep = L.rep;
    L.S = S;
    L.Dsh = part.Dsh;
    L.nitems = part.nitems;
    L.has_xf = has_transform(p) ? 1 : 0;
    for (int k = 0; k < part.Dsh; ++k) L.shl[k] = part.shl[k], L.shxf[k] = part.shxf[k];
    L.terms.assign((size_t)S * nT, LrTerm());
    L.blocks.assign(4 * (size_t)S, 0);
    L.gidx.assign((size_t)S * kLrMaxSlots * 64, -1);
    L.sdata_floats = 0;
    L.mom.assign((size_t)S * kLrMaxSlots * 64 * 4, 0.0f);
    std::vector<int> lane_of(p->D, -1), slot_of_p(p->D, -1);
    bool any_rest = false, any_rest_nonexpr = false;
    for (int s = 0; s < S; ++s) {
        // ---- parameters -> (lane, slot) ----
        const std::vector<int>& pv = part.priv[s];
        std::vector<int> ln, sl;
        if (!deal(p, part, s, L.rs, 64 / rep, ln, sl)) return no(L, "a private parameter finds no lane");
        // (lane groups of `rep` lanes; lane_of = the group's leader lane)
        for (size_t k = 0; k < pv.size(); ++k) {
            lane_of[pv[k]] = ln[k] * rep;
            slot_of_p[pv[k]] = sl[k];
            for (int x = 0; x < rep; ++x)
                L.gidx[((size_t)s * kLrMaxSlots + sl[k]) * 64 + ln[k] * rep + x] = pv[k];
        }
        // ---- terms: the swept ones (lanes.h kLrSweep) first ----
        while (L.data.size() % 4) L.data.push_back(0.0f);
        const int64_t blk0 = (int64_t)L.data.size();
        std::vector<LrTerm> swept, direct, rest;
        LaneLists lists;
        for (int t = 0; t < nT; ++t) {
            if (part.scalar[t] || part.elems[s][t].empty()) continue;
            LrTerm lt;
            int32_t maxlen;
            if (int rc = classify_lane_term(p, part, t, lt, L)) return rc;
            lane_lists(p, part, s, t, rep, lane_of, slot_of_p, lists, lt.nslot);
            if (int rc = tile_lane_term(p, t, lists, blk0, lt, L, maxlen)) return rc;
            const bool dir = (lt.sig == LS_PP_SH_SH || lt.sig == LS_PP_C_C) && maxlen <= 1;
            const bool sw = lt.sig == LS_DATA_PP_SH || lt.sig == LS_DATA_PP_C ||
                            lt.sig == LS_PP_C_C || lt.sig == LS_PP_DATA_SH;
            if (dir && (int)direct.size() < kLrDirect) direct.push_back(lt);
            else if (sw && (int)swept.size() < kLrSweep) swept.push_back(lt);
            else rest.push_back(lt);
        }
        // fast form (lanes_fast.h): one swept term with data value and private
        // loc at most, one direct term at most, nothing else
        const bool core = !(swept.size() > 1 || direct.size() > 1 ||
                            (!swept.empty() && swept[0].sig != LS_DATA_PP_SH &&
                             swept[0].sig != LS_DATA_PP_C));
        if (!rest.empty() || !core) any_rest = true;
        if (core && !swept.empty()) lane_moments(L, s, blk0, swept[0]);
        bool rest_expr = true;  // every other term an expression term (LanePlan::nuts_expr)
        for (const LrTerm& lt : rest) rest_expr &= lt.sig == LS_EXPR;
        if (!rest_expr || !core) any_rest_nonexpr = true;
        int nact = 0;
        for (const std::vector<LrTerm>* v : {&swept, &direct, &rest})
            for (const LrTerm& lt : *v) L.terms[(size_t)s * nT + nact++] = lt;
        while (L.data.size() % 4) L.data.push_back(0.0f);
        const int64_t blen = (int64_t)L.data.size() - blk0;
        if (blen > INT32_MAX / 8) return no(L, "slice data too large");
        L.blocks[4 * s] = blk0;
        L.blocks[4 * s + 1] = blen;
        L.blocks[4 * s + 2] = nact;
        L.blocks[4 * s + 3] = (int64_t)swept.size() | ((int64_t)direct.size() << 8);
        L.sdata_floats = std::max<int>(L.sdata_floats, (int)blen);
    }
    const int lf_generic = lane_sterms(part, L);
    L.sdata_floats = (L.sdata_floats + 3) / 4 * 4;  // the scalar terms follow, 16-byte aligned
    if ((int64_t)L.sdata_floats * 4 + (int64_t)L.sterms.size() * (int64_t)sizeof(LrSterm) >
        kSlLdsBudget)
        return no(L, "slice data exceed the LDS budget");
    if (L.data.empty()) L.data.assign(4, 0.0f);
    plan_lane_rng(L, S);
    L.fast = (!any_rest && lf_generic == 0) ? 1 : 0;
    L.nuts_expr = (L.has_expr && !any_rest_nonexpr && lf_generic == 0) ? 1 : 0;
    L.form = L.fast ? lanes_form(L, nT) : -1;
    L.ok = 1;
    return MC_OK;
}
