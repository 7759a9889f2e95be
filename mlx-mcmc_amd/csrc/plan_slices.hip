// plan_slices.hip — the sliced layout planner (sliced.h), in two stages
// (plan.h): partition_program deals parameters and elements to slices,
// tile_slices lays out the term interpreter's tables of every slice.
#include "plan.h"

void free_slices(SlicePlan& P) {
    if (P.d_terms) (void)hipFree(P.d_terms);
    if (P.d_sterms) (void)hipFree(P.d_sterms);
    if (P.d_data) (void)hipFree(P.d_data);
    if (P.d_index) (void)hipFree(P.d_index);
    if (P.d_blocks) (void)hipFree(P.d_blocks);
    if (P.d_gidx) (void)hipFree(P.d_gidx);
    P = SlicePlan();
}

// ---------------------------------------------------------------------------
// stage 1: the partition
// ---------------------------------------------------------------------------
// Grouped expression terms and the bundles of private parameters their
// elements read (alpha_g, beta_g): bundles that share a parameter merge.
// bmem: per bundle first, its members, ascending.
static int plan_bundles(const mc_program* p, SlPartition& part, std::vector<std::vector<int>>& bmem) {
    const std::vector<DevTerm>& raw = p->raw;
    const int D = p->D, nT = (int)raw.size();
    std::vector<std::vector<int32_t>>&gvec = part.gvec, &gmap = part.gmap;
    std::vector<int>&bfirst = part.bfirst, &bpos = part.bpos;
    gvec.assign(nT, {});
    gmap.assign(nT, {});
    bfirst.resize(D);
    bpos.assign(D, 0);
    std::iota(bfirst.begin(), bfirst.end(), 0);
    for (int t = 0; t < nT; ++t)
        if (raw[t].dist == MC_DIST_EXPR &&
            expr_term_class(p, raw[t], &gvec[t], &gmap[t], nullptr) == 1)
            part.grouped = true;
    if (!part.grouped) return MC_OK;
    std::vector<int> root(D);
    std::iota(root.begin(), root.end(), 0);
    auto find = [&](int x) {
        while (root[x] != x) x = root[x] = root[root[x]];
        return x;
    };
    // a vector's bundles cover every group of its range, with elements or
    // not (an empty group's alpha_g and beta_g still sit together, so a
    // term over beta alone sees one slot offset): the range is the largest
    // group count of any term that reads the vector, shared by the vectors
    // read together
    std::map<int32_t, int32_t> vrange;
    for (int pass = 0; pass < 3; ++pass)
        for (int t = 0; t < nT; ++t) {
            if (gmap[t].empty()) continue;
            int32_t r = *std::max_element(gmap[t].begin(), gmap[t].end()) + 1;
            for (int32_t v : gvec[t]) r = std::max(r, vrange[v]);
            for (int32_t v : gvec[t]) vrange[v] = r;
        }
    for (int t = 0; t < nT; ++t)
        for (size_t v = 1; v < gvec[t].size(); ++v)
            for (int32_t g = 0; g < vrange[gvec[t][0]]; ++g) {
                if (gvec[t][0] + g >= D || gvec[t][v] + g >= D) break;
                const int a = find(gvec[t][0] + g), b = find(gvec[t][v] + g);
                if (a != b) root[std::max(a, b)] = std::min(a, b);  // (the root: the lowest)
            }
    std::vector<int> count(D, 0);
    bmem.assign(D, std::vector<int>());
    for (int j = 0; j < D; ++j) {
        bfirst[j] = find(j);
        bpos[j] = count[bfirst[j]]++;
        bmem[bfirst[j]].push_back(j);
    }
    for (int j = 0; j < D; ++j)
        if (count[bfirst[j]] > kLrMaxSlots)
            return fail(MC_ERR_UNSUPPORTED, "a bundle of %d private parameters read together "
                        "by gathered expression terms (more than %d) does not fit a lane's "
                        "register slots (not sliceable)", count[bfirst[j]], kLrMaxSlots);
    return MC_OK;
}

// The transform of each shared parameter: every transformed use agrees;
// terms that are not scalar read it through the transform only (a scalar
// term may also read the raw parameter: SlPartition::sterm_raw).
static int shared_transforms(const mc_program* p, SlPartition& part) {
    const std::vector<DevTerm>& raw = p->raw;
    const std::vector<int>& jsh = part.jsh;
    std::vector<int>& shxf = part.shxf;
    shxf.assign(part.shl.size(), MC_XF_NONE);
    if (!has_transform(p)) return MC_OK;
    for (const DevTerm& t : raw)
        for (int a = 0; a < 3; ++a) {
            const DevOperand& o = t.op[a];
            if (o.kind != MC_OP_PSCALAR || o.xf == MC_XF_NONE) continue;
            int& x = shxf[jsh[o.poff]];
            if (x != MC_XF_NONE && x != o.xf)
                return fail(MC_ERR_UNSUPPORTED, "a broadcast parameter read through two "
                            "different transforms (mx.exp and mx.log): not sliceable");
            x = o.xf;
        }
    for (const DevTerm& rt : raw) {
        if (is_scalar_term(rt)) continue;
        for (int a = 0; a < 3; ++a) {
            const DevOperand& o = rt.op[a];
            if (o.kind == MC_OP_PSCALAR && o.xf != shxf[jsh[o.poff]])
                return fail(MC_ERR_UNSUPPORTED, "a broadcast parameter read both raw and "
                            "through mx.exp / mx.log by per-element terms: not sliceable");
        }
        // an expression reads a transformed broadcast parameter only
        // through the matching node (mx.exp(log_sigma) for an exp
        // transform): the lane code reads the transformed value there and
        // its cotangent is the value's (jit.hip gen_lane_term)
        if (rt.dist != MC_DIST_EXPR) continue;
        const DevExprNode* N = p->nodes.data() + rt.expr_base;
        for (int k = 0; k < rt.expr_n; ++k) {
            if (N[k].op == MC_EX_LEAF) continue;
            const int args[3] = {N[k].a, N[k].b, N[k].c};
            for (int x = 0; x < 3; ++x) {
                const int a = args[x];
                if (a < 0 || N[a].op != MC_EX_LEAF || N[a].leaf.kind != MC_OP_PSCALAR) continue;
                const int xfk = shxf[jsh[N[a].leaf.poff]];
                if (xfk == MC_XF_NONE) continue;
                const int want = xfk == MC_XF_EXP ? MC_EX_EXP : MC_EX_LOG;
                if (N[k].op != want || x != 0)
                    return fail(MC_ERR_UNSUPPORTED, "a broadcast parameter read raw by an "
                                "expression and through mx.exp / mx.log by a fused term: "
                                "not sliceable");
            }
        }
    }
    return MC_OK;
}

static SlTerm make_slterm(const DevTerm& rt, int t, const SlPartition& part) {
    SlTerm st;
    fill_term(st, rt, part.ppr[t], part.jsh);
    for (int a = 0; a < 3; ++a)  // a shared operand's local slot
        st.kloc[a] = st.kind[a] == SK_SHARED ? part.Pmax + st.jsh[a] : -1;
    return st;
}

int partition_program(const mc_program* p, int S, SlPartition& part) {
    const std::vector<DevTerm>& raw = p->raw;
    if (has_expr(p)) {
        const std::string why = expr_lanes_why(p);
        if (!why.empty()) return fail(MC_ERR_UNSUPPORTED, "%s", why.c_str());
    }
    if (has_affine(p) && !affine_lanes_ok(p))
        return fail(MC_ERR_UNSUPPORTED, "affine loc operands other than `loc + b * x` over "
                    "data x (x a parameter vector, a non-Normal term, a per-element scale) run "
                    "on the chain-per-workgroup kernels (not sliceable)");
    if (has_transform(p) && !transform_on_shared_only(p))
        return fail(MC_ERR_UNSUPPORTED, "transformed parameter operands (mx.exp / mx.log) of "
                    "per-element parameters, and identity terms over them, run on the "
                    "chain-per-workgroup kernels (not sliceable)");
    const std::vector<int32_t>& ip = p->h_index;
    const int D = p->D, nT = (int)raw.size();
    part.S = S;
    std::vector<int>& ppr = part.ppr;
    ppr.assign(nT, -1);
    for (int t = 0; t < nT; ++t)
        for (int a = 0; a < 3; ++a)
            if (raw[t].op[a].kind == MC_OP_PVEC || raw[t].op[a].kind == MC_OP_GATHER) {
                if (ppr[t] >= 0)
                    return fail(MC_ERR_UNSUPPORTED,
                                "term %d has two per-element parameter operands: not sliceable", t);
                ppr[t] = a;
            }
    std::vector<std::vector<int>> bmem;
    if (int rc = plan_bundles(p, part, bmem)) return rc;
    const std::vector<std::vector<int32_t>>&gvec = part.gvec, &gmap = part.gmap;
    const std::vector<int>& bfirst = part.bfirst;
    // shared (broadcast) parameters and the private parameters' costs
    std::vector<char>& shared = part.shared;
    shared.assign(D, 0);
    for (const DevTerm& t : raw) {
        for (int a = 0; a < 3; ++a)
            if (t.op[a].kind == MC_OP_PSCALAR) shared[t.op[a].poff] = 1;
        if (t.affine && t.ab.kind == MC_OP_PSCALAR) shared[t.ab.poff] = 1;  // the slope
        if (t.dist == MC_DIST_EXPR)  // an expression's broadcast leaves
            for (int k = 0; k < t.expr_n; ++k) {
                const DevExprNode& d = p->nodes[t.expr_base + k];
                if (d.op == MC_EX_LEAF && d.leaf.kind == MC_OP_PSCALAR) shared[d.leaf.poff] = 1;
            }
    }
    std::vector<int64_t> cost(D, 1);
    for (int t = 0; t < nT; ++t)
        if (ppr[t] >= 0)
            for (int64_t i = 0; i < raw[t].n; ++i) {
                const int64_t j = pp_index(raw[t], ppr[t], i, ip);
                if (!shared[j]) cost[j] += 1;
            }
    for (int t = 0; t < nT; ++t)
        if (!gmap[t].empty())
            for (int32_t g : gmap[t]) {
                for (int32_t v : gvec[t])
                    if (shared[v + g])
                        return fail(MC_ERR_UNSUPPORTED, "an expression term gathers a parameter "
                                    "that other terms read as a broadcast scalar: not sliceable");
                cost[gvec[t][0] + g] += 1;
            }
    // (a bundle is indivisible: its members' summed cost, at its lowest member)
    std::vector<int64_t> bcost(cost);
    if (part.grouped)
        for (int j = 0; j < D; ++j)
            if (bfirst[j] != j) bcost[bfirst[j]] += cost[j];
    int64_t total = 0;
    for (int j = 0; j < D; ++j)
        if (!shared[j]) total += cost[j];
    // owners: contiguous runs of private parameters of near-equal cost
    part.owner.assign(D, 0);
    part.lidx.assign(D, 0);
    part.jsh.assign(D, -1);
    part.priv.assign(S, {});
    int64_t run = 0;
    for (int j = 0; j < D; ++j) {
        if (shared[j]) {
            part.jsh[j] = (int)part.shl.size();
            part.shl.push_back(j);
            continue;
        }
        if (bfirst[j] != j) continue;  // (placed with its bundle, below)
        const int s = (int)std::min<int64_t>(S - 1, (2 * run + bcost[j]) * S / (2 * std::max<int64_t>(total, 1)));
        const std::vector<int> alone(1, j);
        for (int m : part.grouped ? bmem[j] : alone) {  // the bundle's members, ascending
            part.owner[m] = s;
            part.lidx[m] = (int)part.priv[s].size();
            part.priv[s].push_back(m);
        }
        run += bcost[j];
    }
    if (int rc = shared_transforms(p, part)) return rc;
    part.Dsh = (int)part.shl.size();
    part.nitems = part.Dsh + 3;
    for (int s = 0; s < S; ++s) part.Pmax = std::max<int>(part.Pmax, (int)part.priv[s].size());
    // scalar terms, in every slice
    part.scalar.assign(nT, 0);
    for (int t = 0; t < nT; ++t) {
        if (!(part.scalar[t] = is_scalar_term(raw[t]))) continue;
        SlTerm st = make_slterm(raw[t], t, part);
        if (raw[t].n > INT32_MAX) return fail(MC_ERR_UNSUPPORTED, "scalar term too long");
        st.niter = (int32_t)raw[t].n;  // element count
        part.sterms.push_back(st);
        int rb = 0;
        for (int a = 0; a < 3; ++a) {
            const DevOperand& o = raw[t].op[a];
            if (o.kind == MC_OP_PSCALAR && o.xf == MC_XF_NONE && part.shxf[part.jsh[o.poff]] != MC_XF_NONE)
                rb |= 1 << a;
        }
        part.sterm_raw.push_back(rb);
    }
    // element -> slice
    part.elems.assign(S, std::vector<std::vector<int64_t>>(nT));
    for (int t = 0; t < nT; ++t) {
        if (part.scalar[t]) continue;
        const int64_t n = raw[t].n;
        for (int64_t i = 0; i < n; ++i) {
            int s;
            if (ppr[t] >= 0) {
                const int64_t j = pp_index(raw[t], ppr[t], i, ip);
                s = shared[j] ? 0 : part.owner[j];
            } else if (!gmap[t].empty()) {
                s = part.owner[gx_param(part, t, i)];
            } else if (n < 256) {
                s = t % S;  // small terms go whole to one slice, round robin
            } else {
                s = (int)(i * S / n);
            }
            part.elems[s][t].push_back(i);
        }
    }
    return MC_OK;
}

// ---------------------------------------------------------------------------
// stage 2: one slice's tables
// ---------------------------------------------------------------------------
static constexpr int T = kSlLanes;  // run slots per chain pair
struct Run {
    int32_t k;      // local slot of the run's parameter, -1: a chunk
    int64_t first;  // position in the slice's element list
    int32_t len;
};

// The runs of one term's elements in slice s, and whether every run has its
// own parameter (direct gradient writes).
static void slice_runs(const mc_program* p, const SlPartition& part, int s, int t,
                       std::vector<Run>& R, char& direct) {
    const DevTerm& rt = p->raw[t];
    const std::vector<int64_t>& E = part.elems[s][t];
    const int64_t nE = (int64_t)E.size();
    if (nE > 0 && part.ppr[t] >= 0) {
        std::vector<Run> nat;
        for (int64_t e = 0; e < nE; ++e) {
            const int64_t j = pp_index(rt, part.ppr[t], E[e], p->h_index);
            const int32_t k = part.shared[j] ? part.Pmax + part.jsh[j] : part.lidx[j];
            if (e > 0 && nat.back().k == k && nat.back().len < INT32_MAX) {
                ++nat.back().len;
            } else {
                nat.push_back({k, e, 1});
            }
        }
        // few long runs: split them so that the lanes get near-equal
        // work (m runs per lane); otherwise keep whole runs
        int64_t Lt = INT64_MAX;
        const int64_t nn = (int64_t)nat.size();
        if (nn <= 4 * T) {
            const int64_t m = (nn + T - 1) / T;
            int64_t lo = 1, hi = 1;
            for (const Run& r : nat) hi = std::max<int64_t>(hi, r.len);
            while (lo < hi) {
                const int64_t mid = (lo + hi) / 2;
                int64_t pieces = 0;
                for (const Run& r : nat) pieces += (r.len + mid - 1) / mid;
                if (pieces <= T * m) hi = mid; else lo = mid + 1;
            }
            Lt = lo;
        }
        for (const Run& r : nat) {
            const int64_t pieces = (Lt == INT64_MAX) ? 1 : (r.len + Lt - 1) / Lt;
            const int64_t base = r.len / pieces, rem = r.len % pieces;
            int64_t f = r.first;
            for (int64_t pc = 0; pc < pieces; ++pc) {
                const int32_t pl = (int32_t)(base + (pc < rem ? 1 : 0));
                R.push_back({r.k, f, pl});
                f += pl;
            }
        }
        std::vector<int32_t> ks;
        for (const Run& r : R) ks.push_back(r.k);
        std::sort(ks.begin(), ks.end());
        direct = std::adjacent_find(ks.begin(), ks.end()) == ks.end();
    } else if (nE > 0) {
        const int64_t nch = std::min<int64_t>(T, nE);
        int64_t f = 0;
        for (int64_t c = 0; c < nch; ++c) {
            const int32_t pl = (int32_t)(nE / nch + (c < nE % nch ? 1 : 0));
            R.push_back({-1, f, pl});
            f += pl;
        }
    }
}

// Runs -> (lane rl, iteration rit).  A parameter's direct runs share one lane
// in every term (so direct-write terms need no barrier between them): the map
// is built from the largest direct term first, longest run first onto the
// least loaded lane; other runs likewise per term.
static void assign_lanes(const std::vector<std::vector<Run>>& runs, const std::vector<char>& direct,
                         int Lp, std::vector<std::vector<int32_t>>& rl,
                         std::vector<std::vector<int32_t>>& rit) {
    const int nT = (int)runs.size();
    std::vector<int32_t> lane_of_k(Lp, -1);
    std::vector<int> order(nT);
    std::iota(order.begin(), order.end(), 0);
    auto total = [&](int t) {
        int64_t x = 0;
        for (const Run& r : runs[t]) x += r.len;
        return x;
    };
    std::stable_sort(order.begin(), order.end(),
                     [&](int a2, int b2) { return total(a2) > total(b2); });
    std::vector<int64_t> kload(T, 0);  // load of the shared k->lane map
    for (int t : order) {
        const std::vector<Run>& R = runs[t];
        const int64_t nr = (int64_t)R.size();
        rl[t].assign(nr, 0);
        rit[t].assign(nr, 0);
        std::vector<int64_t> ord(nr);
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(),
                         [&](int64_t a2, int64_t b2) { return R[a2].len > R[b2].len; });
        std::vector<int64_t> load(T, 0);
        std::vector<int32_t> cnt(T, 0);
        for (int64_t r : ord) {
            int lane;
            if (direct[t] && lane_of_k[R[r].k] >= 0) {
                lane = lane_of_k[R[r].k];
            } else {
                std::vector<int64_t>& L = direct[t] ? kload : load;
                lane = 0;
                for (int l = 1; l < T; ++l)
                    if (L[l] < L[lane]) lane = l;
                if (direct[t]) lane_of_k[R[r].k] = lane;
            }
            if (direct[t]) kload[lane] += R[r].len;
            load[lane] += R[r].len;
            rl[t][r] = lane;
            rit[t][r] = cnt[lane]++;
        }
    }
}

// One term's tables and tiled data, appended to the slice block that starts
// at blk0: tiles per iteration, lane records, combine entries.
static int emit_term_tables(const mc_program* p, const SlPartition& part, int s, int t,
                            const std::vector<Run>& R, const std::vector<int32_t>& rl,
                            const std::vector<int32_t>& rit, int64_t blk0, SlTerm& st,
                            SlicePlan& P) {
    const DevTerm& rt = p->raw[t];
    const std::vector<int64_t>& E = part.elems[s][t];
    const int64_t nr = (int64_t)R.size();
    int32_t niter = 0;
    for (int64_t r = 0; r < nr; ++r) niter = std::max(niter, rit[r] + 1);
    st.niter = part.scalar[t] ? 0 : niter;
    // tiles per iteration
    std::vector<int32_t> tiles(3 * (size_t)niter, 0);
    std::vector<int64_t> toff(niter, 0);
    std::vector<int32_t> lmax(niter, 0), lmin(niter, INT32_MAX);
    for (int64_t r = 0; r < nr; ++r) {
        lmax[rit[r]] = std::max(lmax[rit[r]], R[r].len);
        lmin[rit[r]] = std::min(lmin[rit[r]], R[r].len);
    }
    int64_t tot = 0;
    for (int32_t it = 0; it < niter; ++it) {
        const int64_t lpad = (lmax[it] + 3) / 4 * 4;
        toff[it] = tot;
        tiles[3 * it + 1] = lmax[it];
        tiles[3 * it + 2] = lmax[it] > 0 ? lmin[it] / 4 : 0;
        tot += (int64_t)T * lpad;
    }
    // tiled data operands (offsets relative to the slice block)
    for (int a = 0; a < 3; ++a) {
        if (st.kind[a] != SK_DATA) continue;
        while (P.data.size() % 4) P.data.push_back(0.0f);
        const int64_t base = (int64_t)P.data.size();
        P.data.resize(base + tot, 0.0f);
        const int64_t src = rt.op[a].pool;
        for (int64_t r = 0; r < nr; ++r) {
            const int64_t o = base + toff[rit[r]] + rl[r] * 4;
            for (int32_t u = 0; u < R[r].len; ++u)
                P.data[o + (u >> 2) * (4 * T) + (u & 3)] = p->h_data[src + E[R[r].first + u]];
        }
        st.doff[a] = (int32_t)(base - blk0);
    }
    for (int32_t it = 0; it < niter; ++it) {
        if (toff[it] > INT32_MAX / 2) return fail(MC_ERR_UNSUPPORTED, "slice data too large");
        tiles[3 * it] = (int32_t)toff[it];
    }
    // lane records per (iteration, lane); empty {-1, 0}
    std::vector<int32_t> lanes(2 * (size_t)niter * T, 0);
    for (int64_t x = 0; x < (int64_t)niter * T; ++x) lanes[2 * x] = -1;
    for (int64_t r = 0; r < nr; ++r) {
        const int64_t x = (int64_t)rit[r] * T + rl[r];
        lanes[2 * x] = R[r].k;
        lanes[2 * x + 1] = R[r].len;
    }
    // combine entries per round of kSlItr iterations (split runs only):
    // the runs of one parameter, positions in run order
    std::vector<int32_t> roff, ents, plist;
    const int32_t nrounds = (niter + kSlItr - 1) / kSlItr;
    for (int32_t rd = 0; rd < nrounds; ++rd) {
        roff.push_back((int32_t)(ents.size() / 3));
        if (st.direct || st.pp < 0) continue;
        for (int64_t r = 0; r < nr;) {
            int64_t q = r;
            while (q < nr && R[q].k == R[r].k) ++q;
            std::vector<int32_t> ps;
            for (int64_t x = r; x < q; ++x)
                if (rit[x] / kSlItr == rd) ps.push_back((int32_t)((rit[x] % kSlItr) * T + rl[x]));
            if (!ps.empty()) {
                ents.push_back(R[r].k);
                ents.push_back((int32_t)plist.size());
                ents.push_back((int32_t)ps.size());
                plist.insert(plist.end(), ps.begin(), ps.end());
            }
            r = q;
        }
    }
    roff.push_back((int32_t)(ents.size() / 3));
    // the tables go into the slice block as int32 words
    auto put = [&](const std::vector<int32_t>& v, bool even) -> int32_t {
        while (P.data.size() % (even ? 2 : 1)) P.data.push_back(0.0f);
        const int64_t o = (int64_t)P.data.size();
        P.data.resize(o + v.size());
        if (!v.empty()) std::memcpy(&P.data[o], v.data(), v.size() * 4);
        return (int32_t)(o - blk0);
    };
    st.tile_off = put(tiles, false);
    st.lane_off = put(lanes, true);
    st.round_off = put(roff, false);
    st.comb_off = put(ents, false);
    st.pos_off = put(plist, false);
    return MC_OK;
}

int tile_slices(const mc_program* p, const SlPartition& part, SlicePlan& P) {
    const int S = part.S, nT = (int)p->raw.size();
    P.S = S;
    P.Dsh = part.Dsh;
    P.Pmax = part.Pmax;
    P.Lp = std::max(4, (P.Pmax + P.Dsh + 3) / 4 * 4);
    P.nitems = part.nitems;
    P.gidx.assign((size_t)S * P.Lp, -1);
    for (int s = 0; s < S; ++s) {
        std::copy(part.priv[s].begin(), part.priv[s].end(), P.gidx.begin() + (size_t)s * P.Lp);
        std::copy(part.shl.begin(), part.shl.end(), P.gidx.begin() + (size_t)s * P.Lp + P.Pmax);
    }
    P.terms.assign((size_t)S * nT, SlTerm());
    P.sterms = part.sterms;
    P.blocks.assign(4 * (size_t)S, 0);
    P.sdata_floats = 0;
    for (int s = 0; s < S; ++s) {
        while (P.data.size() % 4) P.data.push_back(0.0f);
        const int64_t blk0 = (int64_t)P.data.size();
        std::vector<std::vector<Run>> runs(nT);
        std::vector<char> direct(nT, 0);
        for (int t = 0; t < nT; ++t) {
            slice_runs(p, part, s, t, runs[t], direct[t]);
            if ((int64_t)runs[t].size() > INT32_MAX / 4)
                return fail(MC_ERR_UNSUPPORTED, "slice term too large");
        }
        std::vector<std::vector<int32_t>> rl(nT), rit(nT);
        assign_lanes(runs, direct, P.Lp, rl, rit);
        // in program order; the slice's active terms are stored first, compacted
        int nact = 0;
        for (int t = 0; t < nT; ++t) {
            SlTerm st = make_slterm(p->raw[t], t, part);
            st.direct = direct[t];
            if (int rc = emit_term_tables(p, part, s, t, runs[t], rl[t], rit[t], blk0, st, P))
                return rc;
            if (st.pp >= 0 && !st.direct && st.niter > 0) P.combine = 1;
            if (st.niter > 0) P.terms[(size_t)s * nT + nact++] = st;
        }
        while (P.data.size() % 4) P.data.push_back(0.0f);
        const int64_t blen = (int64_t)P.data.size() - blk0;
        P.blocks[4 * s] = blk0;
        P.blocks[4 * s + 1] = blen;
        P.blocks[4 * s + 2] = (int64_t)part.priv[s].size();
        P.blocks[4 * s + 3] = nact;
        if (blen > INT32_MAX / 8) return fail(MC_ERR_UNSUPPORTED, "slice data too large");
        P.sdata_floats = std::max<int>(P.sdata_floats, (int)blen);
    }
    if (P.index.empty()) P.index.push_back(0);
    if (P.data.empty()) P.data.assign(4, 0.0f);
    return MC_OK;
}

int plan_slices(const mc_program* p, int S, SlicePlan& P, SlPartition& part) {
    if (int rc = partition_program(p, S, part)) return rc;
    return tile_slices(p, part, P);
}
