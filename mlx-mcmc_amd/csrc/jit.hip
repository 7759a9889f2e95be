// jit.hip — expression terms compiled per program (VERDICT r4 "Next round" 3).
//
// The reference differentiates any MLX expression with mx.grad
// (kernels/hmc.py:53-67); the engine records such terms as node DAGs
// (MC_DIST_EXPR, eval.h eval_expr_n) and, by default, walks them with an
// interpreter: ~23 instructions of decode / dispatch / indirect register
// moves per node visit.  Here the DAG of every expression term
// of a program becomes straight-line C++ — each node's forward value and
// reverse step through the interpreter's own ex_fwd / ex_bwd with the op
// folded to a constant, adjoints accumulated in the interpreter's order —
// and hiprtc compiles the tape kernels' EX instantiations (k_hmc, k_nuts,
// k_mh) with it (eval.h MC_JIT hook).  The arithmetic is the interpreter's,
// operation for operation, so a JIT-compiled run is bit-identical to an
// interpreted one (tests/test_gpu_expr_jit.py).
//
// The generated code depends only on the DAGs' structure (ops, argument
// edges, leaf kinds, passes): leaf offsets, pools, slots and constants are
// read from the program's node table at run time (scalar loads), so models of
// the same structure share one code object whatever their data.  Code
// objects are cached per (source, kernel, options with the device arch,
// hiprtc version) in the process and on disk
// ($MC_JIT_CACHE, else ~/.cache/mcmc355; unwritable: in-process only).
// MC_EXPR_JIT=0 in the environment (or mc_debug_expr_jit(0)) keeps the
// interpreter; a failed compilation falls back to it with a kernel note.
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <fstream>
#include <thread>
#include <sstream>

#include "host.h"
#include "jit.h"
#include "jit_src.inc"

namespace {

int g_expr_jit = -1;  // mc_debug_expr_jit; -1: MC_EXPR_JIT from the environment

struct JitState {
    std::mutex mu;
    bool have_src = false;
    std::string src;
    bool have_lsrc = false;
    std::string lsrc;  // the lane-resident kernels' source (gen_lane_source)
    std::map<std::pair<std::string, int>, hipFunction_t> fns;  // (kernel, device)
    std::vector<hipModule_t> mods;
    std::string error;  // the last compilation failure ("" if none)
};

std::mutex g_cache_mu;
// code objects by cache key, shared by every program of the process
std::unordered_map<uint64_t, std::pair<std::string, std::string>> g_code;  // key -> (name, code)

uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}
uint64_t fnv1a(uint64_t h, const std::string& s) { return fnv1a(h, s.data(), s.size() + 1); }

std::string cache_dir() {
    if (const char* e = std::getenv("MC_JIT_CACHE")) return e;
    if (const char* h = std::getenv("HOME")) return std::string(h) + "/.cache/mcmc355";
    return "";
}

// One expression term's evaluator, the structure of eval_expr_n with the node
// loops unrolled.  Node k's value is vK, its adjoint aK, its partial pK.
void gen_term(std::ostringstream& o, const DevTerm& T, const DevExprNode* N) {
    const int nn = T.expr_n;
    const bool seg = T.primary >= 0;
    auto is_part = [&](int k) {  // partial accumulators: broadcast and gathered (run) leaves
        return N[k].op == MC_EX_LEAF && (N[k].leaf.kind == MC_OP_PSCALAR || N[k].prim != 0);
    };
    o << "template <int WPC, bool VALUE_ONLY>\n"
      << "MC_DEV void jit_t" << T.expr_base
      << "(const DevTerm& T, const DevCtx& P, const float* q, float* g, const Group<WPC>& G,\n"
      << "    bool task, int tid, int nthr, float& lp_acc, float* vpart) {\n"
      << "  (void)task; (void)tid; (void)nthr; (void)vpart; (void)G;\n"
      << "  const MC_CONST DevExprNode* N = cptr(P.nodes) + T.expr_base;\n"
      << "  const float w = T.weight;\n";
    // the leaves' run-time fields (uniform: scalar loads)
    for (int k = 0; k < nn; ++k) {
        if (N[k].op == MC_EX_LEAF) {
            const int kind = N[k].leaf.kind;
            if (N[k].prim || kind == MC_OP_PSCALAR || kind == MC_OP_PVEC || kind == MC_OP_GATHER)
                o << "  const int o" << k << " = N[" << k << "].leaf.poff;\n";
            if (!N[k].prim && (kind == MC_OP_DATA || kind == MC_OP_GATHER))
                o << "  const int64_t l" << k << " = N[" << k << "].leaf.pool;\n";
            if (!N[k].prim && kind == MC_OP_CONST)
                o << "  const float c" << k << " = N[" << k << "].leaf.cval;\n";
            if (kind == MC_OP_PSCALAR)
                o << "  const int s" << k << " = N[" << k << "].leaf.slot;\n"
                  << "  const float qv" << k << " = q[o" << k << "];  // (read once per term)\n";
        } else {
            o << "  const float c" << k << " = N[" << k << "].leaf.cval;\n";
        }
    }
    // the pass count is a function of the leaves' passes (program.hip
    // build_expr_term), so it is a constant here: one pass (the usual case)
    // leaves no pass tests in the element code
    int npass_c = 1;
    for (int k = 0; k < nn; ++k)
        if (N[k].op == MC_EX_LEAF && (N[k].leaf.kind == MC_OP_PVEC || N[k].leaf.kind == MC_OP_GATHER))
            npass_c = std::max(npass_c, (N[k].pass & 15) + 1);
    if (npass_c == T.npass)
        o << "  const int npass = VALUE_ONLY ? 1 : " << npass_c << ";\n";
    else
        o << "  const int npass = VALUE_ONLY ? 1 : T.npass;\n";
    o
      << "  for (int pass = 0; pass < npass; ++pass) {\n";
    for (int k = 0; k < nn; ++k)
        if (is_part(k)) o << "    float p" << k << " = 0.0f;\n";
    // data leaves and gather indices are the element's arguments, so that
    // an unrolled loop issues every load of its elements first
    std::string params, args_of_e;  // "float dK, int xK" / "P.data[lK + e], P.index[lK + e]"
    for (int k = 0; k < nn; ++k) {
        const DevExprNode& d = N[k];
        if (d.op != MC_EX_LEAF || d.prim) continue;
        if (d.leaf.kind == MC_OP_DATA) {
            params += ", float d" + std::to_string(k);
            args_of_e += ", P.data[l" + std::to_string(k) + " + @]";
        } else if (d.leaf.kind == MC_OP_GATHER) {
            params += ", int x" + std::to_string(k);
            args_of_e += ", P.index[l" + std::to_string(k) + " + @]";
        }
    }
    auto args_at = [&](const std::string& e) {
        std::string a = args_of_e;
        for (size_t at; (at = a.find('@')) != std::string::npos;) a.replace(at, 1, e);
        return a;
    };
    o << "    auto element = [&](int64_t e, int kr" << params << ") {\n"
      << "      (void)e; (void)kr;\n";
    auto arg = [&](int a) { return a >= 0 ? "v" + std::to_string(a) : std::string("0.0f"); };
    for (int k = 0; k < nn; ++k) {
        const DevExprNode& d = N[k];
        o << "      const float v" << k << " = ";
        if (d.op == MC_EX_LEAF) {
            const int kind = d.leaf.kind;
            if (d.prim) o << "q[o" << k << " + kr]";
            else if (kind == MC_OP_CONST) o << "c" << k;
            else if (kind == MC_OP_PSCALAR) o << "qv" << k;
            else if (kind == MC_OP_DATA) o << "d" << k;
            else if (kind == MC_OP_PVEC) o << "q[o" << k << " + e]";
            else o << "q[o" << k << " + x" << k << "]";
        } else {
            o << "ex_fwd(" << d.op << ", " << arg(d.a) << ", " << arg(d.b) << ", " << arg(d.c)
              << ", c" << k << ")";
        }
        o << ";\n";
    }
    o << "      if (pass == 0) lp_acc += w * v" << nn - 1 << ";\n"
      << "      if constexpr (VALUE_ONLY) return;\n";
    // (adjoints start at -0: -0 + x == x for every x, so a first contribution
    // needs no add; the interpreter starts them at -0 too)
    for (int k = 0; k < nn; ++k) o << "      float a" << k << " = -0.0f;\n";
    o << "      a" << nn - 1 << " = w;\n";
    for (int k = nn - 1; k >= 0; --k) {
        const DevExprNode& d = N[k];
        if (d.op == MC_EX_LEAF) {
            const int kind = d.leaf.kind;
            if (is_part(k)) {
                o << "      p" << k << " += a" << k << ";\n";
            } else if (kind == MC_OP_PVEC || kind == MC_OP_GATHER) {
                o << "      if (pass == " << (d.pass & 15) << ") g[";
                if (kind == MC_OP_PVEC) o << "(int64_t)o" << k << " + e";
                else o << "(int64_t)o" << k << " + x" << k;
                o << "] += a" << k << ";\n";
            }
            continue;
        }
        o << "      { float dx, dy, dz; ex_bwd(" << d.op << ", " << arg(d.a) << ", " << arg(d.b)
          << ", " << arg(d.c) << ", v" << k << ", a" << k << ", c" << k << ", dx, dy, dz);\n"
          << "        a" << d.a << " += dx;";
        if (d.b >= 0) o << " a" << d.b << " += dy;";
        if (d.c >= 0) o << " a" << d.c << " += dz;";
        o << " }\n";
    }
    o << "    };\n";
    // terms over constants, broadcast parameters and data only (no vector
    // parameter leaves, so no gradient writes whose order could change) also
    // get a paired element: two elements' nodes in packed FP32 (eval.h
    // ex2_fwd / ex2_bwd, bit-identical per component), sums taken in element
    // order
    bool pairs = !seg;
    for (int k = 0; k < nn; ++k)
        if (N[k].op == MC_EX_LEAF && (N[k].prim || N[k].leaf.kind == MC_OP_PVEC ||
                                      N[k].leaf.kind == MC_OP_GATHER))
            pairs = false;
    if (pairs) {
        std::string params2;
        for (int k = 0; k < nn; ++k)
            if (N[k].op == MC_EX_LEAF && N[k].leaf.kind == MC_OP_DATA)
                params2 += ", exf2 d" + std::to_string(k);
        o << "    auto element2 = [&](" << (params2.empty() ? std::string() : params2.substr(2))
          << ") {\n";
        auto arg2 = [&](int a) { return a >= 0 ? "v" + std::to_string(a) : std::string("z2"); };
        o << "      const exf2 z2 = {0.0f, 0.0f};\n      (void)z2;\n";
        for (int k = 0; k < nn; ++k) {
            const DevExprNode& d = N[k];
            o << "      const exf2 v" << k << " = ";
            if (d.op == MC_EX_LEAF) {
                const int kind = d.leaf.kind;
                if (kind == MC_OP_CONST) o << "exf2{c" << k << ", c" << k << "}";
                else if (kind == MC_OP_PSCALAR) o << "exf2{qv" << k << ", qv" << k << "}";
                else o << "d" << k;
            } else {
                o << "ex2_fwd(" << d.op << ", " << arg2(d.a) << ", " << arg2(d.b) << ", " << arg2(d.c)
                  << ", c" << k << ")";
            }
            o << ";\n";
        }
        o << "      if (pass == 0) { const exf2 wv = w * v" << nn - 1
          << "; lp_acc += wv.x; lp_acc += wv.y; }\n"
          << "      if constexpr (VALUE_ONLY) return;\n";
        for (int k = 0; k < nn; ++k) o << "      exf2 a" << k << " = {-0.0f, -0.0f};\n";
        o << "      a" << nn - 1 << " = exf2{w, w};\n";
        for (int k = nn - 1; k >= 0; --k) {
            const DevExprNode& d = N[k];
            if (d.op == MC_EX_LEAF) {
                if (is_part(k)) o << "      p" << k << " += a" << k << ".x; p" << k << " += a" << k << ".y;\n";
                continue;
            }
            o << "      { exf2 dx, dy, dz; ex2_bwd(" << d.op << ", " << arg2(d.a) << ", " << arg2(d.b)
              << ", " << arg2(d.c) << ", v" << k << ", a" << k << ", c" << k << ", dx, dy, dz);\n"
              << "        a" << d.a << " += dx;";
            if (d.b >= 0) o << " a" << d.b << " += dy;";
            if (d.c >= 0) o << " a" << d.c << " += dz;";
            o << " }\n";
        }
        o << "    };\n";
    }
    if (!seg) {
        // four elements per trip, their loads first (the element order, and
        // so every sum, is the strided loop's).  (Prefetching the next trip's
        // loads behind this trip's arithmetic measured slower: the loop is
        // issue-bound, and pinning the loads costs the scheduler its freedom.)
        o << "    int64_t i = tid;\n"
          << "    const int64_t st = nthr;\n"
          << "    for (; i + 3 * st < T.n; i += 4 * st) {\n"
          << "      const int64_t e0 = i, e1 = i + st, e2 = i + 2 * st, e3 = i + 3 * st;\n";
        {
            std::string decl[4];
            for (int u = 0; u < 4; ++u) {
                const std::string a = args_at("e" + std::to_string(u));
                // a = ", x, y": named temporaries t<u>_<n>
                std::string names;
                size_t pos = 0;
                int n = 0;
                while ((pos = a.find(", ", pos)) != std::string::npos) {
                    const size_t nxt = a.find(", ", pos + 2);
                    const std::string ex =
                        a.substr(pos + 2, nxt == std::string::npos ? std::string::npos : nxt - pos - 2);
                    const bool isint = ex.rfind("P.index", 0) == 0;
                    o << "      const " << (isint ? "int" : "float") << " t" << u << "_" << n << " = "
                      << ex << ";\n";
                    names += ", t" + std::to_string(u) + "_" + std::to_string(n);
                    ++n;
                    pos += 2;
                }
                decl[u] = names;
            }
            if (pairs) {
                // decl[u] = ", t<u>_0, t<u>_1, ...": pair the loads of elements 2h, 2h + 1
                for (int h = 0; h < 2; ++h) {
                    std::string a = decl[2 * h], b = decl[2 * h + 1], call;
                    size_t pa = 0, pb = 0;
                    while ((pa = a.find(", ", pa)) != std::string::npos) {
                        pb = b.find(", ", pb);
                        const size_t na = a.find(", ", pa + 2), nb = b.find(", ", pb + 2);
                        call += ", exf2{" + a.substr(pa + 2, na == std::string::npos ? std::string::npos : na - pa - 2) +
                                ", " + b.substr(pb + 2, nb == std::string::npos ? std::string::npos : nb - pb - 2) + "}";
                        pa += 2;
                        pb += 2;
                    }
                    o << "      element2(" << (call.empty() ? std::string() : call.substr(2)) << ");\n";
                }
            } else {
                for (int u = 0; u < 4; ++u) o << "      element(e" << u << ", 0" << decl[u] << ");\n";
            }
        }
        o << "    }\n"
          << "    for (; i < T.n; i += st) element(i, 0" << args_at("i") << ");\n";
    } else {
        o << "    const bool split = T.ncomb > 0;\n"
          << "    const int wave = G.tid >> 6;\n"
          << "    const int lane = G.tid & 63;\n"
          << "    const MC_CONST int* tiles = cptr(P.index) + T.tile_base;\n"
          << "    const int* lanes = P.index + T.lane_base;\n"
          << "    for (int t = wave; t < T.ntiles; t += WPC) {\n"
          << "      const int off = tiles[3 * t];\n"
          << "      const int v = t * 64 + lane;\n"
          << "      const bool valid = v < T.nvirt;\n"
          << "      const int kr = valid ? lanes[2 * v] : 0;\n"
          << "      const int len = valid ? lanes[2 * v + 1] : 0;\n";
        for (int k = 0; k < nn; ++k)
            if (N[k].op == MC_EX_LEAF && N[k].prim) o << "      p" << k << " = 0.0f;\n";
        o << "      for (int u = 0; u < len; ++u) { const int64_t e = seg_elem(off, u, lane); "
          << "element(e, kr" << args_at("e") << "); }\n"
          << "      if (!VALUE_ONLY && valid) {\n";
        for (int k = 0; k < nn; ++k) {
            if (N[k].op != MC_EX_LEAF || !N[k].prim) continue;
            o << "        if (pass == " << N[k].pass << ") { if (split) vpart[" << (N[k].prim - 1)
              << " * T.nvirt + v] = p" << k << "; else g[o" << k << " + kr] += p" << k << "; }\n";
        }
        o << "      }\n"
          << "    }\n"
          << "    if (!VALUE_ONLY && split) {\n"
          << "      G.sync();\n"
          << "      const int* comb = P.index + T.comb_base;\n"
          << "      for (int c = G.tid; c < T.ncomb; c += G.T) {\n"
          << "        const int kc = comb[3 * c], vf = comb[3 * c + 1], vc = comb[3 * c + 2];\n"
          << "        (void)kc; (void)vf; (void)vc;\n";
        for (int k = 0; k < nn; ++k) {
            if (N[k].op != MC_EX_LEAF || !N[k].prim) continue;
            o << "        if (pass == " << N[k].pass << ") {\n"
              << "          const float* vp = vpart + " << (N[k].prim - 1) << " * T.nvirt;\n"
              << "          float sum = vp[vf];\n"
              << "          for (int j = 1; j < vc; ++j) sum += vp[vf + j];\n"
              << "          g[o" << k << " + kc] += sum;\n"
              << "        }\n";
        }
        o << "      }\n"
          << "    }\n";
    }
    o << "    if (!VALUE_ONLY && pass == 0) {\n";
    for (int k = 0; k < nn; ++k) {
        if (N[k].op != MC_EX_LEAF || N[k].leaf.kind != MC_OP_PSCALAR) continue;
        o << "      if (task) flush_slot_task(G, s" << k << ", p" << k << "); else flush_slot(G, s" << k
          << ", p" << k << ");\n";
    }
    o << "    }\n"
      << "    if (!VALUE_ONLY && pass + 1 < npass) G.sync();\n"
      << "  }\n"
      << "}\n\n";
}

// The program's generated source: every expression term's evaluator and
// the dispatch the eval.h hook calls.
// eval.h eval_term's choice of path for a fused term (the same predicates):
// a strided moment-sum code 0..11 as bit `code` of *su, else a path bit.
bool host_is_vec(int kind) {
    return kind == MC_OP_DATA || kind == MC_OP_PVEC || kind == MC_OP_GATHER;
}
int host_fast_kind(const DevOperand& o) {
    if (o.xf != MC_XF_NONE && host_is_vec(o.kind)) return -1;
    return o.kind == MC_OP_DATA ? 1 : (o.kind == MC_OP_PVEC ? 2 : (host_is_vec(o.kind) ? -1 : 0));
}
void fused_paths(const mc_program* p, uint32_t* paths, uint32_t* su, uint32_t* dists) {
    *paths = 0;
    *su = 0;
    *dists = 0;
    for (const DevTerm& T : p->terms) {
        if (T.dist == MC_DIST_EXPR) continue;
        *dists |= 1u << T.dist;
        const bool normal = T.dist == MC_DIST_NORMAL;
        const bool moment_dist = normal || T.dist == MC_DIST_HALFNORMAL;
        const bool scale_vec = host_is_vec(T.op[2].kind);
        if (T.primary < 0) {
            const int fv = host_fast_kind(T.op[0]);
            const int fl = normal ? host_fast_kind(T.op[1]) : 0;
            if (moment_dist && !scale_vec && fv >= 0 && fl >= 0 && !T.affine)
                *su |= 1u << (normal ? (fv * 3 + fl) : (9 + fv));
            else
                *paths |= MC_PATH_STRIDED_GENERIC;
        } else {
            const int other_kind = T.primary == 1 ? T.op[0].kind : T.op[1].kind;
            const int prim_xf = T.op[T.primary].xf;
            const bool fast = normal && !scale_vec && T.primary <= 1 && other_kind == MC_OP_DATA &&
                              !T.affine && prim_xf == MC_XF_NONE;
            *paths |= fast ? MC_PATH_SEG_NORMAL : MC_PATH_SEG_GENERIC;
        }
    }
}

std::string gen_source(const mc_program* p) {
    std::ostringstream o;
    uint32_t paths = 0, su = 0, dists = 0;
    fused_paths(p, &paths, &su, &dists);
    o << "// generated by jit.hip for one program: do not edit\n"
      << "#define MC_JIT_PATHS " << paths << "u\n#define MC_JIT_SU " << su << "u\n"
      << "#define MC_JIT_DISTS " << dists << "u\n"
      << "#include \"hmc.h\"\n#include \"nuts.h\"\n#include \"mh.h\"\n"
      << "namespace mc {\n";
    std::vector<int32_t> bases;
    for (const DevTerm& T : p->terms) {
        if (T.dist != MC_DIST_EXPR) continue;
        if (std::find(bases.begin(), bases.end(), T.expr_base) != bases.end()) continue;
        bases.push_back(T.expr_base);
        gen_term(o, T, p->nodes.data() + T.expr_base);
    }
    o << "template <int WPC, bool VALUE_ONLY>\n"
      << "MC_DEV void mc_jit_expr(const DevTerm& T, const DevCtx& P, const float* q, float* g,\n"
      << "    const Group<WPC>& G, bool task, int tid, int nthr, float& lp_acc, float* vpart) {\n"
      << "  switch (T.expr_base) {\n";
    for (int32_t b : bases)
        o << "    case " << b << ": jit_t" << b
          << "<WPC, VALUE_ONLY>(T, P, q, g, G, task, tid, nthr, lp_acc, vpart); break;\n";
    o << "    default: break;\n  }\n}\n}  // namespace mc\n";
    return o.str();
}

// ---- lane-resident expression terms (lanes.h LS_EXPR) -----------------------
// A float constant as its bit pattern (exact in the generated source).
std::string flit(float v) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    char buf[48];
    std::snprintf(buf, sizeof buf, "__uint_as_float(0x%08xu)", b);
    return buf;
}

// One LS_EXPR term's lane sweep: lane j's run of the term's elements in its
// slice (a chunk term: slot 0, lengths at len_off), every node's forward
// value and reverse step through eval.h ex2_fwd / ex2_bwd (the tape's
// arithmetic, component for component), the broadcast leaves' adjoints
// summed over the run.  Data leaf e is tile eoff[e] (one tile per data
// array, in node order).  Constants are literals.  LP = false leaves out
// what only log p needs (the compiler drops the nodes no adjoint reads).
//   two chains (k_hmc_lr, ONE = false): the wave's two chains packed per
//     element (exf2 = chain 0, chain 1); a broadcast leaf reads the raw
//     parameter of shared ordinal K from lane 2K + c of sh.q;
//   one chain (k_nuts_sl, ONE = true): two elements packed (exf2 = elements
//     e, e + 1 of the chain); lane K of sh.q holds shared ordinal K; the
//     pairs' two sums are added at the end.
// A transformed broadcast parameter (LanePlan::shxf) is read through its
// transform node only (the planner checks it): that node reads the lane's
// transformed value sh.v and its adjoint is the value's cotangent.
//   a grouped term (LanePlan::gx_off: parameter-vector / gather leaves, two
//     chains): the sweep is a lambda over one bundle's run (its tile offset,
//     length, the bundle's private values gq<off> of both chains and their
//     adjoint sums ga<off>, summed over the run in element order as the
//     broadcast leaves' p<k>), called once per first slot r0 of the lane with
//     compile-time slot indices (lanes.h lr_slot_q / lr_slot_g_add).
// elements interleaved per trip of a grouped term's run (two chains): 4, or 2
// with MC_LANE_GROUP_INTERLEAVE=2 in the environment (A/B timing)
int grp_interleave() {
    const char* e = std::getenv("MC_LANE_GROUP_INTERLEAVE");
    return (e && e[0] == '2') ? 2 : 4;
}
bool lane_term_grouped(const DevTerm& T, const LanePlan& L) {
    for (int k = 0; k < T.expr_n; ++k)
        if ((size_t)(T.expr_base + k) < L.gx_off.size() && L.gx_off[T.expr_base + k] >= 0)
            return true;
    return false;
}
void gen_lane_term(std::ostringstream& o, const DevTerm& T, const DevExprNode* N,
                   const LanePlan& L, bool one) {
    const int nn = T.expr_n;
    const bool grp = lane_term_grouped(T, L);
    auto goff = [&](int k) { return grp ? L.gx_off[T.expr_base + k] : -1; };
    std::vector<int> goffs;  // the distinct slot offsets, ascending
    for (int k = 0; k < nn; ++k)
        if (goff(k) >= 0 && std::find(goffs.begin(), goffs.end(), goff(k)) == goffs.end())
            goffs.push_back(goff(k));
    std::sort(goffs.begin(), goffs.end());
    auto ordinal = [&](int poff) {
        for (int k = 0; k < L.Dsh; ++k)
            if (L.shl[k] == poff) return k;
        return 0;
    };
    auto sh_read = [&](const char* f, int K) {  // both components of shared ordinal K
        std::ostringstream x;
        if (one) x << "exf2{rl(sh." << f << ", " << K << "), rl(sh." << f << ", " << K << ")}";
        else x << "exf2{rl(sh." << f << ", " << 2 * K << "), rl(sh." << f << ", " << 2 * K + 1 << ")}";
        return x.str();
    };
    if (grp && one)
        o << "template <bool LP, bool G, int RS>\nMC_DEV void jit_lgo" << T.expr_base
          << "(const MC_CONST LrTerm* T, const float* sd, int j, const float (&q)[RS],\n"
          << "    float (&g)[RS], const LrShared& sh, float& lpp, float (&gsh)[kLrMaxShared]) {\n"
          << "  const int32_t* lens = (const int32_t*)sd + T->len_off;\n"
          << "  const int nslot = T->nslot;\n  (void)g;\n";
    else if (grp)
        o << "template <bool LP, int RS>\nMC_DEV void jit_lg" << T.expr_base
          << "(const MC_CONST LrTerm* T, const float* sd, int j, LrPriv<RS>& R, const LrShared& sh,\n"
          << "    float (&lpp)[2], float (&gshp)[kLrMaxShared][2]) {\n"
          << "  const int32_t* lens = (const int32_t*)sd + T->len_off;\n"
          << "  const int nslot = T->nslot;\n";
    else
    o << (one ? "template <bool LP, bool G>\n" : "template <bool LP>\n")
      << "MC_DEV void jit_l" << (one ? "o" : "t") << T.expr_base
      << "(const MC_CONST LrTerm* T, const float* sd, int j, const LrShared& sh,\n"
      << (one ? "    float& lpp, float (&gsh)[kLrMaxShared]) {\n"
              : "    float (&lpp)[2], float (&gshp)[kLrMaxShared][2]) {\n")
      << "  const int len = ((const int32_t*)sd)[T->len_off + j];\n";
    o << "  const exf2 wv = {T->weight, T->weight};\n"
      << "  exf2 lpa = {0.0f, 0.0f}, lpt = {0.0f, 0.0f};\n  (void)lpa; (void)lpt;\n"
      << (one ? "  (void)gsh;\n" : "");
    auto xf_node = [&](int k) {
        const DevExprNode& d = N[k];
        if ((d.op != MC_EX_EXP && d.op != MC_EX_LOG) || d.a < 0) return -1;
        const DevExprNode& x = N[d.a];
        if (x.op != MC_EX_LEAF || x.leaf.kind != MC_OP_PSCALAR) return -1;
        const int K = ordinal(x.leaf.poff);
        const int xf = L.shxf[K];
        if (xf == MC_XF_NONE || d.op != (xf == MC_XF_EXP ? MC_EX_EXP : MC_EX_LOG)) return -1;
        return K;
    };
    auto raw_leaf = [&](int k) {  // a broadcast leaf read raw (its own cotangent)
        return N[k].op == MC_EX_LEAF && N[k].leaf.kind == MC_OP_PSCALAR &&
               L.shxf[ordinal(N[k].leaf.poff)] == MC_XF_NONE;
    };
    auto part = [&](int k) { return xf_node(k) >= 0 || raw_leaf(k); };  // a cotangent sum
    std::vector<int> dleaves;
    for (int k = 0; k < nn; ++k) {
        const DevExprNode& d = N[k];
        if (xf_node(k) >= 0) {
            o << "  const exf2 v" << k << " = " << sh_read("v", xf_node(k)) << ";\n";
        } else if (d.op == MC_EX_LEAF) {
            if (d.leaf.kind == MC_OP_PSCALAR && !raw_leaf(k)) {
                o << "  const exf2 v" << k << " = {0.0f, 0.0f};  // (read through node transforms)\n";
            } else if (d.leaf.kind == MC_OP_CONST) {
                o << "  const exf2 v" << k << " = {" << flit(d.leaf.cval) << ", " << flit(d.leaf.cval)
                  << "};\n";
            } else if (d.leaf.kind == MC_OP_PSCALAR) {
                o << "  const exf2 v" << k << " = " << sh_read("q", ordinal(d.leaf.poff)) << ";\n";
            } else if (d.leaf.kind == MC_OP_DATA) {  // one tile per array (leaves of one array share it)
                bool dup = false;
                for (int r : dleaves) dup |= N[r].leaf.pool == d.leaf.pool;
                if (!dup) {
                    if (!grp)  // (a grouped term: per run, below)
                        o << "  const float* d" << k << " = sd + T->eoff[" << dleaves.size()
                          << "] + 4 * j;\n";
                    dleaves.push_back(k);
                }
            }
        } else {
            o << "  const float c" << k << " = " << flit(d.leaf.cval) << ";\n";
        }
        if (part(k)) o << "  exf2 p" << k << " = {0.0f, 0.0f}, t" << k << " = {0.0f, 0.0f};\n";
    }
    o << "  const exf2 z2 = {0.0f, 0.0f};\n  (void)z2;\n";
    if (grp) {  // one bundle's run
        o << "  auto run = [&](const int toff, const int len";
        for (int g : goffs) o << ", const exf2 gq" << g;
        for (int g : goffs) o << ", exf2& ga" << g;
        if (one)  // (the ragged tail's sums: component x only)
            for (int g : goffs) o << ", exf2& gt" << g;
        o << ") {\n";
        for (size_t i = 0; i < dleaves.size(); ++i)
            o << "  const float* d" << dleaves[i] << " = sd + T->eoff[" << i << "] + toff + 4 * j;\n";
        for (int k = 0; k < nn; ++k)
            if (goff(k) >= 0) o << "  const exf2 v" << k << " = gq" << goff(k) << ";\n";
    }
    // E elements at once, their statements interleaved node by node (the
    // elements' dependency chains are independent, so the hazards of one —
    // transcendental results, packed read-after-write — are covered by the
    // others' instructions); sums in element order.  x[e][i]: element e's
    // value of data array i (an exf2 expression); acc: the accumulators' prefix
    // ("p" / "lpa" for the runs, "t" / "lpt" for a one-chain tail)
    auto emit = [&](int E, const std::vector<std::vector<std::string>>& x, const char* ind,
                    bool tail) {
        auto nm = [&](char c, int k, int e) {
            // leaves outside the element (constants, parameters) keep one name
            const DevExprNode& d = N[k];
            const bool shared = xf_node(k) >= 0 ||
                                (d.op == MC_EX_LEAF && d.leaf.kind != MC_OP_DATA);
            if (c == 'v' && shared) return "v" + std::to_string(k);
            return std::string(1, c) + std::to_string(k) + "_" + std::to_string(e);
        };
        auto argn = [&](int a, int e) { return a >= 0 ? nm('v', a, e) : std::string("z2"); };
        const char* pa = tail ? "t" : "p";
        for (int k = 0; k < nn; ++k) {
            const DevExprNode& d = N[k];
            for (int e = 0; e < E; ++e) {
                if (d.op == MC_EX_LEAF) {
                    if (d.leaf.kind == MC_OP_DATA) {
                        size_t i = 0;
                        while (N[dleaves[i]].leaf.pool != d.leaf.pool) ++i;
                        o << ind << "const exf2 " << nm('v', k, e) << " = " << x[e][i] << ";\n";
                    }
                    continue;
                }
                if (xf_node(k) >= 0) continue;
                o << ind << "const exf2 " << nm('v', k, e) << " = ex2_fwd(" << d.op << ", "
                  << argn(d.a, e) << ", " << argn(d.b, e) << ", " << argn(d.c, e) << ", c" << k
                  << ");\n";
            }
        }
        for (int e = 0; e < E; ++e)
            o << ind << "if constexpr (LP) " << (tail ? "lpt" : "lpa") << " += wv * "
              << nm('v', nn - 1, e) << ";\n";
        // (one chain, G = false: the value only — k_mh_sl's forward pass)
        if (one) o << ind << "if constexpr (G) {\n";
        // (adjoints start at -0, as the tape's: -0 + x == x)
        for (int k = 0; k < nn; ++k)
            for (int e = 0; e < E; ++e)
                o << ind << "exf2 " << nm('a', k, e) << " = {-0.0f, -0.0f};\n";
        for (int e = 0; e < E; ++e) o << ind << nm('a', nn - 1, e) << " = wv;\n";
        for (int k = nn - 1; k >= 0; --k) {
            const DevExprNode& d = N[k];
            if (goff(k) >= 0) {  // a gathered leaf: its bundle slot's adjoint sum
                for (int e = 0; e < E; ++e)
                    o << ind << (tail ? "gt" : "ga") << goff(k) << " += " << nm('a', k, e) << ";\n";
                continue;
            }
            if (d.op == MC_EX_LEAF && !raw_leaf(k)) continue;
            for (int e = 0; e < E; ++e) {
                if (part(k)) {
                    o << ind << pa << k << " += " << nm('a', k, e) << ";\n";
                    continue;
                }
                o << ind << "{ exf2 dx, dy, dz; ex2_bwd(" << d.op << ", " << argn(d.a, e) << ", "
                  << argn(d.b, e) << ", " << argn(d.c, e) << ", " << nm('v', k, e) << ", "
                  << nm('a', k, e) << ", c" << k << ", dx, dy, dz);\n"
                  << ind << "  " << nm('a', d.a, e) << " += dx;";
                if (d.b >= 0) o << " " << nm('a', d.b, e) << " += dy;";
                if (d.c >= 0) o << " " << nm('a', d.c, e) << " += dz;";
                o << " (void)dx; (void)dy; (void)dz; }\n";
            }
        }
        if (one) o << ind << "}\n";
    };
    // four elements per trip (a 16-byte LDS load per data array): two chains,
    // four elements interleaved; one chain, two element pairs interleaved
    const char* comp[4] = {"x", "y", "z", "w"};
    o << "  int u = 0;\n  for (; u + 4 <= len; u += 4) {\n";
    for (int k : dleaves)
        o << "    const float4 X" << k << " = *(const float4*)(d" << k << " + (u >> 2) * 256);\n";
    if (grp && one) {  // two element pairs interleaved, as a chunk term's
        std::vector<std::vector<std::string>> x(2);
        for (int e = 0; e < 2; ++e)
            for (int k : dleaves) {
                const std::string X = "X" + std::to_string(k) + ".";
                x[e].push_back("exf2{" + X + comp[2 * e] + ", " + X + comp[2 * e + 1] + "}");
            }
        emit(2, x, "    ", false);
    } else if (grp) {  // kGrpInterleave elements at once, the trip's four in element order
        const int kGrpInterleave = grp_interleave();
        for (int h = 0; h < 4; h += kGrpInterleave) {
            std::vector<std::vector<std::string>> x(kGrpInterleave);
            for (int e = 0; e < kGrpInterleave; ++e)
                for (int k : dleaves) {
                    const std::string X = "X" + std::to_string(k) + ".";
                    x[e].push_back("exf2{" + X + comp[h + e] + ", " + X + comp[h + e] + "}");
                }
            o << "    {\n";
            emit(kGrpInterleave, x, "    ", false);
            o << "    }\n";
        }
    } else {
        const int E = one ? 2 : 4;
        std::vector<std::vector<std::string>> x(E);
        for (int e = 0; e < E; ++e)
            for (int k : dleaves) {
                const std::string X = "X" + std::to_string(k) + ".";
                x[e].push_back(one ? "exf2{" + X + comp[2 * e] + ", " + X + comp[2 * e + 1] + "}"
                                   : "exf2{" + X + comp[e] + ", " + X + comp[e] + "}");
            }
        emit(E, x, "    ", false);
    }
    // the ragged tail, one element at a time (one chain: the element in both
    // components, its sums taken from component x only)
    o << "  }\n  for (; u < len; ++u) {\n    const int ou = (u >> 2) * 256 + (u & 3);\n";
    {
        std::vector<std::vector<std::string>> x(1);
        for (int k : dleaves) {
            const std::string d = "d" + std::to_string(k) + "[ou]";
            x[0].push_back("exf2{" + d + ", " + d + "}");
        }
        emit(1, x, "    ", one);
    }
    o << "  }\n";
    if (grp) {
        // the lane's bundles, by first slot (unrolled: compile-time slot indices)
        o << "  };\n";
        for (int r0 = 0; r0 < kLrMaxSlots; ++r0) {
            o << "  if constexpr (" << r0 << " < RS) {\n    const int len = " << r0
              << " < nslot ? lens[" << r0 << " * 64 + j] : 0;\n    if (len > 0) {\n";
            for (int g : goffs) o << "      exf2 ga" << g << " = {0.0f, 0.0f};\n";
            if (one)
                for (int g : goffs) o << "      exf2 gt" << g << " = {0.0f, 0.0f};\n";
            o << "      run(T->toff[" << r0 << "], len";
            for (int g : goffs)
                o << (one ? ", lr_slot1_q<RS, " : ", lr_slot_q<RS, ") << r0 + g << (one ? ">(q)" : ">(R)");
            for (int g : goffs) o << ", ga" << g;
            if (one)
                for (int g : goffs) o << ", gt" << g;
            o << ");\n";
            for (int g : goffs) {
                if (one)
                    o << "      if constexpr (G) lr_slot1_g_add<RS, " << r0 + g << ">(g, (ga" << g
                      << ".x + ga" << g << ".y) + gt" << g << ".x);\n";
                else
                    o << "      lr_slot_g_add<RS, " << r0 + g << ">(R, ga" << g << ");\n";
            }
            o << "    }\n  }\n";
        }
    }
    if (one) {
        o << "  if constexpr (LP) lpp += (lpa.x + lpa.y) + lpt.x;\n  if constexpr (G) {\n";
        for (int k = 0; k < nn; ++k) {
            if (!part(k)) continue;
            const int K = xf_node(k) >= 0 ? xf_node(k) : ordinal(N[k].leaf.poff);
            o << "    gsh[" << K << "] += (p" << k << ".x + p" << k << ".y) + t" << k << ".x;\n";
        }
        o << "  }\n";
    } else {
        o << "  if constexpr (LP) {\n    lpp[0] += lpa.x;\n    lpp[1] += lpa.y;\n  }\n";
        for (int k = 0; k < nn; ++k) {
            if (!part(k)) continue;
            const int K = xf_node(k) >= 0 ? xf_node(k) : ordinal(N[k].leaf.poff);
            o << "  gshp[" << K << "][0] += p" << k << ".x;\n  gshp[" << K << "][1] += p" << k
              << ".y;\n";
        }
    }
    o << "}\n\n";
}

// The lane-resident kernels' source for a program with LS_EXPR terms:
// lanes.h and nuts_sliced.h with their expression hooks defined (two chains
// per wave: k_hmc_lr; one: k_nuts_sl).
std::string gen_lane_source(const mc_program* p) {
    std::ostringstream o;
    bool any_grp = false;
    for (const DevTerm& T : p->raw) any_grp |= T.dist == MC_DIST_EXPR && lane_term_grouped(T, p->lr);
    o << "// generated by jit.hip (lane-resident expression terms) for one program: do not edit\n"
      << "#define MC_JIT_LANES 1\n" << (any_grp ? "#define MC_JIT_LANES_GROUPED 1\n" : "")
      << "#include \"mh_sliced.h\"\nnamespace mc {\n";
    std::vector<int32_t> bases, gbases;  // chunk terms, grouped terms
    for (const DevTerm& T : p->raw) {
        if (T.dist != MC_DIST_EXPR) continue;
        if (std::find(bases.begin(), bases.end(), T.expr_base) != bases.end() ||
            std::find(gbases.begin(), gbases.end(), T.expr_base) != gbases.end())
            continue;
        if (lane_term_grouped(T, p->lr)) {  // (the leaves as validated: host.h mc_program::rnodes)
            gbases.push_back(T.expr_base);
            gen_lane_term(o, T, p->rnodes.data() + T.expr_base, p->lr, false);
            gen_lane_term(o, T, p->rnodes.data() + T.expr_base, p->lr, true);
            continue;
        }
        bases.push_back(T.expr_base);
        gen_lane_term(o, T, p->nodes.data() + T.expr_base, p->lr, false);
        gen_lane_term(o, T, p->nodes.data() + T.expr_base, p->lr, true);
    }
    if (any_grp) {
        o << "template <int RS>\n"
          << "MC_DEV void mc_jit_lane_gexpr(const MC_CONST LrTerm* T, const float* sd, int j,\n"
          << "    LrPriv<RS>& R, const LrShared& sh, float (&lpp)[2],\n"
          << "    float (&gshp)[kLrMaxShared][2], bool need_lp) {\n  switch (T->expr_base) {\n";
        for (int32_t b : gbases)
            o << "    case " << b << ":\n      if (need_lp) jit_lg" << b
              << "<true, RS>(T, sd, j, R, sh, lpp, gshp);\n      else jit_lg" << b
              << "<false, RS>(T, sd, j, R, sh, lpp, gshp);\n      break;\n";
        o << "    default: break;\n  }\n}\n"
          << "template <int RS>\n"
          << "MC_DEV void mc_jit_lane_gexpr1(const MC_CONST LrTerm* T, const float* sd, int j,\n"
          << "    const float (&q)[RS], float (&g)[RS], const LrShared& sh, float& lpp,\n"
          << "    float (&gsh)[kLrMaxShared]) {\n  switch (T->expr_base) {\n";
        for (int32_t b : gbases)
            o << "    case " << b << ": jit_lgo" << b
              << "<true, true, RS>(T, sd, j, q, g, sh, lpp, gsh); break;\n";
        o << "    default: break;\n  }\n}\n"
          << "template <int RS>\n"
          << "MC_DEV void mc_jit_lane_gexpr1v(const MC_CONST LrTerm* T, const float* sd, int j,\n"
          << "    const float (&q)[RS], const LrShared& sh, float& lpp) {\n"
          << "  float g[RS], gsh[kLrMaxShared];\n  switch (T->expr_base) {\n";
        for (int32_t b : gbases)
            o << "    case " << b << ": jit_lgo" << b
              << "<true, false, RS>(T, sd, j, q, g, sh, lpp, gsh); break;\n";
        o << "    default: break;\n  }\n}\n";
    }
    o << "MC_DEV void mc_jit_lane_expr(const MC_CONST LrTerm* T, const float* sd, int j,\n"
      << "    const LrShared& sh, float (&lpp)[2], float (&gshp)[kLrMaxShared][2], bool need_lp) {\n"
      << "  switch (T->expr_base) {\n";
    for (int32_t b : bases)
        o << "    case " << b << ":\n      if (need_lp) jit_lt" << b
          << "<true>(T, sd, j, sh, lpp, gshp);\n      else jit_lt" << b
          << "<false>(T, sd, j, sh, lpp, gshp);\n      break;\n";
    o << "    default: break;\n  }\n}\n"
      << "MC_DEV void mc_jit_lane_expr1(const MC_CONST LrTerm* T, const float* sd, int j,\n"
      << "    const LrShared& sh, float& lpp, float (&gsh)[kLrMaxShared]) {\n"
      << "  switch (T->expr_base) {\n";
    for (int32_t b : bases)
        o << "    case " << b << ": jit_lo" << b << "<true, true>(T, sd, j, sh, lpp, gsh); break;\n";
    o << "    default: break;\n  }\n}\n"
      << "MC_DEV void mc_jit_lane_expr1v(const MC_CONST LrTerm* T, const float* sd, int j,\n"
      << "    const LrShared& sh, float& lpp) {\n  float gsh[kLrMaxShared];\n"
      << "  switch (T->expr_base) {\n";
    for (int32_t b : bases)
        o << "    case " << b << ": jit_lo" << b << "<true, false>(T, sd, j, sh, lpp, gsh); break;\n";
    o << "    default: break;\n  }\n}\n}  // namespace mc\n";
    return o.str();
}

bool is_lane_kernel(const std::string& kernel) {
    return kernel.rfind("mc::k_hmc_lr<", 0) == 0 || kernel.rfind("mc::k_nuts_sl<", 0) == 0 ||
           kernel.rfind("mc::k_mh_sl<", 0) == 0;
}

// hiprtc options: the device's own architecture (gcnArchName's processor,
// e.g. "gfx950"), so a library built for another ARCH still compiles for the
// card it runs on; the arch and hiprtc's version are part of the cache key.
std::vector<std::string> jit_opts(int dev) {
    std::string arch = "gfx950";
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.gcnArchName[0]) {
        arch = prop.gcnArchName;
        const size_t colon = arch.find(':');
        if (colon != std::string::npos) arch.resize(colon);
    }
    return {"--offload-arch=" + arch, "-O3", "-std=c++17", "-ffp-contract=off",
            "-fno-gpu-flush-denormals-to-zero", "-fno-slp-vectorize", "-DMC_JIT=1"};
}

uint64_t cache_key(const std::string& src, const std::string& kernel,
                   const std::vector<std::string>& opts) {
    uint64_t h = 1469598103934665603ull;
    h = fnv1a(h, src);
    h = fnv1a(h, kernel);
    for (const std::string& o : opts) h = fnv1a(h, o);
    int major = 0, minor = 0;
    (void)hiprtcVersion(&major, &minor);
    const int ver[2] = {major, minor};
    h = fnv1a(h, ver, sizeof ver);
    for (int i = 0; i < kJitNumHeaders; ++i) {
        h = fnv1a(h, std::string(kJitHeaderNames[i]));
        h = fnv1a(h, std::string(kJitHeaderTexts[i]));
    }
    return h;
}

std::string cache_path(uint64_t key) {
    const std::string dir = cache_dir();
    if (dir.empty()) return "";
    char fn[64];
    std::snprintf(fn, sizeof fn, "/%016llx.co", (unsigned long long)key);
    return dir + fn;
}

bool disk_load(uint64_t key, std::string& name, std::string& code) {
    const std::string path = cache_path(key);
    if (path.empty()) return false;
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    uint32_t n = 0;
    if (!f.read((char*)&n, 4) || n == 0 || n > 4096) return false;
    name.resize(n);
    if (!f.read(&name[0], n)) return false;
    std::ostringstream rest;
    rest << f.rdbuf();
    code = rest.str();
    return !code.empty();
}

void disk_store(uint64_t key, const std::string& name, const std::string& code) {
    const std::string dir = cache_dir();
    if (dir.empty()) return;
    // (mkdir -p of the last two levels; failures leave the cache in-process)
    const size_t cut = dir.find_last_of('/');
    if (cut != std::string::npos && cut > 0) (void)mkdir(dir.substr(0, cut).c_str(), 0755);
    (void)mkdir(dir.c_str(), 0755);
    const std::string path = cache_path(key);
    // a temp name unique to this write (pid, thread, sequence): two threads
    // compiling programs of one structure must not interleave into one file
    static std::atomic<uint64_t> seq{0};
    const std::string tmp = path + ".tmp." + std::to_string((long long)getpid()) + "." +
                            std::to_string((unsigned long long)std::hash<std::thread::id>()(
                                std::this_thread::get_id())) +
                            "." + std::to_string((unsigned long long)seq.fetch_add(1));
    {
        std::ofstream f(tmp, std::ios::binary);
        if (!f) return;
        const uint32_t n = (uint32_t)name.size();
        f.write((const char*)&n, 4);
        f.write(name.data(), n);
        f.write(code.data(), (std::streamsize)code.size());
        if (!f) {
            (void)unlink(tmp.c_str());
            return;
        }
    }
    (void)rename(tmp.c_str(), path.c_str());
}

// Compile `kernel` (a name expression of a template instantiation) with the
// program's source: (lowered name, code object), or an error message.
bool compile(const std::string& src, const std::string& kernel,
             const std::vector<std::string>& opts, std::string& name, std::string& code,
             std::string& err) {
    const std::string full = src;  // (the name expression instantiates the kernel)
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, full.c_str(), "mc_jit.hip", kJitNumHeaders, kJitHeaderTexts,
                            kJitHeaderNames) != HIPRTC_SUCCESS) {
        err = "hiprtcCreateProgram failed";
        return false;
    }
    const std::string expr = "&" + kernel;
    hiprtcAddNameExpression(prog, expr.c_str());
    std::vector<const char*> argv;
    for (const std::string& o : opts) argv.push_back(o.c_str());
    const hiprtcResult r = hiprtcCompileProgram(prog, (int)argv.size(), argv.data());
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        err = "hiprtc: " + std::string(hiprtcGetErrorString(r)) + ": " + log.substr(0, 2000);
        hiprtcDestroyProgram(&prog);
        return false;
    }
    const char* lowered = nullptr;
    if (hiprtcGetLoweredName(prog, expr.c_str(), &lowered) != HIPRTC_SUCCESS || !lowered) {
        err = "hiprtcGetLoweredName failed";
        hiprtcDestroyProgram(&prog);
        return false;
    }
    name = lowered;
    size_t n = 0;
    hiprtcGetCodeSize(prog, &n);
    code.assign(n, '\0');
    hiprtcGetCode(prog, &code[0]);
    hiprtcDestroyProgram(&prog);
    return n > 0;
}

JitState* state_of(const mc_program* p) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!p->jit) p->jit = new JitState();
    return (JitState*)p->jit;
}

}  // namespace

bool jit_enabled() {
    if (g_expr_jit < 0) {
        const char* e = std::getenv("MC_EXPR_JIT");
        g_expr_jit = (e && e[0] == '0') ? 0 : 1;
    }
    return g_expr_jit == 1;
}

void jit_free(mc_program* p) {
    if (!p || !p->jit) return;
    JitState* s = (JitState*)p->jit;
    for (hipModule_t m : s->mods) (void)hipModuleUnload(m);
    delete s;
    p->jit = nullptr;
}

int jit_function(const mc_program* p, const std::string& kernel, hipFunction_t* fn) {
    *fn = nullptr;
    if (!p->ex || !jit_enabled()) return MC_OK;
    JitState* s = state_of(p);
    std::lock_guard<std::mutex> lk(s->mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const auto fkey = std::make_pair(kernel, dev);
    auto it = s->fns.find(fkey);
    if (it != s->fns.end()) {
        *fn = it->second;
        return MC_OK;
    }
    if (!s->error.empty()) return MC_OK;  // a failed compilation: the interpreter runs
    const bool lane = is_lane_kernel(kernel);
    if (lane && !s->have_lsrc) {
        s->lsrc = gen_lane_source(p);
        s->have_lsrc = true;
    }
    if (!lane && !s->have_src) {
        s->src = gen_source(p);
        s->have_src = true;
    }
    const std::string& src = lane ? s->lsrc : s->src;
    const std::vector<std::string> opts = jit_opts(dev);
    const uint64_t key = cache_key(src, kernel, opts);
    std::string name, code;
    int from = 0;  // where the code object came from: 1 process cache, 2 disk, 3 compiled
    {
        std::lock_guard<std::mutex> ck(g_cache_mu);
        auto c = g_code.find(key);
        if (c != g_code.end()) {
            name = c->second.first;
            code = c->second.second;
            from = 1;
        }
    }
    if (!from && disk_load(key, name, code)) from = 2;
    // a cached object that does not load (truncated, corrupt, another
    // toolchain's) is dropped and compiled afresh once; a fresh object that
    // does not load is a compilation failure: the interpreter runs
    for (;;) {
        if (!from) {
            std::string err;
            if (!compile(src, kernel, opts, name, code, err)) {
                s->error = err;
                return MC_OK;
            }
            disk_store(key, name, code);
            from = 3;
        }
        hipModule_t mod;
        hipError_t e = hipModuleLoadData(&mod, code.data());
        hipFunction_t f = nullptr;
        if (e == hipSuccess) {
            e = hipModuleGetFunction(&f, mod, name.c_str());
            if (e != hipSuccess) (void)hipModuleUnload(mod);
        }
        if (e == hipSuccess) {
            s->mods.push_back(mod);
            {
                std::lock_guard<std::mutex> ck(g_cache_mu);
                g_code[key] = std::make_pair(name, code);
            }
            s->fns[fkey] = f;
            *fn = f;
            return MC_OK;
        }
        (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> ck(g_cache_mu);
            g_code.erase(key);
        }
        if (from == 3) {
            s->error = std::string("expression JIT: the compiled code object does not load: ") +
                       hipGetErrorString(e);
            return MC_OK;
        }
        if (from == 2) {
            const std::string path = cache_path(key);
            if (!path.empty()) (void)unlink(path.c_str());
        }
        from = 0;
    }
}

int jit_launch(const mc_program* p, const std::string& kernel, unsigned grid, unsigned block,
               size_t lds, hipStream_t st, void** args, bool* used) {
    *used = false;
    hipFunction_t f = nullptr;
    const int rc = jit_function(p, kernel, &f);
    if (rc != MC_OK || f == nullptr) return rc;
    MC_HIP_TRY(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, (unsigned)lds, st, args, nullptr));
    *used = true;
    return MC_OK;
}

std::string jit_error(const mc_program* p) {
    if (!p->jit) return "";
    JitState* s = (JitState*)p->jit;
    std::lock_guard<std::mutex> lk(s->mu);
    return s->error;
}

std::string jit_source(const mc_program* p) { return p->ex ? gen_source(p) : std::string(); }
std::string jit_lane_source(const mc_program* p) {
    return p->lr.has_expr ? gen_lane_source(p) : std::string();
}

extern "C" int mc_debug_expr_jit(int on) {
    g_expr_jit = on < 0 ? -1 : (on ? 1 : 0);
    return MC_OK;
}

extern "C" int32_t mc_program_expr_jit(const mc_program* p) {
    if (!p) return -1;
    if (!p->ex || !jit_enabled()) return 0;
    return jit_error(p).empty() ? 1 : -2;
}

// Test hooks (host only, no device): the generated source of a program's
// expression terms, and its compilation into `kernel` (a name expression);
// the compiler's log is the error message on failure.
extern "C" int64_t mc_debug_expr_jit_source(const mc_program* p, char* buf, int64_t cap) {
    if (!p) return -1;
    const std::string s = jit_source(p);
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>((size_t)cap - 1, s.size());
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int64_t)s.size();
}

extern "C" int64_t mc_debug_expr_jit_lane_source(const mc_program* p, char* buf, int64_t cap) {
    if (!p) return -1;
    const std::string s = jit_lane_source(p);
    if (buf && cap > 0) {
        const size_t n = std::min<size_t>((size_t)cap - 1, s.size());
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return (int64_t)s.size();
}

extern "C" int mc_debug_expr_jit_compile(const mc_program* p, const char* kernel) {
    if (!p || !kernel) return fail(MC_ERR_INVALID, "NULL argument");
    if (!p->ex) return fail(MC_ERR_INVALID, "the program has no expression terms");
    std::string name, code, err;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const std::string src = is_lane_kernel(kernel) ? jit_lane_source(p) : jit_source(p);
    if (src.empty()) return fail(MC_ERR_INVALID, "the program has no lane-resident expression terms");
    if (!compile(src, kernel, jit_opts(dev), name, code, err)) return fail(MC_ERR_UNSUPPORTED, "%s", err.c_str());
    return MC_OK;
}
