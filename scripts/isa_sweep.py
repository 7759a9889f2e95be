"""Where do a kernel's moment sweeps issue their LDS loads, and where do they
wait for them?  A report from the compiled code, not from the source.

Compiles one translation unit of mlx-mcmc_amd/csrc to gfx950 assembly with the
Makefile's HIPFLAGS (device only, into a temporary directory), picks one
kernel by its template arguments, and for every basic block that holds four
or more ds_read_b128 prints
  * the order of load groups (L<n>), lgkmcnt waits (W<n>) and VALU runs (V<n>);
  * per load group, the VALU instructions between its last load and the first
    wait that covers the group's first load (where the wave can first stall on
    it) and the wait that covers all of it.  A group still in flight at the
    block's end is followed into the successor blocks (the nearest wait over
    every path, eight blocks deep).
and the kernel's register / scratch / occupancy lines.

    python scripts/isa_sweep.py                          # the headline kernel
    python scripts/isa_sweep.py --args 1,3,4,false,31,true,3
    python scripts/isa_sweep.py --unit run_nuts_sl.hip --kernel k_nuts_sl --list
    python scripts/isa_sweep.py --asm saved.s            # a unit compiled before

LDS operations return in order, so `s_waitcnt lgkmcnt(N)` covers every LDS
operation but the last N issued; scalar loads share the counter and are
counted as issued (they can return out of order: the compiler waits for them
with lgkmcnt(0)).  Only load, wait, VALU and branch mnemonics are read."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlx-mcmc_amd", "csrc")
HEADLINE = "1,3,8,false,31,true,3"      # k_hmc_lf<RS, NSH, NW, X1, FORM, XL, SPEC>


def makefile_flags():
    """HIPFLAGS (and HIPCC) as the Makefile sets them."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {}
    for m in re.finditer(r"^(\w+)\s*\?=\s*(.*)$", text, re.M):
        var[m.group(1)] = m.group(2).strip()
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["HIPFLAGS"])
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def compile_unit(unit, out):
    hipcc, flags = makefile_flags()
    cmd = [hipcc] + flags + ["--offload-device-only", "-S", unit, "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


def mangled_args(args):
    """The Itanium encoding of integer / bool template arguments."""
    out = []
    for a in args.split(","):
        a = a.strip()
        if a in ("true", "false"):
            out.append("Lb%dE" % (a == "true"))
        else:
            v = int(a)
            out.append("Li%s%dE" % ("n" if v < 0 else "", abs(v)))
    return "I" + "".join(out) + "E"


LABEL = re.compile(r"^([.\w$]+):")


def kernel_text(lines, kernel, args):
    """(symbol, first line, body lines, trailer lines) of the instantiation."""
    want = "%d%s%s" % (len(kernel), kernel, mangled_args(args) if args else "")
    syms = []
    for i, ln in enumerate(lines):
        m = LABEL.match(ln)
        if m and ("%d%s" % (len(kernel), kernel)) in m.group(1) and not m.group(1).startswith("."):
            syms.append((m.group(1), i))
    hits = [(s, i) for s, i in syms if want in s]
    if not args or len(hits) != 1:
        return syms, None
    sym, i0 = hits[0]
    i1 = i0
    while i1 < len(lines) and not lines[i1].startswith(".Lfunc_end"):
        i1 += 1
    i2 = i1
    while i2 < len(lines) and not lines[i2].lstrip().startswith((".text", ".globl", ".amdgpu")):
        i2 += 1     # (the "Kernel info" comments follow the function's .set lines)
    return syms, (sym, i0, lines[i0 + 1:i1], lines[i1:i2])


def blocks_of(body, line0):
    """Basic blocks: [label, [(line number, mnemonic, operands)], successors]."""
    blocks = [["<entry>", [], None]]
    for k, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            if blocks[-1][1] or blocks[-1][0] != "<entry>":
                blocks.append([m.group(1), [], None])
            else:
                blocks[-1][0] = m.group(1)
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            continue
        parts = s.split(None, 1)
        blocks[-1][1].append((line0 + 2 + k, parts[0], parts[1] if len(parts) > 1 else ""))
        if parts[0].startswith("s_cbranch") or parts[0] in ("s_branch", "s_endpgm", "s_setpc_b64"):
            blocks.append(["<fallthrough>", [], None])
    blocks = [b for b in blocks if b[1]]
    index = {b[0]: n for n, b in enumerate(blocks) if not b[0].startswith("<")}
    for n, b in enumerate(blocks):
        mn, ops = b[1][-1][1], b[1][-1][2]
        succ = []
        if mn == "s_branch":
            succ = [index.get(ops.strip())]
        elif mn.startswith("s_cbranch"):
            succ = [n + 1 if n + 1 < len(blocks) else None, index.get(ops.strip())]
        elif mn not in ("s_endpgm", "s_setpc_b64"):
            succ = [n + 1 if n + 1 < len(blocks) else None]
        b[2] = [s for s in succ if s is not None]
    return blocks


def kind(mn):
    if mn == "ds_read_b128":
        return "L"
    if mn == "s_waitcnt":
        return "W"
    if mn.startswith("v_"):
        return "V"
    if mn.startswith(("ds_", "s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "O"      # another operation of the same counter
    return None


def lgkm_of(ops):
    m = re.search(r"lgkmcnt\((\d+)\)", ops)
    return int(m.group(1)) if m else None


def follow(blocks, n, after, valu, depth, seen):
    """The fewest VALU from here to a wait that leaves at most `after` newer
    operations in flight ... over the successor blocks of block n."""
    best = None
    for s in blocks[n][2]:
        if depth == 0 or (s, after) in seen:
            continue
        a, v, hit = after, valu, None
        for _, mn, ops in blocks[s][1]:
            k = kind(mn)
            if k in ("L", "O"):
                a += 1
            elif k == "V":
                v += 1
            elif k == "W":
                c = lgkm_of(ops)
                if c is not None and c <= a:
                    hit = (v, "lgkmcnt(%d) in %s" % (c, blocks[s][0]))
                    break
        if hit is None:
            hit = follow(blocks, s, a, v, depth - 1, seen | {(s, after)})
        if hit is not None and (best is None or hit[0] < best[0]):
            best = hit
    return best


def report_block(blocks, n, out):
    label, ins, _ = blocks[n]
    if sum(1 for i in ins if i[1] == "ds_read_b128") < 4:
        return 0
    # the sequence, run-length coded
    seq = []
    for _, mn, ops in ins:
        k = kind(mn)
        if k == "W":
            c = lgkm_of(ops)
            if c is None:
                continue
            seq.append("W%d" % c)
        elif k in ("L", "V", "O"):
            if seq and seq[-1][0] == k and k != "W":
                seq[-1] = k + str(int(seq[-1][1:]) + 1)
            else:
                seq.append(k + "1")
    out.append("block %s (lines %d-%d, %d instructions)" % (label, ins[0][0], ins[-1][0], len(ins)))
    out.append("  order: " + " ".join(seq))
    # load groups: runs of ds_read_b128 not separated by a VALU or a wait
    groups, cur = [], None
    for p, (_, mn, ops) in enumerate(ins):
        k = kind(mn)
        if k == "L":
            if cur is None:
                cur = [p, p]
                groups.append(cur)
            cur[1] = p
        elif k in ("V", "W") and not (k == "W" and lgkm_of(ops) is None):
            cur = None
    for g, (p0, p1) in enumerate(groups):
        nload = sum(1 for i in ins[p0:p1 + 1] if i[1] == "ds_read_b128")
        res = {}
        for what, pos in (("first", p0), ("all", p1)):
            after = sum(1 for i in ins[pos + 1:p1 + 1] if kind(i[1]) in ("L", "O"))
            valu, hit = 0, None
            for _, mn, ops in ins[p1 + 1:]:
                k = kind(mn)
                if k in ("L", "O"):
                    after += 1
                elif k == "V":
                    valu += 1
                elif k == "W":
                    c = lgkm_of(ops)
                    if c is not None and c <= after:
                        hit = (valu, "lgkmcnt(%d)" % c)
                        break
            if hit is None:
                hit = follow(blocks, n, after, valu, 8, frozenset())
            res[what] = hit
        fmt = lambda h: "no wait found" if h is None else "%d VALU (%s)" % h
        out.append("  group %d: %d loads at line %d: first load covered after %s, all after %s"
                   % (g, nload, ins[p0][0], fmt(res["first"]), fmt(res["all"])))
    return 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--unit", default="run_lanes_rs1.hip")
    ap.add_argument("--kernel", default="k_hmc_lf")
    ap.add_argument("--args", default=HEADLINE, help="template arguments, e.g. " + HEADLINE)
    ap.add_argument("--asm", help="an assembly file of the unit made before (no compile)")
    ap.add_argument("--list", action="store_true", help="list the unit's instantiations")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm
        if not path:
            path = os.path.join(tmp, "unit.s")
            compile_unit(a.unit, path)
        lines = open(path).read().split("\n")
    syms, hit = kernel_text(lines, a.kernel, None if a.list else a.args)
    if hit is None:
        for s, i in syms:
            print("%8d  %s" % (i + 1, s))
        if not a.list:
            sys.exit("no single instantiation of %s with <%s>" % (a.kernel, a.args))
        return
    sym, i0, body, trailer = hit
    unit = os.path.basename(a.asm) if a.asm else a.unit
    out = ["unit %s, kernel %s<%s>" % (unit, a.kernel, a.args), "symbol %s" % sym]
    for ln in trailer:
        m = re.match(r";\s*(NumVgprs|NumAgprs|TotalNumVgprs|TotalNumSgprs|ScratchSize|Occupancy|"
                     r"codeLenInByte)\b.*", ln.strip())
        if m:
            out.append("  " + ln.strip().lstrip("; "))
    blocks = blocks_of(body, i0)
    nvalu = sum(1 for b in blocks for i in b[1] if kind(i[1]) == "V")
    out.append("  static VALU instructions: %d, ds_read_b128: %d" %
               (nvalu, sum(1 for b in blocks for i in b[1] if i[1] == "ds_read_b128")))
    shown = sum(report_block(blocks, n, out) for n in range(len(blocks)))
    out.append("%d blocks with four or more ds_read_b128" % shown)
    print("\n".join(out))


if __name__ == "__main__":
    main()
