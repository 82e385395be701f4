#!/usr/bin/env python3
"""Static instruction count of one bucket addition in msm_accum_kernel's accumulate loop.

Compiles csrc/msm.hip device-only to assembly with the Makefile's flags (no GPU needed, under a minute) and, for every instantiation
of msm_accum_kernel, prints for the NORMAL PATH of the accumulate loop -- one ordinary mixed addition, no exceptional case:

  valu   VALU instructions per addition: mnemonics beginning `v_`
  mad64  the 64-bit multiply-adds among them (v_mad_u64_u32 / v_mad_i64_i32)

How the normal path is found.  The loop is the kernel's largest loop (LLVM marks every block with its loop header).  Its blocks form
a small graph: every conditional branch either enters or skips a guarded region (the first point of a bucket, the exact test behind
the zero-mod-p filter, the doubling, ...).  All acyclic paths from the loop header back to it are enumerated.  A full mixed addition
has 6 products, 2 squares and one two-product form, 6 * 162 + 2 * 126 + 243 = 1467 multiply-adds, so a path with fewer than 1400 is
not an ordinary addition (it skipped it, or took the doubling instead); of the others the one with the fewest VALU instructions is the
normal path.  The per-block table is printed too, so the choice can be checked by eye.

The UNIT PATH is the addition onto an accumulator that is a bucket's first record (zz = zzz = one: ecu.h xyzzu_add_mixed_nonid with unit set): 1 square,
2 products and the two fused forms, 2 * 126 + 2 * 162 + 243 = 819 multiply-adds on native records; E-form records keep the two
products by one, 1143.  It is found the same way: of the paths with at least 700 and fewer than 1400 multiply-adds the one with the
fewest VALU instructions (a doubling has 945 or more and two exact reductions on top, so it never wins).  The kernel's registers,
scratch and occupancy are printed from the assembly's resource comment.

  python3 tools/accum_inst_count.py [--package DIR] [--json]

--package: the directory holding the Makefile and csrc/ (default: this checkout's); point it at another checkout to count that one.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ADD_MADS = 1400  # see the docstring
UNIT_ADD_MADS = 700
MADS = ("v_mad_u64_u32", "v_mad_i64_i32")


def makefile_flags(package):
    text = open(os.path.join(package, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*\?=\s*(.*)$", text, re.M))
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["CXXFLAGS"])
    return var["HIPCC"], flags.split()


def compile_asm(package):
    hipcc, flags = makefile_flags(package)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "msm.s")
        cmd = [hipcc] + flags + ["--offload-device-only", "-S", "csrc/msm.hip", "-o", out]
        subprocess.run(cmd, cwd=package, check=True, stderr=subprocess.DEVNULL)
        return open(out).read().splitlines()


def kernels(lines):
    """name -> the lines of every function whose symbol contains msm_accum_kernel"""
    found, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(_Z\w*msm_accum_kernel\w*):", ln)
        if m:
            name, body = m.group(1), []
        elif name and ln.startswith(".Lfunc_end"):
            found[name] = body
            name = None
        elif name:
            body.append(ln)
    return found


def resources(lines):
    """name -> {vgprs, sgprs, scratch_bytes, occupancy} from the comment block after each msm_accum_kernel"""
    keys = {"NumVgprs": "vgprs", "NumSgprs": "sgprs", "ScratchSize": "scratch_bytes", "Occupancy": "occupancy"}
    found, name = {}, None
    for ln in lines:
        m = re.match(r"^(_Z\w*msm_accum_kernel\w*):", ln)
        if m:
            name = m.group(1)
            found[name] = {}
            continue
        m = re.match(r"^; (\w+): (\d+)\s*$", ln)
        if name and m and m.group(1) in keys:
            found[name].setdefault(keys[m.group(1)], int(m.group(2)))
        elif name and ln.startswith(("_Z", ".amdhsa_kernel")) and found[name]:
            name = None
    return found


def blocks_of(body):
    """[(label, loop header or None, [mnemonic, operand text] ...)] in layout order; the first block has label None"""
    out = [[None, None, []]]
    for ln in body:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", ln)
        if m:
            note = m.group(2)
            h = re.search(r"Header=(BB\d+_\d+)", note)
            header = "." + "L" + h.group(1) if h else (m.group(1) if "Loop Header" in note else None)
            out.append([m.group(1), header, []])
            continue
        code = ln.split(";")[0].strip()
        if not code or code.startswith("."):
            continue
        parts = code.split(None, 1)
        out[-1][2].append((parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def count(instrs):
    valu = sum(1 for op, _ in instrs if op.startswith("v_"))
    mad = sum(1 for op, _ in instrs if op.startswith(MADS))
    return valu, mad


def normal_path(body):
    blocks = blocks_of(body)
    by_loop = {}
    for i, (label, header, instrs) in enumerate(blocks):
        if header:
            by_loop.setdefault(header, []).append(i)
    if not by_loop:
        return None
    header = max(by_loop, key=lambda h: sum(len(blocks[i][2]) for i in by_loop[h]))
    inside = set(by_loop[header])
    index = {b[0]: i for i, b in enumerate(blocks)}
    start = index[header]
    best = unit = None
    table = [(blocks[i][0],) + count(blocks[i][2]) for i in sorted(inside)]

    # walk instruction by instruction: a block may hold several branches
    def walk(i, k, valu, mad, seen, trail):
        nonlocal best
        instrs = blocks[i][2]
        while k < len(instrs):
            op, arg = instrs[k]
            if op.startswith("v_"):
                valu += 1
                if op.startswith(MADS):
                    mad += 1
            elif op == "s_branch" or op.startswith("s_cbranch"):
                t = index.get(arg.strip())
                if t is not None:
                    leave(t, valu, mad, seen, trail)
                if op == "s_branch":
                    return
            k += 1
        leave(i + 1, valu, mad, seen, trail)

    def leave(t, valu, mad, seen, trail):
        nonlocal best, unit
        if t == start:
            if mad >= FULL_ADD_MADS and (best is None or valu < best[0]):
                best = (valu, mad, list(trail))
            if UNIT_ADD_MADS <= mad < FULL_ADD_MADS and (unit is None or valu < unit[0]):
                unit = (valu, mad, list(trail))
            return
        if t not in inside or t in seen:
            return
        walk(t, 0, valu, mad, seen | {t}, trail + [blocks[t][0]])

    sys.setrecursionlimit(10000)
    walk(start, 0, 0, 0, {start}, [header])
    return header, table, best, unit


def short(name):
    m = re.search(r"msm_accum_kernelILb(\d)E", name)
    if m:
        return "msm_accum_kernel<%s>" % ("native records" if m.group(1) == "1" else "E-form records")
    return "msm_accum_kernel"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package", default=os.path.join(ROOT, "halo2-pse_amd"))
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    res = {}
    lines = compile_asm(args.package)
    res_of = resources(lines)
    for name, body in sorted(kernels(lines).items()):
        r = normal_path(body)
        if not r or not r[2]:
            continue
        header, table, (valu, mad, trail), unit = r
        res[short(name)] = {"valu_per_addition": valu, "mad64_per_addition": mad, "loop_header": header, "path": trail,
                            "unit_path": {"valu_per_addition": unit[0], "mad64_per_addition": unit[1], "path": unit[2]} if unit else None,
                            "resources": res_of.get(name, {}),
                            "loop_blocks": [{"block": b, "valu": v, "mad64": m} for b, v, m in table]}
    if args.json:
        print(json.dumps(res, indent=1))
        return
    for k, r in res.items():
        print("%s: accumulate loop %s, normal path of one addition" % (k, r["loop_header"]))
        print("  VALU instructions per addition : %d" % r["valu_per_addition"])
        print("  64-bit multiply-adds among them: %d" % r["mad64_per_addition"])
        print("  path  : " + " ".join(r["path"]))
        u = r["unit_path"]
        if u:
            print("  unit path (the addition onto a bucket's first record)")
            print("  VALU instructions per addition : %d" % u["valu_per_addition"])
            print("  64-bit multiply-adds among them: %d" % u["mad64_per_addition"])
            print("  path  : " + " ".join(u["path"]))
        else:
            print("  unit path: none found")
        print("  resources: " + ", ".join("%s %d" % kv for kv in sorted(r["resources"].items())))
        print("  blocks of the loop (VALU / 64-bit multiply-adds): " + ", ".join("%s %d/%d" % (b["block"], b["valu"], b["mad64"]) for b in r["loop_blocks"]))


if __name__ == "__main__":
    main()
