#!/usr/bin/env python3
"""Static instruction counts of one kernel's main loop, from the compiler's assembly. Needs no GPU.

    python profiles/isa_loop_counts.py [--tu hip/render_phases_lambert_plain.hip] [--kernel SUBSTRING] [--csrc DIR]
                                       [--begin FILE:REGEX] [--end FILE:REGEX:REGEX] [--top N] [--asm FILE] [--keep FILE]

Compiles one translation unit of csrc/ with the Makefile's HIPFLAGS plus `-S --cuda-device-only -gline-tables-only`, finds the
kernel whose mangled name contains SUBSTRING and counts the instructions of its loop by class and by source line:

    vector  v_*      (of which: register moves v_mov_*, and SGPR spill / lane access v_readlane* v_writelane* v_readfirstlane*)
    scalar  s_*
    LDS     ds_*
    memory  global_* flat_* buffer_* scratch_*

The loop is delimited by source lines, found by regex in the named source file so that the tool follows the code when lines
move: it begins behind the last instruction attributed to the line matching --begin (default: the barrier that ends the LDS scene
copy in setup_trace) and ends at the first later instruction attributed to a line between the two --end matches (default: the
wave sums of flush_counters). Attribution is the innermost `.loc` in force (inlined code counts at its own line). Instructions
before the first `.loc` of a block, and the copies a compiler places at control-flow joins, carry line 0.

The counts are static: an instruction counts once wherever it sits in the loop, whatever the trip counts of inner loops.
--asm FILE counts an assembly file made earlier (e.g. of another commit) instead of compiling.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gradient-based-path-tracing_amd", "csrc")
DEFAULT_KERNEL = "gdpt_render_phasesILb1ELb1ELb1ELb1ELb0ELi3ELi2ELb1EE"  # Lambertian, LDS scene, wide, no spheres, constant textures, batched set-up


def makefile_hipflags(csrc):
    """HIPFLAGS of csrc/Makefile with $(ARCH) filled in (ARCH from the environment, default as in the Makefile)."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = os.environ.get("ARCH") or re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS = (.*)$", text, re.M).group(1).replace("$(ARCH)", arch)
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)", text, re.M).group(1)
    out, cur, quote = [], "", False      # split like a shell would: \" stays a literal quote inside the define
    i = 0
    while i < len(flags):
        c = flags[i]
        if c == "\\" and i + 1 < len(flags):
            cur += flags[i + 1]; i += 2; continue
        if c.isspace():
            if cur:
                out.append(cur); cur = ""
        else:
            cur += c
        i += 1
    if cur:
        out.append(cur)
    return hipcc, out


def compile_asm(csrc, tu, out):
    hipcc, flags = makefile_hipflags(csrc)
    cmd = [hipcc] + flags + ["-S", "--cuda-device-only", "-gline-tables-only", tu, "-o", out]
    subprocess.check_call(cmd, cwd=csrc)


def find_line(csrc, spec):
    """FILE:REGEX[:REGEX] -> (basename, [line numbers of the first match of each regex, each searched behind the previous one])."""
    name, *pats = spec.split(":")
    path = None
    for root, _, files in os.walk(csrc):
        if os.path.basename(name) in files and "build" not in os.path.relpath(root, csrc).split(os.sep)[0]:
            path = os.path.join(root, os.path.basename(name)); break
    if path is None:
        sys.exit(f"{name}: not found under {csrc}")
    lines = open(path).read().splitlines()
    found, start = [], 0
    for p in pats:
        rx = re.compile(p)
        for n in range(start, len(lines)):
            if rx.search(lines[n]):
                found.append(n + 1); start = n + 1; break
        else:
            sys.exit(f"{spec}: no line matches {p!r}")
    return os.path.basename(name), found


def classify(op):
    if op.startswith("v_"):
        return "vector"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "memory"
    return "other"


def kernel_instructions(asm_path, kernel):
    """[(opcode, operands, file basename, line, frames)] of the kernel's body in text order. frames: the `.loc` in force as the
    compiler's comment spells it, innermost first, (basename, line) each; file and line are those of the innermost frame that lies
    in the project (a relative path), so that a barrier or a shuffle counts at the project line that calls it."""
    files = {}
    body, inside, name = [], False, None
    cur = ("", 0, ())
    label = re.compile(r"^([A-Za-z_.$][\w.$]*):")
    for raw in open(asm_path, errors="replace"):
        line, _, comment = raw.partition(";")
        s = line.strip()
        if not s:
            continue
        m = re.match(r"\.file\s+(\d+)\s+(?:\"([^\"]*)\"\s+)?\"([^\"]*)\"", s)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3)); continue
        m = label.match(s)
        if m and not inside:
            if kernel in m.group(1) and not m.group(1).startswith("."):
                inside, name = True, m.group(1)
            continue
        if not inside:
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".section") or s.startswith(".size"):
            break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            chain = re.findall(r"([^\s\[\]@]+):(\d+):\d+", comment)
            frames = tuple((os.path.basename(f), int(l)) for f, l in chain)
            own = next(((os.path.basename(f), int(l)) for f, l in chain if not os.path.isabs(f)), None)
            if own is None:
                own = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            cur = (own[0], own[1], frames); continue
        if label.match(s):
            body.append(("", label.match(s).group(1), cur[0], cur[1], cur[2])); continue     # a label: empty opcode, name as operands
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        body.append((parts[0], parts[1] if len(parts) > 1 else "", cur[0], cur[1], cur[2]))
    if name is None:
        sys.exit(f"no kernel whose name contains {kernel!r} in {asm_path}")
    return name, body


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("--tu", default="hip/render_phases_lambert_plain.hip")
    ap.add_argument("--kernel", default=DEFAULT_KERNEL)
    ap.add_argument("--begin", default=r"render_device.h:GD TraceCtx setup_trace:__syncthreads\(\);")
    ap.add_argument("--end", default=r"render_device.h:GD unsigned wave_sum_u32:GD void reduce_and_store")
    ap.add_argument("--top", type=int, default=40)
    ap.add_argument("--asm", default=None)
    ap.add_argument("--keep", default=None, help="write the compiled assembly to this file")
    a = ap.parse_args()

    tmp = None
    asm = a.asm
    if asm is None:
        tmp = tempfile.TemporaryDirectory()
        asm = os.path.join(tmp.name, "tu.s")
        if a.keep:
            asm = os.path.abspath(a.keep)
        compile_asm(a.csrc, a.tu, asm)
    name, body = kernel_instructions(asm, a.kernel)
    labels_at = {}                    # label -> number of instructions in front of it
    instrs = []
    for x in body:
        if x[0] == "":
            labels_at[x[1]] = len(instrs)
        else:
            instrs.append(x)
    body = instrs
    bfile, blines = find_line(a.csrc, a.begin)
    efile, elines = find_line(a.csrc, a.end)
    bline = blines[-1]
    e0, e1 = elines[0], elines[-1]

    begin = max((i for i, x in enumerate(body) if (bfile, bline) in x[4] or (x[2], x[3]) == (bfile, bline)), default=None)
    if begin is None:
        sys.exit(f"no instruction of the kernel is attributed to {bfile}:{bline}")
    end = next((i for i in range(begin + 1, len(body)) if body[i][2] == efile and e0 <= body[i][3] < e1), len(body))
    # the loop proper begins at the first label behind `begin` that a later instruction of the region branches back to; what lies in
    # front of it (constants, the lane's initial state) runs once per kernel
    head = None
    for lab, pos in sorted(labels_at.items(), key=lambda kv: kv[1]):
        if begin < pos < end and any(lab in re.split(r"[\s,]+", body[i][1]) for i in range(pos, end) if "branch" in body[i][0]):
            head = pos; break
    if head is None:
        sys.exit("no backward branch in the region: not a loop")
    once = body[begin + 1:head]
    loop = body[head:end]

    def totals(seq):
        c = collections.Counter(classify(x[0]) for x in seq)
        return c
    print(f"kernel  {name}")
    kt = totals(body)
    print(f"whole kernel: {kt['vector']} vector / {kt['scalar']} scalar / {kt['LDS']} LDS / {kt['memory']} memory / {kt['other']} other")
    ot, lt = totals(once), totals(loop)
    print(f"region {bfile}:{bline} .. {efile}:{e0}: {ot['vector'] + lt['vector']} vector / {ot['scalar'] + lt['scalar']} scalar / {ot['LDS'] + lt['LDS']} LDS / "
          f"{ot['memory'] + lt['memory']} memory")
    om = sum(1 for x in once if x[0].startswith("v_mov_"))
    print(f"  in front of the loop head, once per kernel: {ot['vector']} vector (of which {om} register moves) / {ot['scalar']} scalar / {ot['LDS']} LDS / {ot['memory']} memory")
    print(f"loop: {lt['vector']} vector / {lt['scalar']} scalar / {lt['LDS']} LDS / {lt['memory']} memory / {lt['other']} other")
    moves = [x for x in loop if x[0].startswith("v_mov_")]
    lanes = [x for x in loop if x[0].startswith(("v_readlane", "v_writelane", "v_readfirstlane"))]
    by_op = collections.Counter(x[0] for x in moves + lanes)
    zero = sum(1 for op, args, *_ in moves if re.search(r",\s*0$", args))
    noline = sum(1 for x in moves if x[3] == 0)
    nv = max(1, lt["vector"])
    print(f"  register moves: {len(moves)} ({100.0 * len(moves) / nv:.1f} % of vector; {noline} at line 0, {zero} write literal 0)")
    print(f"  lane access (SGPR spill lanes and broadcasts): {len(lanes)}")
    print("  " + ", ".join(f"{op} {n}" for op, n in sorted(by_op.items())))

    per = collections.defaultdict(collections.Counter)
    for op, _, f, l, _fr in loop:
        c = classify(op)
        per[(f, l)][c] += 1
        if op.startswith("v_mov_"):
            per[(f, l)]["mov"] += 1
        if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            per[(f, l)]["lane"] += 1
    per_file = collections.defaultdict(collections.Counter)
    for (f, l), c in per.items():
        per_file[f].update(c)
    print("by file:        vector scalar    LDS memory  (moves, lane access)")
    for f, c in sorted(per_file.items(), key=lambda kv: -kv[1]["vector"]):
        print(f"  {f or '(none)':24s} {c['vector']:6d} {c['scalar']:6d} {c['LDS']:6d} {c['memory']:6d}  ({c['mov']}, {c['lane']})")
    print(f"by line, top {a.top} by vector count:")
    for (f, l), c in sorted(per.items(), key=lambda kv: (-kv[1]["vector"], kv[0]))[:a.top]:
        print(f"  {(f or '(none)') + ':' + str(l):32s} {c['vector']:6d} {c['scalar']:6d} {c['LDS']:6d} {c['memory']:6d}  ({c['mov']}, {c['lane']})")
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
