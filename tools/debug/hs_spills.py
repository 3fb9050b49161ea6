#!/usr/bin/env python3
"""Scalar-spill traffic of the conv_hsplit instantiations, read from the device assembly (no GPU needed).

Per kernel: SGPRs / spilled SGPRs / VGPRs / scratch from the code object's metadata, the v_readlane / v_writelane of the whole kernel, and those
inside the LOADER role's phase loop -- the outermost loop around the `; HS_LOADER_PHASE` comment that csrc/conv_hsplit.hip leaves behind the
loaders' barrier when compiled with -DHS_SPILL_MARK (this tool's compile only; an --asm file must come from such a compile), by the loop comments of the assembly (the loop body holds the per-slice code and, behind uniform branches, the per-tile code).

    python tools/debug/hs_spills.py [--asm FILE.s] [filter ...]      (default filters: the four 32-channel f16x2 kernels and <2,2,0>; `ILi` = every instantiation)"""
import os, re, subprocess, sys, tempfile

root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = sys.argv[1:]
asm = None
if args and args[0] == "--asm":
    asm, args = args[1], args[2:]
filters = args or ["ILi1ELi2ELi2E", "ILi1ELi2ELi12E", "ILi1ELi2ELi18E", "ILi1ELi2ELi28E", "ILi2ELi2ELi0E"]
if asm is None:
    asm = os.path.join(tempfile.mkdtemp(), "conv_hsplit.s")
    flags = subprocess.run(["make", "-C", os.path.join(root, "casapose_amd", "csrc"), "-s", "print-FLAGS"], capture_output=True, text=True).stdout.split()
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-DHS_SPILL_MARK", "--cuda-device-only", "-S", os.path.join(root, "casapose_amd", "csrc", "conv_hsplit.hip"), "-o", asm], check=True)
lines = open(asm).read().splitlines()

meta = {}   # amdhsa.kernels: one record per kernel, opened by "  - .key:", keys in alphabetical order
cur = {}
for ln in lines[next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")):]:
    if re.match(r"\s+- \.", ln):
        cur = {}
    m = re.match(r"\s+(?:- )?\.(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", ln)
    if m:
        cur[m.group(1)] = int(m.group(2))
    m = re.match(r"\s+(?:- )?\.name:\s+(\S+)", ln)
    if m:
        meta[m.group(1)] = cur


def lanes(seg):
    return sum(1 for x in seg if re.match(r"\s*v_readlane_b32", x)), sum(1 for x in seg if re.match(r"\s*v_writelane_b32", x))


print("%-14s %5s %7s %5s %7s | %9s %9s | %s" % ("kernel", "SGPRs", "S spill", "VGPRs", "scratch", "readlane", "writelane", "loader phase loop(s): readlane/writelane/instructions"))
for i, ln in enumerate(lines):
    m = re.match(r"^(_ZN\S*conv_hsplit_kernel(ILi\d+ELi\d+ELi\d+E)\S*):", ln)
    if not m or not any(f in m.group(1) for f in filters):
        continue
    name, short = m.group(1), "<%s>" % ",".join(re.findall(r"Li(\d+)E", m.group(2)))
    end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
    body = lines[i:end + 1]
    # basic blocks and the loops the compiler's comments put them in: "in Loop: Header=BBn_m Depth=d" on a member, "Parent Loop BBn_m Depth=d" on an inner header
    blocks, cur = [], None   # [first line, last line, own label, innermost header, parents]
    for j, l in enumerate(body):
        mm = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", l)
        if mm:
            cur = [j, j, mm.group(1), None, []]
            blocks.append(cur)
            hm = re.search(r"in Loop: Header=(BB\d+_\d+)", l)
            if hm:
                cur[3] = hm.group(1)
        elif cur is not None:
            cur[1] = j
            pm = re.match(r"\s*;\s+Parent Loop (BB\d+_\d+)", l)
            if pm:
                cur[4].append(pm.group(1))
            if "Loop Header: Depth=" in l or "Parent Loop" in body[cur[0]]:
                cur[3] = cur[3] or cur[2]
        if mm and "Parent Loop" in l:
            cur[4].append(re.search(r"Parent Loop (BB\d+_\d+)", l).group(1))
            cur[3] = cur[2]
        if mm and "Loop Header: Depth=" in l:
            cur[3] = cur[2]
    parents = {b[2]: b[4] for b in blocks if b[2] and b[3] == b[2]}
    def chain(h):
        return [h] + parents.get(h, []) if h else []
    tops = []
    for b in blocks:
        if any("HS_LOADER_PHASE" in x for x in body[b[0]:b[1] + 1]) and b[3]:
            c = chain(b[3])
            tops.append(c[1] if len(c) > 1 else c[0])   # (the first parent listed is the outermost)
    loops = [[x for b in blocks if t in chain(b[3]) for x in body[b[0]:b[1] + 1]] for t in sorted(set(tops))]
    per = []   # the compiler unswitches the loop on uniform flags (resident weights, image source, ...): one entry per version
    for seg in loops:
        a, b = lanes(seg)
        per.append("%d/%d/%d" % (a, b, sum(1 for x in seg if re.match(r"\s+[sv]_|\s+(buffer|ds|global)_", x))))
    d = meta.get(name, {})
    a, b = lanes(body)
    print("%-14s %5d %7d %5d %7d | %9d %9d | %s" % (short, d.get("sgpr_count", -1), d.get("sgpr_spill_count", -1), d.get("vgpr_count", -1),
                                                                     d.get("private_segment_fixed_size", -1), a, b, "  ".join(per)))
