#!/usr/bin/env python3
"""Per-kernel statistics of a device-only assembly listing (hipcc --cuda-device-only -S): lines, exec-mask regions, branches, MFMAs, waits.
usage: isa_stats.py file.s [substring of the mangled kernel name]"""
import re, sys
src, want = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "")
name, body, out = None, [], []
for ln in open(src):
    # a kernel ends at the next function label or at .Lfunc_end, not at its first s_endpgm: an early exit is one too
    m = re.match(r"^(_Z[\w$]+):|^\.Lfunc_end\d+:", ln)
    if m:
        if name is not None and want in name:
            t = "".join(body)
            out.append((name, len(body), t.count("saveexec"), t.count("s_cbranch"), t.count("v_mfma"), t.count("s_waitcnt vmcnt"), t.count("v_readlane") + t.count("v_writelane"), t.count("scratch_")))
        name, body = m.group(1), []
        continue
    s = ln.split(";")[0].strip()
    if name is not None and not (s.startswith(".") and not s.endswith(":")):  # not the directives of the kernel descriptor that precede .Lfunc_end
        body.append(ln)
print("%-86s %6s %8s %7s %5s %6s %6s %7s" % ("kernel", "lines", "saveexec", "branch", "mfma", "vmcnt", "lanes", "scratch"))
for o in out:
    print("%-86s %6d %8d %7d %5d %6d %6d %7d" % o)
