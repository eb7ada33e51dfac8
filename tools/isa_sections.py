#!/usr/bin/env python3
"""Static instruction counts of the timed frame kernel, per section of its loop.  Needs hipcc only, no GPU.

Compiles rt_kernels.hip for gfx950 with the flags of build.py plus -DRT_ISA_MARKS, which turns every RT_MARK("name") of
rt_persistent_kernel into a `; RTMARK name` comment in the listing, and counts what lies between consecutive marks of ONE
instantiation: instructions, and among them the classes told apart by prefix -- v_ (VALU), s_cbranch (branches), ds_ (LDS),
global_ and scratch_ (vector memory), s_ other than branches, s_waitcnt and s_nop (scalar ALU: the exec-mask bookkeeping of per-lane
control flow lands here), and the s_waitcnt that name vmcnt (waits for vector memory: one per dependent round trip).  Nothing else is
classified.

The listing is in layout order, not execution order: a block the compiler sinks out of line is counted in the section it lands in.
The numbers say how large a section is, not how long it runs.

usage: tools/isa_sections.py [--kernel SUBSTRING] [--list] [--label TEXT] [--src FILE] [extra hipcc flags ...]
  --kernel   substring of the mangled name; default: the shadow frame job's packed, shallow instantiation the headline runs
             (with the identity-root form if the build has one)
  --list     print the mangled names of all instantiations and stop
  --src      another copy of rt_kernels.hip (a checkout of the parent commit, for the comparison)

A kernel built with RT_OCC_LOOP holds the traversal loop twice; the sections of its occlusion-only form carry the prefix occ_ and are
summed in the row "occ_loop", those of the general form in "loop" as before.

The "stack" mark sits between the child tests and the pushes / pops of a node step, but the slab arithmetic has no side effect and
the compiler moves most of it behind the mark: read "node" + "stack" together as the node step."""
import collections
import importlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bld = importlib.import_module("vortex-raytracing_amd.build")
SRC = os.path.join(bld.CSRC, "rt_kernels.hip")
# the library's own flags (build.py) without what only a shared library needs, + a device listing with the marks
FLAGS = [f for f in bld.HIP_FLAGS if f != "-fPIC"] + ["-w", "-S", "--cuda-device-only", "-DRT_ISA_MARKS"]
# <JOB_RENDER_SHADOW, STATS 0, LDEXP false, EXACT false, PACKED true, SHALLOW true, ALPHA false [, IDENT true]>
HEADLINE = ("ILi1ELi0ELb0ELb0ELb1ELb1ELb0ELb1EE", "ILi1ELi0ELb0ELb0ELb1ELb1ELb0EE")
LOOP_SECTIONS = ("loop_top", "node", "stack", "inst", "leaf", "leaf_tris", "leaf_pop", "loop_exit")
CLASSES = (("valu", "v_"), ("branch", "s_cbranch"), ("ds", "ds_"), ("global", "global_"), ("scratch", "scratch_"))


def kernels(lines):
    """{mangled name: body lines} of every rt_persistent_kernel instantiation"""
    out, name = collections.OrderedDict(), None
    for l in lines:
        m = re.match(r"(_Z20rt_persistent_kernel\w+):", l)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None:
            out[name].append(l)
            if l.strip().startswith("s_endpgm"):
                name = None
    return out


def sections(body):
    sec, counts = "prologue", collections.OrderedDict()
    for l in body:
        t = l.strip()
        m = re.match(r";\s*RTMARK (\w+)", t)
        if m:
            sec = m.group(1)
            continue
        if not t or t.startswith((";", ".", "//")) or t.split(";")[0].rstrip().endswith(":"):
            continue
        op = t.split()[0]
        c = counts.setdefault(sec, collections.Counter())
        c["insts"] += 1
        for cls, prefix in CLASSES:
            if op.startswith(prefix):
                c[cls] += 1
        if op.startswith("s_") and not op.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop")):
            c["salu"] += 1
        if op.startswith("s_waitcnt") and "vmcnt" in t:
            c["vmwait"] += 1
    return counts


def main():
    args = sys.argv[1:]
    want, label, listing, src = None, "", False, SRC
    extra = []
    while args:
        a = args.pop(0)
        if a == "--kernel":
            want = args.pop(0)
        elif a == "--label":
            label = args.pop(0)
        elif a == "--src":
            src = args.pop(0)
        elif a == "--list":
            listing = True
        else:
            extra.append(a)
    with tempfile.TemporaryDirectory(prefix="isa_sections_") as tmp:
        out = os.path.join(tmp, "rt_marks.s")
        r = subprocess.run([bld.HIPCC] + FLAGS + extra + ["-o", out, src], stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit("hipcc failed (%d):\n%s" % (r.returncode, r.stderr[-4000:]))
        ks = kernels(open(out).read().split("\n"))
    if listing:
        print("\n".join(ks))
        return
    subs = (want,) if want else HEADLINE
    name = next((n for s in subs for n in ks if s in n), None)
    if name is None:
        raise SystemExit("no instantiation matches %s (see --list)" % (subs,))
    counts = sections(ks[name])
    cols = ("insts",) + tuple(c for c, _ in CLASSES) + ("salu", "vmwait")
    print("# %s" % (label or "rt_kernels.hip"))
    print("# flags: %s" % " ".join(extra or ["(none)"]))
    print("# kernel: %s" % name)
    print("%-14s" % "section" + "".join("%9s" % c for c in cols))
    total = collections.Counter()
    for sec, c in counts.items():
        print("%-14s" % sec + "".join("%9d" % c[k] for k in cols))
        total.update(c)
    # the traversal loop, and its occlusion-only form where the kernel holds one (RT_OCC_LOOP: the same marks with the prefix occ_)
    for prefix, row in (("", "loop"), ("occ_", "occ_loop")):
        loop = collections.Counter()
        for sec in LOOP_SECTIONS:
            loop.update(counts.get(prefix + sec, {}))
        if loop:
            print("%-14s" % row + "".join("%9d" % loop[k] for k in cols))
    print("%-14s" % "kernel" + "".join("%9d" % total[k] for k in cols))


if __name__ == "__main__":
    main()
