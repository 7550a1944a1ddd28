#!/usr/bin/env python3
"""Static instruction counts of one k_trace2 instance, per section of its loop (gfx950, compile only).

    python tools/step_counts.py [--instance 16,5,true,true,false,true,false] [--keep DIR] [extra hipcc flags...]

trace.hip is compiled device-only to assembly twice: as the product builds it, and with
-DIZPI_STEP_MARKS, which puts a comment marker (no instruction) at the head of each section
of the loop: head (idle ballot), dequeue, refill, pick (step choice), prim, node, advance.
Every instruction of the marked kernel is attributed to the last marker above it in the
text, so a cold block the compiler lays out elsewhere (the slow slab, the ring spill) is
counted with the section it lands behind: read the table as the code a section's text
holds, not as one path through it. The markers are `asm volatile`, which code motion does
not cross, so the marked kernel can differ from the product: the whole-kernel totals of both
are printed, with the registers, spills and LDS of each.
Counts move with the compiler; nothing asserts them.
"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter, OrderedDict

SRC = "izpi_amd/csrc/trace.hip"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Iinclude",
         "--cuda-device-only", "-S"]
CLASSES = ["VALU", "SALU", "LDS", "VMEM", "other"]


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep", "s_setprio")):
        return "other"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def mangled(inst):
    return "_Z8k_trace2I" + "".join(("Lb%dE" % (v == "true")) if v in ("true", "false") else "Li%sE" % v
                                    for v in inst.split(",")) + "Ev"


def kernel_text(asm, prefix):
    m = re.search(r"^(%s\w*):.*?$(.*?)^\s*s_endpgm" % re.escape(prefix), asm, re.S | re.M)
    if not m:
        sys.exit("no kernel %s* in the assembly" % prefix)
    meta = {}
    tail = asm[m.end():]
    for key in ("NumVgprs", "ScratchSize", "Occupancy"):
        k = re.search(r"; %s: (\d+)" % key, tail)
        meta[key] = k.group(1) if k else "?"
    k = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", tail)
    meta["LDS"] = k.group(1) if k else "?"
    # spilled VGPRs of this kernel, from the metadata at the end of the file
    md = re.search(r"\.name:\s+%s.*?\.vgpr_spill_count:\s+(\d+)" % re.escape(m.group(1)), asm, re.S)
    if not md:  # key order varies: look inside the kernel's own metadata entry
        for ent in re.split(r"\n  - ", asm[asm.find("amdhsa.kernels"):]):
            if re.search(r"\.name:\s+%s\b" % re.escape(m.group(1)), ent):
                md = re.search(r"\.vgpr_spill_count:\s+(\d+)", ent)
    meta["VGPRs spilled"] = md.group(1) if md else "?"
    return m.group(2), meta


def count(body):
    secs = OrderedDict()
    cur = "(entry)"
    for line in body.split("\n"):
        mk = re.search(r"; IZPI_MARK (\w+)", line)
        if mk:
            cur = mk.group(1)
            continue
        if not line.startswith("\t"):
            continue
        t = line.strip()
        if not t or t.startswith((".", ";")):
            continue
        secs.setdefault(cur, Counter())[classify(t.split()[0])] += 1
    return secs


def compile_asm(out, extra):
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC, *extra], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def main():
    argv = sys.argv[1:]
    inst = "16,5,true,true,false,true,false"
    keep = None
    while argv and argv[0] in ("--instance", "--keep"):
        if argv[0] == "--instance":
            inst = argv[1]
        else:
            keep = argv[1]
        argv = argv[2:]
    tmp = keep or tempfile.mkdtemp()
    os.makedirs(tmp, exist_ok=True)
    plain, plain_meta = kernel_text(compile_asm(os.path.join(tmp, "trace_plain.s"), argv), mangled(inst))
    marked, marked_meta = kernel_text(compile_asm(os.path.join(tmp, "trace_marked.s"), ["-DIZPI_STEP_MARKS"] + argv), mangled(inst))
    print("k_trace2<%s>" % inst)
    print("%-10s %6s %6s %6s %6s %6s" % ("section", *CLASSES))
    secs = count(marked)
    for name, c in secs.items():
        print("%-10s %6d %6d %6d %6d %6d" % (name, *(c[k] for k in CLASSES)))
    for label, body, meta in (("marked", marked, marked_meta), ("product", plain, plain_meta)):
        tot = Counter()
        for c in count(body).values():
            tot.update(c)
        print("%-10s %6d %6d %6d %6d %6d   vgpr %s spilled %s scratch %s lds %s occupancy %s" % (
            label, *(tot[k] for k in CLASSES), meta["NumVgprs"], meta["VGPRs spilled"], meta["ScratchSize"], meta["LDS"],
            meta["Occupancy"]))


if __name__ == "__main__":
    main()
