#!/usr/bin/env python3
"""Static instruction counts of one k_trace2 instance, per section of its loop (gfx950, compile only).

    python tools/step_counts.py [--instance 16,5,true,true,false,true,false,true,true,true] [--keep DIR] [--trips FILE]
                                [--sq VALU,SALU,BRANCH] [extra hipcc flags...]

trace.hip is compiled device-only to assembly twice: as the product builds it, and with
-DIZPI_STEP_MARKS, which puts a comment marker (no instruction) at the head of each section
of the loop: head (idle ballot and the one test for a refill, a dequeue or the exit), due (an iteration in which that
test passes), dequeue, refill, pick (step choice), prim, node (step
counters and the ring-full test), spill, node_loads, slab_fast, slab_twin, node_tail,
advance (the pop candidate's read), spilled (a wave that has spilled tests its pops against the
spilled range), readback, advance_tail, finish, advance_end; overflow (the stack-depth error of the node
step, which no uploaded tree reaches: no trips).
The marked kernel is split into its basic blocks (labels, the compiler's `; %bb.N:` notes,
branches). A block outside the loop (the `in Loop` / `Parent Loop` notes say which are inside)
goes to the row `(entry)` before the loop's header and `(epilogue)` after it: the counter
write-back no longer counts as `advance`. A block of an inner loop (depth 2: the unrolled
ring-spill loops) goes to `(cold loops)`. A block that holds a marker belongs to it, the
instructions above the marker included (a basic block runs as a whole, and plain arithmetic may
be scheduled across an `asm volatile`). A block that holds none takes its row through the
control flow, not the text: the row its predecessors (branch sources and the block that falls
into it) end with; where they differ, the earliest predecessor in the text, which is the branch
around a region and not the region. So the fast slab's body, laid out behind the scalar twin's,
counts as the node step that branches to it. The first table lists every block with its row.
--trips FILE: FILE holds the JSON of an IZPI_TRACE_ICOUNT line (the trip counts of one frame
from a -DIZPI_TRACE_ICOUNT build, tools/variants.py build icount -DIZPI_TRACE_ICOUNT): each
row's instructions are multiplied by the trips of the path that runs it (TRIPS below) and
summed; --sq VALU,SALU,BRANCH prints the measured SQ_INSTS_VALU / SQ_INSTS_SALU / SQ_INSTS_BRANCH of the same frame
(tools/pmc_kernels.sh) beside the sums. A row that runs under a branch inside its section
is counted as if every trip ran all of it, so the sums are upper estimates of those rows.
The markers are `asm volatile`, which code motion does not cross, so the marked kernel can
differ from the product: the whole-kernel totals of both are printed, with the registers,
spills and LDS of each.
Counts move with the compiler; nothing asserts them.
"""
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter, OrderedDict

SRC = "izpi_amd/csrc/trace.hip"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Iinclude",
         "--cuda-device-only", "-S"]
CLASSES = ["VALU", "SALU", "branch", "LDS", "VMEM", "other"]


def classify(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_sleep", "s_setprio")):
        return "other"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call")):
        return "branch"  # (SQ_INSTS_BRANCH counts them, SQ_INSTS_SALU does not)
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


# the trip count (a key of the IZPI_TRACE_ICOUNT line, or a sum of keys) of each row
TRIPS = {"(entry)": ["waves"], "(epilogue)": ["waves"], "(cold loops)": ["spill"], "head": ["iterations"], "due": ["due"],
         "dequeue": ["dequeue"], "refill": ["refill"], "pick": ["iterations"], "prim": ["prim"],
         "node": ["node_fast", "node_twin"], "spill": ["spill"], "node_loads": ["node_fast", "node_twin"],
         "slab_fast": ["node_fast"], "slab_twin": ["node_twin"], "node_tail": ["node_fast", "node_twin"],
         "advance": ["iterations"], "spilled": ["spilled"], "overflow": [], "readback": ["readback"], "advance_tail": ["iterations"], "finish": ["finish"],
         "advance_end": ["iterations"]}


def blocks(body):
    """The kernel's basic blocks in text order: (name, row, Counter). Blocks start at labels, at
    the compiler's `; %bb.N:` notes and after branches; a block that holds markers is listed
    once per row it feeds."""
    # the step loop: the header most blocks name in their notes
    heads = Counter(re.findall(r"(?:Header=|Parent Loop )(BB\d+_\d+)", body))
    main = heads.most_common(1)[0][0] if heads else None
    bl = []  # dicts: name, note, items (marker names and instruction classes in order), last (final opcode), target

    def start(name, note):
        bl.append({"name": name, "note": note, "items": [], "last": None, "target": None, "labelled": name.startswith(".L")})

    start("(top)", "")
    for line in body.split("\n"):
        lb = re.match(r"^(\.LBB\d+_\d+):(.*)$", line) or re.match(r"^; (%bb\.\d+):(.*)$", line)
        if lb:
            if bl[-1]["items"] or bl[-1]["labelled"]:
                start(lb.group(1), lb.group(2))
            else:  # an empty block just opened after a branch: name it
                bl[-1].update(name=lb.group(1), note=lb.group(2), labelled=lb.group(1).startswith(".L"))
            continue
        mk = re.search(r"; IZPI_MARK (\w+)", line)
        if mk:
            bl[-1]["items"].append(("mark", mk.group(1)))
            continue
        if not line.startswith("\t"):
            continue
        t = line.strip()
        if not t or t.startswith((".", ";")):
            continue
        op = t.split()[0]
        bl[-1]["items"].append(("inst", classify(op)))
        bl[-1]["last"] = op
        if op.startswith(("s_cbranch", "s_branch")):
            bl[-1]["target"] = t.split()[1]
            start(bl[-1]["name"] + "'", bl[-1]["note"])
        elif op.startswith(("s_endpgm", "s_setpc")):
            start(bl[-1]["name"] + "'", "")
    bl = [b for b in bl if b["items"] or b["labelled"]]
    index = {b["name"]: k for k, b in enumerate(bl)}
    preds = [[] for _ in bl]
    for k, b in enumerate(bl):
        if b["target"] in index:
            preds[index[b["target"]]].append(k)
        if k + 1 < len(bl) and not (b["last"] or "").startswith(("s_branch", "s_endpgm", "s_setpc")):
            preds[k + 1].append(k)
    # rows: outside the loop and inner loops by the notes; a block with markers by its markers (the
    # instructions before its first marker run as often as the marker: the block's row is the first
    # marker's); a block without one takes the row its predecessors in the control flow end with,
    # the earliest of them in the text (the branch around a region, not the region) if they differ
    seen_loop, where = False, "(entry)"
    for b in bl:
        note = b["note"]
        b["in_loop"] = main is not None and (b["name"].rstrip("'") == ".L" + main or ("=" + main + " ") in note + " " or ("Parent Loop " + main) in note)
        seen_loop = seen_loop or b["in_loop"]
        if not b["in_loop"]:
            where = "(epilogue)" if seen_loop else "(entry)"
        marks = [v for kind, v in b["items"] if kind == "mark"]
        b["fixed"] = None if b["in_loop"] else where
        if b["in_loop"] and ("Depth=2" in note or "Parent Loop" in note):
            b["fixed"] = "(cold loops)"
        b["entry"] = b["fixed"] or (marks[0] if marks else None)
        b["exit"] = b["fixed"] or (marks[-1] if marks else None)
    changed = True
    while changed:
        changed = False
        for k, b in enumerate(bl):
            if b["entry"] is None:
                rows = [bl[p]["exit"] for p in sorted(preds[k]) if bl[p]["exit"] is not None and bl[p]["exit"] not in ("(entry)", "(epilogue)", "(cold loops)")]
                if rows:
                    b["entry"] = b["exit"] = rows[0]
                    changed = True
    out = []
    last = "(entry)"
    for b in bl:
        row = b["entry"] or last  # (unreached through the control flow: as the text has it)
        last = b["exit"] or row
        cnt = Counter()
        for kind, v in b["items"]:
            if kind == "mark":
                if not b["fixed"] and v != row:
                    if sum(cnt.values()):
                        out.append((b["name"], row, cnt))
                    row, cnt = v, Counter()
            else:
                cnt[v] += 1
        if sum(cnt.values()):
            out.append((b["name"], row, cnt))
    return out


def count(body):
    secs = OrderedDict()
    for _, row, c in blocks(body):
        secs.setdefault(row, Counter()).update(c)
    return secs


def compile_asm(out, extra):
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", out, SRC, *extra], check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def main():
    argv = sys.argv[1:]
    inst = "16,5,true,true,false,true,false,true,true,true"
    keep = trips = sq = None
    while argv and argv[0] in ("--instance", "--keep", "--trips", "--sq"):
        if argv[0] == "--instance":
            inst = argv[1]
        elif argv[0] == "--trips":
            trips = json.load(open(argv[1]))
        elif argv[0] == "--sq":
            sq = [float(v) for v in argv[1].split(",")]
        else:
            keep = argv[1]
        argv = argv[2:]
    tmp = keep or tempfile.mkdtemp()
    os.makedirs(tmp, exist_ok=True)
    plain, plain_meta = kernel_text(compile_asm(os.path.join(tmp, "trace_plain.s"), argv), mangled(inst))
    marked, marked_meta = kernel_text(compile_asm(os.path.join(tmp, "trace_marked.s"), ["-DIZPI_STEP_MARKS"] + argv), mangled(inst))
    print("k_trace2<%s>" % inst)
    print("%-28s %-13s %6s %6s %6s %6s %6s %6s" % ("block", "row", *CLASSES))
    for label, row, c in blocks(marked):
        print("%-28s %-13s %6d %6d %6d %6d %6d %6d" % (label, row, *(c[k] for k in CLASSES)))
    print()
    print("%-13s %6s %6s %6s %6s %6s %6s" % ("row", *CLASSES))
    secs = count(marked)
    for name, c in secs.items():
        print("%-13s %6d %6d %6d %6d %6d %6d" % (name, *(c[k] for k in CLASSES)))
    for label, body, meta in (("marked", marked, marked_meta), ("product", plain, plain_meta)):
        tot = Counter()
        for c in count(body).values():
            tot.update(c)
        print("%-13s %6d %6d %6d %6d %6d %6d   vgpr %s spilled %s scratch %s lds %s occupancy %s" % (
            label, *(tot[k] for k in CLASSES), meta["NumVgprs"], meta["VGPRs spilled"], meta["ScratchSize"], meta["LDS"],
            meta["Occupancy"]))
    if trips:
        print()
        print("%-13s %14s %6s %6s %6s %10s %10s %10s" % ("row", "trips", "VALU", "SALU", "branch", "VALU (G)", "SALU (G)", "branch (G)"))
        tot = [0.0, 0.0, 0.0]
        for name, c in secs.items():
            n = sum(trips[k] for k in TRIPS[name])
            g = [n * c[k] for k in ("VALU", "SALU", "branch")]
            tot = [a + b for a, b in zip(tot, g)]
            print("%-13s %14d %6d %6d %6d %10.3f %10.3f %10.3f" % (name, n, c["VALU"], c["SALU"], c["branch"], *(v / 1e9 for v in g)))
        print("%-13s %14s %6s %6s %6s %10.3f %10.3f %10.3f" % ("table", "", "", "", "", *(v / 1e9 for v in tot)))
        if sq:
            print("%-13s %14s %6s %6s %6s %10.3f %10.3f %10.3f" % ("SQ_INSTS", "", "", "", "", *(v / 1e9 for v in sq)))
            print("%-13s %14s %6s %6s %6s %9.1f%% %9.1f%% %9.1f%%" % ("table / SQ", "", "", "", "", *(100 * a / b for a, b in zip(tot, sq))))


if __name__ == "__main__":
    main()
